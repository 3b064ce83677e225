"""GPU: the two device string kernels (csrc/mask_rle.hip) on masks with a PRESCRIBED number of runs, at every count where the code
takes another path: the delta rule switching on (nc 1 .. 4), the runs-per-step loops of the chain (256) and of the fused kernel (two
per thread: 128 at 64 threads, 256 at 128), the run limit, the LDS copy of the list, and capacities one entry / one byte short.
Masks come from seeded run lengths drawn from {1, 9, 16, 31, 40, 1000} (tests/_rle_case.py), both pixel-0 values; the expected strings
are rle.encode_py's.  Random and structured masks, boxes, areas and the cursor's disjoint places are pinned by
test_kernels_gpu.test_device_rle_strings_equal_the_host_encoder / test_fused_run_box_string_kernel; a list over max_runs by far and a
list past the capacity by far are there too — here the limits are met exactly and missed by one."""
import numpy as np
import pytest
import torch

from tests import _rle_case as RC
from zutis_amd import ops, rle

pytestmark = pytest.mark.gpu


def _masks(size, specs):
    """specs (nc, lead) -> masks u8 [n, h, w] and their expected strings."""
    h, w = size
    ms = [RC.mask_from_runs(size, RC.seeded_runs(h * w, nc, lead, seed=1000 * nc + lead)) for nc, lead in specs]
    return np.ascontiguousarray(np.stack(ms)), [rle.encode_py(m)["counts"] for m in ms]


def _kept(n, dev):
    return torch.arange(n, dtype=torch.int32, device=dev).view(1, n), torch.tensor([n], dtype=torch.int32, device=dev)


def _chain(masks, max_runs, dev, pos_len=None, out_len=None):
    """mask_runs_kept(packed=True) + mask_rle_kept over all masks of one image, kept in order -> [(string or None)], nt per mask."""
    n, h, w = masks.shape
    md = torch.from_numpy(masks).to(dev).view(1, n, h, w)
    idx, cnt = _kept(n, dev)
    f = np.stack([m.reshape(-1, order="F") for m in masks])
    nts = (f[:, 1:] != f[:, :-1]).sum(1)
    total = int(np.minimum(nts, max_runs).sum())
    pos = torch.full((total if pos_len is None else pos_len,), -1, dtype=torch.int32, device=dev)
    nr = torch.empty((n, 2), dtype=torch.int32, device=dev)
    ba = torch.empty((n, 5), dtype=torch.int32, device=dev)
    ops.mask_runs_kept(md, idx, cnt, max_runs, pos, nr, ba, packed=True)
    assert nr.cpu().numpy()[:, 0].tolist() == nts.tolist()
    out = torch.zeros((5 * total + 16 * n if out_len is None else out_len,), dtype=torch.uint8, device=dev)
    ln = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ops.mask_rle_kept(pos, nr, cnt, 1, n, max_runs, h * w, out, ln)
    out_h, ln_h = out.cpu().numpy(), ln.cpu().numpy()
    got, off = [], 0
    for i in range(n):
        c0 = 5 * off + 16 * i
        got.append(out_h[c0:c0 + ln_h[i]].tobytes() if ln_h[i] >= 0 else None)
        off += min(int(nts[i]), max_runs)
    return got, nts


SMALL = [(nc, lead) for nc in (1, 2, 3, 4, 255, 256, 257, 513) for lead in (0, 1) if nc > lead]


def test_chain_run_counts_at_the_delta_rule_and_the_256_run_step(dev):
    masks, want = _masks((16, 64), SMALL)
    got, _ = _chain(masks, 8192, dev)
    assert got == want


def test_chain_run_limit_met_and_missed_by_one(dev):
    """nt == max_runs is encoded, nt == max_runs + 1 reports -1 (and takes max_runs entries of the list: the next string is intact)."""
    masks, want = _masks((16, 64), [(21, 0), (22, 0), (22, 1), (23, 1), (9, 0)])
    got, nts = _chain(masks, 20, dev)
    assert nts.tolist() == [20, 21, 20, 21, 8] and got == [want[0], None, want[2], None, want[4]]


@pytest.mark.parametrize("nt", [8192, 8193])
def test_chain_list_in_lds_and_read_in_place(dev, nt):
    """RLE_LDS_RUNS = 8192 transitions are copied to LDS, one more is read where it lies: 64 x 257 masks, both pixel-0 values."""
    ms = [RC.mask_from_runs((64, 257), lead + RC.alternating_prefix_runs(64 * 257, nt)) for lead in ([], [0])]
    got, nts = _chain(np.ascontiguousarray(np.stack(ms)), 8193, dev)
    assert nts.tolist() == [nt, nt] and got == [rle.encode_py(m)["counts"] for m in ms]


def test_chain_capacities_one_short(dev):
    """A packed list one entry too short for the last mask, and an `out` one byte short of the last mask's 5 * nc budget: -1 for that mask,
    the neighbour in front of it encoded in full."""
    masks, want = _masks((16, 64), [(257, 0), (40, 1), (129, 0)])
    _, nts = _chain(masks, 8192, dev)
    total = int(nts.sum())
    assert _chain(masks, 8192, dev, pos_len=total - 1)[0] == [want[0], want[1], None]
    budget = 5 * int(nts[:2].sum()) + 16 * 2 + 5 * 129                  # start of the last string + five characters per run
    assert _chain(masks, 8192, dev, out_len=budget)[0] == want
    assert _chain(masks, 8192, dev, out_len=budget - 1)[0] == [want[0], want[1], None]


def _fused(masks, max_runs, dev, use_bits, out_len=1 << 16):
    n, h, w = masks.shape
    md = torch.from_numpy(masks).to(dev).view(1, n, h, w)
    idx, cnt = _kept(n, dev)
    bits = None
    if use_bits:
        bits = torch.empty((1, n, (h * w + 63) // 64), dtype=torch.int64, device=dev)
        ops.mask_iou_counts(md[0], n, h * w, torch.empty((n, n), dtype=torch.int32, device=dev), torch.empty((n, n), dtype=torch.int32, device=dev),
                            workspace=bits[0])
    out = torch.zeros((out_len,), dtype=torch.uint8, device=dev)
    cursor = torch.zeros((1,), dtype=torch.int32, device=dev)
    info = torch.full((n, 8), -7, dtype=torch.int32, device=dev)
    ops.mask_rle_fused_kept(md, idx, cnt, max_runs, out, cursor, info, bits=bits)
    out_h, info_h = out.cpu().numpy(), info.cpu().numpy()
    got = [out_h[o:o + ln].tobytes() if ln >= 0 else None for o, ln in info_h[:, :2].tolist()]
    return got, info_h, int(cursor.item()), out_h


@pytest.mark.parametrize("use_bits", [False, True])
@pytest.mark.parametrize("W,ncs", [(64, (1, 2, 3, 4, 127, 128, 129, 257)), (65, (1, 2, 3, 4, 255, 256, 257))])
def test_fused_run_counts_at_the_delta_rule_and_the_two_runs_per_thread_step(dev, W, ncs, use_bits):
    """W = 64: 64 threads, 128 runs per step; W = 65: 128 threads, 256 runs per step."""
    specs = [(nc, lead) for nc in ncs for lead in (0, 1) if nc > lead]
    masks, want = _masks((16, W), specs)
    got, info, cursor, _ = _fused(masks, 8192, dev, use_bits)
    assert got == want and cursor == sum(len(s) for s in want)
    assert info[:, 7].tolist() == [nc - 1 - lead for nc, lead in specs]


@pytest.mark.parametrize("use_bits", [False, True])
def test_fused_run_limit_met_and_missed_by_one(dev, use_bits):
    masks, want = _masks((16, 64), [(21, 0), (22, 0), (22, 1), (23, 1), (9, 0)])
    got, info, _, _ = _fused(masks, 20, dev, use_bits)
    assert info[:, 7].tolist() == [20, 21, 20, 21, 8] and got == [want[0], None, want[2], None, want[4]]
    assert info[[1, 3], 1].tolist() == [-1, -1]


def test_fused_out_one_byte_short(dev):
    """`out` too short for the one string by one byte: length -1, nothing written, and the cursor has moved past the string all the same (the
    host sees from it how much room a second pass needs)."""
    masks, want = _masks((16, 64), [(129, 1)])
    got, info, cursor, out_h = _fused(masks, 8192, dev, False, out_len=len(want[0]))
    assert got == want and cursor == len(want[0])
    got, info, cursor, out_h = _fused(masks, 8192, dev, False, out_len=len(want[0]) - 1)
    assert got == [None] and info[0, :2].tolist() == [0, -1] and cursor == len(want[0]) and not out_h.any()
