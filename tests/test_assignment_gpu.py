"""The device assignment solver (zh_linear_assignment) against scipy.optimize.linear_sum_assignment on the same float32 matrices —
rows and columns equal element for element, ties included — and the mask-packing kernel (zh_pack_masks_u8)."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from zutis_amd import _lib, ops

# (n, Q): tiny, square, the transposed branch (n > Q), the training shape, > 16 instances with an odd Q, the lane / loop edges
SHAPES = [(1, 1), (1, 7), (3, 3), (5, 3), (13, 7), (10, 100), (17, 101), (9, 64), (9, 65), (9, 128), (9, 129)]
KINDS = ["uniform", "ints", "duplicate"]


def _matrix(n, Q, kind, seed):
    g = np.random.default_rng(seed)
    if kind == "ints":
        return g.integers(0, 4, (n, Q)).astype(np.float32)                  # heavy ties
    cm = g.random((n, Q), dtype=np.float32)
    if kind == "duplicate":
        if n > 1:
            cm[n - 1] = cm[0]                                               # bit-identical rows
        elif Q > 1:
            cm[:, Q - 1] = cm[:, 0]                                         # a single row has no other row: tie two columns
    return cm


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,Q", SHAPES)
def test_solver_equals_scipy(dev, n, Q, kind):
    for seed in (0, 1, 2):
        cm = _matrix(n, Q, kind, 1000 * seed + 31 * n + Q)
        want_r, want_c = linear_sum_assignment(cm)
        rows, cols = ops.linear_assignment(torch.from_numpy(cm).to(dev))
        assert rows.dtype == cols.dtype == np.int64
        assert np.array_equal(rows, want_r) and np.array_equal(cols, want_c), (n, Q, kind, seed)


def _host_loop(cost_h, off, skip, B, L, Q):
    """The host loop of HipCriterion (assignment='host') on a costs buffer."""
    pairs, total = [], 0.0
    for b in range(B):
        if skip[b]:
            continue
        n_b = int(off[b + 1] - off[b])
        for l in range(L):
            base = (L * int(off[b]) + l * n_b) * Q
            cm = cost_h[base:base + n_b * Q].reshape(n_b, Q)
            ii, qq = linear_sum_assignment(cm)
            total += float(cm[ii, qq].astype(np.float64).sum())
            pairs += [[b, l, int(q), int(i)] for i, q in zip(ii, qq)]
    return np.array(pairs, dtype=np.int32).reshape(-1, 4), np.float32(total / B)


def _batched(dev, cost_h, counts, skip, L, Q):
    B = len(counts)
    off = np.zeros(B + 1, dtype=np.int32)
    off[1:] = np.cumsum(counts)
    n_tot, n_max = int(off[-1]), max(counts)
    cap = ops.assignment_pairs_capacity(B, L, Q, n_max, n_tot)
    out = torch.zeros(8 + 4 * cap, dtype=torch.int32, device=dev)
    ops.linear_assignment_batched(torch.from_numpy(cost_h).to(dev), torch.from_numpy(off).to(dev),
                                  torch.tensor(skip, dtype=torch.int32, device=dev), B, L, Q, n_max, n_tot, out[8:], out[1:2],
                                  out[4:5].view(torch.float32), out[0:1])
    h = out.cpu().numpy()
    return int(h[0]), int(h[1]), h[8:].reshape(-1, 4), h[4:5].view(np.float32)[0], off


@pytest.mark.gpu
@pytest.mark.parametrize("counts,Q", [((4, 3, 0), 7), ((9, 2, 0), 5)])
def test_batched_call_equals_the_host_loop(dev, counts, Q):
    """B = 3, L = 2, image 1 skipped, image 2 without instances: the compacted pairs, their count and their order are the host's."""
    L, skip = 2, [0, 1, 0]
    g = np.random.default_rng(5)
    cost_h = g.random(L * sum(counts) * Q, dtype=np.float32)
    cost_h[:Q] = cost_h[Q:2 * Q]                                            # two tied rows in image 0, layer 0
    status, n_pairs, pairs, loss, off = _batched(dev, cost_h, counts, skip, L, Q)
    want, want_loss = _host_loop(cost_h, off, skip, len(counts), L, Q)
    assert status == 0 and n_pairs == len(want) == L * min(counts[0], Q)
    assert np.array_equal(pairs[:n_pairs], want)
    assert not pairs[n_pairs:].any()                                        # nothing written past the pairs
    assert abs(float(loss) - float(want_loss)) <= float(np.spacing(want_loss))


@pytest.mark.gpu
def test_non_finite_cost_raises_and_the_next_call_is_right(dev):
    cm = _matrix(5, 9, "uniform", 3)
    for bad in (np.nan, np.inf, -np.inf):                                   # +inf: the one deliberate difference from scipy
        x = cm.copy()
        x[2, 4] = bad
        with pytest.raises(ValueError, match="non-finite"):
            ops.linear_assignment(torch.from_numpy(x).to(dev))
    # in a batched call only the bad problem loses its pairs
    costs = np.concatenate([cm.reshape(-1), cm.reshape(-1)])
    costs[7] = np.nan
    status, n_pairs, pairs, _, _ = _batched(dev, costs, (5,), [0], 2, 9)
    want_r, want_c = linear_sum_assignment(cm)
    assert status == ops.STATUS_NONFINITE and n_pairs == 5
    assert np.array_equal(pairs[:5], np.stack([np.zeros(5), np.ones(5), want_c, want_r], 1).astype(np.int32))
    rows, cols = ops.linear_assignment(torch.from_numpy(cm).to(dev))
    assert np.array_equal(rows, want_r) and np.array_equal(cols, want_c)


@pytest.mark.gpu
def test_shape_above_the_cap_is_the_argument_error(dev):
    with pytest.raises(_lib.ZutisHipError, match=r"rc=-1.*exceeds the cap"):
        ops.linear_assignment(torch.zeros((2, ops.ASSIGN_MAX_DIM + 1), device=dev))
    with pytest.raises(_lib.ZutisHipError, match=r"rc=-1.*exceeds the cap"):
        ops.linear_assignment(torch.zeros((ops.ASSIGN_MAX_DIM + 1, 2), device=dev))
    rows, cols = ops.linear_assignment(torch.zeros((2, ops.ASSIGN_MAX_DIM), device=dev))      # at the cap: a constant matrix -> identity
    assert rows.tolist() == [0, 1] and cols.tolist() == [0, 1]


# ---- packing

COUNTS, HW = (2, 0, 5), (24, 24)


def _sources(dtype, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in COUNTS:
        m = torch.randint(0, 2, (n,) + HW, generator=g)
        if dtype == torch.uint8:
            m = m * torch.randint(1, 256, (n,) + HW, generator=g)           # any non-zero byte is "set"
        elif dtype == torch.int64:
            m = m * torch.tensor([1, -3, 1 << 40, 1 << 32])[torch.randint(0, 4, (n,) + HW, generator=g)]     # low bytes may be 0
        out.append(m.to(dtype))
    return out


def _want(srcs):
    return torch.cat([(g != 0).to(torch.uint8) for g in srcs], 0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.int64])
def test_pack_masks_from_separate_allocations(dev, dtype):
    srcs = _sources(dtype, 7)
    on = [g.to(dev) for g in srcs]
    gt, inst_off, counts = ops.pack_masks_u8(on, *HW)
    assert counts == list(COUNTS) and inst_off.cpu().tolist() == [0, 2, 2, 7]
    assert gt.dtype == torch.uint8 and torch.equal(gt.cpu(), _want(srcs))
    assert all(gt.data_ptr() != g.data_ptr() for g in on if g.shape[0])


@pytest.mark.gpu
def test_pack_masks_zero_copy_out_of_order_and_misaligned(dev):
    base = torch.cat(_sources(torch.bool, 9), 0).to(dev)                    # bool [7, 24, 24] in one allocation, as synth delivers it
    views = list(torch.split(base, list(COUNTS), 0))
    gt, inst_off, _ = ops.pack_masks_u8(views, *HW)
    assert gt.data_ptr() == base.data_ptr() and gt.shape == (7,) + HW       # used where it lies
    assert inst_off.cpu().tolist() == [0, 2, 2, 7] and torch.equal(gt.cpu(), base.cpu().to(torch.uint8))
    # the same masks as uint8 views with arbitrary non-zero bytes: not 0 / 1 where they lie, so they are packed
    raw = torch.cat(_sources(torch.uint8, 9), 0).to(dev)
    gt, _, _ = ops.pack_masks_u8(list(torch.split(raw, list(COUNTS), 0)), *HW)
    assert gt.data_ptr() != raw.data_ptr() and torch.equal(gt.cpu(), (raw != 0).to(torch.uint8).cpu())
    # views of one allocation that are NOT in order: packed
    back = [base[2:4], base[0:0], base[0:5]]
    gt, inst_off, _ = ops.pack_masks_u8(back, *HW)
    assert gt.data_ptr() != base.data_ptr() and torch.equal(gt.cpu(), _want([v.cpu() for v in back]))
    # sources at odd byte addresses (the byte path of the kernel)
    flat = torch.zeros(3 + 7 * 576 + 5, dtype=torch.uint8, device=dev)
    flat[3:3 + 7 * 576] = raw.reshape(-1)
    odd = [flat[3:3 + 2 * 576].view(2, *HW), flat[0:0].view(0, *HW), flat[3 + 2 * 576 + 1:3 + 7 * 576 + 1].view(5, *HW)]
    gt, _, _ = ops.pack_masks_u8(odd, *HW)
    assert torch.equal(gt.cpu(), _want([v.cpu() for v in odd]))
    with pytest.raises(_lib.ZutisHipError, match="all bool / uint8 or all int64"):
        ops.pack_masks_u8([views[0], views[2].to(torch.int64)], *HW)
