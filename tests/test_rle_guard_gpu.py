"""The device RLE kernels of csrc/mask_rle.hip — zh_mask_runs, zh_mask_runs_kept (row and packed form), zh_mask_rle_kept and
zh_mask_rle_fused_kept — at their capacity and tile edges, every output (positions, nruns, box_area, out, out_len, info, cursor, the
exact-size workspace) carved out of a 0xA5 arena and every input (masks, kept_index, kept_count, bits, crafted lists) out of a 0xFF
arena of tests/_guard.py; assert_untouched runs after every launch.  All comparisons are exact: whole output buffers are compared with
buffers built from tests/_rle_guard_case.py's references (numpy transition lists, boxes, areas; the host encoder's strings; the
capacity rules restated from include/zutis_hip.h), so an entry past a capacity, a byte of a refused string, a touched slack byte of a
slot or a written row of a slot past an image's count all show.  tests/test_rle_guard_case_cpu.py proves which staging path, list
source, items-per-thread regime and LDS layout branch each case reaches."""
import functools

import numpy as np
import pytest
import torch

from tests import _rle_guard_case as R
from tests._guard import IN_FILL, OUT_FILL, Arena, assert_untouched

pytestmark = pytest.mark.gpu
I32, I64, U8 = torch.int32, torch.int64, torch.uint8
PAD = 1 << 20                                  # behind the last view: an overrun of a whole list or string stays inside the allocation


class _Carve:
    """An arena, its named views and a pad that no launch may touch."""

    def __init__(self, dev, fill):
        self.a, self.v = Arena(fill, dev), {}

    def add(self, name, dtype, M, N, **kw):
        self.v[name] = self.a.add(name, dtype, M, max(int(N), 1), tail_rows=0, **kw)
        return self.v[name]

    def workspace(self, name, nbytes):
        self.v[name] = self.a.workspace(name, nbytes)
        return self.v[name]

    def seal(self):
        self.a.add("_pad", U8, 1, PAD, tail_rows=0)
        self.a.bytes
        return self

    def check(self):
        assert_untouched(self.a, list(self.v.values()))

    def np(self, name):
        return self.v[name].get()[0, 0].numpy()


def _p(view):
    from zutis_amd import ops
    return ops._p(view.t)


def _call(entry, *args):
    from zutis_amd import ops
    ops._call(entry, *args, ops._stream())
    torch.cuda.synchronize()


def _ws_size(n, W):
    from zutis_amd import _lib
    return int(_lib.load(raw=True).zh_mask_runs_workspace_size(int(n), int(W)))


def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = np.argwhere(got != want)[0].tolist()
        raise AssertionError(f"{what}: {int((got != want).sum())} element(s) differ, first at {at}: got {got[tuple(at)]}, want {want[tuple(at)]}")


class _Ref:
    def __init__(self, mask):
        self.mask, self.T, self.lead, self.ba = mask, R.transitions(mask), R.lead_of(mask), R.box_area(mask)
        self.nt = len(self.T)

    @functools.cached_property
    def string(self):
        return R.string_of_mask(self.mask)


@functools.lru_cache(maxsize=None)
def _refs(H, W):
    """name -> reference of the mask set of a shape: built once, shared, never written to."""
    return {k: _Ref(m) for k, m in R.mask_set(H, W, 1000 * H + W).items()}


def _pivots(nt):
    return sorted({1, max(1, nt), max(1, nt - 1)})


# ------------------------------------------------------------------------------------------------ the panel kernels
def _inputs(dev, masks, idx=None, cnt=None, misalign=0, bits_words=0):
    n = masks.shape[0] * (masks.shape[1] if masks.ndim == 4 else 1)
    H, W = masks.shape[-2:]
    c = _Carve(dev, IN_FILL)
    c.add("masks", U8, n, H * W, misalign=misalign)
    if idx is not None:
        c.add("idx", I32, idx.shape[0], idx.shape[1])
        c.add("cnt", I32, 1, len(cnt))
    if bits_words:
        c.add("bits", I64, n, bits_words)
    c.seal()
    c.v["masks"].put(torch.from_numpy(np.ascontiguousarray(masks)))
    if idx is not None:
        c.v["idx"].put(torch.from_numpy(idx))
        c.v["cnt"].put(torch.from_numpy(cnt))
    return c


def _run_outputs(dev, n, W, n_pos_rows, n_pos_cols):
    c = _Carve(dev, OUT_FILL)
    c.add("positions", I32, n_pos_rows, n_pos_cols)
    c.add("nruns", I32, n, 2)
    c.add("box_area", I32, n, 5)
    c.workspace("workspace", _ws_size(n, W))
    return c.seal()


def _expected_rows(refs, rows, n, max_runs):
    """rows: {row index: reference}.  -> positions [n, max_runs], nruns [n, 2], box_area [n, 5] with untouched entries at the fill."""
    pos, nr, ba = (np.full(s, R.FILL32, np.int32) for s in ((n, max_runs), (n, 2), (n, 5)))
    for i, r in rows.items():
        k = min(r.nt, max_runs)
        pos[i, :k] = r.T[:k]
        nr[i] = (r.nt, r.lead)
        ba[i] = r.ba
    return pos, nr, ba


def _check_runs(dev, refs, names, H, W, max_runs, misalign):
    """zh_mask_runs over the whole set through a reversed `sel`."""
    n = len(names)
    masks = np.stack([refs[k].mask for k in names])
    ins = _Carve(dev, IN_FILL)
    ins.add("masks", U8, n, H * W, misalign=misalign)
    ins.add("sel", I32, 1, n)
    ins.seal()
    sel = np.arange(n - 1, -1, -1, dtype=np.int32)
    ins.v["masks"].put(torch.from_numpy(masks))
    ins.v["sel"].put(torch.from_numpy(sel))
    out = _run_outputs(dev, n, W, n, max_runs)
    _call("zh_mask_runs", _p(ins.v["masks"]), _p(ins.v["sel"]), n, H, W, max_runs, _p(out.v["positions"]), _p(out.v["nruns"]),
          _p(out.v["box_area"]), _p(out.v["workspace"]), _ws_size(n, W))
    out.check(); ins.check()
    pos, nr, ba = _expected_rows(refs, {i: refs[names[q]] for i, q in enumerate(sel.tolist())}, n, max_runs)
    what = ("zh_mask_runs", H, W, max_runs, misalign)
    _eq(out.np("nruns"), nr, what + ("nruns",)); _eq(out.np("box_area"), ba, what + ("box_area",)); _eq(out.np("positions"), pos, what + ("positions",))


def _kept_case(refs, names, seed):
    Q = len(names)
    orders = R.kept_orders(Q, seed)
    idx, cnt = R.kept_table(len(orders), Q, orders)
    masks = np.stack([np.stack([refs[k].mask for k in names])] * len(orders))
    return orders, idx, cnt, masks


def _check_kept(dev, refs, names, H, W, max_runs, misalign, packed_caps):
    """zh_mask_runs_kept in row form, then in packed form at every capacity of `packed_caps`."""
    orders, idx, cnt, masks = _kept_case(refs, names, H * 7 + W)
    B, Q = idx.shape
    kept = [(b * Q + j, refs[names[q]]) for b, o in enumerate(orders) for j, q in enumerate(o)]
    ins = _inputs(dev, masks, idx, cnt, misalign)

    def launch(out, cap):
        _call("zh_mask_runs_kept", _p(ins.v["masks"]), _p(ins.v["idx"]), _p(ins.v["cnt"]), B, Q, H, W, max_runs, _p(out.v["positions"]), cap,
              _p(out.v["nruns"]), _p(out.v["box_area"]), _p(out.v["workspace"]), _ws_size(B * Q, W))
        out.check(); ins.check()

    out = _run_outputs(dev, B * Q, W, B * Q, max_runs)
    launch(out, 0)
    pos, nr, ba = _expected_rows(refs, dict(kept), B * Q, max_runs)
    what = ("zh_mask_runs_kept", H, W, max_runs, misalign)
    _eq(out.np("nruns"), nr, what + ("nruns",)); _eq(out.np("box_area"), ba, what + ("box_area",)); _eq(out.np("positions"), pos, what + ("positions",))
    nts = [r.nt for _, r in kept]
    for name, cap in packed_caps(nts, max_runs).items():
        out = _run_outputs(dev, B * Q, W, 1, cap)
        launch(out, cap)
        want, n_short = np.full((cap,), R.FILL32, np.int32), 0
        for (_, r), (off, _, _) in zip(kept, R.place(nts, max_runs)):
            k = R.packed_written(off, r.nt, max_runs, cap)
            want[off:off + k] = r.T[:k]
            n_short += k < min(r.nt, max_runs)
        assert (n_short == 0) == (name == "exact"), (what, name, cap)
        _eq(out.np("nruns"), nr, what + (name, "nruns")); _eq(out.np("box_area"), ba, what + (name, "box_area"))
        _eq(out.np("positions")[0], want, what + (name, cap, "packed positions"))


@pytest.mark.parametrize("W,misalign", [(W, 0) for W in R.PANEL_W] + [(80, 4)])
def test_panel_kernels_write_exactly_their_lists(dev, W, misalign):
    """W in {1, 63, 64, 65, 72, 80, 144} x H in {1, 3, 4, 5, 37} (fewer rows than the four row segments; a 16-column last panel on the
    16-byte staging path; W % 16 != 0 and a base 4 bytes off alignment on the byte path), the whole mask set per shape, max_runs in
    {1, nt, nt - 1} of the noise mask: nruns holds the true count, exactly min(nt, max_runs) entries are written, in row form and in
    packed form with the capacity at the sum of the lists, one below, inside a middle list and at 1."""
    assert R.panel_staging(W, misalign) == ("vector" if (W, misalign) in ((64, 0), (80, 0), (144, 0)) else "scalar")
    for H in R.PANEL_H:
        refs = _refs(H, W)
        names = [k for k in refs]
        for max_runs in _pivots(refs["noise"].nt):
            _check_runs(dev, refs, names, H, W, max_runs, misalign)
            _check_kept(dev, refs, names, H, W, max_runs, misalign, R.packed_capacities)


# ------------------------------------------------------------------------------------------------ the string kernel
def _rle_kept(dev, pos_view, packed_cap, nr_view, cnt_view, B, Q, max_runs, HW, out_cap):
    out = _Carve(dev, OUT_FILL)
    out.add("out", U8, 1, out_cap)
    out.add("out_len", I32, 1, B * Q)
    out.seal()
    _call("zh_mask_rle_kept", _p(pos_view), packed_cap, _p(nr_view), _p(cnt_view), B, Q, max_runs, HW, _p(out.v["out"]), out_cap, _p(out.v["out_len"]))
    out.check()
    return out.np("out")[0], out.np("out_len")[0]


def _check_strings(got, lists, rows, n_slots, max_runs, HW, packed_cap, out_cap, what):
    """lists: per kept mask (positions, lead); rows: its slot.  The whole of `out` and of `out_len` against the reference."""
    out_h, len_h = got
    lens, written = R.expected_strings(lists, max_runs, HW, packed_cap, out_cap)
    want_len = np.full((n_slots,), R.FILL32, np.int32)
    want_len[rows] = lens
    want = np.full((out_cap,), OUT_FILL, np.uint8)
    for c0, s in written.items():
        assert c0 + len(s) <= out_cap
        want[c0:c0 + len(s)] = np.frombuffer(s, np.uint8)
    _eq(len_h, want_len, what + ("out_len",))
    _eq(out_h, want, what + ("out",))
    return lens


def _masks_to_strings(dev, mask_list, orders, H, W, max_runs, out_caps):
    """zh_mask_runs_kept (packed, capacity = the sum of the lists) feeds zh_mask_rle_kept from its guarded outputs."""
    Q = len(mask_list)
    refs = [_Ref(m) for m in mask_list]
    idx, cnt = R.kept_table(len(orders), Q, orders)
    B = len(orders)
    masks = np.stack([np.stack(mask_list)] * B)
    ins = _inputs(dev, masks, idx, cnt)
    kept = [(b * Q + j, refs[q]) for b, o in enumerate(orders) for j, q in enumerate(o)]
    nts = [r.nt for _, r in kept]
    cap = max(R.packed_total(nts, max_runs), 1)
    runs = _run_outputs(dev, B * Q, W, 1, cap)
    _call("zh_mask_runs_kept", _p(ins.v["masks"]), _p(ins.v["idx"]), _p(ins.v["cnt"]), B, Q, H, W, max_runs, _p(runs.v["positions"]), cap,
          _p(runs.v["nruns"]), _p(runs.v["box_area"]), _p(runs.v["workspace"]), _ws_size(B * Q, W))
    runs.check(); ins.check()
    lists = [(r.T, r.lead) for _, r in kept]
    rows = [i for i, _ in kept]
    res = []
    for out_cap in out_caps(lists):
        got = _rle_kept(dev, runs.v["positions"], cap, runs.v["nruns"], ins.v["cnt"], B, Q, max_runs, H * W, out_cap)
        runs.check(); ins.check()                                  # the string kernel writes none of its inputs
        lens = _check_strings(got, lists, rows, B * Q, max_runs, H * W, cap, out_cap, ("zh_mask_rle_kept", H, W, max_runs, out_cap))
        for (_, r), n in zip(kept, lens):
            assert n == -1 or n == len(r.string)                   # the list's string is the host encoder's string of the mask
        res.append(lens)
    return res


def test_string_kernel_at_the_chunk_edges_and_out_capacity(dev):
    """nc in {1, 2, 255, 256, 257, 512, 513} values (the 256-value chunks carry a scan between them), with and without a leading
    run; `out` ending at exactly the last needed byte — every string written — and one below — the last one refused without a byte,
    the earlier ones intact; every slack byte of every slot still the fill."""
    H, W, masks, orders, max_runs = R.nc_edge_case()
    exact, below = _masks_to_strings(dev, masks, orders, H, W, max_runs, lambda lists: (R.last_needed(lists, max_runs), R.last_needed(lists, max_runs) - 1))
    assert min(exact) > 0 and below[:-1] == exact[:-1] and below[-1] == -1


def test_string_kernel_with_a_middle_mask_over_max_runs(dev):
    """max_runs = 300 < nt of the masks in the middle: they report -1, the later ones are placed by min(nt, max_runs)."""
    H, W, masks, orders, max_runs = R.over_max_runs_case()
    (lens,) = _masks_to_strings(dev, masks, orders, H, W, max_runs, lambda lists: (R.last_needed(lists, max_runs),))
    assert [n < 0 for n in lens] == [False, True, False, True, False, False, False, True, False]


def test_string_kernel_either_side_of_the_lds_copy(dev):
    """Lists of 8192 (copied to LDS) and 8193 (read where they lie) transitions at max_runs = 8200, from 96 x 96 masks."""
    H, W, masks, orders, max_runs = R.lds_edge_case()
    assert [R.list_source(len(R.transitions(m))) for m in masks] == ["lds", "global", "lds"]
    exact, below = _masks_to_strings(dev, masks, orders, H, W, max_runs, lambda lists: (R.last_needed(lists, max_runs), R.last_needed(lists, max_runs) - 1))
    assert min(exact) > 0 and below[:-1] == exact[:-1] and below[-1] == -1


def _crafted(dev, lists, HW, max_runs, out_caps, B=1, packed_slack=0):
    """zh_mask_rle_kept from a crafted (positions, nruns) pair with no mask at all: one image, every slot kept but the last."""
    Q = len(lists) + 1
    nts = [len(p) for p, _ in lists]
    cap = max(R.packed_total(nts, max_runs), 1) + packed_slack
    ins = _Carve(dev, IN_FILL)
    ins.add("positions", I32, 1, cap); ins.add("nruns", I32, Q, 2); ins.add("cnt", I32, 1, B)
    ins.seal()
    pos = np.full((cap,), -1, np.int32)
    for (p, _), (off, _, _) in zip(lists, R.place(nts, max_runs)):
        k = min(len(p), max_runs)
        pos[off:off + k] = p[:k]
    nr = np.full((Q, 2), -1, np.int32)
    nr[:len(lists)] = [(len(p), lead) for p, lead in lists]
    ins.v["positions"].put(torch.from_numpy(pos)); ins.v["nruns"].put(torch.from_numpy(nr)); ins.v["cnt"].put(torch.tensor([len(lists)], dtype=I32))
    res = []
    for out_cap in out_caps:
        got = _rle_kept(dev, ins.v["positions"], cap, ins.v["nruns"], ins.v["cnt"], B, Q, max_runs, HW, out_cap)
        ins.check()
        res.append(_check_strings(got, lists, list(range(len(lists))), Q, max_runs, HW, cap, out_cap, ("crafted", HW, max_runs, out_cap)))
    return res


def test_string_kernel_on_both_sides_of_every_group_count_edge(dev):
    """A crafted list whose stored values are 15 | 16, -16 | -17 and the pairs at 2^9, 2^14 and 2^19, through the delta rule, behind a
    lead run: the characters are rle._to_string's of the same runs."""
    runs = R.value_edge_runs()
    lists, HW = R.value_edge_case()
    last = R.last_needed(lists, 64)
    exact, below = _crafted(dev, lists, HW, 64, (last, last - 1))
    assert exact[1] == len(R.string_of_runs(runs)) and min(exact) > 0 and below == exact[:2] + [-1]


def test_string_kernel_measures_masks_of_2_to_the_24_pixels_and_more(dev):
    """H*W = 150 994 970: the 17 runs A, A, 1, 1, ... with A = 2^24 + 2 are 97 characters against a slot of 5 nt + 16 = 96 (and 5 nc =
    85): out_len = -1 and not a byte written, with `out` ending at exactly cstart + 5 nc and with room; the neighbours (whose last
    run is a six-character value) are written exactly where they fit.  The 5 runs A, A, 1, 1, A (H*W = 3 A + 2) are 25 characters in
    a slot of 36: written exactly, also with `out` ending at the string's last byte, refused one below."""
    lists, HW = R.big_case(17)
    c = [x[2] for x in R.place([2, 16, 1], 64)]
    assert c == [0, 26, 122]
    tight, roomy = _crafted(dev, lists, HW, 64, (c[1] + 85, 1024), packed_slack=3)
    assert tight == [8, -1, -1] and roomy == [8, -1, 8]
    lists, HW = R.big_case(5)
    c = [x[2] for x in R.place([2, 4, 1], 64)]
    roomy, exact, below = _crafted(dev, lists, HW, 64, (1024, c[1] + 25, c[1] + 24))
    assert roomy == [8, 25, 8] and exact == [8, 25, -1] and below == [8, -1, -1]


# ------------------------------------------------------------------------------------------------ the fused kernel
def _fused(dev, refs, names, orders, H, W, max_runs, out_cap, use_bits, misalign=0):
    from zutis_amd import ops
    assert ops.mask_rle_fused_supported(H, W, max_runs)
    Q, B = len(names), len(orders)
    idx, cnt = R.kept_table(B, Q, orders)
    masks = np.stack([np.stack([refs[k].mask for k in names])] * B)
    n64 = (H * W + 63) // 64
    ins = _inputs(dev, masks, idx, cnt, misalign, bits_words=n64 if use_bits else 0)
    if use_bits:
        md = torch.from_numpy(masks[0]).to(dev)
        inter, uni = (torch.empty((Q, Q), dtype=I32, device=dev) for _ in range(2))
        for b in range(B):
            ops.mask_iou_counts(md, Q, H * W, inter, uni, workspace=ins.v["bits"].t[0, 0][b * Q:(b + 1) * Q])
        torch.cuda.synchronize()
        ins.check()
    out = _Carve(dev, OUT_FILL)
    out.add("out", U8, 1, out_cap); out.add("cursor", I32, 1, 1); out.add("info", I32, B * Q, 8)
    out.seal()
    out.v["cursor"].t.zero_()
    _call("zh_mask_rle_fused_kept", _p(ins.v["masks"]), _p(ins.v["bits"]) if use_bits else None, _p(ins.v["idx"]), _p(ins.v["cnt"]), B, Q, H, W,
          max_runs, _p(out.v["out"]), out_cap, _p(out.v["cursor"]), _p(out.v["info"]))
    out.check(); ins.check()
    return out.np("out")[0], int(out.np("cursor")[0, 0]), out.np("info")


def _check_fused(got, refs, names, orders, max_runs, out_cap, what):
    out_h, cursor, info = got
    Q = len(names)
    want_info = np.full(info.shape, R.FILL32, np.int32)
    want_out = np.full((out_cap,), OUT_FILL, np.uint8)
    attempted, spans, n_refused = 0, [], 0
    for b, o in enumerate(orders):
        for j, q in enumerate(o):
            r, row = refs[names[q]], info[b * Q + j].tolist()
            c0, ln = row[:2]
            if r.nt > max_runs:
                want_info[b * Q + j] = (0, -1) + r.ba + (r.nt,)
                continue
            s = r.string
            attempted += len(s)
            assert 0 <= c0 <= 0x7fffffff - len(s), (what, b, j, row)
            if ln >= 0:
                assert c0 + len(s) <= out_cap, (what, b, j, row)
                want_out[c0:c0 + len(s)] = np.frombuffer(s, np.uint8)
                spans.append((c0, c0 + len(s)))
            else:
                assert c0 + len(s) > out_cap, (what, b, j, row)    # refused only when it does not fit behind its place
                n_refused += 1
            want_info[b * Q + j] = (c0, len(s) if ln >= 0 else -1) + r.ba + (r.nt,)
    _eq(info, want_info, what + ("info",))                          # boxes, areas and counts of refused strings too; slots past the count
    spans.sort()
    assert all(a1 <= b0 for (_, a1), (b0, _) in zip(spans, spans[1:])), (what, "spans overlap")
    _eq(out_h, want_out, what + ("out",))
    assert cursor == attempted, (what, cursor, attempted)
    assert (n_refused == 0) == (out_cap >= attempted), (what, n_refused)
    return attempted


def _fused_shape(dev, H, W, max_runs_list, sources=(False, True), misalign=0, minus1=True):
    refs = _refs(H, W)
    names = [k for k in refs]
    orders = R.kept_orders(len(names), H * 3 + W)
    for max_runs in max_runs_list:
        total = sum(len(refs[names[q]].string) for o in orders for q in o if refs[names[q]].nt <= max_runs)
        for use_bits in sources:
            for out_cap in [max(total, 1)] + ([total - 1] if minus1 and total > 1 else []):
                what = ("fused", H, W, max_runs, out_cap, "bits" if use_bits else "masks", misalign)
                got = _fused(dev, refs, names, orders, H, W, max_runs, out_cap, use_bits, misalign)
                assert _check_fused(got, refs, names, orders, max_runs, out_cap, what) == total


@pytest.mark.parametrize("H,W", R.FUSED_MULTI + R.FUSED_SINGLE)
def test_fused_kernel_with_more_items_than_threads(dev, H, W):
    """1040x1, 520x33, 640x480, 640x427: a thread of the fused kernel owns more than one (32-column, 16-row) item and recomputes the
    later ones in its second pass; 480x640 and 500x375 are the one-item controls.  From the bytes and from the IoU step's bits, at
    max_runs 8192, nt and nt - 1 of the noise mask, `out` at the sum of the strings and one below."""
    items, threads = R.fused_items_threads(H, W)
    assert (items > threads) == ((H, W) in R.FUSED_MULTI)
    _fused_shape(dev, H, W, [8192] + _pivots(_refs(H, W)["noise"].nt)[1:])


@pytest.mark.parametrize("W", R.FUSED_W)
def test_fused_kernel_at_the_item_edges(dev, W):
    """W in {1, 31, 32, 33, 63, 64, 65, 1023, 1024} x H in {1, 15, 16, 17, 33} (one H at the two widest): panels of fewer than 32
    columns, chunks of fewer than 16 rows, H*W % 16 != 0 (the byte-packing fallback); row stripes fill the fifth counter plane."""
    for H in R.FUSED_WIDE_H.get(W, R.FUSED_H):
        _fused_shape(dev, H, W, sorted({8192, *_pivots(_refs(H, W)["noise"].nt)[1:]}))


@pytest.mark.parametrize("H,W", [(16, 64), (640, 480)])
def test_fused_kernel_from_a_misaligned_base(dev, H, W):
    """H*W % 16 == 0 but the masks' base 4 bytes off alignment: the byte loop packs the bits."""
    assert R.fused_packing(H, W) == "vector" and R.fused_packing(H, W, 4) == "bytes"
    _fused_shape(dev, H, W, [8192], sources=(False,), misalign=4)


@pytest.mark.parametrize("H,W,max_runs,branch", [(8, 8, 8192, "string"), (640, 480, 64, "bits")])
def test_fused_kernel_in_both_layout_branches(dev, H, W, max_runs, branch):
    """8x8 at max_runs 8192: the string buffer is larger than bits + counts; 640x480 at 64: the bits and counts are larger."""
    assert R.frle_layout(H, W, max_runs)["branch"] == branch
    _fused_shape(dev, H, W, [max_runs])


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("H,W", [(640, 480), (640, 427)])
def test_portrait_batches_through_nms_encode(dev, H, W):
    """instances.nms_encode on B = 2 portrait batches, fused and chained: the same kept list, and for every kept mask the host
    encoder's string and numpy's box and area."""
    from zutis_amd import instances
    rng = np.random.default_rng(H + W)
    B, Q = 2, 8
    masks = np.zeros((B, Q, H, W), np.uint8)
    for b in range(B):
        for q in range(Q - 3):
            y0, x0 = int(rng.integers(0, H - 60)), int(rng.integers(0, W - 60))
            masks[b, q, y0:y0 + int(rng.integers(20, 300)), x0:x0 + int(rng.integers(20, 200))] = 1
        masks[b, Q - 3] = rng.random((H, W)) < R.noise_density(H, W)
        masks[b, Q - 2, :, ::7] = 1
        masks[b, Q - 1, H - 1, :] = 1
        masks[b, Q - 1, 0, 0] = 1
    scores = (rng.random((B, Q)) * 0.9 + 0.05).astype(np.float32)
    cats = np.tile(np.arange(1, Q + 1, dtype=np.int64), (B, 1))                # distinct categories: every mask is kept
    md, sd, cd = (torch.from_numpy(x).to(dev) for x in (masks, scores, cats))
    res = [instances.nms_encode(md, sd, cd, "hard", fused=fused) for fused in (True, False)]
    assert tuple(res[0]) == tuple(res[1])
    kept, rles, boxes, areas = res[0][:4]
    assert sorted((b, q) for b, _, q, _ in kept) == [(b, q) for b in range(B) for q in range(Q)]
    for (b, _, q, _), r, box, area in zip(kept, rles, boxes, areas):
        x0, y0, x1, y1, a = R.box_area(masks[b, q])
        assert r == {"size": [H, W], "counts": R.string_of_mask(masks[b, q])}, (b, q)
        assert box == [float(x0), float(y0), float(x1), float(y1)] and area == a, (b, q)
