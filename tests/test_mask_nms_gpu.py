"""zh_mask_nms — mask_nms_wave_kernel (Q <= 128: one wave, a Q x Q float64 IoU table in dynamic LDS, a DPP / readlane argmax) and
mask_nms_kernel (Q <= 1024: block-wide, LDS tree reductions) — against tests/_nms_case.py's float64 restatement of the documented
contract, on synthetic count tables (no masks): every Q at which a path or an element position begins or ends, exact score ties at the
positions each argmax step has to break (largest index wins), count pairs and decayed scores either side of the strict `iou > thr` and
`s > score_thr`, degenerate category / mask sets, the packed row, zero_word, guards around the outputs, refusals.

Hard NMS: count, index, category, emission order and scores (np.array_equal) equal nms_ref.  Linear / gaussian: the same lists, scores
within 1e-12 absolute (the bound of test_device_mask_nms_matches_reference_control_flow).  Derivation: a score takes at most Q - 1 <=
256 decay steps in these cases (one multiply per earlier winner of its category; 128 on the one-wave kernel), each a float64 multiply
by a weight that is a correctly rounded divide, then a subtract or a multiply / divide / exp chain — about 3 ulp per step against
numpy's, 256 * 3 * 1.1e-16 = 9e-14 relative on scores <= 1: the bound has a 10-fold margin.  Every test prints the maximum it
measured.  The cases' margins (check_margins: 1e-9 relative between the best
and the runner-up and around score_thr) keep such rounding from changing an order.  Entries past `count` are not asserted.
The preconditions of every case are proved on the host by tests/test_mask_nms_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from tests import _nms_case as N
from tests._guard import OUT_FILL, Arena, assert_untouched

pytestmark = pytest.mark.gpu

Q_SWEEP = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1024)
Q_TYPES = (64, 128, 129, 257)
RANDOM_B, RANDOM_SEED, PERM_SEED = 3, 5, 11
DEGENERATE = ("all_cat0", "all_empty", "empty_winners", "one_category", "distinct_cats", "big_ids", "two_images")
SCORE_ATOL = 1e-12


@functools.lru_cache(maxsize=None)
def _case(kind, Q, arg=None):
    """(case, the keyword arguments it is run with): built once, shared, never written to."""
    if kind == "permutation":
        return N.permutation_case(Q, PERM_SEED), {}
    if kind == "tie":
        return N.tie_case(Q, arg), {}
    if kind == "degenerate":
        return N.degenerate_cases(Q)[arg], {}
    if kind == "threshold":
        return _threshold(Q, arg)[0], {}
    if kind == "equality":
        case, thr, score_thr = N.equality_case(Q)
        return case, dict(nms_threshold=thr, score_threshold=score_thr)
    assert kind == "random"
    return N.random_case(Q, RANDOM_B, RANDOM_SEED), {}


@functools.lru_cache(maxsize=None)
def _threshold(Q, nms_type):
    return N.threshold_case(Q, nms_type)


@functools.lru_cache(maxsize=None)
def _ref(kind, Q, arg, nms_type):
    case, kw = _case(kind, Q, arg)
    return N.nms_ref(case.inter, case.uni, case.scores, case.cats, nms_type, thr=kw.get("nms_threshold", 0.3),
                     score_thr=kw.get("score_threshold", 0.001))


def _launch(dev, case, nms_type, **kw):
    from zutis_amd import ops
    t = lambda a: torch.from_numpy(a).to(dev)
    return ops.mask_nms(t(case.inter), t(case.uni), t(case.scores), t(case.cats), nms_type, **kw)


def _kept(out):
    """Per image the first `count` (index, score, category) of ops.mask_nms' four outputs."""
    idx, sc, cat, cnt = (x.cpu().numpy() for x in out)
    return [list(zip(idx[b, :n].tolist(), sc[b, :n].tolist(), cat[b, :n].tolist())) for b, n in enumerate(cnt.tolist())]


def _compare(got, ref, nms_type, what):
    """count, index, category, order: equal; scores: equal (hard) or within SCORE_ATOL.  Returns the largest score error."""
    worst = 0.0
    assert len(got) == len(ref)
    for b, (g, r) in enumerate(zip(got, ref)):
        assert len(g) == len(r), (what, b, "count", len(g), len(r))
        assert [(q, c) for q, _, c in g] == [(q, c) for q, _, c in r], (what, b)
        gs, rs = np.array([s for _, s, _ in g], np.float64), np.array([s for _, s, _ in r], np.float64)
        if nms_type == "hard":
            assert np.array_equal(gs, rs), (what, b)
        elif len(g):
            worst = max(worst, float(np.abs(gs - rs).max()))
    print(f"{what} [{nms_type}]: max |score - ref| = {worst:.3e}")
    assert worst <= SCORE_ATOL, (what, worst)
    return worst


def _check(dev, kind, Q, arg, nms_type):
    case, kw = _case(kind, Q, arg)
    got = _kept(_launch(dev, case, nms_type, **kw))
    _compare(got, _ref(kind, Q, arg, nms_type), nms_type, case.name)
    return got


# ------------------------------------------------------------------------------------------------ the Q sweep, hard NMS
@pytest.mark.parametrize("Q", Q_SWEEP)
def test_permutation_every_position_wins_once(dev, Q):
    got = _check(dev, "permutation", Q, None, "hard")
    assert all(sorted(q for q, _, _ in g) == list(range(Q)) for g in got)


@pytest.mark.parametrize("Q,pattern", [(Q, p) for Q in Q_SWEEP for p in N.tie_patterns(Q)])
def test_ties_resolve_to_the_largest_index(dev, Q, pattern):
    got = _check(dev, "tie", Q, pattern, "hard")
    case, _ = _case("tie", Q, pattern)
    assert [q for q, _, _ in got[0]] == sorted(range(Q), key=lambda q: (-float(case.scores[0, q]), -q))


@pytest.mark.parametrize("name", DEGENERATE)
@pytest.mark.parametrize("Q", Q_SWEEP)
def test_degenerate_inputs(dev, Q, name):
    got = _check(dev, "degenerate", Q, name, "hard")
    if name in ("all_cat0", "all_empty"):
        assert got == [[]]
    if name == "distinct_cats":
        assert len(got[0]) == Q


# ------------------------------------------------------------------------------------------------ the three types
@pytest.mark.parametrize("nms_type", N.NMS_TYPES)
@pytest.mark.parametrize("Q", Q_TYPES)
def test_threshold_edges(dev, Q, nms_type):
    """(30000, 100000) is below 0.3 only in float64; decayed scores land 2e-6 relative either side of score_thr."""
    got = _check(dev, "threshold", Q, nms_type, nms_type)
    expect = _threshold(Q, nms_type)[1]
    emitted = {q for q, _, _ in got[0]}
    assert {q: q in emitted for q in expect} == expect


@pytest.mark.parametrize("nms_type", N.NMS_TYPES)
@pytest.mark.parametrize("Q", (64, 129))
def test_comparisons_are_strict_at_equality(dev, Q, nms_type):
    """iou == thr: not suppressed, not decayed; a score == score_thr that is not the best: dropped."""
    got = _check(dev, "equality", Q, None, nms_type)
    emitted = {q for q, _, _ in got[0]}
    assert 2 not in emitted and 5 in emitted and Q // 2 in emitted


@pytest.mark.parametrize("nms_type", N.NMS_TYPES)
@pytest.mark.parametrize("Q", Q_TYPES)
def test_random_rectangles(dev, Q, nms_type):
    got = _check(dev, "random", Q, None, nms_type)
    assert all(len(g) > 10 for g in got)


@pytest.mark.parametrize("nms_type", ("linear", "gaussian"))
@pytest.mark.parametrize("Q", Q_TYPES)
def test_ties_that_survive_a_decay(dev, Q, nms_type):
    """Tied candidates with identical IoU rows against every earlier winner stay bit-equal through the decays: largest index first."""
    got = _check(dev, "tie", Q, "decay", nms_type)
    case, _ = _case("tie", Q, "decay")
    at = {q: i for i, (q, _, _) in enumerate(got[0])}
    for g in case.ties[0]:
        assert sorted(g, key=lambda q: at[q]) == sorted(g, reverse=True)
        if nms_type == "linear":
            assert len({got[0][at[q]][1] for q in g}) == 1


# ------------------------------------------------------------------------------------------------ outputs
def _raw(dev, case, nms_type_code, views, packed=None, range_flag=None, zero_word=None):
    """zh_mask_nms itself, writing into caller-placed outputs (ops.mask_nms allocates its own)."""
    from zutis_amd import ops
    t = lambda a: torch.from_numpy(a).to(dev)
    ins = [t(case.inter), t(case.uni), t(case.scores), t(case.cats)]
    B, Q = case.scores.shape
    p = lambda v: None if v is None else ops._p(v.t)
    ops._call("zh_mask_nms", *[ops._p(x) for x in ins], B, Q, nms_type_code, 0.3, 0.5, 0.001, *[p(v) for v in views], p(packed),
              None if range_flag is None else ops._p(range_flag), p(zero_word), ops._stream())
    torch.cuda.synchronize()


def _arena(dev, B, Q):
    a = Arena(OUT_FILL, dev)
    views = [a.add("index", torch.int32, B, Q, tail_rows=4), a.add("score", torch.float64, B, Q, tail_rows=4),
             a.add("category", torch.int64, B, Q, tail_rows=4), a.add("count", torch.int32, 1, B, tail_rows=4)]
    packed = a.add("packed", torch.float64, B, 4 * Q + 2, tail_rows=4)
    word = a.add("zero_word", torch.int32, 1, 1, tail_rows=4)
    return a, views, packed, word


@pytest.mark.parametrize("with_packed", (False, True))
@pytest.mark.parametrize("Q", (1, 65, 128, 129, 1024))
def test_outputs_stay_inside_their_guards(dev, Q, with_packed):
    """The four outputs (and the packed row and zero_word) carved out of a 0xA5 arena: count / index / score / category equal nms_ref, and
    not a byte outside the logical [B, Q] / [B] / [B, 4Q + 2] / [1] elements is written."""
    case, _ = _case("degenerate", Q, "two_images")
    arena, views, packed, word = _arena(dev, 2, Q)
    _raw(dev, case, 0, views, packed if with_packed else None, None, word)
    used = views + [word] + ([packed] if with_packed else [])
    assert_untouched(arena, used)
    idx, sc, cat, cnt = (v.get()[0, 0] for v in views)
    got = _kept((idx, sc, cat, cnt[0]))
    _compare(got, _ref("degenerate", Q, "two_images", "hard"), "hard", case.name)
    assert int(word.get().item()) == 0


@pytest.mark.parametrize("nms_type", N.NMS_TYPES)
@pytest.mark.parametrize("Q", (65, 128, 129))
def test_packed_row_layout(dev, Q, nms_type):
    """packed f64 [B, 4Q + 2] = [index, -1 past the count | score, 0 past | category, 0 past | every query's category | count, *range_flag]:
    every slot, for range_flag 0, 1 and NULL; the unpacked outputs do not depend on `packed`."""
    case, _ = _case("random", Q, None)
    ref = _ref("random", Q, None, nms_type)
    B = RANDOM_B
    plain = _launch(dev, case, nms_type)
    _compare(_kept(plain), ref, nms_type, case.name)
    for flag in (0, 1, None):
        pk = torch.full((B, 4 * Q + 2), -7.0, dtype=torch.float64, device=dev)
        rf = None if flag is None else torch.full((1,), flag, dtype=torch.int32, device=dev)
        out = _launch(dev, case, nms_type, packed=pk, range_flag=rf)
        got = _kept(out)
        assert got == _kept(plain), flag                                                           # bitwise: same kernel, same inputs
        row = pk.cpu().numpy()
        for b in range(B):
            n = len(got[b])
            want = np.concatenate([[q for q, _, _ in got[b]], np.full(Q - n, -1.0), [s for _, s, _ in got[b]], np.zeros(Q - n),
                                   [c for _, _, c in got[b]], np.zeros(Q - n), case.cats[b].astype(np.float64), [n, flag or 0]])
            assert np.array_equal(row[b], want), (flag, b, np.flatnonzero(row[b] != want)[:8])


@pytest.mark.parametrize("Q", (64, 129))
def test_zero_word_is_cleared(dev, Q):
    case, _ = _case("degenerate", Q, "two_images")
    word = torch.full((3,), 77, dtype=torch.int32, device=dev)
    _launch(dev, case, "hard", zero_word=word[1:2])
    assert word.tolist() == [77, 0, 77]
    _launch(dev, case, "hard")                                                                     # NULL: nothing to clear, no fault
    torch.cuda.synchronize()


@pytest.mark.parametrize("Q", (128, 1024))
def test_two_runs_are_bitwise_equal(dev, Q):
    case, _ = _case("permutation", Q, None)
    a, b = _launch(dev, case, "hard"), _launch(dev, case, "hard")
    assert int(a[3].min()) == Q                                                                     # count == Q: every entry is defined
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_refusals_launch_nothing(dev):
    """Q = 1025 and an nms_type outside {hard, linear, gaussian} are refused by the binding; no output byte is written."""
    from zutis_amd import _lib
    big = N._case("refused", np.zeros((1025, 1025)), np.zeros((1025, 1025)), np.full(1025, 0.5, np.float32), np.ones(1025, np.int64))
    pk = torch.full((1, 4 * 1025 + 2), -7.0, dtype=torch.float64, device=dev)
    word = torch.full((1,), 77, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.ZutisHipError, match="0 < Q <= 1024"):
        _launch(dev, big, "hard", packed=pk, zero_word=word)
    small, _ = _case("degenerate", 64, "two_images")
    with pytest.raises(AssertionError):
        _launch(dev, small, "cosine", zero_word=word)
    torch.cuda.synchronize()
    assert word.item() == 77 and bool((pk == -7.0).all())
    for case, code, msg in ((big, 0, "0 < Q <= 1024"), (small, 3, "nms_type 3"), (small, -1, "nms_type -1")):
        B, Q = case.scores.shape
        arena, views, packed, zw = _arena(dev, B, Q)
        with pytest.raises(_lib.ZutisHipError, match=msg):
            _raw(dev, case, code, views, packed, None, zw)
        torch.cuda.synchronize()
        assert_untouched(arena, [])


# ------------------------------------------------------------------------------------------------ consumers at a full kept list
def test_consumers_at_a_full_kept_list(dev):
    """B = 2, Q = 12, 48 x 64, disjoint masks in 12 distinct categories: every query is kept (count == Q in both images), so the run, RLE
    and string kernels behind the loop see a full kept_count.  nms_encode, fused and chained, gives instances.nms' kept list, rle.encode's
    strings and numpy's boxes and areas."""
    from zutis_amd import instances, rle
    rng = np.random.default_rng(12)
    B, Q, H, W = 2, 12, 48, 64
    masks = np.zeros((B, Q, H, W), np.uint8)
    for b in range(B):
        for q in range(Q):                                                                         # one 16 x 16 cell each: disjoint
            cy, cx = 16 * (q // 4), 16 * (q % 4)
            y0, x0 = cy + rng.integers(0, 6), cx + rng.integers(0, 6)
            masks[b, q, y0:y0 + rng.integers(1, 11), x0:x0 + rng.integers(1, 11)] = 1
    masks[0, 3, :16, 48:] = 1                                                                      # a whole cell, up to the image's corner
    masks[1, 11, 32:, 48:] = 1
    masks[1, 5, 20, 20] ^= 1                                                                       # more than one run per column
    assert masks.reshape(B, Q, -1).any(-1).all() and masks.sum(1).max() == 1
    scores = N._levels(B * Q)[rng.permutation(B * Q)].reshape(B, Q)
    cats = np.stack([1 + rng.permutation(Q) for _ in range(B)]).astype(np.int64)
    md, sd, cd = (torch.from_numpy(x).to(dev) for x in (masks, scores, cats))
    kept = instances.nms(md, sd, cd, "hard")
    want = [(b, int(cats[b, q]), int(q), float(scores[b, q])) for b in range(B) for q in np.argsort(cats[b])]
    assert kept == want and len(kept) == B * Q
    inter, uni = N.counts_from_masks(masks)
    ref = N.nms_ref(inter, uni, scores, cats, "hard")
    assert [(b, c, q, s) for b in range(B) for q, s, c in ref[b]] == kept
    for fused in (True, False):
        r = instances.nms_encode(md, sd, cd, "hard", fused=fused)
        assert r.kept == kept, fused
        for j, (b, _, q, _) in enumerate(kept):
            m = masks[b, q]
            ys, xs = np.nonzero(m)
            assert r.rles[j] == rle.encode(m), (fused, b, q)
            assert r.boxes[j] == [float(xs.min()), float(ys.min()), float(xs.max()), float(ys.max())], (fused, b, q)
            assert r.areas[j] == int(m.sum()), (fused, b, q)
