"""The device mask NMS tests' reference and case builders (tests/_nms_case.py), proved on the host: nms_ref against the oracle on tie-free
inputs, against hand vectors, and every builder's preconditions at every Q and seed tests/test_mask_nms_gpu.py uses."""
import numpy as np
import pytest

from tests import _nms_case as N
from oracle import zutis_ref as O

Q_SWEEP = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1024)
Q_TYPES = (64, 128, 129, 257)
RANDOM_B, RANDOM_SEED, PERM_SEED = 3, 5, 11


# ------------------------------------------------------------------------------------------------ hand vectors, Q = 3
# masks 0 and 1 share 5 pixels of 10 (union 10: IoU = 5 / (10 + 1e-7) = 0.499999995), mask 2 is disjoint from both
HAND_INTER = [[10, 5, 0], [5, 10, 0], [0, 0, 10]]
HAND_UNI = [[10, 10, 20], [10, 10, 20], [20, 20, 10]]


def _hand(scores, nms_type, cats=(1, 1, 1)):
    return N.nms_ref(HAND_INTER, HAND_UNI, np.array(scores, np.float32), np.array(cats, np.int64), nms_type)[0]


def test_hand_vectors_hard():
    assert _hand([0.75, 0.5, 0.25], "hard") == [(0, 0.75, 1), (2, 0.25, 1)]                       # 1 suppressed by 0
    # a tie: 2 is the largest index among the three maxima; then 1 among {0, 1}; 0 is suppressed by 1
    assert _hand([0.5, 0.5, 0.5], "hard") == [(2, 0.5, 1), (1, 0.5, 1)]
    # categories ascending, 0 skipped, whatever the scores: query 1 (category 5) after query 2 (category 3)
    assert _hand([0.75, 0.5, 0.25], "hard", cats=(0, 5, 3)) == [(2, 0.25, 3), (1, 0.5, 5)]
    # the best of a category is emitted below score_thr; the runner-up below it is dropped in the first round
    assert _hand([0.0005, 0.75, 0.0003], "hard", cats=(2, 1, 2)) == [(1, 0.75, 1), (0, float(np.float32(0.0005)), 2)]


def test_hand_vectors_linear_and_gaussian():
    # linear: 1 decays to 0.5 * (1 - 0.499999995) = 0.2500000025, which the 1e-7 in the denominator puts ABOVE query 2's 0.25
    got = _hand([0.75, 0.5, 0.25], "linear")
    assert [(q, c) for q, _, c in got] == [(0, 1), (1, 1), (2, 1)]
    assert got[0][1] == 0.75 and got[2][1] == 0.25 and abs(got[1][1] - 0.2500000025) < 1e-15
    # gaussian: 0.5 * exp(-0.499999995^2 / 0.5) = 0.5 * exp(-0.49999999) = 0.5 * 0.606530665778 > 0.25
    got = _hand([0.75, 0.5, 0.25], "gaussian")
    assert [(q, c) for q, _, c in got] == [(0, 1), (1, 1), (2, 1)]
    assert got[0][1] == 0.75 and got[2][1] == 0.25 and abs(got[1][1] - 0.303265332889) < 1e-12
    # gaussian with a score that the decay takes below score_thr: 0.0015 * 0.6065 = 0.00091, dropped
    assert _hand([0.75, 0.0015, 0.25], "gaussian") == [(0, 0.75, 1), (2, 0.25, 1)]
    assert _hand([0.75, 0.0015, 0.25], "hard") == [(0, 0.75, 1), (2, 0.25, 1)]


def test_argsort_cannot_judge_ties():
    """Why the reference does not lean on np.argsort's default kind: the stable kind takes the last of the equal maxima, the default
    kind is free to take another (and does on some NumPy builds) — nms_ref takes the largest index by construction."""
    s = np.array([.5, .5, .2, .5] + [.1] * 40, np.float32)
    assert np.argsort(s, kind="stable")[-1] == 3
    assert np.argsort(s)[-1] in (0, 1, 3)
    inter, uni = N._tables(np.full(44, 10))
    assert [q for q, _, _ in N.nms_ref(inter, uni, s, np.ones(44, np.int64), "hard")[0][:3]] == [3, 1, 0]


# ------------------------------------------------------------------------------------------------ nms_ref == the oracle, tie-free
@pytest.mark.parametrize("Q", Q_TYPES)
def test_ref_equals_oracle_on_random_masks(Q):
    case = N.random_case(Q, RANDOM_B, RANDOM_SEED)
    inter, uni = N.counts_from_masks(case.masks)
    assert np.array_equal(inter, case.inter) and np.array_equal(uni, case.uni)
    b, q, p = 1, 10, 40
    assert inter[b, q, p] == (case.masks[b, q] & case.masks[b, p]).sum() and uni[b, q, p] == (case.masks[b, q] | case.masks[b, p]).sum()
    for nms_type in N.NMS_TYPES:
        ref = N.nms_ref(case.inter, case.uni, case.scores, case.cats, nms_type)
        for b in range(RANDOM_B):
            orc = O.mask_nms(case.masks[b], case.scores[b], case.cats[b], nms_type)
            orc = sorted(orc, key=lambda t: t[0])                     # stable: categories ascending, selection order inside
            assert [(q, c) for q, _, c in ref[b]] == [(q, c) for c, q, _ in orc], (nms_type, b)
            rs, os_ = np.array([s for _, s, _ in ref[b]]), np.array([s for _, _, s in orc])
            if nms_type == "hard":
                assert np.array_equal(rs, os_)
            else:
                assert np.abs(rs - os_).max() < 1e-12
            assert len(orc) > 10


# ------------------------------------------------------------------------------------------------ the builders' preconditions
@pytest.mark.parametrize("Q", Q_SWEEP)
def test_permutation_case_visits_every_position_once(Q):
    case = N.permutation_case(Q, PERM_SEED)
    ref = N.nms_ref(case.inter, case.uni, case.scores, case.cats, "hard")
    for b in range(2):
        order = [q for q, _, _ in ref[b]]
        assert sorted(order) == list(range(Q))
        assert order == np.argsort(-case.scores[b].astype(np.float64), kind="stable").tolist()     # distinct scores: descending
        assert [s for _, s, _ in ref[b]] == [float(case.scores[b, q]) for q in order]
    assert Q < 3 or not np.array_equal(case.scores[0], case.scores[1])


@pytest.mark.parametrize("Q", Q_SWEEP)
def test_tie_cases_tie_bit_equal_and_resolve_to_the_largest_index(Q):
    pats = N.tie_patterns(Q)
    assert "all_equal" in pats
    if Q >= 63:
        assert {"quad", "half_row", "row", "rows"} <= set(pats)
    assert ("lane64" in pats) == (Q > 64) and ("stride256" in pats) == (Q > 256)
    for p in pats:
        case = N.tie_case(Q, p)
        groups = case.ties[0]
        assert Q == 1 or groups
        bits = case.scores[0].view(np.uint32)
        for g in groups:
            assert len(set(bits[g].tolist())) == 1
        gid = {q: i for i, g in enumerate(groups) for q in g}
        tied_levels = [int(bits[g[0]]) for g in groups]
        assert len(set(tied_levels)) == len(groups)
        assert all(int(bits[q]) not in tied_levels for q in range(Q) if q not in gid)               # nobody else shares a group's level
        order = [q for q, _, _ in N.nms_ref(case.inter, case.uni, case.scores, case.cats, "hard")[0]]
        assert order == sorted(range(Q), key=lambda q: (-float(case.scores[0, q]), -q))
    if Q == 129:
        assert [q for q, _, _ in N.nms_ref(*N.tie_case(Q, "all_equal")[1:5], "hard")[0]] == list(range(Q - 1, -1, -1))


@pytest.mark.parametrize("Q", Q_TYPES)
def test_decay_tie_case_stays_tied_through_the_decay(Q):
    case = N.tie_case(Q, "decay")                                                                # asserts the margins itself
    W, groups = Q // 2, case.ties[0]
    assert len(groups) >= 3 and (Q <= 64 or any(max(g) - min(g) == 64 for g in groups)) and (Q <= 256 or any(max(g) >= 256 for g in groups))
    for nms_type in ("linear", "gaussian"):
        ref = N.nms_ref(case.inter, case.uni, case.scores, case.cats, nms_type)[0]
        assert ref[0][0] == W and len(ref) == Q
        at = {q: i for i, (q, _, _) in enumerate(ref)}
        for g in groups:                                                                           # index-descending
            assert sorted(g, key=lambda q: at[q]) == sorted(g, reverse=True)
            if nms_type == "linear":                                                               # decayed once, by W only: consecutive
                assert [ref[at[max(g)] + i][0] for i in range(len(g))] == sorted(g, reverse=True)
                assert {ref[at[q]][1] for q in g} == {float(case.scores[0, g[0]]) * (1.0 - 4 / (10 + 1e-7))}
            else:                                                                                  # and once more by each earlier member
                assert all(ref[at[q]][1] < float(case.scores[0, q]) * 0.73 for q in g)
                assert len({ref[at[q]][1] for q in g}) == len(g)
        worst = N.check_margins(case, nms_type)
        assert min(worst) > N.MARGIN


@pytest.mark.parametrize("nms_type", N.NMS_TYPES)
@pytest.mark.parametrize("Q", Q_TYPES)
def test_threshold_case_lands_on_the_intended_sides(Q, nms_type):
    # the count pairs either side of thr in float64, and (30000, 100000) on the other side once rounded to float32
    iou = [i / (u + 1e-7) for i, u in N.THRESHOLD_PAIRS]
    assert [x > 0.3 for x in iou] == [False, False, True, True, True]
    assert abs(iou[1] - 0.2999999999997) < 1e-15 and float(np.float32(iou[1])) > 0.3 and float(np.float32(iou[0])) < 0.3
    case, expect = N.threshold_case(Q, nms_type)                                                   # asserts sides and margins itself
    assert not (case.scores == N.F32_SCORE_THR).any()
    ref = N.nms_ref(case.inter, case.uni, case.scores, case.cats, nms_type)[0]
    emitted = {q: s for q, s, _ in ref}
    assert {q: q in emitted for q in expect} == expect
    assert sorted(expect.values()).count(True) >= {"hard": 4, "linear": 6, "gaussian": 7}[nms_type]
    assert sorted(expect.values()).count(False) >= 4
    near = [s for q, s in emitted.items() if case.cats[0, q] == 1 and s < 0.01]
    assert near and all(0.001 < s < 0.001 * (1 + 2e-5) for s in near)                              # survivors just above score_thr
    low = [(q, s) for q, s, c in ref if c in (2, 3)]
    assert [s for _, s in low] == [float(np.float32(0.0005)), float(np.float32(0.0002))]          # emitted below score_thr: the best


@pytest.mark.parametrize("Q", (64, 129))
def test_equality_case_sits_exactly_on_both_thresholds(Q):
    case, thr, score_thr = N.equality_case(Q)
    a, b = Q - 1, Q // 2
    assert case.inter[0, b, a] / (case.uni[0, b, a] + 1e-7) == thr and float(case.scores[0, 2]) == score_thr
    for nms_type in N.NMS_TYPES:
        ref = N.nms_ref(case.inter, case.uni, case.scores, case.cats, nms_type, thr=thr, score_thr=score_thr)[0]
        emitted = {q: s for q, s, _ in ref}
        assert 2 not in emitted and 5 in emitted and len(ref) == Q - 1
        if nms_type != "gaussian":
            assert emitted[b] == float(case.scores[0, b])                                          # iou == thr: not decayed
        # one ulp lower and the pair is suppressed / decayed: the case does sit on the edge
        lower = N.nms_ref(case.inter, case.uni, case.scores, case.cats, nms_type, thr=np.nextafter(thr, 0), score_thr=score_thr)[0]
        assert nms_type == "gaussian" or dict((q, s) for q, s, _ in lower).get(b) != emitted[b]


@pytest.mark.parametrize("Q", Q_SWEEP)
def test_degenerate_cases_are_what_they_say(Q):
    cases = N.degenerate_cases(Q)
    ref = {k: N.nms_ref(c.inter, c.uni, c.scores, c.cats, "hard") for k, c in cases.items()}
    assert ref["all_cat0"] == [[]] and ref["all_empty"] == [[]]
    assert set(cases["all_empty"].cats[0].tolist()) == ({1, 2} if Q > 1 else {1})
    ew = [q for q, _, _ in ref["empty_winners"][0]]
    assert ew == [q for q in range(Q) if q % 3 == 2]                                               # 3j empty, 3j + 1 suppressed by it
    oc = [q for q, _, _ in ref["one_category"][0]]
    assert len(oc) >= (Q + 2) // 3 and (Q == 1 or len(oc) < Q) and all(abs(p - q) > 1 for p in oc for q in oc if p != q)
    dc = ref["distinct_cats"][0]
    assert len(dc) == Q and [c for _, _, c in dc] == list(range(1, Q + 1))
    ids = sorted({i for i in N.BIG_IDS[:Q] if i > 0})
    assert [c for _, _, c in ref["big_ids"][0]] == ids                                             # one survivor per id, ascending
    for q, s, c in ref["big_ids"][0]:
        same = np.flatnonzero(cases["big_ids"].cats[0] == c)
        assert s == float(cases["big_ids"].scores[0, same].max())
    ti = ref["two_images"]
    assert len(ti[0]) == Q and (Q == 1 or len(ti[1]) < Q)


@pytest.mark.parametrize("Q", Q_TYPES)
def test_random_case_is_tie_free_and_inside_the_margins(Q):
    case = N.random_case(Q, RANDOM_B, RANDOM_SEED)                                                 # asserts both itself
    for nms_type in ("linear", "gaussian"):
        assert min(N.check_margins(case, nms_type)) > N.MARGIN
    ref = N.nms_ref(case.inter, case.uni, case.scores, case.cats, "hard")
    assert all(10 < len(r) < Q for r in ref)
    assert not any(q % 17 == 3 for r in ref for q, _, _ in r)                                      # empty masks are never emitted
