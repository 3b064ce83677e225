"""Reference and case builders for the device mask NMS (zh_mask_nms: mask_nms_wave_kernel for Q <= 128, mask_nms_kernel up to 1024).
Host only: numpy, no torch, no GPU — tests/test_mask_nms_cpu.py proves every builder's preconditions, tests/test_mask_nms_gpu.py runs
the kernels on the same cases.

nms_ref restates the kernel's DOCUMENTED contract (the block comment above mask_nms_kernel) over the integer Q x Q intersection / union
counts in float64; it is not a copy of oracle.zutis_ref.mask_nms, which works on masks, walks the categories in set order and leaves
exact ties to np.argsort (on NumPy 2.2.6 argsort's default kind puts index 1 last for [.5, .5, .2, .5, .1 x 40], a stable sort puts 3):
the oracle cannot judge ties, the contract can — among equal maxima the LARGEST query index wins.

A case is a Case tuple of batched arrays (inter / uni int32 [B,Q,Q], scores float32 [B,Q], cats int64 [B,Q]) plus `ties`, per image the
groups of query indices whose scores are bit-equal by construction, and `masks` where the counts came from masks.  Builders assert
their own preconditions.  For linear and gaussian NMS (device exp / multiply may differ from numpy's by an ulp) a case must pass
check_margins: at every selection step the best active score is either bit-equal to the runner-up (a constructed tie whose members
share identical IoU rows against every earlier winner, so both sides keep them bit-equal) or ahead of it by more than 1e-9 relative,
and every decayed score is more than 1e-9 relative away from score_thr — rounding (about 1e-14 after the longest chain of decays)
cannot then legitimately change an order or a keep / drop decision.

float32(0.001) is excluded from every case.  It is 0.0010000000475 as a double, so the kernel, which carries float64 scores and
compares `s > score_thr` in double, KEEPS such a candidate.  The oracle's `s > threshold` on a float32 score drops it under NumPy 2
promotion (the Python float is weak: both sides become float32(0.001)) and keeps it under NumPy 1 (value-based: float64); neither the
oracle nor the code it restates pins a NumPy version, so there is no single reference answer for that one value.

Out of scope, nothing asserted: negative category ids and NaN or negative scores.  The oracle would process them, the kernel never
selects them (ids <= 0 are skipped, the argmax starts from -1.0); they are outside the model's output range (sigmoid products,
argmax ids) and range_flag guards the proposals.
"""
import collections

import numpy as np

NMS_TYPES = ("hard", "linear", "gaussian")
MARGIN = 1e-9
F32_SCORE_THR = np.float32(0.001)

Case = collections.namedtuple("Case", "name inter uni scores cats ties masks")


# ------------------------------------------------------------------------------------------------ reference
def _image(inter, uni, scores, cats, nms_type, thr, sigma, score_thr, on_step=None):
    assert nms_type in NMS_TYPES
    inter, uni = np.asarray(inter, np.int64), np.asarray(uni, np.int64)
    iou = inter.astype(np.float64) / (uni.astype(np.float64) + 1e-7)
    s0 = np.asarray(scores).astype(np.float64)                      # the float32 scores, promoted
    cats = np.asarray(cats, np.int64)
    out = []
    for c in sorted({int(x) for x in cats if x > 0}):               # ascending, ids <= 0 skipped
        act, s = cats == c, s0.copy()
        while act.any():
            live = np.flatnonzero(act)
            m = s[live].max()
            best = int(live[s[live] == m].max())                    # equal maxima: the largest index
            if on_step is not None:
                on_step("select", live, s[live], m)
            act[best] = False
            if inter[best, best] > 0:                               # an empty mask is selected (and decays the others) but not emitted
                out.append((best, float(m), c))
            rest = np.flatnonzero(act)
            x = iou[rest, best]
            if nms_type == "hard":
                w = np.where(x > thr, 0.0, 1.0)
            elif nms_type == "linear":
                w = np.where(x > thr, 1.0 - x, 1.0)
            else:
                w = np.exp(-(x * x) / sigma)
            s[rest] = s[rest] * w
            if on_step is not None:
                on_step("decay", rest, s[rest], score_thr)
            act[rest] = s[rest] > score_thr                         # dropped when not (s > score_thr)
    return out


def nms_ref(inter, uni, scores, cats, nms_type, thr=0.3, sigma=0.5, score_thr=0.001):
    """Per image the list of (index, score, category) in emission order.  inter / uni [B,Q,Q] (or [Q,Q]: one image) integer counts,
    scores [B,Q] float32, cats [B,Q] int64."""
    inter, uni, scores, cats = np.asarray(inter), np.asarray(uni), np.asarray(scores), np.asarray(cats)
    if inter.ndim == 2:
        inter, uni, scores, cats = inter[None], uni[None], scores[None], cats[None]
    return [_image(inter[b], uni[b], scores[b], cats[b], nms_type, thr, sigma, score_thr) for b in range(len(scores))]


def check_margins(case, nms_type, thr=0.3, sigma=0.5, score_thr=0.001):
    """The precondition on linear / gaussian cases (module docstring).  Returns (smallest relative gap best - runner-up, smallest
    relative distance of a decayed score from score_thr) over all images and steps."""
    worst = [np.inf, np.inf]
    for b in range(len(case.scores)):
        groups = [set(g) for g in case.ties[b]]

        def on_step(kind, index, s, ref):
            if kind == "select":
                tied = index[s == ref]
                if len(tied) > 1:
                    assert any(set(tied.tolist()) <= g for g in groups), (case.name, nms_type, b, "an unconstructed tie", tied.tolist())
                lower = s[s < ref]
                if lower.size:
                    gap = (ref - lower.max()) / ref
                    assert gap > MARGIN, (case.name, nms_type, b, "best and runner-up too close", float(ref), float(lower.max()))
                    worst[0] = min(worst[0], gap)
            elif s.size:
                gap = np.abs(s - ref).min() / ref
                assert gap > MARGIN, (case.name, nms_type, b, "a decayed score too close to score_thr", float(s[np.abs(s - ref).argmin()]))
                worst[1] = min(worst[1], gap)

        _image(case.inter[b], case.uni[b], case.scores[b], case.cats[b], nms_type, thr, sigma, score_thr, on_step)
    return tuple(worst)


def counts_from_masks(masks):
    """Exact intersection / union counts int64 [..., Q, Q] of boolean masks [..., Q, H, W]."""
    m = np.asarray(masks).astype(bool)
    flat = m.reshape(m.shape[:-2] + (-1,)).astype(np.float64)        # 0 / 1 sums below 2^53: exact in float64 (BLAS)
    inter = np.rint(flat @ np.swapaxes(flat, -1, -2)).astype(np.int64)
    area = m.sum(axis=(-2, -1)).astype(np.int64)
    assert (np.diagonal(inter, axis1=-2, axis2=-1) == area).all()
    return inter, area[..., :, None] + area[..., None, :] - inter


# ------------------------------------------------------------------------------------------------ pieces
def _tables(area, pairs=()):
    """inter / uni int64 [Q,Q] of masks with the given pixel counts that are pairwise disjoint except for `pairs`: (a, b, n) share n."""
    area = np.asarray(area, np.int64)
    inter = np.diag(area).copy()
    for a, b, n in pairs:
        assert a != b and 0 <= n <= min(area[a], area[b]) and inter[a, b] == 0
        inter[a, b] = inter[b, a] = n
    return inter, area[:, None] + area[None, :] - inter


def _levels(n):
    """n distinct float32 scores in (0.05, 0.95), ascending: 9e-4 apart at n = 1024, all far above score_thr."""
    v = (0.05 + 0.9 * (np.arange(n) + 1) / (n + 1)).astype(np.float32)
    assert len(np.unique(v)) == n and v.min() > 0.05 and v.max() < 0.95
    return v


def _case(name, inter, uni, scores, cats, ties=None, masks=None):
    inter, uni, scores, cats = np.asarray(inter), np.asarray(uni), np.asarray(scores), np.asarray(cats)
    if scores.ndim == 1:
        inter, uni, scores, cats = inter[None], uni[None], scores[None], cats[None]
    B, Q = scores.shape
    assert inter.shape == uni.shape == (B, Q, Q) and cats.shape == (B, Q) and scores.dtype == np.float32
    assert inter.min() >= 0 and uni.max() < 2 ** 31 and (inter <= uni).all()
    assert (inter == np.swapaxes(inter, 1, 2)).all() and (uni == np.swapaxes(uni, 1, 2)).all()
    assert not (scores == F32_SCORE_THR).any() and np.isfinite(scores).all() and (scores >= 0).all()
    ties = [[] for _ in range(B)] if ties is None else ties
    for b in range(B):
        for g in ties[b]:
            assert len(g) > 1 and len(set(scores[b, g].view(np.uint32).tolist())) == 1 and len(set(cats[b, g].tolist())) == 1
    return Case(name, np.ascontiguousarray(inter, np.int32), np.ascontiguousarray(uni, np.int32), np.ascontiguousarray(scores),
                np.ascontiguousarray(cats, np.int64), ties, masks)


# ------------------------------------------------------------------------------------------------ cases
def permutation_case(Q, seed):
    """Two images, one category, disjoint masks (IoU 0 off the diagonal), Q distinct scores in a random permutation: everything is
    emitted, score-descending, so every query index — every lane, both of a lane's elements, every strided element of a thread — is
    the winner of exactly one selection step."""
    rng = np.random.default_rng(seed)
    inter, uni = _tables(np.full(Q, 10))
    off = ~np.eye(Q, dtype=bool)
    assert (inter[off] == 0).all() and (uni[off] == 20).all()
    scores = np.stack([_levels(Q)[rng.permutation(Q)] for _ in range(2)])
    return _case(f"permutation-{Q}-{seed}", np.stack([inter] * 2), np.stack([uni] * 2), scores, np.full((2, Q), 3))


TIE_PATTERNS = ("quad", "half_row", "row", "rows", "lane64", "stride256", "all_equal")


def _tie_groups(Q, pattern):
    """Index groups for tie_case, named after the step of the argmax that has to break them (one-wave kernel: query q sits on lane
    q % 64 as element q // 64; block kernel: on thread q % 256 as its q // 256-th strided element).  Members >= Q are dropped."""
    if pattern == "quad":                 # quad_perm xor 1, xor 2, a whole quad; on rows 0 and 2, a lane's second element, a strided one
        g = [[b + i for i in grp] for b in (0, 32, 80, 304, 512) for grp in ((0, 1), (2, 3), (4, 6), (5, 7), (8, 9, 10, 11))]
    elif pattern == "half_row":           # lane i and 7 - i of a half-row
        g = [[b + i, b + 7 - i] for b in (0, 8, 40, 88, 264) for i in range(4)]
    elif pattern == "row":                # lane i and 15 - i of a row
        g = [[b + i, b + 15 - i] for b in (0, 16, 48, 96, 272) for i in range(8)]
    elif pattern == "rows":               # the same lane of the four 16-lane rows (the readlane merge), and of two of them
        g = [[b + l + 16 * r for r in range(4)] for b, l in ((0, 0), (0, 5), (0, 15), (64, 7), (256, 9))] + [[2, 34], [19, 51]]
    elif pattern == "lane64":             # a lane's two elements (block kernel: other threads)
        g = [[q, q + 64] for q in (0, 1, 17, 62, 63)] + [[q, q + 64, q + 128] for q in (3, 40)]
    elif pattern == "stride256":          # one thread's strided elements; different threads a stride apart
        g = [[q, q + 256, q + 512, q + 768] for q in (0, 100, 255)] + [[1, 258, 516], [200, 457, 715]]
    elif pattern == "all_equal":
        g = [list(range(Q))]
    else:
        raise AssertionError(pattern)
    g = [[q for q in grp if q < Q] for grp in g]
    g = [grp for grp in g if len(grp) > 1]
    flat = [q for grp in g for q in grp]
    assert len(flat) == len(set(flat))
    return g


def tie_patterns(Q):
    """The patterns that tie at least two candidates at this Q (all_equal always counts: at Q = 1 it is the lone candidate)."""
    return [p for p in TIE_PATTERNS if p == "all_equal" or _tie_groups(Q, p)]


DECAY_TIE_GROUPS = ((8, 9, 10, 11), (40, 47), (3, 67), (5, 21, 37, 53), (130, 194), (20, 256), (70, 77))


def tie_case(Q, pattern):
    """One category, groups of EXACTLY equal float32 scores at structured positions, every group and every other candidate on a level
    of its own.  Expected: score-descending, inside a group index-descending.
      the TIE_PATTERNS (hard NMS): disjoint masks, so everything is emitted;
      "decay" (linear / gaussian, the only tie allowed there): query W = Q // 2 has the top score and shares 4 of 7 pixels (union 10,
        IoU 0.4) with every tied candidate; the members of a group share 1 pixel with each other (union 13) and nothing with anyone
        else.  Every tied candidate therefore meets the same IoU against every earlier winner — 0.4 for W, 1 / 13 for a member of its
        own group, 0 for the rest — and the group's decayed scores stay bit-identical on the reference and on the device alike."""
    rng = np.random.default_rng(1000 * Q + len(pattern))
    if pattern == "decay":
        W = Q // 2
        groups = [[q for q in g if q < Q] for g in DECAY_TIE_GROUPS]
        groups = [g for g in groups if len(g) > 1]
        assert groups and all(W not in g for g in groups)
        pairs = [(q, W, 4) for g in groups for q in g] + [(g[i], g[j], 1) for g in groups for i in range(len(g)) for j in range(i)]
        inter, uni = _tables(np.full(Q, 7), pairs)              # (a count table: the kernel's input; no masks are drawn for it)
        for g in groups:
            assert (inter[g, W] == 4).all() and (uni[g, W] == 10).all() and all(uni[g[i], g[j]] == 13 for i in range(len(g)) for j in range(i))
    else:
        groups = _tie_groups(Q, pattern)
        inter, uni = _tables(np.full(Q, 10))
    gid = np.full(Q, -1)
    for i, g in enumerate(groups):
        gid[g] = i
    free = np.flatnonzero(gid < 0)
    gid[free] = len(groups) + np.arange(len(free))
    n = len(groups) + len(free)
    scores = _levels(n)[rng.permutation(n)][gid]
    if pattern == "decay":
        scores[W] = np.float32(0.99)
    if pattern == "all_equal":
        scores[:] = np.float32(0.5)
    case = _case(f"tie-{pattern}-{Q}", inter, uni, scores, np.full(Q, 2), ties=[groups])
    if pattern == "decay":
        for t in ("linear", "gaussian"):
            check_margins(case, t)
    return case


THRESHOLD_PAIRS = ((3, 10), (30000, 100000), (30001, 100000), (4, 13), (50, 50))     # (intersection, union); the last: identical masks


def _weight(i, u, nms_type, thr, sigma):
    iou = i / (u + 1e-7)
    if nms_type == "gaussian":
        return float(np.exp(-(iou * iou) / sigma))
    if iou > thr:
        return 0.0 if nms_type == "hard" else 1.0 - iou
    return 1.0


def threshold_case(Q, nms_type, thr=0.3, sigma=0.5, score_thr=0.001):
    """The strict comparisons.  Category 1 holds ten pairs (a, b), two for each of THRESHOLD_PAIRS: a has a high score, b meets a (and
    nobody else) with those counts and carries a score chosen so that b's score times the weight w of the pair, in float64, lands
    (2 + k) * 1e-6 relative ABOVE score_thr (even k) or BELOW it (odd k): float32 rounding of the score moves that by 6e-8.
      (3, 10) and (30000, 100000) are below thr = 0.3 in float64 — 30000 / (100000 + 1e-7) = 0.2999999999997 — the second only in
        float64: rounded to float32 it is 0.30000001 > 0.3;  (30001, 100000), (4, 13) and identical masks are above.
      w = 1 (not suppressed under hard / linear): the "below" b is dropped in the first round of its category, as any candidate that is
        not the best and not above score_thr;  w = 0 (hard, suppressed) and w * 0.9 <= score_thr (linear on identical masks, w = 2e-9):
        no score <= 1 can land above, b gets a mid score and is dropped either way.
    Category 2: initial scores 0.0005 and 0.0003, both below score_thr — the best of a category is emitted whatever its score, the
    other is dropped in the first round.  Category 3: a lone 0.0002, emitted.  Category 4: the other queries, disjoint, distinct levels.
    Returns (case, expect): expect[q] = True / False for every b and every category 2 / 3 query: emitted or not."""
    n_special = 4 * len(THRESHOLD_PAIRS) + 3
    assert Q >= 2 * n_special
    slot = [(j * Q) // n_special for j in range(n_special)]                    # spread over the lanes / elements / strided threads
    assert len(set(slot)) == n_special
    iou = {p: p[0] / (p[1] + 1e-7) for p in THRESHOLD_PAIRS}
    assert iou[(3, 10)] < 0.3 and iou[(30000, 100000)] < 0.3 < float(np.float32(iou[(30000, 100000)]))
    assert all(iou[p] > 0.3 and float(np.float32(iou[p])) > 0.3 for p in THRESHOLD_PAIRS[2:])
    area, pairs = np.full(Q, 9), []
    scores, cats, expect = _levels(Q)[np.random.default_rng(Q).permutation(Q)] * np.float32(0.5), np.full(Q, 4), {}
    for k in range(2 * len(THRESHOLD_PAIRS)):
        (i, u), a, b = THRESHOLD_PAIRS[k // 2], slot[2 * k], slot[2 * k + 1]
        area[a] = i + (u - i) // 2
        area[b] = u - area[a] + i
        pairs.append((a, b, i))
        cats[[a, b]] = 1
        scores[a] = np.float32(0.9 - 0.005 * k)
        w = _weight(i, u, nms_type, thr, sigma)
        want = score_thr * (1 + (2 + k) * 1e-6 * (1 if k % 2 == 0 else -1))    # where b's score should land after the decay
        if w * 0.9 > score_thr:
            scores[b] = np.float32(want / w)
            landed = float(scores[b]) * w
            assert (landed > score_thr) == (k % 2 == 0) and abs(landed - score_thr) > 1e-6 * score_thr and 0 < scores[b] < 0.8
            expect[b] = k % 2 == 0
        else:
            scores[b] = np.float32(0.6 - 0.005 * k)
            assert float(scores[b]) * w < 0.5 * score_thr
            expect[b] = False
    lo = slot[4 * len(THRESHOLD_PAIRS):]
    cats[lo[:2]], cats[lo[2]] = 2, 3
    scores[lo] = np.array([0.0005, 0.0003, 0.0002], np.float32)
    expect.update({lo[0]: True, lo[1]: False, lo[2]: True})
    inter, uni = _tables(area, pairs)
    for k, (a, b, i) in enumerate(pairs):
        assert (inter[a, b], uni[a, b]) == THRESHOLD_PAIRS[k // 2] == (inter[b, a], uni[b, a])
    case = _case(f"threshold-{nms_type}-{Q}", inter, uni, scores, cats)
    assert len(np.unique(case.scores)) == Q
    if nms_type != "hard":
        check_margins(case, nms_type, thr, sigma, score_thr)
    return case, expect


def equality_case(Q):
    """Both strict comparisons AT equality, which needs thresholds that are results of the same IEEE operations as the kernel's: returns
    (case, thr, score_thr) with thr = 3 / (10 + 1e-7), the very quotient of a pair's counts — `iou > thr` is false, the pair is not
    suppressed under hard and not decayed under linear — and score_thr = 0.25 = the exact score of query 2, which is not the best of
    its category: `s > score_thr` is false and it is dropped in the first round, while query 5, one float32 step above, stays.
    One category, everything else disjoint with scores above 0.3."""
    assert Q >= 16
    thr, score_thr = 3 / (10 + 1e-7), 0.25
    a, b = Q - 1, Q // 2
    area = np.full(Q, 9)
    area[a], area[b] = 6, 7
    inter, uni = _tables(area, [(a, b, 3)])
    assert inter[b, a] / (uni[b, a] + 1e-7) == thr
    scores = (np.float32(0.3) + _levels(Q)[np.random.default_rng(Q + 1).permutation(Q)] * np.float32(0.5)).astype(np.float32)
    scores[a], scores[b] = np.float32(0.9), np.float32(0.85)
    scores[2], scores[5] = np.float32(0.25), np.nextafter(np.float32(0.25), np.float32(1))
    case = _case(f"equality-{Q}", inter, uni, scores, np.full(Q, 1))
    assert len(np.unique(case.scores)) == Q and float(case.scores[0, 2]) == score_thr < float(case.scores[0, 5])
    for t in ("linear", "gaussian"):
        worst = [np.inf]

        def on_step(kind, index, s, ref):                       # check_margins, apart from the one decayed score that IS score_thr
            if kind == "select":
                lower = s[s < ref]
                assert (s == ref).sum() == 1 and (not lower.size or (ref - lower.max()) / ref > MARGIN)
            else:
                d = np.abs(s - ref)[index != 2]
                assert not d.size or d.min() / ref > MARGIN
                worst[0] = min(worst[0], d.min() / ref if d.size else np.inf)

        _image(case.inter[0], case.uni[0], case.scores[0], case.cats[0], t, thr, 0.5, score_thr, on_step)
    return case, thr, score_thr


BIG_IDS = (2 ** 40 + 3, 5, 2 ** 62 + 1, 2 ** 62 + 3, 0, 2 ** 31 + 7, 2 ** 33 + 1)


def degenerate_cases(Q):
    """{name: Case}, for hard NMS:
      all_cat0        every category 0: nothing is processed, count 0;
      all_empty       every mask empty (all counts 0, IoU 0 / 1e-7 = 0), two categories: Q selection steps, nothing emitted;
      empty_winners   queries 0, 3, 6, ... are empty, hold the top scores and, in the count table, overlap their right neighbour 5 / 10:
                      they win, are not emitted, and still suppress the neighbour;
      one_category    all Q in category 7, each mask overlapping its neighbours 6 / 14: greedy suppression along a chain;
      distinct_cats   Q identical masks in Q distinct categories: nothing suppresses anything, count == Q, category-ascending;
      big_ids         BIG_IDS by q % 7 over identical masks: one survivor per id.  2**62 + 1 and 2**62 + 3 are different int64 ids and
                      the same float64; ids above 2**53 are not exact in the packed row's float64 slots, so callers leave `packed`
                      out for this case;
      two_images      distinct_cats and one_category in one call: counts Q and less, so the image strides of all six arrays matter."""
    rng = np.random.default_rng(7 * Q + 1)
    lv = lambda: _levels(Q)[rng.permutation(Q)]
    disjoint = _tables(np.full(Q, 10))
    same = (np.full((Q, Q), 10), np.full((Q, Q), 10))
    out = {"all_cat0": _case(f"all_cat0-{Q}", *disjoint, lv(), np.zeros(Q, np.int64)),
           "all_empty": _case(f"all_empty-{Q}", np.zeros((Q, Q)), np.zeros((Q, Q)), lv(), 1 + np.arange(Q) % 2)}
    inter, uni = _tables(np.where(np.arange(Q) % 3 == 0, 0, 10))
    scores = np.sort(lv())[::-1].copy()                         # descending: the empty q = 3 j outranks its neighbour 3 j + 1
    for e in range(0, Q - 1, 3):
        inter[e, e + 1] = inter[e + 1, e] = 5
        uni[e, e + 1] = uni[e + 1, e] = 10
    out["empty_winners"] = _case(f"empty_winners-{Q}", inter, uni, scores, np.full(Q, 4))
    chain = _tables(np.full(Q, 10), [(q, q + 1, 6) for q in range(Q - 1)])
    assert Q == 1 or chain[1][0, 1] == 14
    out["one_category"] = _case(f"one_category-{Q}", *chain, lv(), np.full(Q, 7))
    perm_cats = 1 + rng.permutation(Q)
    out["distinct_cats"] = _case(f"distinct_cats-{Q}", *same, lv(), perm_cats)
    big = np.array(BIG_IDS, np.int64)[np.arange(Q) % len(BIG_IDS)]
    assert np.float64(BIG_IDS[2]) == np.float64(BIG_IDS[3]) and BIG_IDS[2] != BIG_IDS[3]
    out["big_ids"] = _case(f"big_ids-{Q}", *same, lv(), big)
    out["two_images"] = _case(f"two_images-{Q}", np.stack([same[0], chain[0]]), np.stack([same[1], chain[1]]), np.stack([lv(), lv()]),
                              np.stack([perm_cats, np.full(Q, 7)]))
    return out


def random_case(Q, B, seed):
    """Random overlapping rectangles on 48 x 64 as in test_device_mask_nms_matches_reference_control_flow — empty masks (q % 17 == 3),
    one identical pair, class 0, a score that falls below score_thr once decayed, one single-class image, one image with COCO-range
    ids — through counts_from_masks.  Tie-free, and inside the linear / gaussian margins (asserted here: the seed is chosen for it)."""
    rng = np.random.default_rng(seed)
    H, W = 48, 64
    masks = np.zeros((B, Q, H, W), bool)
    for b in range(B):
        for q in range(Q):
            if q % 17 == 3:
                continue
            y0, x0 = rng.integers(0, H - 8), rng.integers(0, W - 8)
            hh, ww = rng.integers(4, 24), rng.integers(4, 32)
            masks[b, q, y0:y0 + hh, x0:x0 + ww] = True
        masks[b, 10] = masks[b, 11]
    scores = rng.random((B, Q)).astype(np.float32) * np.float32(0.9) + np.float32(0.05)
    scores[:, 20] = 0.0009
    cats = rng.integers(0, 6, (B, Q)).astype(np.int64)
    if B > 1:
        cats[1] = 2
    if B > 2:
        cats[2] = np.array([33, 2, 40, 3, 80, 65], np.int64)[rng.integers(0, 6, Q)]
    assert all(len(np.unique(scores[b])) == Q for b in range(B))
    inter, uni = counts_from_masks(masks)
    case = _case(f"random-{Q}-{B}-{seed}", inter, uni, scores, cats, masks=masks)
    for t in ("linear", "gaussian"):
        check_margins(case, t)
    return case
