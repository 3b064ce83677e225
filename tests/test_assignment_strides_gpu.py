"""zh_linear_assignment past one wave: both sides above 64 (every `k = lane; k < nr; k += 64` loop takes a second trip), tall problems
with more than 64 instances, the cap, negative and wide-range costs — against scipy.optimize.linear_sum_assignment on the same float32
matrix, rows and columns equal element for element — and assignment_finish_kernel across its 64-row wave and 256-row step boundaries
(R = L * n_tot = 336) against the host loop of the criterion.  The cap-sized shapes (40 x 1024, 1024 x 40: 40 augmenting paths) take
0.5 - 0.6 ms per solve on the MI355X, copy back included (printed with -s)."""
import time

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from tests.test_assignment_gpu import _batched, _host_loop, _matrix as _matrix3
from zutis_amd import ops

pytestmark = pytest.mark.gpu

# both sides above 64 and the edges; tall with more than 64 instances; at the cap, rectangular so the serial solve stays at 40 paths
SHAPES = [(64, 64), (65, 65), (70, 130), (130, 70), (100, 100), (129, 129), (200, 64), (65, 3), (40, 1024), (1024, 40)]
KINDS = ["uniform", "ints", "duplicate", "signed", "wide"]


def _matrix(n, Q, kind, seed):
    if kind in ("uniform", "ints", "duplicate"):
        return _matrix3(n, Q, kind, seed)
    g = np.random.default_rng(seed)
    if kind == "signed":
        return (g.random((n, Q), dtype=np.float32) * np.float32(2) - np.float32(1))              # uniform in [-1, 1)
    assert kind == "wide"                                                   # +-2^e, e uniform in [-60, 60], times a uniform mantissa
    mant = np.float32(0.5) + np.float32(0.5) * g.random((n, Q), dtype=np.float32)
    sign = np.where(g.integers(0, 2, (n, Q)) == 1, np.float32(-1), np.float32(1))
    return (sign * np.ldexp(mant, g.integers(-60, 61, (n, Q)).astype(np.int32))).astype(np.float32)


def _explain(cm, rows, cols, want_r, want_c):
    """For a failure message: is the device result a valid assignment, and of the optimum's total cost in float64?"""
    n = min(cm.shape)
    valid = (len(rows) == len(cols) == n and len(set(rows.tolist())) == n and len(set(cols.tolist())) == n
             and (np.diff(rows) > 0).all() and rows.min() >= 0 and rows.max() < cm.shape[0] and cols.min() >= 0 and cols.max() < cm.shape[1])
    got = float(cm[rows, cols].astype(np.float64).sum()) if valid else float("nan")
    want = float(cm[want_r, want_c].astype(np.float64).sum())
    first = int(np.flatnonzero((rows != want_r) | (cols != want_c))[0]) if valid else -1
    return f"valid={valid} cost got={got!r} want={want!r} first difference at pair {first}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,Q", SHAPES)
def test_solver_equals_scipy(dev, n, Q, kind):
    spent = 0.0
    for seed in (0, 1, 2):
        cm = _matrix(n, Q, kind, 1000 * seed + 31 * n + Q)
        assert cm.dtype == np.float32 and np.isfinite(cm).all()
        want_r, want_c = linear_sum_assignment(cm)
        cd = torch.from_numpy(cm).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows, cols = ops.linear_assignment(cd)
        spent += time.perf_counter() - t0
        assert rows.shape == want_r.shape and cols.shape == want_c.shape, (n, Q, kind, seed)
        assert np.array_equal(rows, want_r) and np.array_equal(cols, want_c), (n, Q, kind, seed, _explain(cm, rows, cols, want_r, want_c))
    if max(n, Q) == ops.ASSIGN_MAX_DIM:
        print(f"\nlinear_assignment {n} x {Q} {kind}: {1e3 * spent / 3:.1f} ms per solve (with the copy back)")


def test_matrix_kinds():
    s, w = _matrix(70, 130, "signed", 1), _matrix(70, 130, "wide", 1)
    assert s.dtype == w.dtype == np.float32 and s.min() < -0.9 and s.max() > 0.9 and -1 <= s.min() and s.max() < 1
    e = np.frexp(w)[1]
    assert (w < 0).any() and (w > 0).any() and e.min() <= -55 and e.max() >= 55 and -60 <= e.min() and e.max() <= 60


# ---- the batched call: assignment_finish_kernel across its wave (64) and step (256) boundaries

L, Q = 3, 7


def _problem_of_row(r, off, B):
    """(b, l, i) of row r of the match array (the (b, l, i) order of the costs' rows)."""
    b = next(b for b in range(B) if L * off[b] <= r < L * off[b + 1])
    n_b = int(off[b + 1] - off[b])
    rr = r - L * int(off[b])
    return b, rr // n_b, rr % n_b


def _costs(counts, matched, seed):
    """Uniform [0, 1) costs in which each boundary row r is forced: matched[r] True -> one entry of -10 (a tall problem's optimum must
    use that row), False -> the whole row at +10 (with at least Q cheaper rows it stays a hole)."""
    B = len(counts)
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    g = np.random.default_rng(seed)
    cost = g.random(L * int(off[-1]) * Q, dtype=np.float32)
    for r, m in matched.items():
        b, _, _ = _problem_of_row(r, off, B)
        assert counts[b] > Q + 2                                            # a tall problem: holes exist
        cost[r * Q:(r + 1) * Q] = np.float32(10)
        if m:
            cost[r * Q + (r % Q)] = np.float32(-10)
    return cost


def _rows_of_pairs(pairs, off):
    return [L * int(off[b]) + l * int(off[b + 1] - off[b]) + i for b, l, q, i in pairs.tolist()]


@pytest.mark.parametrize("counts,skip,matched", [
    ((30, 0, 9, 70, 3), [0, 0, 1, 0, 0], {63: True, 64: False, 255: False, 256: True}),
    ((70, 3, 30, 0, 9), [0, 0, 0, 0, 1], {63: False, 64: True, 255: True, 256: False}),
], ids=["as-issued", "permuted"])
def test_batched_call_across_wave_and_step_boundaries(dev, counts, skip, matched):
    """B = 5, L = 3, Q = 7: R = 336 rows of `match`, 51 pairs.  The 70-instance image is solved transposed; tall problems leave -1 holes
    on both sides of rows 63 / 64 and 255 / 256, one of each pair matched and the other a hole."""
    B = len(counts)
    cost_h = _costs(counts, matched, 17)
    status, n_pairs, pairs, loss, off = _batched(dev, cost_h, counts, skip, L, Q)
    want, want_loss = _host_loop(cost_h, off, skip, B, L, Q)
    assert L * int(off[-1]) == 336
    got_rows = set(_rows_of_pairs(want, off))
    assert all((r in got_rows) == m for r, m in matched.items())            # the host agrees that the boundary rows are what they were built as
    assert status == 0
    assert n_pairs == len(want) == 51 == L * (7 + 7 + 3)
    assert np.array_equal(pairs[:n_pairs], want)
    assert not pairs[n_pairs:].any()                                        # nothing written past the pairs
    assert abs(float(loss) - float(want_loss)) <= abs(float(np.spacing(want_loss)))    # the forced costs make the loss negative


def test_nan_in_the_tall_problem_costs_only_that_problem(dev):
    counts, skip = (30, 0, 9, 70, 3), [0, 0, 1, 0, 0]
    B, b_bad, l_bad = len(counts), 3, 1
    cost_h = _costs(counts, {63: True, 64: False, 255: False, 256: True}, 23)
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    want, _ = _host_loop(cost_h, off, skip, B, L, Q)                        # of the clean costs: every other problem reads the same numbers
    keep = ~((want[:, 0] == b_bad) & (want[:, 1] == l_bad))
    assert keep.sum() == 51 - 7
    want = want[keep]
    bad = cost_h.copy()
    base = (L * int(off[b_bad]) + l_bad * counts[b_bad]) * Q
    bad[base + 69 * Q + 6] = np.nan                                         # the last entry of the 70 x 7 problem
    status, n_pairs, pairs, loss, off32 = _batched(dev, bad, counts, skip, L, Q)
    assert status == ops.STATUS_NONFINITE
    assert n_pairs == len(want) == 44
    assert np.array_equal(pairs[:n_pairs], want)
    assert not pairs[n_pairs:].any()
    # the loss is the other problems' matched costs (float64, in (b, l, i) order) over B
    total = sum(float(cost_h[r * Q + int(q)]) for r, q in zip(_rows_of_pairs(want, off), want[:, 2]))
    want_loss = np.float32(total / B)
    assert abs(float(loss) - float(want_loss)) <= abs(float(np.spacing(want_loss)))    # the forced costs make the loss negative
