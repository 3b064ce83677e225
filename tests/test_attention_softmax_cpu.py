"""The attention softmax cases themselves (tests/_attention_case.py), checked without a GPU and without the library:

  * every builder produces the structure it claims, measured on the operands as the kernel sees them (fp16 / split pair);
  * the float64 reference is honest: the same softmax in float32 with the kernel's scale constant stays within a quarter of the tolerance;
  * the cases discriminate: a numpy restatement of the key-tile loop as attention.hip's comments describe it — fp16 (or split-pair) P,
    fp32 accumulators, a reference point that only moves when a tile's max exceeds it by more than L, the fp16 row sum of the rounded P
    / the x3 fp32 row sum of the unrounded exponentials — is within tolerance as written, and outside it with subnormal P flushed (peak
    over a tail), with the row sum not rescaled (staircase at 1.01 L and 2 L), and with the causal mask off by one key (uniform causal).
"""
import math

import numpy as np
import pytest
import torch

from tests import _attention_case as ac

L = ac.LAZY
VARIANTS = [(False, 64), (False, 96), (True, 64), (True, 96)]
variants = pytest.mark.parametrize("x3,dh", VARIANTS)


def _all(x3, dh, families=ac.FAMILIES):
    return [c for fam in families for c in ac.cases(fam, x3, dh)]


def _tile_max(case, bi, h, row, s=None):
    s = ac.scores_log2(case) if s is None else s
    kt = case.desc["kt"]
    r = s[bi, h, row]
    return [float(r[t:t + kt].max()) for t in range(0, case.Tk, kt)]


# ------------------------------------------------------------------------------------------------------------------ structure
def test_constants_read_from_source():
    assert (ac.LAZY, ac.KT_F16, ac.KT_X3) == ac.kernel_constants()
    assert ac.LAZY > 0 and ac.KT_F16 % 32 == 0 and ac.KT_X3 % 32 == 0


def _expected_moves(step_l, ntiles):
    """Which tiles of a RISING staircase move the reference point; None where the ideal levels put the decision on the threshold itself."""
    if step_l > 1.0:
        return [True] * ntiles                          # every tile exceeds the last reference by step > L
    if step_l == 0.99:
        return [t % 2 == 0 for t in range(ntiles)]      # 0.99 L stays, 1.98 L moves
    return None                                         # 0.5 L: two steps are exactly L (the jitter decides; either way is a valid schedule)


@variants
def test_staircase_crosses_where_intended(x3, dh):
    """Tile maxima after the operands' rounding: a falling staircase never moves the reference after tile 0; a rising one moves it at every
    tile for steps 1.01 L and 2 L, at every second tile for 0.99 L, and each of those decisions keeps >= 0.03 log2 units from the threshold
    (the fp32 score error at these magnitudes is < 1e-4).  At 0.5 L the reference moves two or three times in seven tiles."""
    for case in ac.cases("staircase", x3, dh):
        s = ac.scores_log2(case)
        assert case.Tk == 6 * case.desc["kt"] + 5
        for (bi, h), spec in case.desc["heads"].items():
            tm = _tile_max(case, bi, h, 0, s)
            assert len(tm) == 7
            assert np.allclose(tm, spec["levels"].numpy() + ac.JITTER, atol=ac.JITTER + 0.05), (case, bi, h, tm)   # level + jitter +- rounding
            moves, margins = ac.lazy_schedule(tm)
            if not spec["rising"]:
                assert moves == [True] + [False] * 6, (case, bi, h, moves)
                continue
            want = _expected_moves(spec["step"], 7)
            if want is None:
                assert moves[0] and 2 <= sum(moves[1:]) <= 3, (case, bi, h, moves)
            else:
                assert moves == want, (case, bi, h, moves, tm)
                assert min(margins) >= 0.03, (case, bi, h, margins)


@variants
def test_row_schedule_mixes_lanes(x3, dh):
    """Rows i, i + 1, i + 2 of one wave: one moves its reference at a tile past the first, one never does (flat: a = 0), one has its max in
    tile 0 — so alpha != 1 and alpha == 1 lanes share a wave."""
    for case in ac.cases("row_schedule", x3, dh):
        s = ac.scores_log2(case)
        for (bi, h) in case.desc["heads"]:
            for i0 in (0, case.Tq - 3):
                kinds = set()
                for i in range(i0, i0 + 3):
                    moves, _ = ac.lazy_schedule(_tile_max(case, bi, h, i, s))
                    kinds.add("moves" if any(moves[1:]) else "stays")
                    flat = float(s[bi, h, i].max() - s[bi, h, i].min()) < 0.01
                    kinds.add("flat" if flat else "steep")
                assert kinds == {"moves", "stays", "flat", "steep"}, (case, bi, h, i0, kinds)


@variants
def test_peak_tail_structure(x3, dh):
    for case in ac.cases("peak_tail", x3, dh):
        s = ac.scores_log2(case)
        p = torch.softmax(s * math.log(2.0), -1)
        kt, depth = case.desc["kt"], case.desc["depth"]
        places = set()
        for (bi, h), spec in case.desc["heads"].items():
            row = s[bi, h, 0]
            assert int(row.argmax()) == spec["peak"]
            rest = torch.cat([row[:spec["peak"]], row[spec["peak"] + 1:]]) - row[spec["peak"]]
            assert float((rest - depth).abs().max()) < 0.02, (case, float((rest - depth).abs().max()))
            mass = float(1.0 - p[bi, h, 0, spec["peak"]])
            assert abs(mass - case.desc["tail_mass"]) < 0.02 * case.desc["tail_mass"]
            if case.Tk == 1029 and depth >= -15.3:
                assert mass >= 0.02, (case, mass)           # the heavy tail: 1028 keys at -15.3 carry 2.5 % of the row
            places.add(spec["peak"])
        assert places == {0, kt - 1, (case.Tk - 1) // kt * kt, case.Tk - 1}
        assert (case.Tk - 1) // kt * kt + 5 == case.Tk       # a ragged last tile of 5 keys


@variants
def test_one_hot_margin(x3, dh):
    for case in ac.cases("one_hot", x3, dh):
        s = ac._mask(case, ac.scores_log2(case))
        top2 = s.topk(min(2, case.Tk), -1).values
        if case.desc.get("diagonal"):
            assert torch.equal(s.argmax(-1), torch.arange(case.Tq).expand(case.B, case.heads, -1))
            top2 = top2[..., 1:, :]                          # row 0 has one key
        else:
            for (bi, h), spec in case.desc["heads"].items():
                assert bool((s[bi, h].argmax(-1) == spec["hot"]).all())
        assert float((top2[..., 0] - top2[..., 1]).min()) >= 40.0, case
        # O is the hot key's V row: what the rest contributes is below 2^-40 Tk max|v|
        ref, vh = ac.reference(case), case.per_head(case.v.double())
        hot = torch.gather(vh, 2, s.argmax(-1)[..., None].expand(-1, -1, -1, case.dh)).transpose(1, 2).reshape(case.B, case.Tq, -1)
        assert float((ref - hot).abs().max()) < 1e-7


@variants
def test_uniform_is_the_mean(x3, dh):
    for case in ac.cases("uniform", x3, dh) + [c for c in ac.cases("key_split", x3, dh) if c.name.startswith("uniform")]:
        assert float(case.q.abs().max()) == 0.0
        ref, vh = ac.reference(case), case.per_head(case.v.double())
        mean = vh.mean(2, keepdim=True).expand(-1, -1, case.Tq, -1).transpose(1, 2).reshape(case.B, case.Tq, -1)
        assert float((ref - mean).abs().max()) < 1e-12
        assert float((vh[:, 0] - 0.75).abs().max()) == 0.0
        # the ramp's mean, (Tk - 1) / (2 Tk), differs from that of one key more or fewer by 1 / (2 Tk) ... as far as V's rounding lets it
        assert abs(float(vh[0, 1, :, 0].mean()) - (case.Tk - 1) / (2 * case.Tk)) < 2.0 ** -11


@variants
def test_common_offset_is_common(x3, dh):
    cs = ac.cases("common_offset", x3, dh)
    assert {c.desc["C"] for c in cs} == ({64.0} if x3 else {64.0, 1000.0})
    for case in cs:
        base = case.desc["base"]
        d = ac.scores_log2(case) - ac.scores_log2(base)
        C = case.desc["C"]
        for h, want in enumerate((C, -C, 0.0)):
            assert float((d[:, h] - want).abs().max()) <= 1e-3 * max(C, 1.0)          # the shift itself, to fp16 rounding of 1 / c
            assert float((d[:, h] - d[:, h, :, :1]).abs().max()) < 1e-9               # and exactly the same for every key of a row
        assert float(ac.scores_log2(case).abs().max()) <= C * (1 + 2.0 ** -11) + 1e-3
        # the result must equal the unshifted case's reference
        assert float((ac.reference(case) - ac.reference(base)).abs().max()) < 1e-9


@variants
def test_causal_cases(x3, dh):
    cs = ac.cases("causal", x3, dh)
    assert {c.Tq for c in cs} == set(ac.CAUSAL_T) and {c.layout for c in cs} == {"packed", "slice"} and any(c.scale for c in cs)
    for case in cs:
        assert case.Tq == case.Tk
        ref, vh = ac.reference(case), case.per_head(case.v.double())
        running = (vh.cumsum(2) / torch.arange(1, case.Tk + 1, dtype=torch.float64)[:, None])
        for h in case.desc["uniform_heads"]:
            got = ref.view(case.B, case.Tq, case.heads, case.dh)[:, :, h]
            assert float((got - running[:, h]).abs().max()) < 1e-12                   # row i is the mean of V[0..i]


@variants
def test_key_split_chunks_unequal(x3, dh):
    cs = ac.cases("key_split", x3, dh)
    assert {c.ksplit for c in cs if not c.expect_error} == {2, 4}
    refused = [c for c in cs if c.expect_error]
    assert len(refused) == 1 and refused[0].Tk == 8 * refused[0].desc["kt"] + 5 and refused[0].ksplit == 4
    for case in cs:
        if not case.name.startswith("unequal"):
            continue
        s = ac.scores_log2(case)
        kc, S = case.desc["kchunk"], case.ksplit
        assert kc % case.desc["kt"] == 0 and (S - 1) * kc < case.Tk <= S * kc
        cmax = torch.stack([s[:, :, 0, i * kc:(i + 1) * kc].max(-1).values for i in range(S)], -1)    # [B, heads, S]
        gap = cmax.max(-1, keepdim=True).values - cmax
        assert int(cmax[0, 0].argmax()) == 0 and int(cmax[0, 1].argmax()) == S - 1               # dominant key: first / last chunk
        assert float(gap[:, :2].max()) > 19.0
        assert float(gap[0, 2, 0]) >= 149.5 and float(gap[1, 2, S - 1]) >= 149.5                  # 2^-149.5 is 0 in fp32 arithmetic with flushed denormals
        live = s[:, 2].clone()
        live[0, :, :kc] = 0
        live[1, :, (S - 1) * kc:] = 0
        assert float(live.abs().max()) <= 64.0                                                    # every key that carries weight


# ------------------------------------------------------------------------------------------------------------------ honest reference
@variants
def test_float32_reference_within_quarter_tolerance(x3, dh):
    """The cases' float64 reference against the same softmax in float32 with the kernel's float32(scale) * 1.4426950408889634f: what the
    inputs alone cost (score rounding at their magnitude, the scale constant) stays under a quarter of the tolerance, for every case."""
    worst = {}
    for case in _all(x3, dh):
        err = float((ac.reference_f32(case).double() - ac.reference(case)).abs().max())
        worst[case.family] = max(worst.get(case.family, 0.0), err)
        assert err <= case.tol / 4, (case, err)
    print(f"float32 reference x3={x3} dh={dh}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------------------------ restatement
def _f16(x):
    return x.astype(np.float16).astype(np.float32)


def _flush(x):
    return np.where(np.abs(x) < 2.0 ** -14, np.float32(0), x)


def tile_loop(q, k, v, c, kt, x3, causal=False, flush=False, rescale_sum=True, mask_shift=0):
    """One head, as attention.hip describes its loop.  q [Tq, dh], k, v [Tk, dh]: float32 operands as seen; c = float32 scale * log2(e).
    Scores in fp32; per key tile of kt keys: m_cand = c * tile max; the reference point m moves to m_cand only if m_cand > m + L; alpha =
    2^(m_old - m) rescales the fp32 accumulators; p = 2^(c s - m) is rounded to fp16 (x3: split into hi = f16(p), lo = f16(p - hi));
    O += p V in fp32; the row sum adds the ROUNDED p (fp16 kernels) or the fp32 exponentials (x3).  Knobs restate three bugs: `flush`
    zeroes subnormal fp16 values of P, `rescale_sum` = False forgets alpha on the row sum, `mask_shift` = 1 lets one key past the diagonal."""
    Tq, Tk = q.shape[0], k.shape[0]
    s = (q.astype(np.float64) @ k.astype(np.float64).T).astype(np.float32)
    m = np.full(Tq, -np.inf, np.float32)
    o = np.zeros((Tq, v.shape[1]), np.float32)
    l = np.zeros(Tq, np.float32)
    rows = np.arange(Tq)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        for t0 in range(0, Tk, kt):
            st = s[:, t0:t0 + kt].copy()
            if causal:
                if t0 > Tq - 1:                      # key tiles entirely above the last query are skipped
                    break
                st[np.arange(t0, t0 + st.shape[1])[None, :] > rows + mask_shift] = -np.inf
            m_cand = (st.max(1) * c).astype(np.float32)
            m_new = np.where(m_cand > m + np.float32(L), m_cand, m).astype(np.float32)
            alpha = np.exp2(m - m_new).astype(np.float32)
            alpha[np.isnan(alpha)] = 1.0
            e = np.exp2((st.astype(np.float64) * np.float64(c) - m_new[:, None]).astype(np.float32)).astype(np.float32)
            hi = _f16(e)
            lo = _f16(e - hi) if x3 else np.zeros_like(hi)
            if flush:
                hi, lo = _flush(hi), _flush(lo)
            p = hi.astype(np.float64) + lo
            o = (o * alpha[:, None] + (p @ v[t0:t0 + kt].astype(np.float64))).astype(np.float32)
            l = (l * (alpha if rescale_sum else 1) + (e.sum(1) if x3 else p.sum(1))).astype(np.float32)
            m = m_new
    out = o / l[:, None]
    hi = _f16(out)
    return (hi.astype(np.float64) + _f16(out - hi)) if x3 else hi.astype(np.float64)


def restate(case, rows=None, **knobs):
    c = np.float32(case.sc) * np.float32(ac.LOG2E)
    qh, kh, vh = (case.per_head(t).numpy() for t in (case.q, case.k, case.v))
    rows = np.arange(case.Tq) if rows is None else rows
    out = np.zeros((case.B, len(rows), case.heads, case.dh))
    for bi in range(case.B):
        for h in range(case.heads):
            out[bi, :, h] = tile_loop(qh[bi, h][rows], kh[bi, h], vh[bi, h], c, case.desc["kt"], case.x3, causal=case.causal, **knobs)
    return out


def _err(case, rows=None, **knobs):
    """[B, Tq, heads]: max |restatement - float64 reference| over each head's columns (rows: a subset of the queries, not for causal)."""
    assert rows is None or not case.causal
    ref = ac.reference(case).numpy().reshape(case.B, case.Tq, case.heads, case.dh)
    return np.abs(restate(case, rows, **knobs) - (ref if rows is None else ref[:, rows])).max(-1)


@variants
def test_restatement_within_tolerance(x3, dh):
    """Faithful arithmetic passes every case (the key-split cases run here as one pass over all keys, which is what the merge must equal)."""
    worst = {}
    for case in _all(x3, dh):
        if case.expect_error:
            continue
        rows = None if case.causal or case.Tq <= 40 else np.r_[0:36, case.Tq - 4:case.Tq]     # rows are independent: the packed cases' first and last
        err = float(_err(case, rows).max())
        worst[case.family] = max(worst.get(case.family, 0.0), err)
        assert err <= case.tol, (case, err)
    print(f"restatement x3={x3} dh={dh}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


@variants
def test_flushed_subnormal_p_is_caught(x3, dh):
    """Tail keys at -15.3 (any Tk) and at -17.3 (Tk = 1029) have subnormal fp16 P (x3: subnormal hi and lo): flushing them loses the tail,
    2 w mass / (1 + mass) >= 3.3e-3 w for the opposite-sign V at x3's 133 keys and 1.3e-2 w at fp16's 261 (w >= 0.5).  At -12 P is a
    normal fp16 number and at -17.3 the short tail weighs too little for the fp16 tolerance: those cases run for their values only.  So do the heads
    whose peak lies in the last tile: until it arrives the reference point is the tail itself and the tail's P is 1."""
    n = 0
    for case in ac.cases("peak_tail", x3, dh):
        d = case.desc
        if d["vmode"] != "opposite" or not (d["depth"] == -15.3 or (d["depth"] == -17.3 and case.Tk == 1029)):
            continue
        err = _err(case, flush=True)
        early = [bh for bh, spec in d["heads"].items() if spec["peak"] < d["kt"]]
        assert len(early) == 4
        for bi, h in early:                                                   # every row of every head whose peak comes first
            assert float(err[bi, :, h].min()) > case.tol, (case, bi, h, float(err[bi, :, h].min()))
        n += 1
    assert n == 3


@variants
def test_unscaled_row_sum_is_caught(x3, dh):
    """Rising staircases of 1.01 L and 2 L move the reference at every tile: a row sum that is not multiplied by alpha keeps the early
    tiles' sums at full weight.  Every head whose pattern is one of the two must fail, in every row."""
    n = 0
    for case in ac.cases("staircase", x3, dh) + ac.cases("row_schedule", x3, dh):
        err = _err(case, rescale_sum=False)
        for (bi, h), spec in case.desc["heads"].items():
            if spec["step"] > 1.0 and spec.get("rising", True):
                rows = slice(None) if case.family == "staircase" else slice((-h) % 3, None, 3)    # row_schedule: the a = +1 rows
                assert float(err[bi, rows, h].min()) > case.tol, (case, bi, h, float(err[bi, rows, h].min()))
                n += 1
    assert n >= 8


@variants
def test_causal_mask_off_by_one_is_caught(x3, dh):
    """A mask that lets key i + 1 through changes row i's uniform mean by (v[i + 1] - mean) / (i + 2): over a head's randn columns that
    is past the tolerance at every row but the last (which has no key behind it), for every T."""
    for case in ac.cases("causal", x3, dh):
        err = _err(case, mask_shift=1)
        for h in case.desc["uniform_heads"]:
            assert float(err[:, :-1, h].min()) > case.tol, (case, h, float(err[:, :-1, h].min()))
