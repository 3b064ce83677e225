"""No GPU, no library: the cases of tests/_norm_case.py themselves.

1. every builder has the structure it claims, measured on the operands as the kernel reads them;
2. the reference is honest: a float32 restatement of each kernel of norm.hip stays below HALF of the derived tolerance on every case
   (a condition on the inputs — a family that misses it is changed, never the tolerance);
3. the cases discriminate: each wrong restatement exceeds the tolerance on its family.  Where the earlier tests' data (randn * 3 + 1 rows,
   randn * 2 + 0.3 images) is blind to the same mistake, that is asserted too — it is the gap these cases close:
     one-pass variance                    blind at every D
     mean from the fp16-rounded row       blind at D = 1024 only (0.59 of the flat tolerance; 1.3 at D = 192 / 516, 7.5 at D = 8)
     between-chunk variance term dropped  blind at every shape with l2_eps = 1e-7, and so are the structured images: rstd cancels
     chunk count capped at 64             blind at (1, 257, 1024) (0.59)
   The other two are seen by benign data as well and are listed for what the structured cases add: an unweighted chunk mean exceeds the flat
   tolerance 64 x on the benign (2, 37, 516) image but only 1.75 x on (1, 257, 1024), against 881 x and 108 x on `step`; a last float4 left
   out of the statistics shows on any row whose tail is not zero, and `outlier` puts -180 there.
Ratios are |restatement - float64| / bound, largest element.
"""
import numpy as np
import pytest
import torch

from tests import _norm_case as nc


def _ratio(got, ref, bound):
    ok = torch.isfinite(ref)
    assert bool((torch.isfinite(got) == ok).all())
    return float(((got.double() - ref).abs() / bound)[ok].max())


def _row_ratio(case, wrong=None):
    g, b = nc.affine(case.D)
    ref = nc.ln64(case.x, g, b, case.eps)
    return _ratio(nc.ln_rows_f32(case.x, g, b, case.eps, h8=case.in_f16, wrong=wrong), ref, nc.row_bound(case.x, g, case.eps, ref, nc.TOL_F32))


def _benign_row_ratio(D, wrong):
    g, b = nc.affine(D)
    x = nc.benign_rows(D)
    ref = nc.ln64(x, g, b, 1e-5)
    return _ratio(nc.ln_rows_f32(x, g, b, 1e-5, wrong=wrong), ref, nc.TOL_F32[0] + nc.TOL_F32[1] * ref.abs())


def _image_ratio(x, eps, l2_eps, wrong=None, flat_only=False):
    ref = nc.gln64(x, eps, l2_eps)
    bound = nc.TOL_IMG_F32[0] + nc.TOL_IMG_F32[1] * ref.abs() if flat_only else nc.image_bound(x, eps, ref, nc.TOL_IMG_F32)
    return _ratio(nc.gln_f32(x, eps, l2_eps, wrong=wrong), ref, bound)


# ------------------------------------------------------------------------------------------------------------ 1. structure
@pytest.mark.parametrize("D", nc.ROW_DIMS)
def test_offset_rows_are_conditioned_as_claimed(D):
    """mean|x| / std of every offset row is within 10 % of |c| / sigma (fp32 form; the fp16 grid is too coarse for sigma = 1 at 1e4, where the
    rounded row is a constant or three-valued one: its conditioning is measured, not claimed).  cond_row, which adds eps under the root, is
    the same number except where var is not far above eps = 1e-5: c = 1, sigma = 1e-3 gives 1 / sqrt(1.1e-5) = 301."""
    cases = nc.row_cases("offset", D)
    assert [(c.desc["c"], c.desc["sigma"]) for c in cases] == list(nc.OFFSETS)
    for case in cases:
        assert case.rows % 4 in (1, 2, 3) and case.x.dtype == torch.float32
        assert sorted(set(torch.sign(case.x.mean(-1)).tolist())) == [-1.0, 1.0]                 # both signs of c
        want = case.desc["c"] / case.desc["sigma"]
        data = nc.cond_row(case.x, 0.0)
        assert bool(((data / want - 1).abs() < 0.10).all()), (case.name, data.flatten().tolist())
        with_eps = nc.cond_row(case.x, case.eps)
        assert bool((with_eps <= data).all())
        if case.desc["sigma"] >= 1:
            assert bool(((with_eps / data - 1).abs() < 1e-4).all())
        else:
            assert bool(((with_eps / (1 / np.sqrt(1e-6 + 1e-5)) - 1).abs() < 0.1).all())
    for case in nc.row_cases("offset", D, in_f16=True):
        assert bool((case.x == case.x.half().float()).all()) and case.D % 8 == 0
        assert bool(torch.isfinite(nc.cond_row(case.x, case.eps)).all())


@pytest.mark.parametrize("in_f16", [False, True])
@pytest.mark.parametrize("D", nc.ROW_DIMS)
def test_outliers_sit_in_the_first_and_the_last_valid_float4(D, in_f16):
    (case,) = nc.row_cases("outlier", D, in_f16)
    D = case.D
    big = case.x.abs() > 100
    for r in range(case.rows):
        cols = torch.nonzero(big[r]).flatten().tolist()
        want = [c for c in (case.desc["first"][r], None if case.desc["last"][r] is None else D - 4 + case.desc["last"][r]) if c is not None]
        assert cols == want and all(c < 4 or c >= D - 4 for c in cols), (r, cols)
        assert sorted(case.x[r, cols].abs().tolist(), reverse=True) == [abs(o) for o in nc.OUTLIERS][:len(cols)] or len(cols) == 1
    assert any(case.desc["first"][r] is not None and case.desc["last"][r] is not None for r in range(case.rows))
    assert bool(big[:, :4].any()) and bool(big[:, D - 4:].any()) and not bool(big[:, 4:D - 4].any())
    # the last valid float4 belongs to lane (D / 4 - 1) % 64, register (D / 4 - 1) / 64: lane 0's third register at D = 516
    nv = D // 4
    if D == 516:
        assert ((nv - 1) % 64, (nv - 1) // 64) == (0, 2)


@pytest.mark.parametrize("D", nc.ROW_DIMS)
def test_constant_tiny_large_mixed_rows(D):
    (const,) = nc.row_cases("constant", D)
    g, b = nc.affine(D)
    assert const.x[:, 0].tolist() == [float(np.float32(c)) for c in nc.CONSTANTS] and bool((const.x == const.x[:, :1]).all())
    assert bool((nc.ln64(const.x, g, b, const.eps) == b.double()).all())                       # the reference of a constant row is exactly beta
    want = torch.tensor([abs(float(np.float32(c))) for c in nc.CONSTANTS], dtype=torch.float64) / np.sqrt(const.eps)
    assert torch.allclose(nc.cond_row(const.x, const.eps).flatten(), want, rtol=1e-12)
    (tiny,) = nc.row_cases("tiny", D)
    assert float(tiny.x.abs().max()) < 1e-29 and float(tiny.x.abs().min()) > 0
    assert bool(((tiny.x * tiny.x) == 0).all())                                                # squares underflow: eps alone sets the scale
    (large,) = nc.row_cases("large", D)
    assert 1e4 < float(large.x.abs().max()) <= 6e4
    (mixed,) = nc.row_cases("mixed", D)
    assert mixed.rows == 7 and bool((mixed.x[6] == 0).all()) and bool((mixed.x[3] == mixed.x[3, 0]).all())
    assert abs(float(mixed.x[0].mean()) - 1e3) < 1 and abs(float(mixed.x[1].mean()) + 1e4) < 1 and float(mixed.x[2].abs().max()) == 300
    for case in (const, tiny, large, mixed):
        assert case.rows in (5, 6, 7)


@pytest.mark.parametrize("D", nc.ROW_DIMS)
def test_fp16_grid_rows(D):
    (case,) = nc.row_cases("fp16_grid", D, in_f16=True)
    x = case.x
    assert bool((x == x.half().float()).all()) and case.rows == 6
    assert bool(((x[:2] * 2) == (x[:2] * 2).round()).all()) and float((x[:2] - 1000).abs().max()) < 6           # spacing 0.5 at 1000
    sub = x[2:4].abs()
    assert bool(((sub < 2.0 ** -14) & (sub > 0)).any()) and float(sub.max()) < 1e-3                               # fp16 subnormals among them
    assert sorted(x[4][x[4].abs() > 1e4].tolist()) == [float(torch.tensor(-3e4).half()), float(torch.tensor(3e4).half())]
    with pytest.raises(AssertionError):
        nc.row_cases("fp16_grid", D, in_f16=False)


@pytest.mark.parametrize("B,M,C", nc.IMAGE_SHAPES)
def test_image_cases_have_their_chunks(B, M, C):
    n = M * C
    nch = nc.n_chunks(M, C)
    assert nch == {(2, 37, 516): 5, (1, 257, 1024): 65, (3, 1, 8): 1}[(B, M, C)]
    last = n - (nch - 1) * nc.GLN_CHUNK
    assert last == {(2, 37, 516): 2708, (1, 257, 1024): 1024, (3, 1, 8): 8}[(B, M, C)]
    (step,) = nc.image_cases("step", B, M, C)
    flat = step.x.reshape(B, n)
    assert bool((flat[:, n - 4:] == 900).all()) and float(flat[:, :n - 4].abs().max()) < 60
    third = step.desc["third"]
    for b in range(B):
        part = nc.chunk_partials_f32(flat[b].numpy())
        assert part.shape == (nch, 3) and part[:, 0].tolist() == [float(nc.GLN_CHUNK)] * (nch - 1) + [float(last)]
        if nch > 1:
            assert third % nc.GLN_CHUNK != 0                                                   # the step is not chunk-aligned
            assert float(part[0, 1]) - float(part[nch - 2, 1]) >= 60                           # chunk means at least 60 apart
            assert abs(float(part[nch - 1, 1]) - (-20 + 920 * 4 / last)) < 0.2                 # the ragged last chunk carries the four 900s
    (off,) = nc.image_cases("offset", B, M, C)
    assert bool(((nc.cond_image(off.x, 1e-5) / 1e3 - 1).abs() < (0.1 if n > 8 else 0.6)).all())
    (per,) = nc.image_cases("per_image", B, M, C)
    for b in range(B):
        assert abs(float(per.x[b].mean()) - per.desc["offsets"][b]) < 0.6 * per.desc["scales"][b] * (1 if n > 8 else 2)
    consts = nc.image_cases("constant", B, M, C)
    assert [c.desc["c"] for c in consts] == list(nc.IMAGE_CONSTANTS)
    for c in consts:
        assert bool((c.x == c.desc["c"]).all())
        for eps, l2_eps in nc.IMAGE_EPS:
            assert bool((nc.gln64(c.x, eps, l2_eps) == 0).all()) and bool((nc.gln_f32(c.x, eps, l2_eps) == 0).all())


@pytest.mark.parametrize("D", nc.ROW_DIMS)
def test_l2_cases(D):
    (dom,) = nc.l2_cases("dominant", D)
    for r, c in enumerate(dom.desc["cols"]):
        assert abs(float(dom.x[r, c])) == 1e3 and int((dom.x[r].abs() > 1).sum()) == 1
    unit = nc.l2_64(dom.x, 0.0) * 1024                                                         # UNIT_NORM_SCALE = 2^10
    hi = unit.float().half()
    lo = (unit.float() - hi.float()).half()
    assert float(((lo.float().abs() < 2.0 ** -14) & (lo != 0)).float().mean()) > 0.5            # the lo plane is subnormal for most columns
    assert [c.desc["scale"] for c in nc.l2_cases("scaled", D)] == [1e-3, 1.0, 1e3]
    (zero,) = nc.l2_cases("zero", D)
    for r in zero.desc["zero_rows"]:
        assert bool((zero.x[r] == 0).all())
        assert bool(torch.isnan(nc.l2_64(zero.x, 0.0)[r]).all()) and bool((nc.l2_64(zero.x, 1e-7)[r] == 0).all())
        assert bool(torch.isnan(nc.l2_rows_f32(zero.x, 0.0)[r]).all()) and bool((nc.l2_rows_f32(zero.x, 1e-7)[r] == 0).all())


def test_cancelling_parts_sum_to_the_structured_row():
    row = nc.row_cases("mixed", 192)[0].x
    for n_parts in (1, 2, 3, 4):
        parts = nc.cancelling_parts(row, n_parts, 9)
        assert parts.shape == (n_parts,) + row.shape and parts.dtype == torch.float32
        x = nc.plane_sum(parts)
        if n_parts > 1:
            assert float(parts[0].abs().mean()) > 500 and bool((parts[0] * parts[1] <= 0).float().mean() > 0.7)
        assert float((x - row).abs().max()) <= 1e-2                       # the roundings at |big| ~ 4e3 and the small planes (randn * 1e-3)
        assert bool(((nc.cond_row(x, 1e-5) / nc.cond_row(row, 1e-5))[:2] - 1).abs().max() < 0.01)


# ------------------------------------------------------------------------------------------------------------ 2. honest reference
@pytest.mark.parametrize("in_f16", [False, True])
@pytest.mark.parametrize("D", nc.ROW_DIMS)
def test_float32_row_restatement_within_half_tolerance(D, in_f16):
    worst = 0.0
    for case in nc.all_row_cases(D, in_f16):
        r = _row_ratio(case)
        assert r < 0.5, (case.name, r)
        worst = max(worst, r)
    print(f"rows D={D} in_f16={in_f16}: restatement at most {worst:.3f} of the bound")


@pytest.mark.parametrize("D", nc.ROW_DIMS)
def test_float32_chained_restatement_within_half_tolerance(D):
    """The chained LayerNorm of zh_sum_layernorm_f32 on a badly conditioned y (gamma1 ~ 0.01, beta1 ~ 50 + noise: mean / std of y about 50)."""
    g1, b1, g2, b2 = nc.chain_affine(D)
    for ci, case in enumerate(nc.sum_cases(D)):
        for n_parts in (1, 2, 3, 4):
            x = nc.plane_sum(*nc.sum_operands(case, n_parts, ci))
            y = nc.ln64(x, g1, b1, 1e-5)
            z = nc.ln64(y, g2, b2, 1e-6)
            tol1 = nc.row_bound(x, g1, 1e-5, y, nc.TOL_SUM_F32)
            y32 = nc.ln_rows_f32(x, g1, b1, 1e-5)
            z32 = nc.ln_rows_f32(y32, g2, b2, 1e-6)
            assert _ratio(y32, y, tol1) < 0.5 and _ratio(z32, z, nc.chain_bound(y, g2, 1e-6, tol1)) < 0.5, (case.name, n_parts)
            assert float(nc.cond_row(y, 1e-6).min()) > 20


@pytest.mark.parametrize("B,M,C", nc.IMAGE_SHAPES)
def test_float32_image_restatement_within_half_tolerance(B, M, C):
    for case in nc.all_image_cases(B, M, C):
        for eps, l2_eps in nc.IMAGE_EPS:
            r = _image_ratio(case.x, eps, l2_eps)
            assert r < 0.5, (case.name, l2_eps, r)


@pytest.mark.parametrize("D", nc.ROW_DIMS)
def test_float32_l2_restatement_within_half_tolerance(D):
    for case in nc.all_l2_cases(D):
        for eps in (0.0, 1e-7):
            ref = nc.l2_64(case.x, eps)
            assert _ratio(nc.l2_rows_f32(case.x, eps), ref, nc.TOL_L2_F32[0] + nc.TOL_L2_F32[1] * ref.abs()) < 0.5, (case.name, eps)


# ------------------------------------------------------------------------------------------------------------ 3. the cases discriminate
@pytest.mark.parametrize("D", nc.ROW_DIMS)
def test_one_pass_variance_is_caught_by_offset_rows_only(D):
    assert min(_row_ratio(c, "one_pass") for c in nc.row_cases("offset", D)) > 1              # by every (c, sigma), 7 x to 1e5 x
    assert _benign_row_ratio(D, "one_pass") < 1                                              # randn * 3 + 1 never saw it


@pytest.mark.parametrize("D", nc.ROW_DIMS)
def test_mean_of_the_fp16_rounded_row_is_caught_by_offset_rows(D):
    assert max(_row_ratio(c, "mean_fp16") for c in nc.row_cases("offset", D)) > 1
    if D == 1024:
        assert _benign_row_ratio(D, "mean_fp16") < 1                                         # 0.59; narrower rows average less rounding noise away


@pytest.mark.parametrize("in_f16", [False, True])
@pytest.mark.parametrize("D", nc.ROW_DIMS)
def test_a_last_float4_left_out_is_caught_by_outlier_rows(D, in_f16):
    (case,) = nc.row_cases("outlier", D, in_f16)
    assert _row_ratio(case, "drop_last_float4") > 1e3


def test_unweighted_chunk_mean_is_caught_by_step_images():
    for shape, least in (((2, 37, 516), 500), ((1, 257, 1024), 50)):
        (step,) = nc.image_cases("step", *shape)
        for eps, l2_eps in nc.IMAGE_EPS:
            assert _image_ratio(step.x, eps, l2_eps, "unweighted") > least
    assert _image_ratio(nc.benign_image(1, 257, 1024), 1e-5, 1e-7, "unweighted", flat_only=True) < 2   # 1.75: benign data at the tolerance itself


def test_dropped_between_chunk_term_shows_only_with_l2_eps_one():
    for shape in nc.IMAGE_SHAPES[:2]:
        (step,) = nc.image_cases("step", *shape)
        assert _image_ratio(step.x, 1e-5, 1.0, "no_between") > 100
        assert _image_ratio(step.x, 1e-5, 1e-7, "no_between") < 0.5                            # rstd cancels: why the second setting exists
        for l2_eps in (1e-7, 1.0):
            assert _image_ratio(nc.benign_image(*shape), 1e-5, l2_eps, "no_between", flat_only=True) < 1


def test_chunk_count_capped_at_64_is_caught_at_65_chunks():
    (step,) = nc.image_cases("step", 1, 257, 1024)
    for eps, l2_eps in nc.IMAGE_EPS:
        assert _image_ratio(step.x, eps, l2_eps, "cap64") > 10
        assert _image_ratio(nc.benign_image(1, 257, 1024), eps, l2_eps, "cap64", flat_only=True) < 1
    (small,) = nc.image_cases("step", 2, 37, 516)
    assert _image_ratio(small.x, 1e-5, 1e-7, "cap64") == _image_ratio(small.x, 1e-5, 1e-7)     # five chunks: nothing to cap
