"""-m gpu: the arithmetic of norm.hip on structured rows and images (tests/_norm_case.py) against float64.

zh_layernorm_f32 / _f16, zh_sum_layernorm_f32 (split-K combine, first and chained LayerNorm), zh_assemble_tokens_ln / _f16, zh_l2norm_rows and
zh_global_ln_l2 on rows with a common offset, outlier channels in the first and the last valid float4, constant / zero / tiny / large rows,
rows on the fp16 grid, and images whose chunks differ in mean.  Everything runs in the guard-banded arenas of tests/_guard.py through the
row views of test_layout_guard_norm_gpu.py; every call is followed by assert_untouched on both arenas and the status word is 0 on every
finite case.  The bounds are the project's flat tolerances plus the derived conditioning term of _norm_case.py (its docstring has the
derivation); tests/test_norm_structured_cpu.py shows that a float32 restatement stays under half of them and that wrong kernels do not.

Largest |out - float64| observed on an MI355X and the largest share of the element's bound it reached (a record, not a threshold; maxima
over D / the image shapes and over the mapped and identity launches):
  entry / family                   fp32 out and split pairs       plain fp16 out
  layernorm        offset           1.5e-03  (0.21 of its bound)   2.1e-03  (0.15)
  layernorm        outlier          4.0e-06  (0.01)                7.7e-03  (0.16)
  layernorm        constant         2.5e-02  (0.10)                2.5e-02  (0.09)     c = 1000.1: the bound is 0.23 there
  layernorm        tiny             3.5e-07  (0.01)                9.7e-04  (0.09)
  layernorm        large            8.9e-07  (0.01)                2.0e-03  (0.15)
  layernorm        mixed            2.5e-02  (0.09)                2.5e-02  (0.17)
  layernorm        fp16_grid        1.8e-05  (0.02)                7.2e-03  (0.17)
  sum_layernorm    first LN         7.0e-05  (0.13; pair 0.29)     —                   y ~ 50: the pair's lo half rounds at 7.6e-6
  sum_layernorm    chained LN       3.0e-05  (0.10)                —
  assemble_tokens  ln_pre           4.2e-03  (0.15, both output types)                 cat + pos alone: bitwise (fp32), 0.25 at |t| ~ 1e3 (fp16, 0.13)
  l2norm_rows      dominant         3.0e-08  (0.003)               5.4e-08  (0.000)
  l2norm_rows      scaled / zero    1.0e-07  (0.02)                2.4e-04  (0.24)
  global_ln_l2     step             5.5e-08  (0.02)                1.1e-04  (0.11)     both l2_eps settings
  global_ln_l2     offset           1.4e-05  (0.05)                1.6e-04  (0.12)     (3, 1, 8): cond_image 1.3e3 over sqrt(8)
  global_ln_l2     per_image        2.7e-06  (0.05)                2.2e-04  (0.22)
  global_ln_l2     constant         exactly 0 in every output, both settings
No case exceeded its bound; the conditioning term was reached to at most 2.6 / 12 (offset rows).
"""
import pytest
import torch

from tests import _norm_case as nc
from tests._guard import IN_FILL, OUT_FILL, Arena, assert_equal, assert_untouched, assert_within
from tests.test_layout_guard_norm_gpu import ROW_GROUP, rows_view

pytestmark = pytest.mark.gpu

f16, f32, f64 = torch.float16, torch.float32, torch.float64
GROUPS = {5: (1, 5), 6: (2, 3), 7: (7, 1)}                       # rows -> (groups, rows per group) of the row mappings


class _Record:
    """assert_within per output, the largest |out - float64| and the largest share of its bound kept per (family, output) and printed."""

    def __init__(self, what):
        self.what, self.worst = what, {}

    def check(self, family, output, got, ref, bound, what):
        got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).double()
        share = assert_within(got, ref, bound, what)
        e, s = self.worst.get((family, output), (0.0, 0.0))
        self.worst[(family, output)] = (max(e, float((got - ref).abs().max())), max(s, share))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for (family, output), (e, s) in sorted(self.worst.items()):
            print(f"{self.what} {family:10s} {output:14s} max |out - float64| {e:.1e}  ({s:.3f} of its bound)")
        return False


def _status(dev):
    return torch.zeros((1,), dtype=torch.int32, device=dev)


@pytest.mark.parametrize("in_f16", [False, True])
@pytest.mark.parametrize("D", nc.ROW_DIMS)
def test_layernorm_structured_rows(dev, D, in_f16):
    """Every row family: all four outputs as split pairs through the drop-cls input mapping and the stacked output mapping with gamma, beta
    and add; then the identity mapping without affine, fp32 and plain fp16 output."""
    from zutis_amd import ops
    xdt = f16 if in_f16 else f32
    cases = nc.all_row_cases(D, in_f16)
    assert {c.family for c in cases} == set(nc.ROW_FAMILIES) | ({"fp16_grid"} if in_f16 else set())
    with _Record(f"layernorm D={D} in_f16={in_f16}") as rec:
        for case in cases:
            D, rows, x, eps = case.D, case.rows, case.x, case.eps
            B, R = GROUPS[rows]
            T = R + 1
            assert rows % 4 in (1, 2, 3)
            ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
            vx, xback = rows_view(ia, "x", xdt, B, R, T, 1, D)                                   # the cls row of every group is NaN
            vg, vb = ia.add("gamma", f32, 1, D, tail_rows=0), ia.add("beta", f32, 1, D, tail_rows=0)
            vadd = ia.add("add", f32, R, D, tail_rows=ROW_GROUP)
            omap = dict(G=B, group_rows=R, group_stride=2 * R, offset=R, D=D)
            (o32, back), (o16, _), (p16, _), (p32, _) = (rows_view(oa, "out_f32", f32, **omap), rows_view(oa, "out_f16", f16, planes=2, **omap),
                                                         rows_view(oa, "out_f16_plus", f16, planes=2, **omap), rows_view(oa, "out_f32_plus", f32, **omap))
            (g, b), add = nc.affine(D), nc.randn((R, D), 34)
            vx.put(x.view(B, R, D)); vg.put(g); vb.put(b); vadd.put(add)
            assert bool((vx.get()[0].float().reshape(rows, D) == x).all())                       # the operand is the case, bit for bit
            status = _status(dev)
            ops.layernorm(vx.origin(xback), vg.m2.reshape(-1), vb.m2.reshape(-1), eps, rows, D, out_f32=o32.origin(back), out_f16=o16.origin(back),
                          out_f16_plus=p16.origin(back), out_f32_plus=p32.origin(back), add=vadd.m2, add_rows=R,
                          in_group_rows=R, in_group_stride=T, in_offset=1, out_group_rows=R, out_group_stride=2 * R, out_offset=R, status=status)
            ref = nc.ln64(x, g, b, eps).view(B, R, D)
            refp = ref + add.double()[None]
            xg = x.view(B, R, D)
            bound = lambda r, flat: nc.row_bound(xg, g, eps, r, flat)
            fam = case.family
            rec.check(fam, "out_f32", o32.pair(), ref, bound(ref, nc.TOL_F32), case.name + " out_f32")
            rec.check(fam, "out_f16 pair", o16.pair(), ref, bound(ref, nc.TOL_F32), case.name + " out_f16 pair")
            rec.check(fam, "out_f16 hi", o16.get()[0], ref, bound(ref, nc.TOL_F16), case.name + " out_f16 hi")
            rec.check(fam, "out_f32_plus", p32.pair(), refp, bound(refp, nc.TOL_F32), case.name + " out_f32_plus")
            rec.check(fam, "plus pair", p16.pair(), refp, bound(refp, nc.TOL_F32), case.name + " out_f16_plus pair")
            rec.check(fam, "plus hi", p16.get()[0], refp, bound(refp, nc.TOL_F16_PLUS), case.name + " out_f16_plus hi")
            assert int(status.item()) == 0, case.name
            assert_untouched(oa)
            assert_untouched(ia)
            # identity mapping, no affine, one output at a time
            ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
            vx = ia.add("x", xdt, rows, D, tail_rows=ROW_GROUP)
            o32, o16 = oa.add("out_f32", f32, rows, D, tail_rows=ROW_GROUP), oa.add("out_f16", f16, rows, D, tail_rows=ROW_GROUP)
            vx.put(x)
            status = _status(dev)
            ops.layernorm(vx.m2, None, None, eps, rows, D, out_f32=o32.m2, status=status)
            ops.layernorm(vx.m2, None, None, eps, rows, D, out_f16=o16.m2, status=status)
            ref = nc.ln64(x, None, None, eps)
            rec.check(fam, "identity f32", o32.m2, ref, nc.row_bound(x, None, eps, ref, nc.TOL_F32), case.name + " identity f32")
            rec.check(fam, "identity f16", o16.m2, ref, nc.row_bound(x, None, eps, ref, nc.TOL_F16), case.name + " identity f16")
            if fam == "constant":                                                                # float64 gives exactly 0; a zero row must too
                assert bool((o32.m2[0] == 0).all()) and bool((o16.m2[0] == 0).all())
            assert int(status.item()) == 0, case.name
            assert_untouched(oa)
            assert_untouched(ia)


@pytest.mark.parametrize("n_parts", [1, 2, 3, 4])
@pytest.mark.parametrize("D", nc.ROW_DIMS)
def test_sum_layernorm_cancelling_planes_and_conditioned_chain(dev, D, n_parts):
    """The structured row is the SUM: parts[0] = +big, parts[1] = -big + row, the rest small, + bias + residual.  out_sum is bitwise the fp32
    plane-order sum; the first LayerNorm (gamma1 ~ 0.01, beta1 ~ 50 + noise) goes through a gapped mapping with skip_first_in_group, which
    makes the chained LayerNorm's input y badly conditioned (mean / std about 50)."""
    from zutis_amd import ops
    cases = nc.sum_cases(D)
    g1, b1, g2, b2 = nc.chain_affine(D)
    with _Record(f"sum_layernorm D={D} n_parts={n_parts}") as rec:
        for ci, case in enumerate(cases):
            rows = case.rows
            B, T = GROUPS[rows]
            ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
            vparts = ia.add("parts", f32, rows, D, batch=n_parts, bstride=rows * D + 12, tail_rows=ROW_GROUP)
            vbias = ia.add("bias", f32, 1, D, tail_rows=0)
            vg1, vb1, vg2, vb2 = (ia.add(n, f32, 1, D, tail_rows=0) for n in ("gamma", "beta", "gamma2", "beta2"))
            in_place = ci % 2 == 0
            vres = None if in_place else ia.add("residual", f32, rows, D, tail_rows=ROW_GROUP)
            vsum = oa.add("out_sum", f32, rows, D, tail_rows=ROW_GROUP)
            m1 = dict(G=B, group_rows=T, group_stride=T + 2, offset=3, D=D, skip_first=T > 1)     # every skipped row is a sentinel row
            (y32, yb), (y16, _) = rows_view(oa, "out_f32", f32, **m1), rows_view(oa, "out_f16", f16, planes=2, **m1)
            m2 = dict(G=B, group_rows=T, group_stride=2 * T, offset=T, D=D)
            (z32, zb), (z16, _) = rows_view(oa, "out2_f32", f32, **m2), rows_view(oa, "out2_f16", f16, planes=2, **m2)
            parts, bias, res = nc.sum_operands(case, n_parts, ci)
            vparts.put(parts); vbias.put(bias); vg1.put(g1); vb1.put(b1); vg2.put(g2); vb2.put(b2)
            (vsum if in_place else vres).put(res)
            x = nc.plane_sum(parts, bias, res)                                                  # fp32, plane order, bias, residual
            y = nc.ln64(x, g1, b1, 1e-5)
            z = nc.ln64(y, g2, b2, 1e-6)
            status = _status(dev)
            ops.sum_layernorm(vparts.hi, n_parts, rows, D, part_stride=vparts.bstride, bias=vbias.m2.reshape(-1),
                              residual=(vsum if in_place else vres).m2, out_sum=vsum.m2,
                              gamma=vg1.m2.reshape(-1), beta=vb1.m2.reshape(-1), eps=1e-5, out_f32=y32.origin(yb), out_f16=y16.origin(yb),
                              out_group_rows=T, out_group_stride=T + 2, out_offset=3, skip_first_in_group=T > 1,
                              gamma2=vg2.m2.reshape(-1), beta2=vb2.m2.reshape(-1), eps2=1e-6, out2_f32=z32.origin(zb), out2_f16=z16.origin(zb),
                              out2_group_rows=T, out2_group_stride=2 * T, out2_offset=T, status=status)
            what, fam = f"{case.name} n_parts={n_parts} in_place={in_place}", case.family
            assert_equal(vsum.m2, x, what + " out_sum")
            tol1 = nc.row_bound(x, g1, 1e-5, y, nc.TOL_SUM_F32)
            first = 1 if T > 1 else 0
            ydrop, tdrop = y.view(B, T, D)[:, first:], tol1.view(B, T, D)[:, first:]
            rec.check(fam, "out_f32", y32.pair(), ydrop, tdrop, what + " out_f32")
            rec.check(fam, "out_f16 pair", y16.pair(), ydrop, tdrop, what + " out_f16 pair")
            assert_equal(y16.get()[0], y32.get()[0].to(f16), what + " out_f16 hi plane is the rounded fp32 output")
            tol2 = nc.chain_bound(y, g2, 1e-6, tol1).view(B, T, D)
            rec.check(fam, "out2_f32", z32.pair(), z.view(B, T, D), tol2, what + " out2_f32")
            rec.check(fam, "out2_f16 pair", z16.pair(), z.view(B, T, D), tol2, what + " out2_f16 pair")
            assert int(status.item()) == 0, what
            assert_untouched(oa)
            assert_untouched(ia)


@pytest.mark.parametrize("out_f16", [False, True])
@pytest.mark.parametrize("D", nc.ROW_DIMS)
def test_assemble_tokens_offset_pos_and_outlier_cls(dev, D, out_f16):
    """pos_embed with a common offset of 1e3, class_embedding with +300 / -180 in its first and last float4, with and without ln_pre.  The
    row the kernel normalises is fp32(src + pos): the reference is the float64 LayerNorm of that row."""
    from zutis_amd import ops
    with _Record(f"assemble_tokens_ln D={D} f16={out_f16}") as rec:
        for B, hw in ((2, 6), (3, 4), (3, 2)):
            T = 1 + hw
            for affine in (True, False):
                ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
                vpe, vcls, vpos = ia.add("patch_emb", f32, B * hw, D, tail_rows=ROW_GROUP), ia.add("cls", f32, 1, D, tail_rows=0), ia.add("pos", f32, T, D, tail_rows=ROW_GROUP)
                vg, vb = ia.add("gamma", f32, 1, D, tail_rows=0), ia.add("beta", f32, 1, D, tail_rows=0)
                vo = oa.add("out", f16 if out_f16 else f32, B * T, D, tail_rows=ROW_GROUP)
                pe, pos = nc.randn((B * hw, D), 41), nc.randn((T, D), 43) + 1e3
                cls = nc._outlier_row(D, 42, 0, 3)
                g, b = nc.affine(D, 12)
                vpe.put(pe); vcls.put(cls); vpos.put(pos); vg.put(g); vb.put(b)
                ops.assemble_tokens_ln(vpe.m2, vcls.m2.reshape(-1), vpos.m2, vg.m2.reshape(-1) if affine else None, vb.m2.reshape(-1) if affine else None,
                                       1e-5, vo.m2.view(B, T, D), B, T, D)
                t = (torch.cat([cls[None, None].expand(B, 1, D), pe.view(B, hw, D)], 1) + pos[None]).reshape(B * T, D)     # fp32, one rounding
                assert t.dtype == f32 and float(nc.cond_row(t, 1e-5).max()) > 300
                flat = nc.TOL_F16 if out_f16 else nc.TOL_F32
                what = f"assemble_tokens_ln D={D} f16={out_f16} B={B} T={T} affine={affine}"
                if affine:
                    ref = nc.ln64(t, g, b, 1e-5)
                    rec.check("offset pos", "ln_pre", vo.m2, ref, nc.row_bound(t, g, 1e-5, ref, flat), what)
                elif out_f16:
                    rec.check("offset pos", "cat + pos", vo.m2, t.double(), flat[0] + flat[1] * t.double().abs(), what)
                else:
                    assert_equal(vo.m2, t, what)
                assert_untouched(oa)
                assert_untouched(ia)


@pytest.mark.parametrize("D", nc.ROW_DIMS)
def test_l2norm_rows_dominant_scaled_zero(dev, D):
    """eps in {0, 1e-7}, f16_scale = UNIT_NORM_SCALE: fp32, plain fp16 and split pair.  A zero row is exactly 0 with eps = 1e-7 and NaN with
    eps = 0 (x / x.norm() in torch), and leaves its neighbours in the workgroup alone."""
    from zutis_amd import ops
    S = ops.UNIT_NORM_SCALE
    with _Record(f"l2norm_rows D={D}") as rec:
        for case in nc.all_l2_cases(D):
            for eps in (0.0, 1e-7):
                for planes in (2, 1):
                    rows, x = case.rows, case.x
                    ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
                    vx = ia.add("x", f32, rows, D, tail_rows=ROW_GROUP)
                    o32 = oa.add("out_f32", f32, rows, D, tail_rows=ROW_GROUP)
                    o16 = oa.add("out_f16", f16, rows, D, planes=planes, plane=rows * D + 20, tail_rows=ROW_GROUP)
                    vx.put(x)
                    ops.l2norm_rows(vx.m2, rows, D, out_f32=o32.m2, out_f16=o16.act(1.0 / S), eps=eps)
                    ref = nc.l2_64(x, eps)
                    got32, hi = o32.m2.cpu(), o16.get()[0, 0].double() / S
                    zero = list(case.desc.get("zero_rows", ()))
                    keep = [r for r in range(rows) if r not in zero]
                    what = f"{case.name} eps={eps:g} planes={planes}"
                    for r in zero:
                        if eps == 0.0:
                            assert bool(torch.isnan(got32[r]).all()) and bool(torch.isnan(hi[r]).all()), what
                        else:
                            assert bool((got32[r] == 0).all()) and bool((o16.get()[:, 0, r] == 0).all()), what
                    bound = lambda flat: (flat[0] + flat[1] * ref.abs())[keep]
                    rec.check(case.family, "f32", got32[keep], ref[keep], bound(nc.TOL_L2_F32), what + " f32")
                    rec.check(case.family, "f16", hi[keep], ref[keep], bound(nc.TOL_L2_F16), what + " f16")
                    if planes == 2:
                        rec.check(case.family, "pair", (o16.pair()[0] / S)[keep], ref[keep], bound(nc.TOL_L2_F32), what + " pair")
                    assert_untouched(oa)
                    assert_untouched(ia)


@pytest.mark.parametrize("B,M,C", nc.IMAGE_SHAPES)
def test_global_ln_l2_structured_images(dev, B, M, C):
    """4.66 chunks, 65 chunks (the lane-strided combine loops twice) and one short chunk, at the engine's (eps, l2_eps) and at (1e-5, 1.0),
    where the per-image variance does not cancel; the workspace exactly zh_global_ln_l2_workspace_size bytes between guards.  A constant
    image is exactly 0 everywhere."""
    from zutis_amd import ops
    need = ops.global_ln_l2_workspace_size(B, M, C)
    assert need == B * nc.n_chunks(M, C) * 16
    cases = nc.all_image_cases(B, M, C)
    assert {c.family for c in cases} == set(nc.IMAGE_FAMILIES)
    with _Record(f"global_ln_l2 B={B} M={M} C={C}") as rec:
        for case in cases:
            for eps, l2_eps in nc.IMAGE_EPS:
                ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
                vx = ia.add("x", f32, M, C, batch=B, tail_rows=ROW_GROUP)
                o32 = oa.add("out_f32", f32, M, C, batch=B, tail_rows=ROW_GROUP)
                o16 = oa.add("out_f16", f16, M, C, batch=B, planes=2, plane=B * M * C + 12, tail_rows=ROW_GROUP)
                ws = oa.workspace("workspace", need)
                vx.put(case.x)
                status = _status(dev)
                ops.global_ln_l2(vx.hi, B, M, C, out_f32=o32.hi, out_f16=o16.origin(0), eps=eps, l2_eps=l2_eps, workspace=ws.t.reshape(-1), status=status)
                ref = nc.gln64(case.x, eps, l2_eps)
                what, fam = f"{case.name} l2_eps={l2_eps:g}", f"{case.family} l2_eps={l2_eps:g}"
                if case.family == "constant":
                    assert bool((ref == 0).all())
                    assert_equal(o32.hi, torch.zeros(B, M, C), what + " f32")
                    assert_equal(o16.get(), torch.zeros(2, B, M, C, dtype=f16), what + " f16 planes")
                else:
                    rec.check(fam, "f32", o32.hi, ref, nc.image_bound(case.x, eps, ref, nc.TOL_IMG_F32), what + " f32")
                    rec.check(fam, "pair", o16.pair(), ref, nc.image_bound(case.x, eps, ref, nc.TOL_IMG_F32), what + " pair")
                    rec.check(fam, "f16", o16.get()[0], ref, nc.image_bound(case.x, eps, ref, nc.TOL_IMG_F16), what + " f16")
                assert int(status.item()) == 0, what
                assert_untouched(oa)
                assert_untouched(ia)
