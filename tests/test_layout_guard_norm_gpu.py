"""-m gpu: the row kernels of norm.hip (one wave per row, four rows per workgroup) through their row-group mappings, inside guard bands
(tests/_guard.py).

A row kernel has no leading dimension: its layouts are the group mappings row(r) = (r / group_rows) * group_stride + offset + r % group_rows
of input and outputs (ln_post drops the cls row, the decoder stacks layers as [B, L, Q, D]) and the split-pair plane offset.  Here the
rows a mapping skips are guard bytes: 0xFF = NaN on the input side (a row read from the wrong place shows in the values), 0xA5 on the output
side (a skipped row that is written, or a row group's fourth wave that stores past `rows`, is reported by assert_untouched()).

References: float64 LayerNorm from the logical rows; for the fp16-input form from the fp16-rounded input.  Tolerances are those of
test_layernorm, test_sum_layernorm, test_assemble_tokens_ln and test_l2norm_and_global_ln; guard comparisons are exact.
"""
import pytest
import torch
import torch.nn.functional as F

from tests._guard import IN_FILL, OUT_FILL, Arena, assert_close, assert_equal, assert_untouched

pytestmark = pytest.mark.gpu

f16, f32, f64 = torch.float16, torch.float32, torch.float64
ROW_GROUP = 4                                                    # rows per workgroup: the trailing guard of every row view


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def rows_view(arena, name, dtype, G, group_rows, group_stride, offset, D, planes=1, skip_first=False):
    """The rows a mapping (group_rows, group_stride, offset) touches for r = 0 .. G * group_rows - 1 (minus each group's first row when
    skip_first) as a guard view [G, rows per group, D]; returns (view, back) with `back` = elements from the BUFFER pointer the kernel is
    handed to the view's base (view.origin(back) is that pointer)."""
    first = 1 if skip_first else 0
    back = (offset + first) * D
    assert back >= 0
    isz = 2 if dtype == f16 else 4
    M = group_rows - first
    inner = (G - 1) * group_stride * D + M * D
    v = arena.add(name, dtype, M, D, batch=G, bstride=group_stride * D, planes=planes, plane=inner + 40, lead=back * isz, tail_rows=ROW_GROUP)
    return v, back


def _ln64(x, g, b, eps):
    return F.layer_norm(x.double(), (x.shape[-1],), None if g is None else g.double(), None if b is None else b.double(), eps)


# rows % 4 in {1, 2, 3}: (groups B, tokens T) -> B * (T - 1) mapped rows
SHAPES = [(3, 8), (2, 6), (3, 6)]


@pytest.mark.parametrize("in_f16", [False, True])
@pytest.mark.parametrize("D", [8, 192, 516, 1024])
def test_layernorm_group_mappings(dev, D, in_f16):
    """zh_layernorm_f32 / zh_layernorm_f16 (D = 520 in place of 516: the fp16 form needs D % 8 == 0): all four outputs through the drop-cls
    input mapping and the stacked output mapping, split-pair fp16 outputs with padded planes, rows % 4 in {1, 2, 3}; then the identity
    mapping with plain fp16 outputs and no affine.  Skipped output rows keep 0xA5; the cls rows of the input are NaN."""
    from zutis_amd import ops
    if in_f16 and D == 516:
        D = 520
    xdt = f16 if in_f16 else f32
    for (B, T), split in zip(SHAPES, (True, True, False)):
        rows = B * (T - 1)
        assert rows % 4 in (1, 2, 3)
        ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
        vx, xback = rows_view(ia, "x", xdt, B, T - 1, T, 1, D)                                   # in_row = (r / (T-1)) * T + 1 + r % (T-1)
        vg, vb = ia.add("gamma", f32, 1, D, tail_rows=0), ia.add("beta", f32, 1, D, tail_rows=0)
        vadd = ia.add("add", f32, T - 1, D, tail_rows=ROW_GROUP)
        omap = dict(G=B, group_rows=T - 1, group_stride=2 * (T - 1), offset=T - 1, D=D)          # second half of every [2, T-1] block
        (o32, back), (o16, _), (p16, _), (p32, _) = (rows_view(oa, "out_f32", f32, **omap), rows_view(oa, "out_f16", f16, planes=2 if split else 1, **omap),
                                                     rows_view(oa, "out_f16_plus", f16, planes=2 if split else 1, **omap), rows_view(oa, "out_f32_plus", f32, **omap))
        x = (_randn((B, T - 1, D), 31 + D) * 3 + 1).to(xdt)
        g, b, add = _randn((D,), 32) * 0.1 + 1, _randn((D,), 33) * 0.1, _randn((T - 1, D), 34)
        vx.put(x); vg.put(g); vb.put(b); vadd.put(add)
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
        ops.layernorm(vx.origin(xback), vg.m2.reshape(-1), vb.m2.reshape(-1), 1e-5, rows, D, out_f32=o32.origin(back), out_f16=o16.origin(back),
                      out_f16_plus=p16.origin(back), out_f32_plus=p32.origin(back), add=vadd.m2, add_rows=T - 1,
                      in_group_rows=T - 1, in_group_stride=T, in_offset=1, out_group_rows=T - 1, out_group_stride=2 * (T - 1), out_offset=T - 1,
                      status=status)
        ref = _ln64(x.float(), g, b, 1e-5)
        refp = ref + add.double()
        what = f"layernorm D={D} in_f16={in_f16} B={B} T={T} split={split}"
        assert_close(o32.pair(), ref, 2e-5, 1e-5, what + " out_f32")
        assert_close(o16.get()[0], ref, 4e-3, 2e-3, what + " out_f16")
        assert_close(p32.pair(), refp, 2e-5, 1e-5, what + " out_f32_plus")
        assert_close(p16.get()[0], refp, 6e-3, 2e-3, what + " out_f16_plus")
        if split:                                                # hi + lo: the fp32 value to 22 bits
            assert_close(o16.pair(), ref, 2e-5, 1e-5, what + " out_f16 pair")
            assert_close(p16.pair(), refp, 2e-5, 1e-5, what + " out_f16_plus pair")
        assert int(status.item()) == 0
        assert_untouched(oa)
        assert_untouched(ia)
    # identity mapping, no affine, one output at a time (the others NULL)
    for rows in (1, 5, 6, 7):
        ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
        vx = ia.add("x", xdt, rows, D, tail_rows=ROW_GROUP)
        o32, o16 = oa.add("out_f32", f32, rows, D, tail_rows=ROW_GROUP), oa.add("out_f16", f16, rows, D, tail_rows=ROW_GROUP)
        x = (_randn((rows, D), 41 + D) * 3 + 1).to(xdt)
        vx.put(x)
        ops.layernorm(vx.m2, None, None, 1e-6, rows, D, out_f32=o32.m2)
        ops.layernorm(vx.m2, None, None, 1e-6, rows, D, out_f16=o16.m2)
        ref = _ln64(x.float(), None, None, 1e-6)
        assert_close(o32.m2, ref, 2e-5, 1e-5, f"layernorm identity D={D} rows={rows} f32")
        assert_close(o16.m2, ref, 4e-3, 2e-3, f"layernorm identity D={D} rows={rows} f16")
        assert_untouched(oa)


@pytest.mark.parametrize("n_parts", [1, 2, 3, 4])
@pytest.mark.parametrize("D", [8, 192, 516, 1024])
def test_sum_layernorm_padded_planes_and_mappings(dev, D, n_parts):
    """zh_sum_layernorm_f32: n_parts fp32 planes at part_stride > rows * D (the space between planes is NaN) + bias + residual -> out_sum
    (bitwise the fp32 sum in the stated order; in place over the residual in every other case), LN -> fp32 / split pair with
    skip_first_in_group through ln_post's dense drop-first mapping (a skipped row shares its address with the previous group's last row) and
    through two gapped mappings in which every skipped row is a sentinel row that must keep 0xA5, chained second LN -> fp32 / split pair with the stacked mapping."""
    from zutis_amd import ops
    for ci, (B, T) in enumerate(((3, 7), (2, 5), (3, 5))):         # rows % 4 = 1, 2, 3
        rows = B * T
        ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
        vparts = ia.add("parts", f32, rows, D, batch=n_parts, bstride=rows * D + 12, tail_rows=ROW_GROUP)
        vbias = ia.add("bias", f32, 1, D, tail_rows=0)
        vg1, vb1, vg2, vb2 = (ia.add(n, f32, 1, D, tail_rows=0) for n in ("gamma", "beta", "gamma2", "beta2"))
        in_place = ci % 2 == 0
        vres = None if in_place else ia.add("residual", f32, rows, D, tail_rows=ROW_GROUP)
        vsum = oa.add("out_sum", f32, rows, D, tail_rows=ROW_GROUP)
        # ln_post's dense drop-first map, out_row = (r / T) * (T-1) - 1 + r % T: the skipped row of group g >= 1 has the address of group
        # g - 1's last row, only group 0's lies in a guard.  The gapped map (stride T, offset 0) makes EVERY skipped row a sentinel row.
        gs1, off1 = ((T - 1, -1), (T, 0), (T + 2, 3))[ci]
        m1 = dict(G=B, group_rows=T, group_stride=gs1, offset=off1, D=D, skip_first=True)
        (y32, yb), (y16, _) = rows_view(oa, "out_f32", f32, **m1), rows_view(oa, "out_f16", f16, planes=2, **m1)
        m2 = dict(G=B, group_rows=T, group_stride=2 * T, offset=T, D=D)
        (z32, zb), (z16, _) = rows_view(oa, "out2_f32", f32, **m2), rows_view(oa, "out2_f16", f16, planes=2, **m2)
        parts = _randn((n_parts, rows, D), 80 + D)
        bias, res = _randn((D,), 81), _randn((rows, D), 82) * 3 + 0.5
        g1, b1, g2, b2 = _randn((D,), 83) * 0.1 + 1, _randn((D,), 84) * 0.1, _randn((D,), 85) * 0.2 + 1, _randn((D,), 86) * 0.1
        vparts.put(parts); vbias.put(bias); vg1.put(g1); vb1.put(b1); vg2.put(g2); vb2.put(b2)
        (vsum if in_place else vres).put(res)
        x = parts[0].clone()
        for s in range(1, n_parts):
            x = x + parts[s]
        x = (x + bias) + res                                     # the kernel's order: fp32, plane order, bias, residual
        y = _ln64(x, g1, b1, 1e-5)
        z = _ln64(y, g2, b2, 1e-6)
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
        ops.sum_layernorm(vparts.hi, n_parts, rows, D, part_stride=vparts.bstride, bias=vbias.m2.reshape(-1),
                          residual=(vsum if in_place else vres).m2, out_sum=vsum.m2,
                          gamma=vg1.m2.reshape(-1), beta=vb1.m2.reshape(-1), eps=1e-5, out_f32=y32.origin(yb), out_f16=y16.origin(yb),
                          out_group_rows=T, out_group_stride=gs1, out_offset=off1, skip_first_in_group=True,
                          gamma2=vg2.m2.reshape(-1), beta2=vb2.m2.reshape(-1), eps2=1e-6, out2_f32=z32.origin(zb), out2_f16=z16.origin(zb),
                          out2_group_rows=T, out2_group_stride=2 * T, out2_offset=T, status=status)
        what = f"sum_layernorm D={D} n_parts={n_parts} B={B} T={T} in_place={in_place}"
        assert_equal(vsum.m2, x, what + " out_sum")
        ydrop = y.view(B, T, D)[:, 1:]
        assert_close(y32.pair(), ydrop, 2e-5, 0.0, what + " out_f32")
        assert_close(y16.pair(), ydrop, 2e-5, 0.0, what + " out_f16 pair")
        assert_equal(y16.get()[0], y32.get()[0].to(f16), what + " out_f16 hi plane is the rounded fp32 output")
        assert_close(z32.pair(), z.view(B, T, D), 4e-5, 0.0, what + " out2_f32")
        assert_close(z16.pair(), z.view(B, T, D), 4e-5, 0.0, what + " out2_f16 pair")
        assert int(status.item()) == 0
        assert_untouched(oa)
        assert_untouched(ia)


@pytest.mark.parametrize("out_f16", [False, True])
@pytest.mark.parametrize("D", [8, 192, 516, 1024])
def test_assemble_tokens_ln(dev, D, out_f16):
    """zh_assemble_tokens_ln / _f16: cat(cls, patches) + pos -> ln_pre, B * T % 4 in {1, 2, 3}, with gamma / beta and with gamma = None (no
    LayerNorm: DINO's prepare_tokens)."""
    from zutis_amd import ops
    for B, hw in ((2, 6), (3, 4), (3, 2)):
        T = 1 + hw
        for affine in (True, False):
            ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
            vpe, vcls, vpos = ia.add("patch_emb", f32, B * hw, D, tail_rows=ROW_GROUP), ia.add("cls", f32, 1, D, tail_rows=0), ia.add("pos", f32, T, D, tail_rows=ROW_GROUP)
            vg, vb = ia.add("gamma", f32, 1, D, tail_rows=0), ia.add("beta", f32, 1, D, tail_rows=0)
            vo = oa.add("out", f16 if out_f16 else f32, B * T, D, tail_rows=ROW_GROUP)
            pe, cls, pos = _randn((B * hw, D), 41), _randn((D,), 42), _randn((T, D), 43)
            g, b = _randn((D,), 44) * 0.1 + 1, _randn((D,), 45) * 0.1
            vpe.put(pe); vcls.put(cls); vpos.put(pos); vg.put(g); vb.put(b)
            ops.assemble_tokens_ln(vpe.m2, vcls.m2.reshape(-1), vpos.m2, vg.m2.reshape(-1) if affine else None, vb.m2.reshape(-1) if affine else None,
                                   1e-5, vo.m2.view(B, T, D), B, T, D)
            t = torch.cat([cls[None, None].expand(B, 1, D), pe.view(B, hw, D)], 1).double() + pos.double()[None]
            ref = (_ln64(t, g, b, 1e-5) if affine else t).reshape(B * T, D)
            what = f"assemble_tokens_ln D={D} f16={out_f16} B={B} T={T} affine={affine}"
            if out_f16:
                assert_close(vo.m2, ref, 4e-3, 2e-3, what)          # test_layernorm's fp16-output bound
            else:
                assert_close(vo.m2, ref, 2e-5, 1e-5, what)          # test_assemble_tokens_ln
            assert_untouched(oa)
            assert_untouched(ia)


@pytest.mark.parametrize("D", [8, 192, 516, 1024])
def test_l2norm_rows_eps_and_scaled_pair(dev, D):
    """zh_l2norm_rows with eps > 0 and f16_scale = 1024 (the unit-norm producers): fp32 out, split pair with a padded plane and plain fp16."""
    from zutis_amd import ops
    for rows in (1, 5, 6, 7, 50):
        for planes in (2, 1):
            ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
            vx = ia.add("x", f32, rows, D, tail_rows=ROW_GROUP)
            o32 = oa.add("out_f32", f32, rows, D, tail_rows=ROW_GROUP)
            o16 = oa.add("out_f16", f16, rows, D, planes=planes, plane=rows * D + 20, tail_rows=ROW_GROUP)
            x = _randn((rows, D), 51 + rows)
            vx.put(x)
            ops.l2norm_rows(vx.m2, rows, D, out_f32=o32.m2, out_f16=o16.act(1.0 / ops.UNIT_NORM_SCALE), eps=1e-7)
            ref = x.double() / (x.double().norm(dim=-1, keepdim=True) + 1e-7)
            what = f"l2norm_rows D={D} rows={rows} planes={planes}"
            assert_close(o32.m2, ref, 1e-6, 1e-5, what + " f32")                               # test_l2norm_and_global_ln
            assert_close(o16.get()[0, 0].double() / ops.UNIT_NORM_SCALE, ref, 1e-3, 1e-5, what + " f16")
            if planes == 2:
                assert_close(o16.pair()[0] / ops.UNIT_NORM_SCALE, ref, 1e-6, 1e-5, what + " pair")
            assert_untouched(oa)
            assert_untouched(ia)


@pytest.mark.parametrize("B,M,C", [(2, 10, 64), (1, 4, 1024), (3, 37, 516), (2, 9, 1024), (1, 1, 8)])
def test_global_ln_l2_workspace_exact(dev, B, M, C):
    """zh_global_ln_l2: per-image volumes of one 4096-float chunk (640, exactly 4096, 8 floats) and of several with a ragged last one
    (19092 = 4.66 chunks, 9216 = 2.25), M % 4 in {0, 1, 2}; the workspace EXACTLY zh_global_ln_l2_workspace_size bytes between guards."""
    from zutis_amd import ops
    need = ops.global_ln_l2_workspace_size(B, M, C)
    ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
    vx = ia.add("x", f32, M, C, batch=B, tail_rows=ROW_GROUP)
    o32 = oa.add("out_f32", f32, M, C, batch=B, tail_rows=ROW_GROUP)
    o16 = oa.add("out_f16", f16, M, C, batch=B, planes=2, plane=B * M * C + 12, tail_rows=ROW_GROUP)
    ws = oa.workspace("workspace", need)
    x = _randn((B, M, C), 52) * 2 + 0.3
    vx.put(x)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ops.global_ln_l2(vx.hi, B, M, C, out_f32=o32.hi, out_f16=o16.origin(0), workspace=ws.t.reshape(-1), status=status)
    xd = x.double()
    ref = F.layer_norm(xd, xd.shape[1:], eps=1e-5)
    ref = ref / (ref.norm(dim=-1, keepdim=True) + 1e-7)
    what = f"global_ln_l2 B={B} M={M} C={C} workspace={need}"
    assert_close(o32.hi, ref, 2e-6, 1e-5, what + " f32")                                       # test_l2norm_and_global_ln
    assert_close(o16.get()[0], ref, 1e-3, 1e-5, what + " f16")
    assert int(status.item()) == 0
    assert_untouched(oa)
    assert_untouched(ia)
