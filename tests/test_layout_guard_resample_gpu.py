"""-m gpu: the resampling and glue kernels of resample.hip inside guard bands (tests/_guard.py): every input is surrounded by 0xFF (NaN /
255 / -1), every output by 0xA5, and after each call assert_untouched() proves that only the logical output elements were written.

These kernels take dense tensors: what can go wrong is the flat-index tail (element counts that are not multiples of the 256-thread
workgroup or of the vector width), the clamped taps at the image border (a tap one pixel outside reads NaN here), zero padding that must
be written and not run over, and — for zh_upsample_argmax — a low-resolution LDS window that must cover every tap of its output tile.

Values: integer, u8 and the bit-exact resamplers are compared exactly against oracle/resample.py; the others with the bound of their
existing direct test (test_upsample2x_and_sine, test_posembed_bicubic_vs_golden_and_oracle, test_split_producers_write_hi_plus_lo).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests._guard import IN_FILL, OUT_FILL, Arena, assert_close, assert_equal, assert_untouched, assert_within

pytestmark = pytest.mark.gpu

f16, f32, f64 = torch.float16, torch.float32, torch.float64
i64, u8 = torch.int64, torch.uint8


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _flat(arena, name, dtype, n, planes=1, plane=None, misalign=0):
    """n contiguous elements; the guard behind them is one 256-thread workgroup of 16-byte vectors."""
    return arena.add(name, dtype, 1, n, planes=planes, plane=plane, misalign=misalign, tail_rows=1)


# ------------------------------------------------------------------------------------------------ x2 bilinear, channels last
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("D", [4, 24, 768, 1280])
def test_upsample2x_bilinear_cl(dev, D, relu):
    """h = 1, w = 1, both, and a general shape; D = 4 (one lane), 24, 768, 1280 (320 float4 per pixel: the `c += blockDim.x` loop); fp32 and
    split-pair fp16 outputs with a padded plane."""
    from zutis_amd import ops
    from oracle import resample as R
    for B, h, w in ((2, 1, 1), (1, 1, 5), (1, 4, 1), (2, 3, 5)):
        n_in, n_out = B * h * w * D, B * 4 * h * w * D
        ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
        vx = _flat(ia, "x", f32, n_in)
        o32 = _flat(oa, "out_f32", f32, n_out)
        o16 = _flat(oa, "out_f16", f16, n_out, planes=2, plane=n_out + 12)
        x = _randn((B, h, w, D), 61 + D)
        vx.put(x)
        ops.upsample2x_cl(vx.m2, B, h, w, D, out_f32=o32.m2, out_f16=o16.origin(0), relu=relu)
        ref = torch.from_numpy(R.bilinear_up2_cl(x.numpy())).double()
        ref = F.relu(ref) if relu else ref
        what = f"upsample2x_cl B={B} h={h} w={w} D={D} relu={relu}"
        assert_close(o32.m2.reshape(ref.shape), ref, 1e-6, 0.0, what + " f32")
        assert_close(o16.get()[0].reshape(ref.shape), ref, 4e-3, 0.0, what + " f16")
        assert_close(o16.pair().reshape(ref.shape), ref, 1e-6, 3e-7, what + " pair")      # hi + lo: the fp32 value to 22 bits
        assert_untouched(oa)
        assert_untouched(ia)


# ------------------------------------------------------------------------------------------------ bicubic positional embedding
@pytest.mark.parametrize("has_cls", [0, 1])
@pytest.mark.parametrize("g,h,w,D", [(14, 21, 21, 48), (7, 7, 7, 20), (4, 5, 7, 12), (14, 30, 40, 4)])
def test_posembed_bicubic(dev, g, h, w, D, has_cls):
    from zutis_amd import ops
    from oracle import resample as R
    ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
    vp = _flat(ia, "pos", f32, (g * g + has_cls) * D)
    vo = _flat(oa, "out", f32, (h * w + has_cls) * D)
    pe = _randn((g * g + has_cls, D), 7 + g)
    vp.put(pe)
    ops.posembed_bicubic(vp.m2, vo.m2, g, h, w, D, np.float32(1.0 / ((h + 0.1) / g)), np.float32(1.0 / ((w + 0.1) / g)), has_cls=bool(has_cls))
    got = vo.m2.reshape(h * w + has_cls, D)
    orc = R.bicubic_cl(pe[has_cls:].numpy().reshape(g, g, D), h, w, (h + 0.1) / g, (w + 0.1) / g).reshape(h * w, D)
    assert_close(got[has_cls:], torch.from_numpy(np.ascontiguousarray(orc)), 5e-6, 0.0, f"posembed g={g} {h}x{w} D={D} cls={has_cls}")
    if has_cls:
        assert_equal(got[0], pe[0], "cls row is copied")
    assert_untouched(oa)
    assert_untouched(ia)


# ------------------------------------------------------------------------------------------------ sine PE, row-periodic add, cast, fill
@pytest.mark.parametrize("h,w,D", [(3, 5, 4), (10, 14, 96), (7, 9, 36), (1, 1, 8)])
def test_sine_pe(dev, h, w, D):
    from zutis_amd import ops
    oa = Arena(OUT_FILL, dev)
    vo = _flat(oa, "out", f32, h * w * D)
    ops.sine_pe(vo.m2, h, w, D)
    npf = D // 2
    c = torch.arange(D)
    i = torch.where(c < npf, c, c - npf)
    y, x = torch.meshgrid(torch.arange(h, dtype=f64), torch.arange(w, dtype=f64), indexing="ij")
    ey = ((y + 1) / (h + 1e-6) * 2 * np.pi).reshape(-1, 1)
    ex = ((x + 1) / (w + 1e-6) * 2 * np.pi).reshape(-1, 1)
    e = torch.where(c[None] < npf, ey, ex)
    a = e / (10000.0 ** (2 * (i // 2).double() / npf))[None]
    ref = torch.where((i % 2 == 1)[None], torch.cos(a), torch.sin(a))
    assert_close(vo.m2.reshape(h * w, D), ref, 2e-5, 0.0, f"sine_pe {h}x{w} D={D}")        # test_upsample2x_and_sine
    assert_untouched(oa)


@pytest.mark.parametrize("rows,D,add_rows", [(5, 4, 5), (35, 36, 7), (70, 768, 35), (3, 1028, 1)])
def test_add_rowperiodic_cast_fill(dev, rows, D, add_rows):
    """zh_add_rowperiodic_f16 (plain and split pairs with padded planes), zh_cast_f32_f16 with and without `add` (f16_scale 1 and 1024),
    zh_fill_f32 with n % 4 != 0 and n % 256 != 0."""
    from zutis_amd import ops
    n = rows * D
    for planes in (1, 2):
        ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
        va = _flat(ia, "a", f16, n, planes=planes, plane=n + 8)
        vadd = _flat(ia, "add", f32, add_rows * D)
        vx = _flat(ia, "x", f32, n)
        vo = _flat(oa, "out", f16, n, planes=planes, plane=n + 20)
        vc = _flat(oa, "cast", f16, n, planes=planes, plane=n + 4)
        vc2 = _flat(oa, "cast_add", f16, n, planes=planes, plane=n + 4)
        a32, add, x = _randn((rows, D), 1), _randn((add_rows, D), 2), _randn((rows, D), 3, 0.04)
        hi = a32.to(f16)
        lo = (a32 - hi.float()).to(f16)
        va.put(torch.stack([hi, lo]) if planes == 2 else hi)
        vadd.put(add); vx.put(x)
        addr = add.repeat(rows // add_rows, 1)
        ops.add_rowperiodic_f16(va.origin(0), vadd.m2, vo.origin(0), rows, D, add_rows)
        ops.cast_f16(vx.m2, vc.act(1.0 / 1024) if planes == 1 else vc.origin(0, out_scale=1.0 / 1024), rows, D)
        ops.cast_f16(vx.m2, vc2.origin(0), rows, D, add=vadd.m2, add_rows=add_rows)
        what = f"rows={rows} D={D} planes={planes}"
        if planes == 1:                                          # test_split_producers_write_hi_plus_lo: exactly the rounded fp32 sum
            assert_equal(vo.get()[0, 0, 0], (hi.float() + addr).to(f16).reshape(-1), "add_rowperiodic " + what)
            assert_equal(vc.get()[0, 0, 0], (x * 1024).to(f16).reshape(-1), "cast x1024 " + what)
            assert_equal(vc2.get()[0, 0, 0], (x + addr).to(f16).reshape(-1), "cast + add " + what)
        else:                                                    # ... and hi + lo within 3e-7 relative (|ref| clamped at 0.25)
            for v, ref in ((vo, (hi.float() + lo.float()) + addr), (vc, x * 1024), (vc2, x + addr)):
                r = ref.double().reshape(-1)
                assert_within(v.pair().reshape(-1), r, 3e-7 * r.abs().clamp_min(0.25), f"{v.name} pair {what}")
        assert_untouched(oa)
        assert_untouched(ia)
    for nn in (1, 3, 255, 257, n + 1):
        oa = Arena(OUT_FILL, dev)
        vf = _flat(oa, "fill", f32, nn)
        ops.fill_f32(vf.m2.reshape(-1), 0.0 if nn % 2 else 2.5)
        assert_equal(vf.m2.reshape(-1), torch.full((nn,), 0.0 if nn % 2 else 2.5), f"fill n={nn}")
        assert_untouched(oa)


# ------------------------------------------------------------------------------------------------ im2col
@pytest.mark.parametrize("B,Cin,H,W,p,Kpad,pad_to_patch,misalign", [
    (2, 3, 80, 112, 16, 768, False, 0),        # vector path (p % 8 == 0, W % 4 == 0, x aligned), Kpad == Cin p p
    (2, 3, 80, 112, 16, 776, False, 0),        # ... Kpad > Cin p p: 8 zero columns behind every row
    (1, 3, 37, 45, 8, 200, True, 0),           # pad_to_patch, H and W not multiples of the patch, W % 4 != 0 (scalar), 8 pad columns
    (1, 3, 37, 44, 8, 192, True, 0),           # pad_to_patch on the vector path: a patch row that straddles the right edge
    (2, 3, 32, 48, 16, 768, False, 4),         # x off by 4 bytes: scalar path
    (1, 1, 30, 30, 14, 200, False, 0),         # p % 8 != 0 (ViT-L/14's patch): scalar; trailing pixels dropped; 4 pad columns
    (1, 2, 9, 5, 4, 40, True, 0),              # tiny: one thread group mostly idle
])
def test_im2col(dev, B, Cin, H, W, p, Kpad, pad_to_patch, misalign):
    """zh_im2col_f16: the pad columns [Cin p p, Kpad) must be WRITTEN (as zero) and nothing beyond them; pixels past the image (pad_to_patch)
    are zero, never read (they are NaN here, as is everything around x); plain and split-pair outputs."""
    from zutis_amd import ops
    gh = -(-H // p) if pad_to_patch else (H - p) // p + 1
    gw = -(-W // p) if pad_to_patch else (W - p) // p + 1
    rows, kreal = B * gh * gw, Cin * p * p
    x = _randn((B, Cin, H, W), 61)
    xp = F.pad(x, (0, gw * p - W, 0, gh * p - H)) if pad_to_patch else x[:, :, :gh * p, :gw * p]
    cols = F.unfold(xp, p, stride=p).transpose(1, 2).reshape(rows, kreal)
    ref = torch.zeros((rows, Kpad))
    ref[:, :kreal] = cols
    for planes in (1, 2):
        ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
        vx = _flat(ia, "x", f32, x.numel(), misalign=misalign)
        vo = oa.add("out", f16, rows, Kpad, planes=planes, plane=rows * Kpad + 24, tail_rows=1)
        vx.put(x)
        ops.im2col(vx.m2.view(B, Cin, H, W), vo.act() if planes == 1 else vo.origin(0), p, Kpad, pad_to_patch=pad_to_patch)
        what = f"im2col {B}x{Cin}x{H}x{W} p={p} Kpad={Kpad} pad={pad_to_patch} misalign={misalign} planes={planes}"
        assert_equal(vo.get()[0, 0], ref.to(f16), what + " hi plane")
        if planes == 2:
            assert_close(vo.pair()[0], ref, 1e-6, 0.0, what + " pair")                     # test_split_producers_write_hi_plus_lo
            assert_equal(vo.get()[1, 0][:, kreal:], torch.zeros((rows, Kpad - kreal), dtype=f16), what + " lo pad columns")
        assert_untouched(oa)
        assert_untouched(ia)


# ------------------------------------------------------------------------------------------------ fused upsample + argmax
UA_T, UA_CH, UA_CHP = 32, 32, 36


def _ua_kernel(h, w, H, W):
    """The launcher's choice (zh_upsample_argmax), restated: the worst-case low-res window of a 32 x 32 output tile is wr x wc with
    wr = 32 for an identity size, else int(32 * float32(h / H)) + 3."""
    wr = UA_T if h == H else int(np.float32(UA_T) * (np.float32(h) / np.float32(H))) + 3
    wc = UA_T if w == W else int(np.float32(UA_T) * (np.float32(w) / np.float32(W))) + 3
    lds = UA_CH * wr * (wc + UA_T) * 4
    lds_pk = UA_CHP * wr * (wc + UA_T) * 4
    if wr * wc <= 64 and lds_pk <= 48 * 1024:
        return "pk", wr, wc
    return ("lds" if lds <= 48 * 1024 else "direct"), wr, wc


@pytest.mark.parametrize("h,w,H,W,kernel,window", [
    # threshold 1, wr * wc <= 64 -> the packed-window kernel
    (12, 12, 72, 72, "pk", (8, 8)),            # 1/6: int(5.33) + 3 = 8 -> 64 pixels, AT the threshold; 72 = 2.25 tiles
    (12, 12, 72, 60, "lds", (8, 9)),           # 1/5 across: 9 columns -> 72 > 64: the other side
    (32, 32, 518, 518, "pk", (4, 4)),          # x16.2, non-integer, ragged tiles
    (2, 23, 100, 40, "pk", (3, 21)),           # 63 pixels, a wide flat window; downsampled rows 23 -> 40 across
    (23, 2, 40, 100, "direct", (21, 3)),       # 63 pixels but 36 * 21 * 35 * 4 B > 48 KiB (and the plain window too): direct
    # threshold 2, 32 * wr * (wc + 32) * 4 <= 48 KiB  <=>  wr * (wc + 32) <= 384 -> the LDS-window kernel
    (21, 21, 100, 100, "lds", (9, 9)),         # 0.21: int(6.72) + 3 = 9 -> 369
    (12, 21, 72, 50, "lds", (8, 16)),          # 8 * 48 = 384: AT the threshold
    (12, 9, 72, 20, "direct", (8, 17)),        # 8 * 49 = 392: the other side
    (23, 23, 100, 100, "direct", (10, 10)),    # 0.23: 10 * 42 = 420
    (10, 14, 77, 145, "pk", (7, 6)),           # the golden test's odd size: 4.15 + 3, 3.09 + 3
    (21, 21, 21, 21, "direct", (32, 32)),      # identity
    (21, 21, 21, 131, "direct", (32, 8)),      # identity rows, x6.2 columns: 32 * 40 > 384
    (40, 50, 33, 37, "direct", (41, 46)),      # downsampling
    (1, 1, 45, 70, "pk", (3, 3)),              # a single low-res pixel: every tap clamps
])
def test_upsample_argmax_every_kernel_both_sides_of_both_thresholds(dev, h, w, H, W, kernel, window):
    """Labels exactly oracle.resample.bilinear_argmax_nchw for shapes on each side of both selection thresholds of the launcher (stated per
    case: kernel and the window (wr, wc) it sizes its LDS for), non-integer ratios, H and W not multiples of the 32 x 32 tile.  The
    logits are surrounded by NaN, which argmax treats as the maximum: a tap outside the image, or a window estimate
    (int)(32 * scale) + 3 one row or column too small, changes labels."""
    from zutis_amd import ops
    from oracle import resample as R
    assert _ua_kernel(h, w, H, W) == (kernel, *window)
    for B, n in ((2, 37), (1, 4)):                               # 37 classes: a chunk of 32 and a remainder; 4: one group
        ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
        vx = _flat(ia, "logits", f32, B * n * h * w)
        vl = _flat(oa, "labels", i64, B * H * W)
        x = _randn((B, n, h, w), h * 100 + W)
        vx.put(x)
        ops.upsample_argmax(vx.m2.view(B, n, h, w), vl.m2.view(B, H, W), B, n, h, w, H, W)
        assert_equal(vl.m2.view(B, H, W), torch.from_numpy(R.bilinear_argmax_nchw(x.numpy(), H, W)), f"upsample_argmax {h}x{w}->{H}x{W} n={n} [{kernel}]")
        assert_untouched(oa)
        assert_untouched(ia)


# ------------------------------------------------------------------------------------------------ bilinear NCHW, selected mask, nearest
@pytest.mark.parametrize("h,w,H,W,mis,kernel", [
    (10, 14, 37, 52, 0, "rows"),               # mask only, W % 4 == 0, aligned mask: the row-wise kernel (37 rows: 4 groups of 8 + 5)
    (10, 14, 37, 51, 0, "flat"),               # W % 4 != 0
    (10, 14, 37, 52, 1, "flat"),               # a mask pointer off by 1 byte
    (9, 13, 50, 1028, 0, "rows"),              # wider than one 1024-pixel block column
    (7, 5, 7, 5, 0, "flat"),                   # identity, 35 pixels
])
def test_upsample_bilinear_nchw_both_kernels(dev, h, w, H, W, mis, kernel):
    """fp32 output + mask (always the flat kernel) and mask only (row-wise kernel when W % 4 == 0 and the mask is 4-byte aligned),
    planes * H * W % 256 != 0: bit-exact against oracle.resample.bilinear_nchw, mask = value > threshold."""
    from zutis_amd import ops
    from oracle import resample as R
    planes, thr = 5, 0.5
    assert (planes * H * W) % 256 != 0 and (H * W) % 256 != 0
    assert kernel == ("rows" if (W % 4 == 0 and mis % 4 == 0) else "flat")
    ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
    vx = _flat(ia, "x", f32, planes * h * w)
    vo = _flat(oa, "out", f32, planes * H * W)
    vm1 = _flat(oa, "mask_with_out", u8, planes * H * W, misalign=mis)
    vm2 = _flat(oa, "mask_only", u8, planes * H * W, misalign=mis)
    x = torch.rand((planes, h, w), generator=torch.Generator().manual_seed(h * W))
    vx.put(x)
    ops.upsample_bilinear_nchw(vx.m2, planes, h, w, H, W, out=vo.m2, mask_u8=vm1.m2, threshold=thr)
    ops.upsample_bilinear_nchw(vx.m2, planes, h, w, H, W, mask_u8=vm2.m2, threshold=thr)
    ref = torch.from_numpy(R.bilinear_nchw(x.numpy()[None], H, W)[0])
    what = f"bilinear_nchw {h}x{w}->{H}x{W} mask misalign {mis}"
    assert_equal(vo.m2.view(planes, H, W), ref, what + " out")
    assert_equal(vm1.m2.view(planes, H, W), (ref > thr).to(u8), what + " mask (flat kernel)")
    assert_equal(vm2.m2.view(planes, H, W), (ref > thr).to(u8), what + f" mask ({kernel} kernel)")
    assert_untouched(oa)
    assert_untouched(ia)


@pytest.mark.parametrize("B,Q,h,w,H,W", [(2, 5, 10, 14, 37, 51), (1, 20, 8, 8, 30, 31), (3, 1, 3, 4, 11, 13)])
def test_select_upsample_mask(dev, B, Q, h, w, H, W):
    """The query with the largest objectness per image (first maximum), that mask plane upsampled by 4 (scale 0.25), cropped to H x W
    (H * W % 256 != 0) and thresholded; index int64 [B]."""
    from zutis_amd import ops
    from oracle import resample as R
    assert (H * W) % 256 != 0 and H <= 4 * h and W <= 4 * w
    ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
    vobj, vmask = _flat(ia, "objectness", f32, B * Q), _flat(ia, "masks", f32, B * Q * h * w)
    vout, vidx = _flat(oa, "out_u8", u8, B * H * W), _flat(oa, "index", i64, B)
    obj = _randn((B, Q), 5)
    if Q > 2:
        obj[0, 1] = obj[0, 3] = obj[0].max() + 1                  # a tie: the first wins
    masks = torch.rand((B, Q, h, w), generator=torch.Generator().manual_seed(6))
    vobj.put(obj); vmask.put(masks)
    ops.select_upsample_mask(vobj.m2.view(B, Q), vmask.m2.view(B, Q, h, w), vout.m2.view(B, H, W), vidx.m2.reshape(-1), B, Q, h, w, H, W, 0.25, 0.25, 0.5)
    best = obj.argmax(dim=1)
    assert_equal(vidx.m2.reshape(-1), best, "selected query")
    y0, y1, ly0, ly1 = R.linear_index_weights(h, H, scale=0.25)
    x0, x1, lx0, lx1 = R.linear_index_weights(w, W, scale=0.25)
    for b in range(B):
        p = masks[b, best[b]].numpy()
        top, bot = p[y0], p[y1]
        r0 = R.fma(top[:, x0], lx0, top[:, x1] * lx1)
        r1 = R.fma(bot[:, x0], lx0, bot[:, x1] * lx1)
        v = R.fma(r0, ly0[:, None], r1 * ly1[:, None])
        assert_equal(vout.m2.view(B, H, W)[b], torch.from_numpy((v > np.float32(0.5)).astype(np.uint8)), f"selected mask image {b}")
    assert_untouched(oa)
    assert_untouched(ia)


@pytest.mark.parametrize("h,w,H,W", [(10, 14, 37, 51), (37, 51, 10, 14), (7, 7, 7, 7), (1, 1, 3, 100), (480, 640, 33, 45)])
def test_resize_nearest_u8(dev, h, w, H, W):
    """F.interpolate(mode='nearest') of a u8 mask, H * W % 256 != 0, up- and downsampling; the bytes around the input are 255."""
    from zutis_amd import ops
    assert (H * W) % 256 != 0
    ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
    vx, vo = _flat(ia, "x", u8, h * w), _flat(oa, "out", u8, H * W)
    x = torch.randint(0, 200, (h, w), generator=torch.Generator().manual_seed(h + W), dtype=u8)
    vx.put(x)
    ops.resize_nearest_u8(vx.m2.view(h, w), H, W, out=vo.m2.view(H, W))
    ref = F.interpolate(x[None, None].float(), size=(H, W), mode="nearest")[0, 0].to(u8)
    assert_equal(vo.m2.view(H, W), ref, f"resize_nearest {h}x{w}->{H}x{W}")
    assert_untouched(oa)
    assert_untouched(ia)
