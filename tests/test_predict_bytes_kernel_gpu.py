"""-m gpu: zh_upsample_argmax_bytes — the arg-max launch whose epilogue leaves the label as the bytes of its PNG and blends a palette
colour over the decoded image — against zh_upsample_argmax's int64 map on the same logits and the NumPy integer blend.  Byte equality
throughout; every operand sits in a guard-band arena (tests/_guard.py): an image, palette or logit byte read from outside its logical
extent is 0xFF (a NaN logit, a white pixel) and shows in the comparison; a write outside [B,H,W] / [B,H,W,3] is reported by
assert_untouched()."""
import numpy as np
import pytest
import torch

from tests._guard import IN_FILL, OUT_FILL, Arena, assert_equal, assert_untouched

pytestmark = pytest.mark.gpu

f32, i64, u8, i32 = torch.float32, torch.int64, torch.uint8, torch.int32
UA_T, UA_CH, UA_CHP = 32, 32, 36
ALIGN, DESC_INTS = 16, 8
B = 2


def _ua_kernel(h, w, H, W):
    """The launcher's choice (ua_launch, csrc/resample.hip), restated from its conditions."""
    wr = UA_T if h == H else int(np.float32(UA_T) * (np.float32(h) / np.float32(H))) + 3
    wc = UA_T if w == W else int(np.float32(UA_T) * (np.float32(w) / np.float32(W))) + 3
    if wr * wc <= 64 and UA_CHP * wr * (wc + UA_T) * 4 <= 48 * 1024:
        return "pk"
    return "lds" if UA_CH * wr * (wc + UA_T) * 4 <= 48 * 1024 else "direct"


# (h, w, H, W, kernel): every branch of the launcher; H, W no multiples of the 32 x 32 tile, H != W
SHAPES = [
    (5, 4, 43, 35, "pk"),              # 2 x 2 tiles per image, three of them partial
    (7, 6, 37, 33, "lds"),             # 2 x 2 tiles, the second column one pixel wide
    (9, 8, 9, 8, "direct"),            # identity: 144 pixels, one block of which 112 lanes have left
    (9, 8, 18, 16, "direct"),          # x2: 576 pixels, the third block a quarter full
]
FORMATS = [(3, "u8"), (256, "u8"), (300, "rg16"), (920, "rg16")]


def _flat(arena, name, dtype, n):
    return arena.add(name, dtype, 1, n, tail_rows=1)


def _peak_class(n, h, w):
    """The class that wins at low-res pixel (b, y, x): spread over the whole of [0, n), so that "rg16" meets labels of 256 and more."""
    b, y, x = np.meshgrid(np.arange(B), np.arange(h), np.arange(w), indexing="ij")
    return ((7 * y + 3 * x) * 41 + 13 * b) % n


def _logits(n, h, w, seed):
    x = torch.randn((B, n, h, w), generator=torch.Generator().manual_seed(seed))
    peak = torch.from_numpy(_peak_class(n, h, w))
    x.scatter_add_(1, peak[:, None], torch.full((B, 1, h, w), 12.0))               # 12 sigma above the noise: the peak wins at its own pixel
    return x, peak.numpy()


def _images(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def _palette(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


_REF = {}


def _ref_labels(dev, x, key, H, W):
    """zh_upsample_argmax's label map for logits x: computed once per key, shared, never written."""
    if key not in _REF:
        from zutis_amd import ops
        Bx, n, h, w = x.shape
        lab = torch.empty((Bx, H, W), dtype=i64, device=dev)
        ops.upsample_argmax(x.to(dev), lab, Bx, n, h, w, H, W)
        _REF[key] = lab.cpu().numpy()
        _REF[key].setflags(write=False)
    return _REF[key]


def _decode(raw, fmt):
    """The label a reader takes from the bytes: the byte, or R + 256 G (imagenet_s.py:93)."""
    return raw.astype(np.int64) if fmt == "u8" else raw[..., 0].astype(np.int64) + 256 * raw[..., 1].astype(np.int64)


def _blend(img, colours, alpha):
    return ((img.astype(np.int64) * (256 - alpha) + colours.astype(np.int64) * alpha + 128) >> 8).astype(np.uint8)


def _run(dev, x, fmt, H, W, img=None, pal=None, alpha=128, want_labels=True, want_overlay=True):
    """One launch on arena operands: (label bytes or None, overlay bytes or None).  The two images lie at different, non-zero ALIGN-unit
    offsets of `packed`, with 0xFF between them."""
    from zutis_amd import ops
    Bx, n, h, w = x.shape
    ch = 1 if fmt == "u8" else 3
    ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
    vx = _flat(ia, "logits", f32, x.numel())
    per = -(-3 * H * W // ALIGN)                                                     # ALIGN units of one image
    offs = [3, 3 + per + 5]                                                          # units: 48 bytes in front, 80 bytes between the two
    nbytes = (offs[1] + per) * ALIGN
    vp, vd, vc = _flat(ia, "packed", u8, nbytes), _flat(ia, "desc", i32, Bx * DESC_INTS), _flat(ia, "palette", u8, 3 * n)
    vl, vo = _flat(oa, "labels", u8, Bx * H * W * ch), _flat(oa, "overlay", u8, Bx * H * W * 3)
    vx.put(x)
    packed = np.full(nbytes, 0xFF, np.uint8)
    rows = np.zeros((Bx, DESC_INTS), np.int32)
    for b in range(Bx):
        if img is not None:
            packed[offs[b] * ALIGN:offs[b] * ALIGN + 3 * H * W] = img[b].reshape(-1)
        rows[b] = (offs[b], W, H, W, H, 0, 0, 0)
    vp.put(torch.from_numpy(packed))
    vd.put(torch.from_numpy(rows))
    vc.put(torch.from_numpy(pal if pal is not None else np.zeros((n, 3), np.uint8)))
    vl.put(torch.full((vl.N,), 0x5A, dtype=u8))
    vo.put(torch.full((vo.N,), 0x5A, dtype=u8))
    lab_t = vl.m2.view((Bx, H, W) if ch == 1 else (Bx, H, W, 3))
    ops.upsample_argmax_bytes(vx.m2.view(Bx, n, h, w), Bx, n, h, w, H, W, label_format=fmt, labels_out=lab_t if want_labels else None,
                              overlay_out=vo.m2.view(Bx, H, W, 3) if want_overlay else None, packed=vp.m2.view(-1), desc=vd.m2.view(Bx, DESC_INTS),
                              palette=vc.m2.view(n, 3), alpha=alpha)
    torch.cuda.synchronize()
    assert_untouched(oa)
    assert_untouched(ia)
    labels, overlay = lab_t.cpu().numpy().copy(), vo.m2.view(Bx, H, W, 3).cpu().numpy().copy()
    if not want_labels:
        assert (labels == 0x5A).all(), "labels_out=None wrote label bytes"
    if not want_overlay:
        assert (overlay == 0x5A).all(), "overlay_out=None wrote overlay bytes"
    return (labels if want_labels else None), (overlay if want_overlay else None)


@pytest.mark.parametrize("n,fmt", FORMATS)
@pytest.mark.parametrize("h,w,H,W,kernel", SHAPES)
def test_bytes_are_the_int64_labels_and_the_overlay_is_the_integer_blend(dev, h, w, H, W, kernel, n, fmt):
    assert _ua_kernel(h, w, H, W) == kernel and H != W and H % UA_T and W % UA_T
    what = f"bytes {h}x{w}->{H}x{W} n={n} {fmt} [{kernel}]"
    x, peak = _logits(n, h, w, 1000 * n + H)
    ref = _ref_labels(dev, x, (h, w, H, W, n), H, W)
    assert set(np.unique(peak)) <= set(np.unique(ref))                              # every peak class is the label of some pixel
    if (h, w) == (H, W):
        assert np.array_equal(ref, peak)                                            # identity: the label of every pixel is known outright
    if fmt == "rg16":
        assert (ref >= 256).any() and (ref < 256).any()                             # the G byte is non-zero at known pixels, and zero at others
    img, pal, alpha = _images(H, W, 7 * n + W), _palette(n, n), 77
    labels, overlay = _run(dev, x, fmt, H, W, img, pal, alpha)
    print(f"{what}: {len(np.unique(ref))} distinct labels up to {int(ref.max())}, {int((_decode(labels, fmt) != ref).sum())} of {ref.size} labels differ, "
          f"{int((overlay != _blend(img, pal[ref], alpha)).sum())} overlay bytes differ")
    assert_equal(torch.from_numpy(_decode(labels, fmt)), torch.from_numpy(ref.copy()), f"{what}: labels")
    if fmt == "rg16":
        assert (labels[..., 2] == 0).all() and (labels[..., 1] == (ref >> 8)).all() and (labels[..., 0] == (ref & 255)).all()
    assert_equal(torch.from_numpy(overlay), torch.from_numpy(_blend(img, pal[ref], alpha)), f"{what}: overlay")
    _, only_overlay = _run(dev, x, fmt, H, W, img, pal, alpha, want_labels=False)
    assert_equal(torch.from_numpy(only_overlay), torch.from_numpy(overlay), f"{what}: overlay with labels_out=None")
    only_labels, _ = _run(dev, x, fmt, H, W, None, None, alpha, want_overlay=False)  # packed is all 0xFF: it must not matter
    assert_equal(torch.from_numpy(only_labels), torch.from_numpy(labels), f"{what}: labels with overlay_out=None")


@pytest.mark.parametrize("alpha", [0, 1, 255, 256])
def test_overlay_at_the_ends_of_alpha(dev, alpha):
    h, w, H, W, kernel = SHAPES[0]
    n = 256
    x, _ = _logits(n, h, w, 5)
    ref = _ref_labels(dev, x, ("alpha", h, w, H, W), H, W)
    img, pal = _images(H, W, 3), _palette(n, 4)
    img[0, :4, :4] = 255; pal[ref[0, 0, 0]] = 255                                    # the largest sum: 255 * 256 + 128 stays a byte
    _, overlay = _run(dev, x, "u8", H, W, img, pal, alpha, want_labels=False)
    assert_equal(torch.from_numpy(overlay), torch.from_numpy(_blend(img, pal[ref], alpha)), f"overlay alpha={alpha}")
    if alpha == 0:
        assert np.array_equal(overlay, img)
    if alpha == 256:
        assert np.array_equal(overlay, pal[ref])


@pytest.mark.parametrize("h,w,H,W,kernel", SHAPES)
def test_ties_and_nan_columns_give_the_labels_of_the_int64_kernel(dev, h, w, H, W, kernel):
    """The tie and NaN cases of tests/test_kernels_gpu.py::test_upsample_argmax_bit_exact, at this file's shapes: ties inside a group of four
    classes and across chunks (the first index wins), -0.0 against +0.0, a NaN column (the first NaN is the maximum), -inf everywhere."""
    for n in (6, 37):
        x = -np.abs(torch.randn((B, n, h, w), generator=torch.Generator().manual_seed(74 + n)).numpy()) - 0.5
        x[0, 1] = x[0, 3] = np.abs(x[0, 3])                                          # same group, first and third member
        x[1, 2] = -0.0; x[1, 5] = 0.0                                                # -0.0 (class 2) before +0.0 (class 5): equal, class 2 wins
        if n > 36:
            x[0, 33] = x[0, 1]                                                       # and again in the next chunk: never replaces
        x = torch.from_numpy(x)
        ref = _ref_labels(dev, x, ("tie", n, h, w, H, W), H, W)
        assert (ref[0] == 1).all() and (ref[1] == 2).all()
        for fmt in ("u8", "rg16"):
            labels, _ = _run(dev, x, fmt, H, W, want_overlay=False)
            assert_equal(torch.from_numpy(_decode(labels, fmt)), torch.from_numpy(ref.copy()), f"ties n={n} {fmt} [{kernel}]")
    x = torch.randn((B, 40, h, w), generator=torch.Generator().manual_seed(73))
    x[0, 35, 2, 3] = float("nan"); x[0, 3, 2, 3] = float("nan"); x[1, :, 3:, 2:] = float("-inf"); x[1, 20, 0, 0] = float("inf")
    ref = _ref_labels(dev, x, ("nan", h, w, H, W), H, W)
    assert (ref[0] == 3).any() and ref[1, -1, -1] == 0 and ref[1, 0, 0] == 20
    img, pal = _images(H, W, 1), _palette(40, 2)
    labels, overlay = _run(dev, x, "u8", H, W, img, pal, 200)
    assert_equal(torch.from_numpy(_decode(labels, "u8")), torch.from_numpy(ref.copy()), f"nan [{kernel}]")
    assert_equal(torch.from_numpy(overlay), torch.from_numpy(_blend(img, pal[ref], 200)), f"nan overlay [{kernel}]")


def test_binding_refuses_wrong_operands(dev):
    from zutis_amd import _lib, ops
    H, W = 6, 5
    lo = torch.zeros((1, 4, 3, 3), dtype=f32, device=dev)
    lab = torch.full((1, H, W), 9, dtype=u8, device=dev)
    ops.upsample_argmax_bytes(lo, 1, 4, 3, 3, H, W, labels_out=lab)
    assert int(lab.max()) == 0                                                       # all-zero logits: the first index
    packed = torch.zeros((3 * H * W + 32,), dtype=u8, device=dev)
    pal = torch.zeros((4, 3), dtype=u8, device=dev)
    ovl = torch.empty((1, H, W, 3), dtype=u8, device=dev)

    def desc(*row):
        return torch.tensor([list(row) + [0] * (8 - len(row))], dtype=i32, device=dev)
    ops.upsample_argmax_bytes(lo, 1, 4, 3, 3, H, W, overlay_out=ovl, packed=packed, desc=desc(2, W, H), palette=pal)
    with pytest.raises(_lib.ZutisHipError, match="257 classes"):
        ops.upsample_argmax_bytes(torch.zeros((1, 257, 3, 3), dtype=f32, device=dev), 1, 257, 3, 3, H, W, label_format="u8", labels_out=lab)
    with pytest.raises(_lib.ZutisHipError, match="both None"):
        ops.upsample_argmax_bytes(lo, 1, 4, 3, 3, H, W)
    with pytest.raises(_lib.ZutisHipError, match="descriptor row 0 holds a 6 x 5 image"):
        ops.upsample_argmax_bytes(lo, 1, 4, 3, 3, H, W, overlay_out=ovl, packed=packed, desc=desc(0, H, W), palette=pal)
    with pytest.raises(_lib.ZutisHipError, match="outside packed"):
        ops.upsample_argmax_bytes(lo, 1, 4, 3, 3, H, W, overlay_out=ovl, packed=packed, desc=desc(3, W, H), palette=pal)
    for bad in (dict(labels_out=lab.view(1, W, H)), dict(labels_out=lab.to(torch.int64)), dict(label_format="u16", labels_out=lab),
                dict(label_format="rg16", labels_out=lab), dict(overlay_out=ovl, packed=packed, desc=desc(0, W, H)),
                dict(overlay_out=ovl, packed=packed, desc=desc(0, W, H), palette=pal[:3]),
                dict(overlay_out=ovl, packed=packed, desc=desc(0, W, H), palette=pal, alpha=300)):
        with pytest.raises(_lib.ZutisHipError):
            ops.upsample_argmax_bytes(lo, 1, 4, 3, 3, H, W, **bad)
    torch.cuda.synchronize()
