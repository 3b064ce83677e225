"""-m gpu: zh_upsample_argmax_score — the arg-max launch with RunningScore._fast_hist as its epilogue — against the pieces it fuses:
the labels of zh_upsample_argmax and np.bincount(n * gt[m] + pred[m]).  Integer equality throughout; every operand sits in a guard-band
arena (tests/_guard.py): a ground-truth byte read from outside decodes as 255 (an ignored label) and shows as a missing count, a write
outside the histogram or the label map is reported by assert_untouched()."""
import numpy as np
import pytest
import torch

from tests._guard import IN_FILL, OUT_FILL, Arena, assert_equal, assert_untouched

pytestmark = pytest.mark.gpu

f32, i64, u8 = torch.float32, torch.int64, torch.uint8
UA_T, UA_CH, UA_CHP = 32, 32, 36
IGNORE = {"u8": 255, "rg16": 1000}


def _ua_kernel(h, w, H, W):
    """The launcher's choice (ua_launch, csrc/resample.hip), restated from its conditions."""
    wr = UA_T if h == H else int(np.float32(UA_T) * (np.float32(h) / np.float32(H))) + 3
    wc = UA_T if w == W else int(np.float32(UA_T) * (np.float32(w) / np.float32(W))) + 3
    if wr * wc <= 64 and UA_CHP * wr * (wc + UA_T) * 4 <= 48 * 1024:
        return "pk"
    return "lds" if UA_CH * wr * (wc + UA_T) * 4 <= 48 * 1024 else "direct"


# (h, w, H, W, kernel): one per dispatch branch, every output a partial tile / block somewhere; B = 2 throughout
SHAPES = [
    (5, 7, 70, 98, "pk"),              # 3 x 4 tiles per image, the last row and column of tiles partial
    (9, 8, 45, 40, "lds"),             # 2 x 2 tiles, all but one partial
    (20, 16, 40, 32, "direct"),        # x2: ten whole blocks
    (20, 16, 40, 33, "direct"),        # 2640 pixels: the last block holds one whole wave and 16 lanes of the next
    (24, 40, 24, 40, "direct"),        # identity
]
CLASSES = [5, 33, 81, 130]             # not a multiple of 4; one past a 32-class chunk; zh_confusion_hist's LDS regime; n * n above it
B = 2


def _flat(arena, name, dtype, n):
    return arena.add(name, dtype, 1, n, tail_rows=1)


def _logits(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _gt(fmt, n, shape, seed, ignore_every=9):
    """(values int64 [B,H,W], bytes as the kernel reads them).  Values are uniform over [0, n) with every `ignore_every`-th replaced by the
    format's ignore label; "rg16": R + 256 G interleaved with a non-zero B channel, which must be ignored."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, n, shape, dtype=np.int64)
    if ignore_every:
        v[rng.integers(0, ignore_every, shape) == 0] = IGNORE[fmt]
    if fmt == "u8":
        return v, v.astype(np.uint8)
    raw = np.stack([v & 255, v >> 8, rng.integers(1, 256, shape)], axis=-1).astype(np.uint8)
    return v, raw


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


def _bincount(n, g, pred):
    m = g < n
    return np.bincount(n * g[m] + pred[m], minlength=n * n), int(m.sum())


def _run(dev, x, raw, fmt, H, W, what, calls=(True, False)):
    """The fused kernel on arena operands, once per entry of `calls` (True: with a label map) into ONE histogram that starts at zero:
    (histogram after each call, the label map of the last call that asked for one)."""
    from zutis_amd import ops
    Bx, n, h, w = x.shape
    ia, oa = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
    vx, vg = _flat(ia, "logits", f32, x.numel()), _flat(ia, "gt", u8, raw.size)
    vh, vl = _flat(oa, "hist", i64, n * n), _flat(oa, "labels", i64, Bx * H * W)
    vx.put(x)
    vg.put(torch.from_numpy(raw))
    vh.put(torch.zeros(n * n, dtype=i64))
    vl.put(torch.full((Bx * H * W,), -7, dtype=i64))
    hists, labels = [], None
    for with_labels in calls:
        ops.upsample_argmax_score(vx.m2.view(Bx, n, h, w), vg.m2.view(raw.shape), vh.m2.view(-1), Bx, n, h, w, H, W, gt_format=fmt,
                                  labels=vl.m2.view(Bx, H, W) if with_labels else None)
        hists.append(vh.m2.view(-1).cpu().numpy().copy())
        if with_labels:
            labels = vl.m2.view(Bx, H, W).cpu().numpy().copy()
            vl.put(torch.full((Bx * H * W,), -7, dtype=i64))
        else:
            assert_equal(vl.m2.view(-1), torch.full((Bx * H * W,), -7, dtype=i64), f"{what}: labels=NULL wrote a label map")
    assert_untouched(oa)
    assert_untouched(ia)
    return hists, labels


@pytest.mark.parametrize("fmt", ["u8", "rg16"])
@pytest.mark.parametrize("n", CLASSES)
@pytest.mark.parametrize("h,w,H,W,kernel", SHAPES)
def test_fused_histogram_equals_argmax_plus_bincount(dev, h, w, H, W, kernel, n, fmt):
    assert _ua_kernel(h, w, H, W) == kernel
    what = f"score {h}x{w}->{H}x{W} n={n} {fmt} [{kernel}]"
    x = _logits((B, n, h, w), 1000 * n + H)
    pred = _ref_labels(dev, x, (h, w, H, W, n), H, W)
    g, raw = _gt(fmt, n, (B, H, W), 17 * n + W)
    ref, counted = _bincount(n, g, pred)
    assert 0 < counted < g.size                                   # some pixels carry the ignore label, most do not
    (h1, h2), labels = _run(dev, x, raw, fmt, H, W, what)
    print(f"{what}: {counted} of {g.size} pixels counted, {int((ref > 0).sum())} bins hit, {int((h1 != ref).sum())} bins differ")
    assert_equal(torch.from_numpy(h1), torch.from_numpy(ref), f"{what}: histogram")
    assert int(h1.sum()) == counted                               # nothing read from outside the ground truth, nothing counted twice
    assert_equal(torch.from_numpy(labels), torch.from_numpy(pred.copy()), f"{what}: label map")
    assert_equal(torch.from_numpy(h2), torch.from_numpy(2 * ref), f"{what}: second call (labels=NULL) into the same histogram")


@pytest.mark.parametrize("h,w,H,W,kernel", [SHAPES[0], SHAPES[1], SHAPES[3]])
def test_worst_contention_and_widest_spread(dev, h, w, H, W, kernel):
    """Constant ground truth under one dominant class: ONE bin holds B * H * W, every wave merges to a single atomic.  Ground truth uniform
    over 130 classes against random logits: nearly every lane of a wave holds a key of its own."""
    n = 81
    x = _logits((B, n, h, w), 5)
    x[:, 2] += 50.0
    pred = _ref_labels(dev, x, ("dominant", h, w, H, W), H, W)
    assert (pred == 2).all()
    for fmt in ("u8", "rg16"):
        g = np.full((B, H, W), 3, np.int64)
        raw = g.astype(np.uint8) if fmt == "u8" else np.stack([g, 0 * g, 0 * g + 9], axis=-1).astype(np.uint8)
        (h1,), _ = _run(dev, x, raw, fmt, H, W, f"contention {kernel} {fmt}", calls=(False,))
        ref = np.zeros(n * n, np.int64)
        ref[3 * n + 2] = B * H * W
        assert_equal(torch.from_numpy(h1), torch.from_numpy(ref), f"contention {kernel} {fmt}")
    n = 130
    x = _logits((B, n, h, w), 6)
    pred = _ref_labels(dev, x, ("spread", h, w, H, W), H, W)
    for fmt in ("u8", "rg16"):
        g, raw = _gt(fmt, n, (B, H, W), 23, ignore_every=0)
        ref, counted = _bincount(n, g, pred)
        assert counted == g.size and (ref > 0).sum() > g.size // 2          # most pixels sit in a bin of their own
        (h1, h2), labels = _run(dev, x, raw, fmt, H, W, f"spread {kernel} {fmt}")
        assert_equal(torch.from_numpy(h1), torch.from_numpy(ref), f"spread {kernel} {fmt}")
        assert_equal(torch.from_numpy(h2), torch.from_numpy(2 * ref), f"spread {kernel} {fmt}: second call")
        assert_equal(torch.from_numpy(labels), torch.from_numpy(pred.copy()), f"spread {kernel} {fmt}: label map")


@pytest.mark.parametrize("h,w,H,W,kernel", [SHAPES[0], SHAPES[1], SHAPES[3]])
def test_nan_and_all_minus_inf_pixels_take_the_slow_path(dev, h, w, H, W, kernel):
    """A NaN in one class of one low-res pixel (arg-max treats it as the maximum) and a low-res pixel that is -inf in every class: the
    chunks that see them walk the NaN-aware loop, and its labels reach the histogram as they reach zh_upsample_argmax's map."""
    n = 33
    x = _logits((B, n, h, w), 77)
    x[0, 20, 1, 2] = float("nan")
    x[1, 32, h - 1, w - 1] = float("nan")                          # the last class: the chunk of one
    x[1, :, 2, 1] = float("-inf")
    pred = _ref_labels(dev, x, ("nan", h, w, H, W), H, W)
    assert (pred[0] == 20).any() and (pred[1] == 32).any()
    for fmt in ("u8", "rg16"):
        g, raw = _gt(fmt, n, (B, H, W), 31)
        ref, counted = _bincount(n, g, pred)
        (h1, h2), labels = _run(dev, x, raw, fmt, H, W, f"nan {kernel} {fmt}")
        assert_equal(torch.from_numpy(h1), torch.from_numpy(ref), f"nan {kernel} {fmt}")
        assert int(h1.sum()) == counted
        assert_equal(torch.from_numpy(labels), torch.from_numpy(pred.copy()), f"nan {kernel} {fmt}: label map")
        assert_equal(torch.from_numpy(h2), torch.from_numpy(2 * ref), f"nan {kernel} {fmt}: second call")


def test_wrapper_refuses_wrong_operands(dev):
    from zutis_amd import _lib, ops
    lo = torch.zeros((1, 4, 3, 3), dtype=f32, device=dev)
    gt = torch.zeros((1, 6, 6), dtype=u8, device=dev)
    hist = torch.zeros(16, dtype=i64, device=dev)
    ops.upsample_argmax_score(lo, gt, hist, 1, 4, 3, 3, 6, 6)
    assert int(hist[0]) == 36 and int(hist.sum()) == 36            # all-zero logits: first index; all-zero ground truth
    for bad in (dict(gt=gt.to(torch.int64)), dict(hist=hist[:15]), dict(gt_format="rg16"), dict(gt_format="u16"),
                dict(labels=torch.zeros((1, 6, 5), dtype=i64, device=dev))):
        kw = dict(gt=gt, hist=hist, gt_format="u8", labels=None)
        kw.update(bad)
        with pytest.raises(_lib.ZutisHipError):
            ops.upsample_argmax_score(lo, kw["gt"], kw["hist"], 1, 4, 3, 3, 6, 6, gt_format=kw["gt_format"], labels=kw["labels"])
