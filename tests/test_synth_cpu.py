"""CPU: the host restatements of zutis_amd.synth against their yardsticks — Pillow (ImageEnhance, ImageStat, Image.convert,
Image.resize), torch (F.interpolate nearest, pad, flip) and, where a reference checkout is present, the reference's own copy_paste —
and draw_recipe's distributions.  The GPU tests compare the kernels against these restatements."""
import math
import pickle
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image, ImageEnhance, ImageOps, ImageStat

import _synth_case as K
from zutis_amd import preprocess, synth

FACTORS = (0.2, 0.37, 0.999, 1.0, 1.3, 1.8)


# ------------------------------------------------------------------------------------------------------------------- photometric
@pytest.mark.parametrize("f", FACTORS)
def test_blend_all_byte_pairs(f):
    a = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, 1)
    b = np.ascontiguousarray(a.T)
    want = np.asarray(Image.blend(Image.fromarray(a, "L"), Image.fromarray(b, "L"), f))
    assert np.array_equal(synth.blend_u8(a, b, f), want)


def test_grey_and_contrast_mean():
    for seed, (h, w) in enumerate([(64, 64), (37, 91), (120, 50)]):
        a = K.photo(h, w, seed)
        im = Image.fromarray(a)
        assert np.array_equal(synth.grey_u8(a), np.asarray(im.convert("L")))
        assert synth.contrast_mean(a) == int(ImageStat.Stat(im.convert("L")).mean[0] + 0.5)
    for v in (0, 1, 127, 128, 254, 255):          # constant images, and one whose mean is exactly k + 1/2
        a = np.full((4, 4, 3), v, np.uint8)
        assert synth.contrast_mean(a) == int(ImageStat.Stat(Image.fromarray(a).convert("L")).mean[0] + 0.5)
    a = np.zeros((2, 2, 3), np.uint8)
    a[0] = 1
    assert synth.contrast_mean(a) == int(ImageStat.Stat(Image.fromarray(a).convert("L")).mean[0] + 0.5) == 1


@pytest.mark.parametrize("f", FACTORS)
def test_enhancers(f):
    a = K.photo(80, 70, 3)
    im = Image.fromarray(a)
    assert np.array_equal(synth.blend_u8(0, a, f), np.asarray(ImageEnhance.Brightness(im).enhance(f)))
    assert np.array_equal(synth.blend_u8(synth.contrast_mean(a), a, f), np.asarray(ImageEnhance.Contrast(im).enhance(f)))
    assert np.array_equal(synth.blend_u8(synth.grey_u8(a)[..., None], a, f), np.asarray(ImageEnhance.Color(im).enhance(f)))


def _all_triples():
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def test_rgb_to_hsv_all_triples():
    t = _all_triples()
    want = np.asarray(Image.fromarray(t, "RGB").convert("HSV"))
    assert int((synth.rgb_to_hsv_u8(t) != want).any(-1).sum()) == 0


def test_hsv_to_rgb_all_triples():
    t = _all_triples()
    want = np.asarray(Image.frombytes("HSV", (4096, 4096), t.tobytes()).convert("RGB"))
    assert int((synth.hsv_to_rgb_u8(t) != want).any(-1).sum()) == 0


def _pil_hue(im: Image.Image, shift: int) -> Image.Image:
    """torchvision.transforms.functional_pil.adjust_hue with the uint8 shift already formed."""
    h, s, v = im.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.uint8(shift)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def _pil_photometric(a: np.ndarray, sub) -> np.ndarray:
    im = Image.fromarray(a)
    if sub.jitter:
        for op in sub.order:
            if op == 0:
                im = ImageEnhance.Brightness(im).enhance(sub.brightness)
            elif op == 1:
                im = ImageEnhance.Contrast(im).enhance(sub.contrast)
            elif op == 2:
                im = ImageEnhance.Color(im).enhance(sub.saturation)
            else:
                im = _pil_hue(im, sub.hue_shift)
    if sub.grey:                                    # RandomGrayscale: rgb_to_grayscale(img, num_output_channels=3)
        g = np.asarray(im.convert("L"))
        im = Image.fromarray(np.dstack([g, g, g]))
    return np.asarray(im)


JITTERS = [((0, 1, 2, 3), (0.2, 1.8, 0.5), 13, False), ((3, 2, 1, 0), (1.8, 0.2, 1.7), 231, False), ((1, 0, 3, 2), (1.3, 1.3, 0.21), 0, True),
           ((2, 3, 0, 1), (0.999, 0.37, 1.0), 51, False), ((1, 3, 2, 0), (0.66, 1.21, 1.44), 205, True), ((2, 0, 1, 3), (1.0, 1.0, 1.0), 128, False)]


@pytest.mark.parametrize("case", range(len(JITTERS)))
def test_jitter_sequences(case):
    order, factors, hue, grey = JITTERS[case]
    for seed, (h, w) in enumerate([(64, 64), (50, 77)]):
        a = K.photo(h, w, 10 * case + seed)
        s = K.sub((w, h), 1.0, jitter=True, order=order, factors=factors, hue=hue, grey=grey)
        assert np.array_equal(synth.photometric_np(a, s), _pil_photometric(a, s))
    s = K.sub((64, 64), 1.0, jitter=False, grey=True)
    a = K.photo(64, 64, case)
    assert np.array_equal(synth.photometric_np(a, s), _pil_photometric(a, s))


def test_hue_shift_is_the_uint8_cast():
    """torchvision's adjust_hue forms the shift as a FLOAT to uint8 cast, np.array(hue_factor * 255).astype("uint8"): a negative value
    truncates towards zero and wraps."""
    for hf in (-0.2, -0.1999, -0.1, -0.0039, -0.0, 0.0, 0.0039, 0.1, 0.1999, 0.2):
        with np.errstate(invalid="ignore"):
            want = int(np.array(hf * 255, dtype=np.float64).astype(np.uint8))
        assert synth.hue_shift(hf) == want, hf
    assert synth.hue_shift(-0.2) == 205 and synth.hue_shift(0.2) == 51 and synth.hue_shift(-0.0039) == 0


# ---------------------------------------------------------------------------------------------------------------------- geometry
def _pil_geometry(a: np.ndarray, m: np.ndarray, sub, C: int):
    """random_scale + random_crop + random_hflip with Pillow and torch, the recipe's draws in place of the random calls."""
    nw, nh = sub.scaled
    im = Image.fromarray(a).resize((nw, nh), Image.BILINEAR)
    mask = F.interpolate(torch.from_numpy(m.astype(np.int64))[None, None].float(), size=(nh, nw), mode="nearest")[0, 0].long()
    fill = tuple(np.array(im).mean(axis=(0, 1)).astype(np.uint8).tolist())
    pad_w, pad_h = max(C - nw, 0), max(C - nh, 0)
    padding = [[pad_w, pad_h, 0, 0], [pad_w, 0, 0, pad_h], [0, pad_h, pad_w, 0], [0, 0, pad_w, pad_h]][sub.corner]       # left, top, right, bottom
    im = ImageOps.expand(im, border=tuple(padding), fill=fill)
    mask = F.pad(mask, (padding[0], padding[2], padding[1], padding[3]), value=K.IGNORE)
    w, h = im.size
    top, left = synth.resolve(sub.u_crop_top, h - C), synth.resolve(sub.u_crop_left, w - C)
    im = im.crop((left, top, left + C, top + C))
    mask = mask[top:top + C, left:left + C]
    if sub.flip:
        im, mask = ImageOps.mirror(im), torch.flip(mask, dims=[-1])
    return np.asarray(im), mask.numpy().astype(np.uint8)


# (h, w) of the source, scale, crop size: padding in none / one / both axes, scale 0.1 and 1.0, non-square sources
GEOMETRY = [((120, 160), 1.0, 64), ((120, 160), 0.1, 64), ((160, 120), 0.5, 64), ((200, 70), 0.6, 64), ((64, 300), 0.7, 64),
            ((90, 90), 0.3, 64), ((333, 250), 0.37, 96), ((64, 64), 1.0, 64), ((700, 500), 0.1, 64)]


@pytest.mark.parametrize("case", range(len(GEOMETRY)))
def test_geometry(case):
    (h, w), scale, C = GEOMETRY[case]
    a, m = K.photo(h, w, case), K.blob(h, w, case)
    seen = set()
    for corner in range(4):
        for flip in (False, True):
            s = K.sub((w, h), scale, corner=corner, u_crop=(0.13 + 0.2 * corner, 0.91 - 0.2 * corner), flip=flip)
            img, mask = synth.geometry_np(a, m, s, C, K.IGNORE)
            want_img, want_mask = _pil_geometry(a, m, s, C)
            assert np.array_equal(img, want_img) and np.array_equal(mask, want_mask)
            seen.add((s.scaled[0] < C, s.scaled[1] < C))
    assert len(seen) == 1


def test_geometry_cases_cover_every_padding_pattern():
    pats = {(int(w * s) < C, int(h * s) < C) for (h, w), s, C in GEOMETRY}
    assert pats == {(False, False), (True, False), (False, True), (True, True)}


def test_resolve_covers_the_range():
    assert synth.resolve(0.0, 5) == 0 and synth.resolve(math.nextafter(1.0, 0.0), 5) == 5 and synth.resolve(0.5, 0) == 0
    assert [synth.resolve(k / 6 + 1e-9, 5) for k in range(6)] == list(range(6))


# ---------------------------------------------------------------------------------------------------------------------- compose
def _compose_case(kind: str, C: int = 32):
    rng = np.random.default_rng(len(kind))
    masks = []

    def rect(y0, y1, x0, x1):
        m = np.zeros((C, C), np.uint8)
        m[y0:y1, x0:x1] = 1
        return m

    if kind == "empty":                 # sub-image 1 has no object: no paste
        masks = [rect(4, 20, 4, 20), np.zeros((C, C), np.uint8), rect(10, 18, 12, 30)]
    elif kind == "overwritten":         # object 1 is fully covered by object 2 (same box, pasted at the same place)
        masks = [rect(2, 8, 2, 8), rect(10, 20, 10, 20), rect(9, 22, 9, 22)]
    elif kind == "border":              # objects touching the crop's borders
        masks = [rect(0, C, 0, 5), rect(0, 12, 0, 12), rect(20, C, 18, C)]
    elif kind == "ignore0":             # image 0 has a padded ignore region, the pasted object lands on it; 1 has ignore pixels too
        m0 = rect(12, 28, 12, 28)
        m0[:10] = K.IGNORE
        m1 = rect(5, 25, 3, 17)
        m1[:, 20:] = K.IGNORE
        masks = [m0, m1]
    elif kind == "many":
        masks = [K.blob(C, C, 50 + k) for k in range(10)]
    n = len(masks)
    images = [rng.standard_normal((C, C, 3)).astype(np.float32) for _ in range(n)]
    us = rng.random((n, 2))
    if kind == "overwritten":
        us[1] = us[2] = (0.4, 0.4)
    subs = [K.sub((C, C), 1.0, u_paste=(float(us[k, 0]), float(us[k, 1])), label=3 + k) for k in range(n)]
    return images, masks, synth.SampleRecipe(subs, C, K.IGNORE)


@pytest.mark.parametrize("kind", ["empty", "overwritten", "border", "ignore0", "many"])
def test_compose_against_reference_copy_paste(kind, monkeypatch):
    ref = K.reference_copy_paste()
    if ref is None:
        pytest.skip("no reference checkout next to this repository")
    images, masks, recipe = _compose_case(kind)
    offs = [o for o in synth.paste_offsets(masks, recipe) if o is not None]
    draws = iter([v for o in offs for v in o])          # offset_top, offset_left per pasting object, in the reference's call order
    monkeypatch.setattr(ref, "randint", lambda lo, hi: next(draws))
    sem = [torch.from_numpy(np.where(m == 1, s.label_id, m).astype(np.int64)) for m, s in zip(masks, recipe.subs)]
    inst = [torch.from_numpy(np.where(m == 1, k + 1, m).astype(np.int64)) for k, m in enumerate(masks)]
    want_img, want_sem, want_inst = ref.copy_paste([torch.from_numpy(i.transpose(2, 0, 1).copy()) for i in images], sem, inst, 0, K.IGNORE)
    assert next(draws, None) is None                    # every resolved offset was consumed: empty objects draw nothing
    image, semantic, onehot = synth.compose_np(images, masks, recipe)
    assert np.array_equal(image.transpose(2, 0, 1), want_img.numpy())
    assert np.array_equal(semantic, want_sem.numpy())
    want_onehot = torch.stack([want_inst == k for k in range(1, len(masks) + 1)], 0).numpy()       # index_dataset.py:371-373
    assert onehot.shape == want_onehot.shape and np.array_equal(onehot, want_onehot)
    if kind == "overwritten":
        assert not onehot[1].any() and onehot.shape[0] == 3    # the row of a completely overwritten instance exists and is empty


def test_compose_exclusive_maxima():
    """The reference slices [ymin:ymax, xmin:xmax] with the maxima of the coordinates: the object's last row and column stay behind."""
    C = 16
    m1 = np.zeros((C, C), np.uint8)
    m1[4:9, 5:11] = 1
    masks = [np.zeros((C, C), np.uint8), m1]
    images = [np.zeros((C, C, 1), np.float32), np.ones((C, C, 1), np.float32)]
    recipe = synth.SampleRecipe([K.sub((C, C), 1.0), K.sub((C, C), 1.0, u_paste=(0.0, 0.0))], C, K.IGNORE)
    image, semantic, onehot = synth.compose_np(images, masks, recipe)
    assert int(onehot[1].sum()) == 4 * 5 and onehot[1][:4, :5].all()


# ------------------------------------------------------------------------------------------------------------------ draw_recipe
def _fields(n=6, **kw):
    paths = [f"/img{i}.jpg" for i in range(n)]
    f = synth.DatasetFields(paths, [p.replace(".jpg", ".json") for p in paths], {p: 1 + i % 3 for i, p in enumerate(paths)},
                            {"a": paths[:3], "b": paths[3:]}, K.IGNORE, **kw)
    return f, (lambda p: (500 + 10 * int(p[4]), 375))


def test_draw_recipe_deterministic_and_picklable():
    f, size_of = _fields()
    a = [synth.draw_recipe(random.Random(7), f, size_of) for _ in range(2)]
    assert a[0] == a[1]
    assert synth.draw_recipe(random.Random(8), f, size_of) != a[0]
    assert pickle.loads(pickle.dumps(a[0])) == a[0]


def test_draw_recipe_ranges_and_corner_frequencies():
    f, size_of = _fields(random_duplicate=True)
    rng = random.Random(11)
    subs, n_samples = [], 3000
    for _ in range(n_samples):
        r = synth.draw_recipe(rng, f, size_of)
        assert 1 <= len(r.subs) <= f.max_n_masks and r.crop_size == 384 and r.ignore_index == K.IGNORE
        subs += r.subs
    for s in subs:
        w, h = s.size
        assert s.p_mask == s.p_image.replace(".jpg", ".json") and s.label_id == f.p_image_to_label_id[s.p_image]
        assert int(w * 0.1) <= s.scaled[0] <= w and int(h * 0.1) <= s.scaled[1] <= h
        assert s.corner in (0, 1, 2, 3) and sorted(s.order) == [0, 1, 2, 3]
        assert all(0.0 <= u < 1.0 for u in (s.u_crop_top, s.u_crop_left, s.u_paste_top, s.u_paste_left))
        assert all(0.2 <= v <= 1.8 for v in (s.brightness, s.contrast, s.saturation))
        assert 0 <= s.hue_shift <= 255 and (s.hue_shift <= 51 or s.hue_shift >= 205)     # int(+-0.2 * 255) = +-51
        assert 0.1 <= s.sigma <= 2.0
    n = len(subs)
    z = 5.0         # a count of a Binomial(n, p) lies within z standard deviations of n p except with probability < 6e-7 (normal tail)
    for k, p in enumerate(synth.CORNER_P):
        count = sum(s.corner == k for s in subs)
        assert abs(count - n * p) <= z * math.sqrt(n * p * (1 - p)), (k, count, n * p)
    assert abs(sum(synth.CORNER_P) - 1.0) < 1e-12 and synth.CORNER_P[3] == 0.75 ** 3
    for name, p in (("flip", 0.5), ("jitter", 0.8), ("grey", 0.2), ("blur", 0.5)):
        count = sum(bool(getattr(s, name)) for s in subs)
        assert abs(count - n * p) <= z * math.sqrt(n * p * (1 - p)), (name, count, n * p)


def test_unserved_datasets_raise():
    for kw, word in (({"crop_size": None}, "crop_size"), ({"scale_range": None}, "scale_range")):
        f, size_of = _fields(**kw)
        with pytest.raises(NotImplementedError, match=word):
            synth.draw_recipe(random.Random(0), f, size_of)


# ------------------------------------------------------------------------------------------------------- files, packing, the chain
def test_sample_np_from_files_and_pack_layout(tmp_path):
    pairs, labels = K.corpus(tmp_path, 6)
    fields = synth.DatasetFields.from_dataset(K.Dataset(pairs, labels, crop_size=64))
    recipes = K.drawn_recipes(fields, 4, seed=3)
    out = synth.sample_np(recipes[0], blur=False)
    n = len(recipes[0].subs)
    assert out["image"].shape == (3, 64, 64) and out["image"].dtype == np.float32 and out["semantic_mask"].dtype == np.int64
    assert out["instance_mask"].shape == (n, 64, 64) and out["instance_mask"].dtype == bool and out["category_ids"] == recipes[0].category_ids
    arrays = [[synth.load_files(s) for s in r.subs] for r in recipes]
    again = synth.sample_np(recipes[0], arrays[0], blur=False)
    assert all(np.array_equal(out[k], again[k]) for k in ("image", "semantic_mask", "instance_mask"))
    packed = synth.pack_arrays(recipes, arrays)
    N = sum(len(r.subs) for r in recipes)
    assert packed.n_sub == N and packed.n_samples == 4 and packed.head % 16 == 0 and packed.ksize == synth.blur_ksize(64) == 7
    desc = packed.staging[:N * 128].numpy().view(np.int32).reshape(N, 32)
    pix = packed.staging[packed.head:].numpy()
    k = 0
    for r, arr in zip(recipes, arrays):
        for s, (image, mask) in zip(r.subs, arr):
            w, h = s.size
            assert tuple(desc[k, 1:5]) == (w, h) + tuple(s.scaled)
            assert np.array_equal(pix[desc[k, 0] * 16:desc[k, 0] * 16 + 3 * w * h].reshape(h, w, 3), image)
            assert np.array_equal(pix[desc[k, 5] * 16:desc[k, 5] * 16 + w * h].reshape(h, w), mask)
            k += 1


def test_blur_restatement_is_a_normalised_reflect101_gaussian():
    a = K.photo(40, 52, 5)
    w = synth.gaussian_weights(7, 1.3)
    assert abs(w.sum() - 1.0) < 1e-15 and np.allclose(w, w[::-1]) and np.isclose(w[2] / w[3], math.exp(-1 / (2 * 1.3 ** 2)))
    flat = np.full((20, 20, 3), 77, np.uint8)
    assert np.array_equal(synth.gaussian_blur_np(flat, 7, 0.4), flat)
    out = synth.gaussian_blur_f64(a, 7, 1.3)
    r = 3                               # the corner pixel by hand: indices reflect WITHOUT repeating the border (101)
    idx = [abs(t - r) for t in range(7)]
    want = sum(w[i] * w[j] * float(a[idx[i], idx[j], 0]) for i in range(7) for j in range(7))
    assert abs(out[0, 0, 0] - want) < 1e-9


def test_loader_batches_do_not_depend_on_workers(tmp_path):
    pairs, labels = K.corpus(tmp_path, 6)
    fields = synth.DatasetFields.from_dataset(K.Dataset(pairs, labels, crop_size=64))
    runs = []
    for workers in (1, 8):
        loader = synth.TrainBatchLoader(fields, batch_size=3, n_workers=workers, seed=5, n_batches=3, pin=False)
        assert len(loader) == 3 and loader.n_threads == workers
        runs.append([(b.recipes, K.packed_items(b.packed)) for b in loader])
    assert synth.TrainBatchLoader(fields, 3, n_workers=64, pin=False).n_threads == 16
    for (r1, items1), (r8, items8) in zip(*runs):
        assert r1 == r8 and len(items1) == len(items8) and all(np.array_equal(a, b) for a, b in zip(items1, items8))
    bad = synth.DatasetFields.from_dataset(K.Dataset(pairs[:1] + [(str(tmp_path / "missing.png"), pairs[1][1])], labels[:2], crop_size=64))
    with pytest.raises(FileNotFoundError):
        list(synth.TrainBatchLoader(bad, 2, n_workers=2, seed=0, n_batches=4, pin=False))
