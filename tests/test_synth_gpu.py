"""-m gpu: the kernels of csrc/synth.hip against the host restatements of zutis_amd.synth (which tests/test_synth_cpu.py pins against
Pillow, torch and the reference's copy_paste): every stage with torch.equal, whole samples bitwise with the blur disabled, the blur
stage within ONE level of its float64 evaluation, the loader, the adapter and HipCriterion on its batches."""
import random

import numpy as np
import pytest
import torch

import _synth_case as K
from zutis_amd import ops, preprocess, synth

pytestmark = pytest.mark.gpu

GEOMETRY = [((120, 160), 1.0, 64), ((120, 160), 0.1, 64), ((160, 120), 0.5, 64), ((200, 70), 0.6, 64), ((64, 300), 0.7, 64),
            ((90, 90), 0.3, 64), ((333, 250), 0.37, 96), ((64, 64), 1.0, 64), ((700, 500), 0.1, 64), ((375, 500), 0.93, 384),
            ((500, 375), 0.31, 384)]


def _stage_inputs(packed, dev):
    staged = packed.staging.to(dev)
    return synth.device_views(packed, staged)


def _geometry_batch(C):
    """One sample per (case of crop size C, corner, flip): (recipes, arrays)."""
    recipes, arrays = [], []
    for case, ((h, w), scale, c) in enumerate(GEOMETRY):
        if c != C:
            continue
        a, m = K.photo(h, w, case), K.blob(h, w, case, "border" if case % 3 == 0 else "ellipse")
        for corner in range(4):
            for flip in (False, True):
                s = K.sub((w, h), scale, corner=corner, u_crop=(0.13 + 0.2 * corner, 0.91 - 0.2 * corner), flip=flip, label=2)
                recipes.append(synth.SampleRecipe([s], C, K.IGNORE))
                arrays.append([(a, m)])
    return recipes, arrays


@pytest.mark.parametrize("C", [64, 96, 384])
def test_geometry_stage(dev, C):
    recipes, arrays = _geometry_batch(C)
    packed = synth.pack_arrays(recipes, arrays)
    desc, samples, work, weights, pix = _stage_inputs(packed, dev)
    out = ops.synth_geometry(pix, desc, C, K.IGNORE, packed.kmax, packed.fill_wh, work).cpu().numpy()
    boxes = work.cpu().numpy()[:, 8:]
    for n, (r, arr) in enumerate(zip(recipes, arrays)):
        img, mask = synth.geometry_np(*arr[0], r.subs[0], C, K.IGNORE)
        assert np.array_equal(out[n, ..., :3], img), (n, r.subs[0])
        assert np.array_equal(out[n, ..., 3], mask), (n, r.subs[0])
        box = synth.object_box(mask, 2, K.IGNORE)
        assert (boxes[n, 1] < 0) if box is None else (tuple(boxes[n]) == box)


def _photo_recipes(n, seed):
    rng = random.Random(seed)
    subs = []
    for k in range(n):
        order = list(range(4))
        rng.shuffle(order)
        subs.append(K.sub((64, 64), 1.0, jitter=(k % 5 != 4), order=order, factors=tuple(rng.uniform(0.2, 1.8) for _ in range(3)),
                          hue=synth.hue_shift(rng.uniform(-0.2, 0.2)), grey=(k % 3 == 0)))
    subs.append(K.sub((64, 64), 1.0, jitter=True, order=(2, 0, 1, 3), factors=(1.0, 1.0, 1.0), hue=128))
    subs.append(K.sub((64, 64), 1.0, jitter=True, order=(3, 1, 0, 2), factors=(1.8, 0.2, 0.2), hue=0, grey=True))
    return subs


def test_photometric_stage(dev):
    subs = _photo_recipes(22, 4)
    arrays = [[(K.photo(64, 64, 200 + k), K.blob(64, 64, k))] for k in range(len(subs))]
    arrays[3][0] = (np.stack(np.meshgrid(np.arange(64), np.arange(64)), -1).astype(np.uint8).repeat(2, -1)[..., :3] * 4, arrays[3][0][1])
    recipes = [synth.SampleRecipe([s], 64, K.IGNORE) for s in subs]
    packed = synth.pack_arrays(recipes, arrays)
    desc, samples, work, weights, pix = _stage_inputs(packed, dev)
    rgbm = ops.synth_geometry(pix, desc, 64, K.IGNORE, packed.kmax, packed.fill_wh, work)
    before = rgbm.cpu().numpy()
    after = ops.synth_photometric(rgbm, desc, work).cpu().numpy()
    for n, s in enumerate(subs):
        assert np.array_equal(before[n, ..., :3], arrays[n][0][0])            # scale 1.0, no pad: the geometry is the identity
        assert np.array_equal(after[n, ..., :3], synth.photometric_np(before[n, ..., :3], s)), (n, s)
        assert np.array_equal(after[n, ..., 3], before[n, ..., 3])


def test_hue_round_trip_on_a_colour_cube_slice(dev):
    """4096 x 64 colours per shift through the kernel's RGB -> HSV -> RGB: the planes the two restatements were closed on."""
    g = np.arange(64, dtype=np.uint8) * 4 + 1
    subs, arrays = [], []
    for k, shift in enumerate((0, 1, 37, 128, 205, 255)):
        r = np.full((64, 64), (41 * k + 7) % 256, np.uint8)
        a = np.stack([r, np.repeat(g[:, None], 64, 1), np.repeat(g[None, :], 64, 0)], -1)
        a = np.roll(a, k, axis=-1)
        subs.append(K.sub((64, 64), 1.0, jitter=True, order=(3, 0, 1, 2), hue=shift))
        arrays.append([(np.ascontiguousarray(a), K.blob(64, 64, 1))])
    recipes = [synth.SampleRecipe([s], 64, K.IGNORE) for s in subs]
    packed = synth.pack_arrays(recipes, arrays)
    desc, samples, work, weights, pix = _stage_inputs(packed, dev)
    rgbm = ops.synth_geometry(pix, desc, 64, K.IGNORE, packed.kmax, packed.fill_wh, work)
    after = ops.synth_photometric(rgbm, desc, work).cpu().numpy()
    for n, s in enumerate(subs):
        assert np.array_equal(after[n, ..., :3], synth.photometric_np(arrays[n][0][0], s)), n


@pytest.mark.parametrize("C", [64, 384])
def test_blur_stage_within_one_level(dev, C):
    """fp32 sums of at most 39 products of a byte and a weight (the weights sum to 1) are within 39 * 2^-24 * 255 < 1e-3 of the exact
    value per pass, so the rounded byte can differ from the rounded float64 value by one level and no more."""
    sigmas = (0.1, 0.35, 1.0, 2.0)
    subs = [K.sub((C, C), 1.0, blur=(k != 2), sigma=sigmas[k % 4]) for k in range(5)]
    arrays = [[(K.photo(C, C, 300 + k), K.blob(C, C, k))] for k in range(5)]
    recipes = [synth.SampleRecipe([s], C, K.IGNORE) for s in subs]
    packed = synth.pack_arrays(recipes, arrays)
    desc, samples, work, weights, pix = _stage_inputs(packed, dev)
    rgbm = ops.synth_geometry(pix, desc, C, K.IGNORE, packed.kmax, packed.fill_wh, work)
    canary = torch.full_like(rgbm, 7)
    out = ops.synth_blur(rgbm, desc, weights, out=canary).cpu().numpy()
    ks = synth.blur_ksize(C)
    assert ks == {64: 7, 384: 39}[C]
    differing = total = 0
    for n, s in enumerate(subs):
        if not s.blur:
            assert (out[n] == 7).all()                  # not written: compose reads such a sub-image from the plain buffer
            continue
        exact = synth.gaussian_blur_f64(arrays[n][0][0], ks, s.sigma)
        want = np.clip(np.rint(exact), 0, 255).astype(np.int64)
        d = np.abs(out[n, ..., :3].astype(np.int64) - want)
        differing, total = differing + int((d != 0).sum()), total + d.size
        print(f"blur C={C} sigma={s.sigma}: max |diff| = {int(d.max())} levels, {int((d != 0).sum())} of {d.size} bytes differ")
        assert int(d.max()) <= 1
        assert np.array_equal(out[n, ..., 3], rgbm.cpu().numpy()[n, ..., 3])
    print(f"blur C={C}: share of bytes off by one level = {differing / total:.3e}")


def _compose_case(kind, C=32):
    rng = np.random.default_rng(len(kind))

    def rect(y0, y1, x0, x1):
        m = np.zeros((C, C), np.uint8)
        m[y0:y1, x0:x1] = 1
        return m

    if kind == "empty":
        masks = [rect(4, 20, 4, 20), np.zeros((C, C), np.uint8), rect(10, 18, 12, 30)]
    elif kind == "overwritten":
        masks = [rect(2, 8, 2, 8), rect(10, 20, 10, 20), rect(9, 22, 9, 22)]
    elif kind == "border":
        masks = [rect(0, C, 0, 5), rect(0, 12, 0, 12), rect(20, C, 18, C)]
    elif kind == "ignore0":
        m0 = rect(12, 28, 12, 28)
        m0[:10] = K.IGNORE
        m1 = rect(5, 25, 3, 17)
        m1[:, 20:] = K.IGNORE
        masks = [m0, m1]
    else:
        masks = [K.blob(C, C, 50 + k) for k in range(10)]
    n = len(masks)
    images = [rng.integers(0, 256, (C, C, 3), dtype=np.uint8) for _ in range(n)]
    us = rng.random((n, 2))
    if kind == "overwritten":
        us[1] = us[2] = (0.4, 0.4)
    subs = [K.sub((C, C), 1.0, u_paste=(float(us[k, 0]), float(us[k, 1])), label=3 + k) for k in range(n)]
    return images, masks, synth.SampleRecipe(subs, C, K.IGNORE)


def test_compose_stage(dev):
    """All five copy_paste cases as one batch: the sub-images enter through the geometry stage as identity crops (scale 1, no pad), with
    masks that hold ignore pixels already."""
    kinds = ["empty", "overwritten", "border", "ignore0", "many"]
    cases = [_compose_case(k) for k in kinds]
    recipes = [c[2] for c in cases]
    arrays = [list(zip(c[0], c[1])) for c in cases]
    packed = synth.pack_arrays(recipes, arrays)
    desc, samples, work, weights, pix = _stage_inputs(packed, dev)
    rgbm = ops.synth_geometry(pix, desc, 32, K.IGNORE, packed.kmax, packed.fill_wh, work)
    lut_np = preprocess.normalise_table(synth.MEAN, synth.STD)
    image, semantic, onehot = ops.synth_compose(rgbm, rgbm, desc, samples, work, torch.from_numpy(lut_np).to(dev), K.IGNORE)
    rows = torch.split(onehot, [len(r.subs) for r in recipes], 0)
    for b, (images, masks, recipe) in enumerate(cases):
        u8, sem, oh = synth.compose_np(images, masks, recipe)
        assert torch.equal(image[b].cpu(), torch.from_numpy(synth.normalise_np(u8, lut_np))), kinds[b]
        assert torch.equal(semantic[b].cpu(), torch.from_numpy(sem)), kinds[b]
        assert rows[b].dtype == torch.bool and torch.equal(rows[b].cpu(), torch.from_numpy(oh)), kinds[b]


def _assert_batch_equal(out, recipes, arrays=None):
    B = len(recipes)
    C = recipes[0].crop_size
    assert out["image"].shape == (B, 3, C, C) and out["image"].dtype == torch.float32
    assert out["semantic_mask"].shape == (B, C, C) and out["semantic_mask"].dtype == torch.int64
    assert len(out["instance_mask"]) == B and len(out["category_ids"]) == B
    for b, r in enumerate(recipes):
        want = synth.sample_np(r, None if arrays is None else arrays[b], blur=False)
        assert torch.equal(out["image"][b].cpu(), torch.from_numpy(want["image"])), b
        assert torch.equal(out["semantic_mask"][b].cpu(), torch.from_numpy(want["semantic_mask"])), b
        assert out["instance_mask"][b].dtype == torch.bool and out["instance_mask"][b].shape == (len(r.subs), C, C)
        assert torch.equal(out["instance_mask"][b].cpu(), torch.from_numpy(want["instance_mask"])), b
        assert out["category_ids"][b] == want["category_ids"]


def _hand_batch(tmp_path, C):
    """A ragged batch of 8 samples with 1, 2 and 10 sub-images among them, every edge of the stages in it."""
    pairs, labels = K.corpus(tmp_path, 8)
    pairs.append(K.write_pair(tmp_path, "empty", 100, 140, 77, kind="empty"))
    pairs.append(K.write_pair(tmp_path, "full", 80, 80, 78, kind="full", jpeg=True))
    pairs.append(K.write_pair(tmp_path, "big", 500, 640, 79, jpeg=True))            # larger than a 384 crop: no padding at scale 0.8 and 1.0
    labels += [4, 2, 3]
    rng = random.Random(21)
    counts = [1, 2, 10, 3, 1, 5, 2, 7]
    recipes = []
    for b, n in enumerate(counts):
        subs = []
        for k in range(n):
            i = (3 * b + k) % len(pairs)
            w, h = synth.image_size(pairs[i][0])
            order = list(range(4))
            rng.shuffle(order)
            scale = (0.1, 1.0, 0.45, 0.8, 0.27)[(b + k) % 5]
            subs.append(K.sub((w, h), scale, corner=(b + k) % 4, u_crop=(rng.random(), rng.random()), flip=bool((b + k) % 2), jitter=(k % 4 != 3),
                              order=order, factors=tuple(rng.uniform(0.2, 1.8) for _ in range(3)), hue=synth.hue_shift(rng.uniform(-0.2, 0.2)),
                              grey=(k % 5 == 2), blur=(k % 2 == 0), sigma=rng.uniform(0.1, 2.0), u_paste=(rng.random(), rng.random()),
                              label=labels[i], p_image=pairs[i][0], p_mask=pairs[i][1]))
        recipes.append(synth.SampleRecipe(subs, C, K.IGNORE))
    return recipes


@pytest.mark.parametrize("C", [64, 384])
def test_whole_samples_bitwise_without_blur(dev, tmp_path, C):
    recipes = _hand_batch(tmp_path, C)
    assert sorted({len(r.subs) for r in recipes})[:2] == [1, 2] and max(len(r.subs) for r in recipes) == 10 and len(recipes) == 8
    arrays = [[synth.load_files(s) for s in r.subs] for r in recipes]
    out = synth.synthesize(synth.pack_arrays(recipes, arrays), recipes, device=dev, blur=False)
    _assert_batch_equal(out, recipes, arrays)


def test_whole_samples_with_blur_within_one_level(dev, tmp_path):
    C = 64
    recipes = _hand_batch(tmp_path, C)
    arrays = [[synth.load_files(s) for s in r.subs] for r in recipes]
    out = synth.synthesize(synth.pack_arrays(recipes, arrays), recipes, device=dev, stages=True)
    u8 = out["u8"].cpu().numpy()
    n = 0
    for b, r in enumerate(recipes):
        host = synth.sample_np(r, arrays[b], blur=False, stages=True)
        for k, s in enumerate(r.subs):
            if s.blur:
                want = np.clip(np.rint(synth.gaussian_blur_f64(host["u8"][k], synth.blur_ksize(C), s.sigma)), 0, 255).astype(np.int64)
                assert int(np.abs(u8[n, ..., :3].astype(np.int64) - want).max()) <= 1, (b, k)
            else:
                assert np.array_equal(u8[n, ..., :3], host["u8"][k]), (b, k)
            assert np.array_equal(u8[n, ..., 3], host["masks"][k]), (b, k)
            n += 1
    # masks do not depend on the blur: semantic and instance maps stay bitwise
    for b, r in enumerate(recipes):
        want = synth.sample_np(r, arrays[b], blur=False)
        assert torch.equal(out["semantic_mask"][b].cpu(), torch.from_numpy(want["semantic_mask"]))
        assert torch.equal(out["instance_mask"][b].cpu(), torch.from_numpy(want["instance_mask"]))


def test_host_scaled_source_outside_the_tap_envelope(dev):
    """A 16000-pixel side scaled to 100 needs 321 taps: Pillow scales it in the decode path and the kernel sees an identity image."""
    h, w = 24, 16000
    a, m = K.photo(h, w, 9), K.blob(h, w, 9)
    s = K.sub((w, h), 1.0, corner=3)
    s.scaled = (100, 24)
    recipes = [synth.SampleRecipe([s], 64, K.IGNORE)]
    packed = synth.pack_arrays(recipes, [[(a, m)]])
    assert packed.n_host == 1
    _assert_batch_equal(synth.synthesize(packed, recipes, device=dev, blur=False), recipes, [[(a, m)]])


def test_loader_identical_for_1_and_8_workers(dev, tmp_path):
    pairs, labels = K.corpus(tmp_path, 8)
    ds = K.Dataset(pairs, labels, crop_size=64, device=dev)
    fields = synth.DatasetFields.from_dataset(ds)
    runs = []
    for workers in (1, 8):
        loader = synth.TrainBatchLoader(fields, batch_size=4, n_workers=workers, seed=9, n_batches=3)
        runs.append([{k: (v.clone() if torch.is_tensor(v) else [t.clone() if torch.is_tensor(t) else t for t in v]) for k, v in out.items()}
                     for out in loader.batches(dev)])
    assert len(runs[0]) == len(runs[1]) == 3
    for a, b in zip(*runs):
        assert torch.equal(a["image"], b["image"]) and torch.equal(a["semantic_mask"], b["semantic_mask"]) and a["category_ids"] == b["category_ids"]
        assert all(torch.equal(x, y) for x, y in zip(a["instance_mask"], b["instance_mask"]))
    # and the batches are the host chain's (the blur aside): the first batch again, through the recipes the loader drew
    batch = next(iter(synth.TrainBatchLoader(fields, batch_size=4, n_workers=2, seed=9, n_batches=1)))
    _assert_batch_equal(synth.synthesize(batch.packed, batch.recipes, device=dev, blur=False), batch.recipes)


def test_adapter_batch_goes_into_the_criterion(dev, tmp_path):
    from zutis_amd.criterion import HipCriterion
    pairs, labels = K.corpus(tmp_path, 8)
    ds = K.Dataset(pairs, labels, crop_size=64, device=dev)
    batch = next(iter(synth.dataset_train_batches(ds, batch_size=4, n_workers=4, seed=1, n_batches=1)))
    assert batch["image"].is_cuda and batch["image"].shape == (4, 3, 64, 64) and torch.isfinite(batch["image"]).all()
    g = torch.Generator().manual_seed(0)
    n_cat, D, Q = 6, 16, 12
    te = torch.nn.functional.normalize(torch.randn(n_cat, D, generator=g), dim=-1).to(dev)
    props = torch.rand(4, Q, 16, 16, generator=g).to(dev).requires_grad_()
    tokens = torch.randn(4, 8, 8, D, generator=g).to(dev).requires_grad_()
    out = HipCriterion(te, ignore_index=K.IGNORE)(props, batch["instance_mask"], batch["category_ids"], tokens, batch["semantic_mask"])
    assert np.isfinite(out["ce_loss"]) and np.isfinite(out["mask_loss"]) and torch.isfinite(out["loss"])
    out["loss"].backward()
    assert torch.isfinite(props.grad).all() and torch.isfinite(tokens.grad).all()


def test_unserved_datasets_raise(dev, tmp_path):
    pairs, labels = K.corpus(tmp_path, 2)
    with pytest.raises(NotImplementedError, match="crop_size"):
        next(iter(synth.dataset_train_batches(K.Dataset(pairs, labels, crop_size=None, device=dev), batch_size=2)))
    with pytest.raises(NotImplementedError, match="scale_range"):
        next(iter(synth.dataset_train_batches(K.Dataset(pairs, labels, scale_range=None, device=dev), batch_size=2)))
