"""CPU: the host side of pseudo-label generation from image files (zutis_amd/preprocess.py: the filter argument of the NumPy
restatement of Pillow's resampler, MaskDataset's size rule, the shape-bucketing loader) and the new entry point's declaration.
The bilinear restatement is compared with the installed Pillow byte for byte: it is the oracle's oracle of the GPU tests."""
import random
import re

import numpy as np
import pytest
import torch
from PIL import Image

from tests import _preprocess_case as PC
from zutis_amd import _lib, preprocess as P

IMAGE_SIZE = 512
# the shapes Pillow's resampler was restated on (tests/_preprocess_case.py), each in both orientations, with 512 in place of n_px,
# and sources whose shorter side already is 512 (one or both passes are the identity: Pillow skips them)
SHAPES = list(dict.fromkeys([(h, w) for h, w, _ in PC.SHAPES] + [(w, h) for h, w, _ in PC.SHAPES] + [(512, 512), (512, 700), (700, 512)]))


def _torchvision_rule(w, h, size):
    """torchvision.transforms.functional.resize(img, int) as MaskDataset calls it (datasets/index_dataset.py:408-409), restated from
    its published source: unchanged when the shorter side is `size`, else short -> size, long -> int(size * long / short)."""
    if size is None:
        return w, h
    short, long = (w, h) if w <= h else (h, w)
    if short == size:
        return w, h
    new_short, new_long = size, int(size * long / short)
    return (new_short, new_long) if w <= h else (new_long, new_short)


@pytest.mark.parametrize("h,w", SHAPES)
def test_bilinear_restatement_equals_pillow_byte_for_byte(h, w):
    a = PC.pixels(h, w, seed=h * 10007 + w)
    nw, nh = P.mask_dataset_size(w, h, IMAGE_SIZE)
    ref = np.asarray(Image.fromarray(a).resize((nw, nh), Image.BILINEAR))
    got = P.pil_resize_reference(a, nw, nh, filter="bilinear")
    assert got.shape == ref.shape and got.dtype == np.uint8
    bad = int((got != ref).sum())
    assert bad == 0, f"{h}x{w} -> {nh}x{nw}: {bad} of {ref.size} bytes differ from Pillow {Image.__version__} BILINEAR"


@pytest.mark.parametrize("h,w,n_px", [(375, 500, 336), (640, 427, 224), (64, 48, 224), (336, 500, 336)])
def test_bicubic_through_the_filter_argument_is_the_old_function(h, w, n_px):
    a = PC.pixels(h, w, seed=h + w)
    (nw, nh), _ = PC.dropin().resize_crop_box(w, h, n_px)
    old = P.pil_resize_reference(a, nw, nh)
    assert np.array_equal(P.pil_resize_reference(a, nw, nh, filter="bicubic"), old)
    assert np.array_equal(old, np.asarray(Image.fromarray(a).resize((nw, nh), Image.BICUBIC)))
    for i, o in ((w, nw), (h, nh)):
        assert P.ksize(i, o) == P.ksize(i, o, "bicubic")
        (k0, b0), (k1, b1) = P.pil_coefficients(i, o), P.pil_coefficients(i, o, "bicubic")
        assert np.array_equal(k0, k1) and np.array_equal(b0, b1)


def test_bilinear_taps_and_identity_pass():
    assert P.ksize(375, 512, "bilinear") == 3 and P.ksize(512, 512, "bilinear") == 3 and P.ksize(2000, 682, "bilinear") == 7
    assert P.ksize(75 * 64, 64, "bilinear") == 151 <= P.KMAX < P.ksize(76 * 64, 64, "bilinear")
    kk, bounds = P.pil_coefficients(512, 512, "bilinear")        # an unchanged axis: one unit tap — the identity
    assert all(int(kk[i, :bounds[i, 1]].sum()) == 1 << 22 and int((kk[i] != 0).sum()) == 1 for i in range(512))
    a = PC.pixels(40, 52, seed=1)
    assert np.array_equal(P.pil_resize_reference(a, 52, 40, "bilinear"), a)


def test_size_rule_is_mask_datasets():
    want = {(375, 500): (682, 512), (500, 375): (512, 682), (333, 500): (768, 512), (427, 640): (767, 512), (640, 427): (512, 767),
            (17, 900): (27105, 512), (512, 700): (700, 512), (700, 512): (512, 700), (512, 512): (512, 512), (2000, 1500): (512, 682)}
    for (h, w), (nw, nh) in want.items():                     # (h, w) of the file -> (nw, nh), worked out by hand
        assert P.mask_dataset_size(w, h, IMAGE_SIZE) == (nw, nh), (h, w)
    for h, w in SHAPES:
        for size in (IMAGE_SIZE, 64, 333, None):
            assert P.mask_dataset_size(w, h, size) == _torchvision_rule(w, h, size), (h, w, size)
    assert P.mask_dataset_size(640, 427, None) == (640, 427)
    try:                                                         # the real thing, where torchvision is installed
        import torchvision.transforms.functional as TF
    except ImportError:
        return
    for h, w in SHAPES[:8]:
        assert TF.resize(Image.new("RGB", (w, h)), size=IMAGE_SIZE, interpolation=Image.BILINEAR).size == P.mask_dataset_size(w, h, IMAGE_SIZE)


def test_normalise_table_is_the_torch_normalisation():
    """MaskDataset normalises in torch (to_tensor: byte / 255 in fp32; normalize: (x - mean) / std with fp32 tensors): the table the
    kernel gathers from holds those values bit for bit."""
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    x = torch.arange(256, dtype=torch.uint8)[None, :, None].expand(3, 256, 1).contiguous().to(torch.float32).div(255)
    ref = (x - torch.tensor(mean, dtype=torch.float32)[:, None, None]) / torch.tensor(std, dtype=torch.float32)[:, None, None]
    assert np.array_equal(P.normalise_table(mean, std), ref[:, :, 0].numpy())


# ------------------------------------------------------------------------------------------------------------------ bucketing
def _consecutive_groups(keys, batch_size):
    """The parent's grouping (pseudo_masks.dataset_generate_pseudo_masks): consecutive images of one shape, up to batch_size."""
    out = []
    for i, k in enumerate(keys):
        if out and keys[out[-1][0]] == k and len(out[-1]) < batch_size:
            out[-1].append(i)
        else:
            out.append([i])
    return out


def _check_grouping(groups, keys, batch_size):
    assert sorted(i for g in groups for i in g) == list(range(len(keys)))            # every image exactly once
    assert all(1 <= len(g) <= batch_size and len({keys[i] for i in g}) == 1 for g in groups)


def test_bucket_batches_full_batches_where_consecutive_grouping_gives_singletons():
    keys = [k % 4 for k in range(64)]
    random.Random(2024).shuffle(keys)
    for window in (64, 100, 512):
        groups = P.bucket_batches(keys, 8, window)
        _check_grouping(groups, keys, 8)
        assert len(groups) == 8 and all(len(g) == 8 for g in groups)
        assert groups == P.bucket_batches(list(keys), 8, window)                       # a function of its arguments
    old = _consecutive_groups(keys, 8)
    _check_grouping(old, keys, 8)
    singles = sum(len(g) == 1 for g in old)
    print(f"consecutive grouping: {len(old)} groups, {singles} singletons, mean {64 / len(old):.2f}; bucketed: 8 groups of 8")
    assert singles > len(old) / 2 and len(old) > 4 * len(groups)


def test_bucket_batches_window_bounds_the_wait():
    keys = ["a"] + ["b"] * 20 + ["a"] + ["c"]
    groups = P.bucket_batches(keys, 8, 4)
    _check_grouping(groups, keys, 8)
    assert groups[0] == [0]                                        # the lone "a" leaves when the window closes on it, before any "b" batch fills
    assert [21] in groups and groups[-1] == [22]
    assert max(max(g) - min(g) for g in groups) <= 8               # no image waits beyond the window (or its own batch)
    assert P.bucket_batches([], 8, 4) == [] and P.bucket_batches(keys, 1, 4) == [[i] for i in range(len(keys))]
    with pytest.raises(ValueError):
        P.bucket_batches(keys, 0, 4)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """4 source shapes x 16 files in a seeded shuffle: (paths, (h, w) of each)."""
    d = tmp_path_factory.mktemp("bucket_corpus")
    shapes = [(20, 30), (30, 20), (24, 24), (18, 40)]
    hw = [shapes[k % 4] for k in range(64)]
    random.Random(7).shuffle(hw)
    return [PC.write_rgb(d, f"f{k:02d}.png", h, w, seed=300 + k) for k, (h, w) in enumerate(hw)], hw


@pytest.mark.parametrize("n_workers", [1, 4])
def test_shape_bucket_loader_on_files(corpus, n_workers):
    paths, hw = corpus
    image_size, batch_size = 32, 8
    keys = [P.mask_dataset_size(w, h, image_size) for h, w in hw]
    want = P.bucket_batches(keys, batch_size, 64)
    runs = []
    for _ in range(2):
        got = []
        for batch in P.ShapeBucketLoader(paths, image_size, batch_size, n_workers, window=64, pin=False):
            B, (oh, ow) = len(batch.paths), batch.out_hw
            assert batch.n_host == 0 and batch.kmax == 3 and batch.desc.shape == (B, 8)
            assert batch.paths == [paths[i] for i in batch.indices] and batch.sizes_hw == [hw[i] for i in batch.indices]
            for i, row in zip(batch.indices, batch.desc.tolist()):
                h, w = hw[i]
                assert keys[i] == (ow, oh) and row[1:] == [w, h, ow, oh, 0, 0, 0]
                off = row[0] * 16
                ref = np.asarray(Image.open(paths[i]).convert("RGB"))
                assert np.array_equal(batch.packed.numpy()[off:off + 3 * w * h].reshape(h, w, 3), ref)
            got.append(list(batch.indices))
        runs.append(got)
    assert runs[0] == runs[1] == want                              # deterministic, and the documented function of the list
    _check_grouping(runs[0], keys, batch_size)
    assert all(len(g) == batch_size for g in runs[0])
    old = _consecutive_groups(keys, batch_size)
    assert sum(len(g) == 1 for g in old) > len(old) / 2


def test_shape_bucket_loader_small_window_no_resize_and_thread_cap(corpus):
    paths, hw = corpus
    loader = P.ShapeBucketLoader(paths, None, 4, 64, window=8, pin=False)            # image_size None: buckets of the files' own shapes
    assert loader.n_threads == 16
    groups = [(list(b.indices), b.out_hw) for b in loader]
    assert [g for g, _ in groups] == P.bucket_batches([(w, h) for h, w in hw], 4, 8)
    assert all(out_hw == hw[g[0]] for g, out_hw in groups)
    _check_grouping([g for g, _ in groups], hw, 4)
    assert list(P.ShapeBucketLoader([], 32, 4, 2, pin=False)) == []


def test_shape_bucket_loader_missing_file_raises(corpus, tmp_path):
    paths, _ = corpus
    bad = paths[:20] + [str(tmp_path / "missing.png")] + paths[20:30]
    with pytest.raises(FileNotFoundError):
        for _ in P.ShapeBucketLoader(bad, 32, 8, 4, window=16, pin=False):
            pass
    broken = tmp_path / "broken.png"
    broken.write_bytes(open(paths[0], "rb").read()[:40])           # a header that ends early
    with pytest.raises(Exception):
        for _ in P.ShapeBucketLoader(paths[:5] + [str(broken)], 32, 8, 4, window=16, pin=False):
            pass


def test_loader_resizes_on_the_host_outside_the_envelope(tmp_path):
    """THE designated image: 200 x 160 at image_size 2 resizes to 2 x 2 and needs 161 / 201 taps per output pixel (> KMAX): its worker
    hands over Pillow's own BILINEAR result and a descriptor whose two passes are the identity."""
    big = PC.write_rgb(tmp_path, "big.png", 160, 200, seed=9)
    small = PC.write_rgb(tmp_path, "small.png", 4, 5, seed=10)
    assert P.mask_dataset_size(200, 160, 2) == (2, 2) == P.mask_dataset_size(5, 4, 2)
    assert P.ksize(160, 2, "bilinear") == 161 > P.KMAX and P.ksize(5, 2, "bilinear") == 7
    (batch,) = list(P.ShapeBucketLoader([big, small], 2, 2, 2, pin=False))
    assert batch.n_host == 1 and batch.out_hw == (2, 2) and batch.sizes_hw == [(160, 200), (4, 5)] and batch.kmax == 7
    assert batch.desc.tolist() == [[0, 2, 2, 2, 2, 0, 0, 0], [1, 5, 4, 2, 2, 0, 0, 0]]
    ref = np.asarray(Image.open(big).convert("RGB").resize((2, 2), Image.BILINEAR))
    assert np.array_equal(batch.packed.numpy()[:12].reshape(2, 2, 3), ref)


def test_entry_point_is_declared_exported_and_the_abi_moved():
    import ctypes
    e = _lib.entries()["zh_resize_normalize_u8"]
    assert [n for _, n in e.params] == ["packed", "packed_bytes", "desc", "B", "out_h", "out_w", "filter", "kmax", "lut", "out", "stream"]
    assert e.plannable and e.params[1][0] == "long" and e.params[-1][0] == "zh_stream_t"
    assert "zh_resize_crop_normalize_u8" in _lib.entries()          # the crop entry keeps its declaration
    assert len(_lib.entries()["zh_resize_crop_normalize_u8"].params) == 9
    text = open(_lib.HEADER).read()
    assert re.search(r"^#define\s+ZH_FILTER_BILINEAR\s+2\b", text, re.M) and re.search(r"^#define\s+ZH_FILTER_BICUBIC\s+3\b", text, re.M)
    assert (Image.BILINEAR, Image.BICUBIC) == (2, 3)
    assert _lib.header_abi_version() > 228                           # 228 declared zh_resize_crop_normalize_u8 alone
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "zh_resize_normalize_u8") and lib.zh_version() == _lib.header_abi_version()
    # argument validation happens before any launch
    bound = _lib.load(raw=True)
    assert bound.zh_resize_normalize_u8(None, 0, None, 0, 0, 0, 2, 3, None, None, None) == -1 and b"null" in bound.zh_last_error()


def test_numpy_rle_decode_is_the_python_decode(golden_dir):
    """rle.decode_np (the writers' read-back check) against rle.decode on the hand-derived format vectors (multi-character values,
    negative deltas, the sign-guard group) and on random, empty, full and photograph-sized masks, bytes and str counts alike."""
    import json
    from zutis_amd import rle
    for v in json.load(open(f"{golden_dir}/rle_vectors.json"))["vectors"]:
        r = {"size": v["size"], "counts": v["counts"]}
        assert np.array_equal(rle.decode_np(r), rle.decode(r)), v["name"]
    rng = np.random.default_rng(11)
    masks = [np.zeros((5, 7), np.uint8), np.ones((5, 7), np.uint8), np.zeros((0, 0), np.uint8), np.eye(9, dtype=np.uint8)]
    masks += [(rng.random(tuple(rng.integers(1, 90, 2))) < rng.random()).astype(np.uint8) for _ in range(40)]
    big = np.zeros((1200, 1600), np.uint8)
    big[100:1100, 5:1500] = 1                                    # runs of 1000 and 200: two- and three-character values
    big[0, 0] = 1                                                # pixel 0 set: the leading empty run of zeros
    big[300:900:7, 40:1400:3] = 0
    masks.append(big)
    for m in masks:
        r = rle.encode_py(m)
        assert np.array_equal(rle.decode_np(r), m) and np.array_equal(rle.decode(r), m), m.shape
        assert np.array_equal(rle.decode_np({"size": r["size"], "counts": r["counts"].decode("ascii")}), m)
