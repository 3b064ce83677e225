"""Host side of evaluation from files (zutis_amd/evaluate.py, preprocess.EvalBatchLoader): the ImageNet-S size rule, the loader's grouping
and staging, the ground-truth checks, the dataset adapter and the C declaration.  No GPU."""
import importlib.util
import os
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from tests import _preprocess_case as PC
from zutis_amd import _lib, evaluate
from zutis_amd import preprocess as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the size rule
# (w, h, max_size) -> (nw, nh), by hand from compute_size's `int(float(a) / b * size)` (the quotient first, then truncation)
SIZE_CASES = [
    ((1600, 1200, 1024), (1024, 768)),          # landscape, exact: 0.75 * 1024
    ((1200, 1600, 1024), (768, 1024)),          # portrait
    ((1500, 1001, 1024), (1024, 683)),          # 1001 / 1500 * 1024 = 683.349... truncates
    ((1001, 1500, 1024), (683, 1024)),
    ((1025, 1024, 1024), (1024, 1023)),         # 1024 / 1025 * 1024 = 1023.0009...
    ((2000, 2000, 1024), (1024, 1024)),         # square: the `else` branch, 1.0 * 1024
    ((1024, 700, 1024), (1024, 700)),           # a side exactly AT max_size: untouched
    ((700, 1024, 1024), (700, 1024)),
    ((640, 480, 1024), (640, 480)),             # below the cap
    ((3000, 7, 1024), (1024, 2)),               # 7 / 3000 * 1024 = 2.389...
    ((500, 375, 96), (96, 72)),
    ((640, 480, None), (640, 480)),             # no cap at all (coco2017.py, coco20k.py)
]


@pytest.mark.parametrize("args,want", SIZE_CASES)
def test_longer_edge_size_by_hand(args, want):
    assert P.longer_edge_size(*args) == want


def _reference_compute_size():
    base = os.environ.get("ZUTIS_REFERENCE_DIR") or os.path.join(os.path.dirname(ROOT), "reference")
    path = os.path.join(base, "datasets", "augmentations", "geometric_transforms.py")
    if not os.path.exists(path):
        return None
    try:
        spec = importlib.util.spec_from_file_location("zutis_reference_geometric_transforms", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    except ImportError:                         # its imports (torchvision) are not dependencies of this project
        return None
    return mod.compute_size


def test_longer_edge_size_equals_the_reference_compute_size():
    compute_size = _reference_compute_size()
    if compute_size is None:
        pytest.skip("no importable reference checkout next to the repository (ZUTIS_REFERENCE_DIR)")
    rng = np.random.default_rng(5)
    cases = [a[:2] for a, _ in SIZE_CASES] + [tuple(int(v) for v in rng.integers(1025, 5000, 2)) for _ in range(300)]
    for w, h in cases:
        for size in (1024, 640, 97):
            if max(w, h) > size:                # imagenet_s.py:73 resizes only then
                rh, rw = compute_size(input_size=(h, w), output_size=size, edge="longer")
                assert P.longer_edge_size(w, h, size) == (rw, rh), (w, h, size)


# ------------------------------------------------------------------------------------------------------------------ grouping
def test_grouping_is_bucket_batches_of_resized_and_ground_truth_shape():
    wh = [(96, 64), (64, 80), (96, 64), (192, 128), (80, 48), (64, 80), (96, 64), (80, 48), (64, 80), (96, 64)]
    keys = [P.eval_bucket_key(w, h, w, h, 96) for w, h in wh]
    assert keys[0] == ((96, 64), (96, 64)) and keys[3] == ((96, 64), (192, 128))       # the same resized shape, another file size: apart
    groups = P.bucket_batches(keys, 3, 512)
    assert groups == [[0, 2, 6], [1, 5, 8], [3], [4, 7], [9]]        # full buckets as they fill, then the rest, oldest image first
    assert sorted(i for g in groups for i in g) == list(range(10)) and all(len({keys[i] for i in g}) == 1 for g in groups)
    assert P.bucket_batches(keys, 1, 512) == [[i] for i in range(10)]
    assert P.eval_bucket_key(640, 480, 640, 480, None) == ((640, 480), (640, 480))


def _gt_u8(path, h, w, seed, n=7, mode="L"):
    v = np.random.default_rng(seed).integers(0, n, (h, w)).astype(np.uint8)
    v[::5, ::3] = 255
    im = Image.fromarray(v, "L")
    if mode == "P":
        im.putpalette([c for i in range(256) for c in (i, 255 - i, (7 * i) % 256)])    # becomes a palette image over the same indices
    im.save(path)
    return v


def _gt_rg16(path, h, w, seed, n=7):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, n, (h, w))
    v[::5, ::3] = 1000
    a = np.stack([v & 255, v >> 8, rng.integers(1, 256, (h, w))], axis=-1).astype(np.uint8)
    Image.fromarray(a, "RGB").save(path)
    return a


def test_loader_stages_images_and_ground_truth_in_one_buffer(tmp_path):
    """No GPU: unpinned staging.  Every batch's staging splits into the descriptor rows, the decoded image bytes and the ground-truth
    bytes; both formats; grey and palette PNGs give the same bytes; no decode thread is left behind."""
    hw = [(64, 96), (80, 64), (64, 96), (128, 192), (64, 96)]
    imgs = [PC.write_rgb(tmp_path, f"i{k}.png", h, w, seed=k) for k, (h, w) in enumerate(hw)]
    for fmt in ("u8", "rg16"):
        gts, want = [], []
        for k, (h, w) in enumerate(hw):
            p = str(tmp_path / f"g_{fmt}_{k}.png")
            want.append(_gt_u8(p, h, w, 50 + k, mode="P" if k % 2 else "L") if fmt == "u8" else _gt_rg16(p, h, w, 50 + k))
            gts.append(p)
        seen = []
        for batch in P.EvalBatchLoader(imgs, gts, 96, 2, 4, gt_format=fmt, pin=False):
            B = len(batch.paths)
            packed, desc, gt = P.split_eval_staging(batch.staging, B, batch.packed_bytes, tuple(batch.gt.shape))
            assert gt.shape == ((B,) + batch.size_hw if fmt == "u8" else (B,) + batch.size_hw + (3,))
            assert packed.numel() == batch.packed_bytes and batch.staging.numel() == 32 * B + batch.packed_bytes + gt.numel()
            for b, i in enumerate(batch.indices):
                assert batch.paths[b] == imgs[i] and batch.gt_paths[b] == gts[i] and batch.size_hw == hw[i]
                assert batch.out_hw == tuple(reversed(P.longer_edge_size(hw[i][1], hw[i][0], 96)))
                assert np.array_equal(gt[b].numpy(), want[i])
                off, w, h = int(desc[b, 0]) * 16, int(desc[b, 1]), int(desc[b, 2])
                assert np.array_equal(packed[off:off + 3 * w * h].numpy().reshape(h, w, 3), np.asarray(Image.open(imgs[i]).convert("RGB")))
            seen.append(list(batch.indices))
        assert seen == P.bucket_batches([P.eval_bucket_key(w, h, w, h, 96) for h, w in hw], 2, 512) == [[0, 2], [1], [3], [4]]
    assert not [t for t in threading.enumerate() if t.name.startswith("zutis-decode")]


# ------------------------------------------------------------------------------------------------------------------ refusals
def _drain(loader):
    for _ in loader:
        pass


def test_ground_truth_of_another_mode_or_size_is_a_value_error_naming_the_file(tmp_path):
    img = PC.write_rgb(tmp_path, "img.png", 40, 56, seed=1)
    ok_u8, ok_rg = str(tmp_path / "ok_u8.png"), str(tmp_path / "ok_rg.png")
    _gt_u8(ok_u8, 40, 56, 2)
    _gt_rg16(ok_rg, 40, 56, 3)
    sixteen = str(tmp_path / "sixteen.png")
    Image.fromarray(np.random.default_rng(4).integers(0, 60000, (40, 56)).astype(np.uint16)).save(sixteen)      # mode I;16
    palette = str(tmp_path / "palette.png")
    _gt_u8(palette, 40, 56, 5, mode="P")
    rgba = str(tmp_path / "rgba.png")
    Image.fromarray(PC.pixels(40, 56, 6, 4), "RGBA").save(rgba)
    small = str(tmp_path / "small.png")
    _gt_u8(small, 40, 55, 7)
    assert Image.open(sixteen).mode.startswith("I") and Image.open(palette).mode == "P"
    cases = [("u8", sixteen), ("rg16", sixteen),            # 16 bits per pixel: neither format
             ("rg16", palette), ("rg16", ok_u8),            # one channel where R + 256 G needs two
             ("u8", ok_rg), ("u8", rgba), ("rg16", rgba),   # three / four channels where the byte is the label; RGBA is not RGB
             ("u8", small)]                                 # one column short of its image
    for fmt, gt in cases:
        with pytest.raises(ValueError, match=os.path.basename(gt).replace(".", r"\.")):
            _drain(P.EvalBatchLoader([img, img], [ok_u8 if fmt == "u8" else ok_rg, gt], None, 2, 2, gt_format=fmt, pin=False))
        assert not [t for t in threading.enumerate() if t.name.startswith("zutis-decode")]
    _drain(P.EvalBatchLoader([img, img], [ok_u8, palette], None, 2, 2, gt_format="u8", pin=False))                  # a palette PNG's indices are labels
    with pytest.raises(FileNotFoundError):
        _drain(P.EvalBatchLoader([img], [str(tmp_path / "none.png")], None, 2, 2, pin=False))
    with pytest.raises(ValueError):
        P.EvalBatchLoader([img], [ok_u8], None, 2, 2, gt_format="u16", pin=False)
    with pytest.raises(ValueError):
        P.EvalBatchLoader([img, img], [ok_u8], None, 2, 2, pin=False)


# ------------------------------------------------------------------------------------------------------------------ the adapter
class _ImageNetS:
    name, max_size = "imagenet-s919", 1024
    p_images, p_gts = ["a/1.JPEG", "a/2.JPEG"], ["b/1.png", "b/2.png"]


class _ImageNetSTest:
    name, max_size, p_images = "imagenet-s50", 1024, ["a/1.JPEG"]          # the test split: no p_gts (imagenet_s.py:46-47)


class _Coco:
    def __init__(self, name):
        self.name, self.dir_dataset, self.image_ids = name, "/data/coco", [9, 4]

    def get_image_path(self, image_id):
        return f"/data/coco/images/val2017/{image_id:012d}.jpg"


class _Coca:
    name, p_images, p_gts = "coca", ["x.jpg"], ["x.png"]


def test_eval_files_of_on_stand_ins():
    assert evaluate.eval_files_of(_ImageNetS()) == (["a/1.JPEG", "a/2.JPEG"], ["b/1.png", "b/2.png"], "rg16", 1024)
    for name in ("coco2017", "coco20k"):
        p_images, p_gts, fmt, max_size = evaluate.eval_files_of(_Coco(name))
        assert p_images == ["/data/coco/images/val2017/000000000009.jpg", "/data/coco/images/val2017/000000000004.jpg"]
        assert p_gts == ["/data/coco/annotations/semantic_segmentation_masks/000000000009.png",
                         "/data/coco/annotations/semantic_segmentation_masks/000000000004.png"]
        assert (fmt, max_size) == ("u8", None)
    with pytest.raises(TypeError, match="coca"):            # its __getitem__ rewrites 255 to the directory's label
        evaluate.eval_files_of(_Coca())
    with pytest.raises(TypeError, match="no ground truth"):
        evaluate.eval_files_of(_ImageNetSTest())
    for other in (object(), _Coco("voc2012"), torch.nn.Linear(2, 2)):
        with pytest.raises(TypeError):
            evaluate.eval_files_of(other)


def test_confusion_scores_are_get_scores():
    """The four scores and the per-class IoU of a small matrix, by hand; a class that never occurs gives NaN IoU and is skipped by the means."""
    cm = np.array([[3.0, 1.0, 0.0], [2.0, 4.0, 0.0], [0.0, 0.0, 0.0]])
    scores, cls_iu = evaluate.confusion_scores(cm)
    assert scores["Pixel Acc"] == 7 / 10 and scores["Mean Acc"] == np.mean([3 / 4, 4 / 6])
    assert cls_iu[0] == 3 / 6 and cls_iu[1] == 4 / 7 and np.isnan(cls_iu[2])
    assert scores["Mean IoU"] == np.mean([3 / 6, 4 / 7]) and scores["FreqW Acc"] == 0.4 * (3 / 6) + 0.6 * (4 / 7)


def test_evaluate_refuses_a_module_that_is_not_the_drop_in():
    with pytest.raises(TypeError, match="no torch / CPU fallback"):
        evaluate.evaluate_from_files(torch.nn.Linear(2, 2), ["a.png"], ["b.png"], 3)
    with pytest.raises(ValueError):
        evaluate.evaluate_from_files(torch.nn.Linear(2, 2), ["a.png"], [], 3)


# ------------------------------------------------------------------------------------------------------------------ the C header
def test_header_declares_the_fused_entry():
    e = _lib.entries()["zh_upsample_argmax_score"]
    assert e.plannable and [t for t, _ in e.params] == ["const float*", "const unsigned char*", "int", "long long*", "long long*",
                                                        "int", "int", "int", "int", "int", "int", "float", "float", "zh_stream_t"]
    assert [n for _, n in e.params][:5] == ["logits_lo", "gt", "gt_format", "hist_accum", "labels"]
    assert _lib.header_abi_version() >= 231
    text = open(_lib.HEADER).read()
    assert "#define ZH_GT_U8 0" in text and "#define ZH_GT_RG16 1" in text
    from zutis_amd import ops
    assert ops.GT_FORMATS == {"u8": 0, "rg16": 1}
