"""Host side of predictions from files (zutis_amd/predict_files.py, preprocess.PredictBatchLoader): output-path rules, validation, the
palette, the two byte formats and the blend stated in NumPy, the loader's grouping, the JSON form, the dataset adapter and the C
declaration.  No GPU."""
import json
import os
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from zutis_amd import _lib, ops, predict_files as PF
from zutis_amd import preprocess as P


# ------------------------------------------------------------------------------------------------------------------ output paths
def test_out_dir_maps_the_stem_and_out_paths_are_taken_as_given(tmp_path):
    images = ["/data/a/im0.jpg", "/data/b/im1.png", "/data/b/deep.name.jpeg"]
    labels, overlays = PF.resolve_output_paths(images, str(tmp_path), None, overlay=True)
    assert labels == [str(tmp_path / "im0.png"), str(tmp_path / "im1.png"), str(tmp_path / "deep.name.png")]
    assert overlays == [str(tmp_path / "im0_overlay.png"), str(tmp_path / "im1_overlay.png"), str(tmp_path / "deep.name_overlay.png")]
    given = [str(tmp_path / "x" / "0.png"), str(tmp_path / "y" / "1.png"), str(tmp_path / "2.png")]
    labels, overlays = PF.resolve_output_paths(images, None, given)
    assert labels == given and overlays is None


def test_exactly_one_of_out_dir_and_out_paths():
    for kw in (dict(out_dir=None, out_paths=None), dict(out_dir="o", out_paths=["o/a.png"])):
        with pytest.raises(ValueError, match="exactly one"):
            PF.resolve_output_paths(["a.jpg"], kw["out_dir"], kw["out_paths"])
    with pytest.raises(ValueError, match="one output path per image"):
        PF.resolve_output_paths(["a.jpg", "b.jpg"], None, ["o/a.png"])


def test_two_images_on_one_output_path_is_refused():
    with pytest.raises(ValueError, match="d1/im.jpg and d2/im.png map to one output path"):
        PF.resolve_output_paths(["d1/im.jpg", "d2/im.png"], "out", None)
    with pytest.raises(ValueError, match="one output path"):
        PF.resolve_output_paths(["a.jpg", "b.jpg"], None, ["o/x.png", "o/../o/x.png"])
    with pytest.raises(ValueError, match="one output path"):                      # image b's label map on image a's overlay
        PF.resolve_output_paths(["a.jpg", "a_overlay.jpg"], "out", None, overlay=True)
    PF.resolve_output_paths(["a.jpg", "a_overlay.jpg"], "out", None, overlay=False)


# ------------------------------------------------------------------------------------------------------------------ validation
class _Net:
    """What predict_from_files looks at before it touches a device."""

    def __init__(self, n):
        self.text_embeddings = torch.zeros((n, 4))

    def _get_engine(self):
        raise AssertionError("validation must come before any device work")

    def predict(self, **kw):
        raise AssertionError("validation must come before any device work")


def test_every_validation_error_comes_before_device_work(tmp_path):
    out = str(tmp_path / "out")
    with pytest.raises(ValueError, match="rg16"):
        PF.predict_from_files(_Net(257), ["a.jpg"], out_dir=out)
    with pytest.raises(ValueError, match="65536"):
        PF.predict_from_files(_Net(65537), ["a.jpg"], out_dir=out, label_format="rg16")
    with pytest.raises(ValueError, match="semantic=False and instance=False"):
        PF.predict_from_files(_Net(7), ["a.jpg"], out_dir=out, semantic=False, instance=False)
    with pytest.raises(ValueError, match="one image id per image"):
        PF.predict_from_files(_Net(7), ["a.jpg", "b.jpg"], out_dir=out, instance=True, image_ids=[1])
    with pytest.raises(ValueError, match="one output path per image"):
        PF.predict_from_files(_Net(7), ["a.jpg", "b.jpg"], out_paths=[out + "/a.png"])
    with pytest.raises(ValueError, match="exactly one"):
        PF.predict_from_files(_Net(7), ["a.jpg"])
    with pytest.raises(ValueError, match="needs a palette"):
        PF.predict_from_files(_Net(7), ["a.jpg"], out_dir=out, overlay=True)
    with pytest.raises(ValueError, match="alpha"):
        PF.predict_from_files(_Net(2), ["a.jpg"], out_dir=out, overlay=True, palette=[(0, 0, 0), (1, 1, 1)], alpha=257)
    with pytest.raises(ValueError, match="label_format"):
        PF.predict_from_files(_Net(7), ["a.jpg"], out_dir=out, label_format="u16")
    with pytest.raises(ValueError, match="no colour for label 6"):
        PF.predict_from_files(_Net(7), ["a.jpg"], out_dir=out, palette={i: (i, i, i) for i in range(6)})
    with pytest.raises(ValueError, match="map to one output path"):
        PF.predict_from_files(_Net(7), ["x/a.jpg", "y/a.jpg"], out_dir=out)
    with pytest.raises(TypeError, match="drop-in ZUTIS"):
        PF.predict_from_files(torch.nn.Identity(), ["a.jpg"], out_dir=out)
    assert not os.path.exists(out)                                                # nothing was created on the way to a refusal
    # 257 categories are fine when no label file is asked for
    with pytest.raises(AssertionError, match="device work"):
        PF.predict_from_files(_Net(257), ["a.jpg"], semantic=False, instance=True)


def test_an_empty_list_is_an_empty_result(tmp_path):
    got = PF.predict_from_files(_Net(7), [], out_dir=str(tmp_path / "o"), instance=True, predictions_json=str(tmp_path / "p" / "pred.json"))
    assert got == {"label_paths": [], "overlay_paths": None, "instance_predictions": [], "n_images": 0}
    assert json.load(open(tmp_path / "p" / "pred.json")) == []


# ------------------------------------------------------------------------------------------------------------------ palette
def test_palette_from_a_dict_and_from_an_array():
    d = {0: (0, 0, 0), 1: (128, 0, 0), 2: (0, 128, 255), 255: (9, 9, 9)}          # get_palette's dicts carry extra keys (the ignore label)
    a = PF.normalise_palette(d, 3)
    assert a.dtype == np.uint8 and a.shape == (3, 3) and a.flags.c_contiguous and a.tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 255]]
    assert np.array_equal(PF.normalise_palette(np.array(a, np.int64), 3), a)
    assert np.array_equal(PF.normalise_palette(np.arange(30).reshape(10, 3), 3), np.arange(9).reshape(3, 3))      # longer than n: cut
    assert np.array_equal(PF.normalise_palette([[0.0, 1.0, 2.0]], 1), [[0, 1, 2]])


@pytest.mark.parametrize("bad,n", [({0: (0, 0, 0), 2: (1, 1, 1)}, 3), (np.zeros((2, 3), np.uint8), 3), (np.zeros((3, 4), np.uint8), 3),
                                   ([[0, 0, 256]], 1), ([[0, -1, 0]], 1), ([[0.5, 0.1, 0.2]], 1), ({0: (1, 2)}, 1)])
def test_palette_must_cover_every_label_with_byte_colours(bad, n):
    with pytest.raises(ValueError):
        PF.normalise_palette(bad, n)


# ------------------------------------------------------------------------------------------------------------------ bytes and blend
def test_the_two_byte_formats_in_numpy():
    v = np.array([[0, 1, 255], [3, 200, 17]])
    assert PF.encode_labels(v, "u8").dtype == np.uint8 and np.array_equal(PF.encode_labels(v, "u8"), v)
    v = np.array([[0, 255, 256], [919, 65535, 300]])
    raw = PF.encode_labels(v, "rg16")
    assert raw.dtype == np.uint8 and raw.shape == (2, 3, 3)
    assert raw.tolist() == [[[0, 0, 0], [255, 0, 0], [0, 1, 0]], [[151, 3, 0], [255, 255, 0], [44, 1, 0]]]
    # imagenet_s.py:93 reads it back: R + 256 G; and so does the evaluation's loader (decode_labels restates it)
    assert np.array_equal(raw[..., 1].astype(np.int64) * 256 + raw[..., 0], v) and np.array_equal(PF.decode_labels(raw, "rg16"), v)
    assert np.array_equal(PF.decode_labels(PF.encode_labels(v % 256, "u8"), "u8"), v % 256)
    for fmt, too_big in (("u8", 256), ("rg16", 65536)):
        with pytest.raises(ValueError):
            PF.encode_labels(np.array([too_big]), fmt)


@pytest.mark.parametrize("alpha", [0, 1, 128, 255, 256])
def test_the_blend_in_numpy(alpha):
    img, col = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")          # every (image byte, palette byte) pair
    got = PF.blend(img.astype(np.uint8), col.astype(np.uint8), alpha)
    want = np.array([[(i * (256 - alpha) + c * alpha + 128) >> 8 for c in range(256)] for i in range(256)])
    assert got.dtype == np.uint8 and np.array_equal(got, want) and want.max() <= 255
    if alpha == 0:
        assert np.array_equal(got, img)                                           # the image
    if alpha == 256:
        assert np.array_equal(got, col)                                           # the pure palette colour
    if alpha == 128:
        assert np.array_equal(got, (img + col + 1) >> 1)                          # the mean, halves rounded up


def test_blend_refuses_an_alpha_outside_0_256():
    for alpha in (-1, 257, 0.5):
        with pytest.raises(ValueError):
            PF.blend(np.zeros(3, np.uint8), np.zeros(3, np.uint8), alpha)


# ------------------------------------------------------------------------------------------------------------------ the loader
FILE_HW = [(64, 96), (80, 64), (64, 96), (128, 192), (48, 80), (80, 64), (64, 96), (48, 80), (80, 64), (64, 96), (96, 64)]
MAX_SIZE = 96


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("predict_cpu")
    paths = []
    for i, (h, w) in enumerate(FILE_HW):
        p = str(d / (f"im{i:02d}.jpg" if i == 2 else f"im{i:02d}.png"))
        a = np.random.default_rng(40 + i).integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(a).save(p)
        paths.append(p)
    return paths


@pytest.mark.parametrize("batch_size,window", [(4, 512), (3, 512), (2, 3), (1, 1)])
def test_groups_are_bucket_batches_of_the_evaluation_key(files, batch_size, window):
    want = P.bucket_batches([P.eval_bucket_key(w, h, w, h, MAX_SIZE) for h, w in FILE_HW], batch_size, window)
    loader = P.PredictBatchLoader(files, MAX_SIZE, batch_size, 4, window=window, pin=False)
    got = []
    for batch in loader:
        got.append(list(batch.indices))
        assert batch.paths == [files[i] for i in batch.indices]
        H, W = batch.size_hw
        assert all(FILE_HW[i] == (H, W) for i in batch.indices)                   # ONE file size per batch
        nw, nh = P.longer_edge_size(W, H, MAX_SIZE)
        assert batch.out_hw == (nh, nw) and batch.n_host == 0 and batch.host_paths == []
        packed, desc = P.split_staging(batch.staging, len(batch.indices))
        rows = desc.numpy()
        assert [tuple(r[1:5]) for r in rows] == [(W, H, nw, nh)] * len(batch.indices)
        for b, i in enumerate(batch.indices):                                     # the decoded image at FILE size, where the overlay reads it
            o = int(rows[b, 0]) * P.ALIGN
            assert np.array_equal(packed.numpy()[o:o + 3 * H * W].reshape(H, W, 3), np.asarray(Image.open(files[i]).convert("RGB")))
    assert got == want
    assert not [t for t in threading.enumerate() if t.name.startswith("zutis-decode")]


def test_groups_are_those_of_the_evaluation_loader(files, tmp_path):
    gts = []
    for i, (h, w) in enumerate(FILE_HW):
        g = str(tmp_path / f"gt{i:02d}.png")
        Image.fromarray(np.zeros((h, w), np.uint8)).save(g)
        gts.append(g)
    a = [list(b.indices) for b in P.PredictBatchLoader(files, MAX_SIZE, 3, 2, window=5, pin=False)]
    b = [list(b.indices) for b in P.EvalBatchLoader(files, gts, MAX_SIZE, 3, 2, window=5, pin=False)]
    assert a == b and sorted(i for g in a for i in g) == list(range(len(files)))


def test_a_file_over_max_size_resizes_on_the_way_in_and_is_predicted_at_file_size(files):
    batches = {tuple(b.indices): (b.size_hw, b.out_hw) for b in P.PredictBatchLoader(files, MAX_SIZE, 4, 2, pin=False)}
    assert batches[(3,)] == ((128, 192), (64, 96))                                # a shape key of its own: 64 x 96 FILES are another batch
    assert batches[(0, 2, 6, 9)] == ((64, 96), (64, 96))
    assert batches[(10,)] == ((96, 64), (96, 64))                                 # exactly at the cap: untouched


def test_a_missing_file_is_raised_by_the_loader_and_its_threads_end(files, tmp_path):
    with pytest.raises(FileNotFoundError):
        for _ in P.PredictBatchLoader(files[:3] + [str(tmp_path / "missing.png")] + files[3:], MAX_SIZE, 2, 4, pin=False):
            pass
    assert not [t for t in threading.enumerate() if t.name.startswith("zutis-decode")]


def test_decoders_and_writers_share_the_thread_budget():
    assert PF.thread_split(16, True) == (8, 8) and PF.thread_split(64, True) == (8, 8)
    assert PF.thread_split(2, True) == (1, 1) and PF.thread_split(3, True) == (2, 1) and PF.thread_split(5, True) == (3, 2)
    assert PF.thread_split(1, True) == (1, 1)                                     # one of each at the least
    assert PF.thread_split(16, False) == (16, 0) and PF.thread_split(40, False) == (16, 0) and PF.thread_split(1, False) == (1, 0)
    for n in range(2, 40):
        d, w = PF.thread_split(n, True)
        assert d >= 1 and w >= 1 and d + w == min(n, 16)


# ------------------------------------------------------------------------------------------------------------------ JSON form
def test_json_form_drops_bbox_and_writes_counts_as_str(tmp_path):
    preds = [{"category_id": np.int64(3), "segmentation": {"size": [4, 6], "counts": b"0a1b<2"}, "score": 0.5, "image_id": 17,
              "image_size": (4, 6), "bbox": [0.0, 1.0, 2.0, 3.0]},
             {"category_id": 1, "segmentation": {"size": (4, 6), "counts": "already"}, "score": 0.25, "image_id": 18, "image_size": (4, 6),
              "bbox": [1, 1, 1, 1], "pred_class": "cat"}]
    form = PF.predictions_json_form(preds)
    assert all("bbox" not in q for q in form) and all("bbox" in p for p in preds)                  # the caller's dicts stay whole
    assert form[0]["segmentation"]["counts"] == "0a1b<2" and isinstance(form[0]["segmentation"]["counts"], str)
    assert preds[0]["segmentation"]["counts"] == b"0a1b<2" and form[1]["segmentation"]["counts"] == "already" and form[1]["pred_class"] == "cat"
    back = json.loads(json.dumps(form, default=PF._jsonable))
    assert back[0] == {"category_id": 3, "segmentation": {"size": [4, 6], "counts": "0a1b<2"}, "score": 0.5, "image_id": 17, "image_size": [4, 6]}


# ------------------------------------------------------------------------------------------------------------------ dataset adapter
class _Stub:
    def __init__(self, name, **kw):
        self.name = name
        self.__dict__.update(kw)

    def get_image_path(self, image_id):
        return f"{self.dir_dataset}/val2017/{image_id:012d}.jpg"


def test_predict_files_of_is_the_image_half_of_eval_files_of():
    from zutis_amd import evaluate
    s = _Stub("imagenet-s300", p_images=["a/x.JPEG", "b/y.JPEG"], p_gts=["a/x.png", "b/y.png"], max_size=1024)
    assert PF.predict_files_of(s) == (["a/x.JPEG", "b/y.JPEG"], 1024, None)
    assert PF.predict_files_of(s)[0] == evaluate.eval_files_of(s)[0] and PF.predict_files_of(s)[1] == evaluate.eval_files_of(s)[3]
    test_split = _Stub("imagenet-s919", p_images=["t/0.JPEG"], max_size=1024)                      # no p_gts: the test split
    assert PF.predict_files_of(test_split) == (["t/0.JPEG"], 1024, None)
    with pytest.raises(TypeError):
        evaluate.eval_files_of(test_split)
    for name in ("coco2017", "coco20k"):
        c = _Stub(name, dir_dataset="/d/coco", image_ids=[139, 285])
        assert PF.predict_files_of(c) == (["/d/coco/val2017/000000000139.jpg", "/d/coco/val2017/000000000285.jpg"], None, [139, 285])
        assert PF.predict_files_of(c)[0] == evaluate.eval_files_of(c)[0]
    for other in (_Stub("coca"), _Stub("voc2012"), object()):
        with pytest.raises(TypeError):
            PF.predict_files_of(other)


# ------------------------------------------------------------------------------------------------------------------ the C declaration
def test_header_declares_the_entry_and_the_binding_exists():
    e = _lib.entries()["zh_upsample_argmax_bytes"]
    names = [n for _, n in e.params]
    assert names == ["logits_lo", "labels_out", "label_format", "overlay_out", "packed", "desc", "palette", "alpha", "B", "n", "h", "w", "H", "W",
                     "scale_h", "scale_w", "stream"]
    assert e.plannable and e.ret == "int"
    assert callable(ops.upsample_argmax_bytes) and ops.GT_FORMATS == {"u8": 0, "rg16": 1}
    from zutis_amd.engine import ZutisEngine
    assert callable(ZutisEngine.label_bytes)
    assert _lib.header_abi_version() >= 233
