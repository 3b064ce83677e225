"""-m gpu: predictions from image files (zutis_amd/predict_files.py) on the TINY drop-in ZUTIS against the loop as it is: a host transform
with Pillow + torch, net(x), predict("semantic", size=...) to NumPy, predict("instance").  Byte equality of every written PNG, and the
written files read back by evaluate_from_files as ground truth.

The existing path is fed the SAME groups the loader forms (preprocess.bucket_batches of preprocess.eval_bucket_key): how many images
share a forward can move a value (tests/test_pseudo_files_gpu.py), so identity across different groupings is not asserted."""
import json
import os
import sys
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from tests import _preprocess_case as PC
from zutis_amd import preprocess as P

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
N_CAT, N_MANY = 7, 300
MAX_SIZE = 96
# (H, W) of the files, mixed order, three shapes plus ONE file larger than MAX_SIZE (128 x 192 -> 64 x 96: resized on the way in, predicted
# at 128 x 192); every side a multiple of the 16-pixel patch, before and after the resize
FILE_HW = [(64, 96), (80, 64), (64, 96), (128, 192), (48, 80), (80, 64), (64, 96), (48, 80), (80, 64), (64, 96)]
JPEG_INDEX = 2
PALETTE = {i: ((37 * i + 11) % 256, (91 * i + 5) % 256, (53 * i + 200) % 256) for i in range(N_CAT)}
# variant -> (categories, label_format, palette, Pillow mode of the label PNG)
VARIANTS = {"u8": (N_CAT, "u8", None, "L"), "u8-palette": (N_CAT, "u8", PALETTE, "P"), "rg16": (N_MANY, "rg16", None, "RGB")}


def _photo(h, w, seed):
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 256, (max(2, h // 16), max(2, w // 16), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(low).resize((w, h), Image.BICUBIC), np.float32) + rng.normal(0.0, 6.0, (h, w, 3)).astype(np.float32)
    return Image.fromarray(np.clip(a, 0, 255).astype(np.uint8))


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    d = tmp_path_factory.mktemp("predict")
    paths = []
    for i, (h, w) in enumerate(FILE_HW):
        p = str(d / (f"im{i:02d}.jpg" if i == JPEG_INDEX else f"im{i:02d}.png"))
        _photo(h, w, 900 + i).save(p, **({"quality": 90} if i == JPEG_INDEX else {"compress_level": 1}))
        paths.append(p)
    return paths


def _build(dev, n):
    from zutis_amd import detgen
    if PC.DROPIN not in sys.path:
        sys.path.insert(0, PC.DROPIN)
    from networks.zutis import ZUTIS
    cfg = detgen.TINY
    m = ZUTIS(categories=[f"c{i}" for i in range(n)], clip_arch="ViT-B/16", n_queries=cfg.n_queries, n_decoder_layers=cfg.dec_layers,
              n_heads=cfg.dec_heads, device=dev, text_embeddings=torch.from_numpy(detgen.text_embeddings(n, cfg.embed_dim)),
              vision_config=(cfg.width, cfg.layers, cfg.patch, cfg.grid, cfg.embed_dim))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in detgen.zutis_state_dict(cfg).items()}, strict=True)
    return m.to(dev).eval().requires_grad_(False)


@pytest.fixture(scope="module")
def nets(dev):
    """{categories: the TINY drop-in ZUTIS with that many text embeddings (detgen.text_embeddings, seed 7)}."""
    return {N_CAT: _build(dev, N_CAT), N_MANY: _build(dev, N_MANY)}


def _host_transform(path, max_size):
    """The validation datasets' __getitem__ on the host (imagenet_s.py:68-82; coco2017.py:126,138 with max_size None): Pillow's BILINEAR
    cap of the longer edge, then to_tensor and normalize as torch computes them."""
    im = Image.open(path).convert("RGB")
    nw, nh = P.longer_edge_size(*im.size, max_size)
    if (nw, nh) != im.size:
        im = im.resize((nw, nh), Image.BILINEAR)
    x = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return (x - torch.tensor(MEAN)[:, None, None]) / torch.tensor(STD)[:, None, None]


def _groups(batch_size, max_size, window=512):
    return P.bucket_batches([P.eval_bucket_key(w, h, w, h, max_size) for h, w in FILE_HW], batch_size, window)


_EXISTING = {}


def _existing_labels(net, dev, images, n, batch_size, max_size):
    """{index: int64 label map} of net.predict(mask_type="semantic", size=(H, W)) over host-made tensors, one forward per group of the
    loader's grouping: computed once per (categories, batch_size, max_size), shared, never written."""
    key = (n, batch_size, max_size)
    if key not in _EXISTING:
        labels = {}
        with torch.no_grad():
            for g in _groups(batch_size, max_size):
                H, W = FILE_HW[g[0]]
                out = net(torch.stack([_host_transform(images[i], max_size) for i in g]).to(dev))
                sem = net.predict(dict_outputs=out, mask_type="semantic", size=(H, W))
                for b, i in enumerate(g):
                    labels[i] = sem[b].copy()
                    labels[i].setflags(write=False)
        _EXISTING[key] = labels
    return _EXISTING[key]


def _decode(path, fmt, mode):
    with Image.open(path) as im:
        assert im.mode == mode, (path, im.mode)
        raw = np.asarray(im)
        pal = im.getpalette() if mode == "P" else None
    if fmt == "u8":
        return raw.astype(np.int64), raw, pal
    return raw[..., 0].astype(np.int64) + 256 * raw[..., 1].astype(np.int64), raw, pal


def _no_threads():
    return not [t for t in threading.enumerate() if t.name.startswith(("zutis-decode", "zutis-write"))]


def _predict(nets, images, out_dir, variant, batch_size, n_workers, **kw):
    from zutis_amd import predict_files
    n, fmt, pal, mode = VARIANTS[variant]
    got = predict_files.predict_from_files(nets[n], images, out_dir=str(out_dir), label_format=fmt, palette=pal, max_size=MAX_SIZE, mean=MEAN, std=STD,
                                           batch_size=batch_size, n_workers=n_workers, **kw)
    assert _no_threads()
    return got


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("batch_size,n_workers", [(4, 16), (3, 2)])
def test_same_batches_same_bytes(dev, nets, images, tmp_path, variant, batch_size, n_workers):
    """Every written label PNG, decoded, is predict("semantic")'s map of the existing loop on the same groups.  300 categories: detgen's
    text embeddings (seed 7) give labels of 256 and more — oracle/zutis_ref.py on the CPU: 3285 of the corpus's 72192 pixels — so the
    model exercises the G byte."""
    n, fmt, pal, mode = VARIANTS[variant]
    groups = _groups(batch_size, MAX_SIZE)
    assert max(len(g) for g in groups) > 1 and len(groups) >= 4 and [3] in groups        # the large file has a shape of its own
    got = _predict(nets, images, tmp_path / "out", variant, batch_size, n_workers)
    want = _existing_labels(nets[n], dev, images, n, batch_size, MAX_SIZE)
    assert got["n_images"] == len(images) and got["overlay_paths"] is None and got["instance_predictions"] == []
    assert got["label_paths"] == [str(tmp_path / "out" / (os.path.splitext(os.path.basename(p))[0] + ".png")) for p in images]
    differ, high = 0, 0
    for i, p in enumerate(got["label_paths"]):
        lab, raw, file_pal = _decode(p, fmt, mode)
        assert lab.shape == FILE_HW[i]
        differ += int((lab != want[i]).sum())
        high += int((lab >= 256).sum())
        if fmt == "rg16":
            assert (raw[..., 2] == 0).all()
        if mode == "P":
            assert file_pal[:3 * n] == [c for k in range(n) for c in PALETTE[k]]          # the palette bytes as given
    print(f"{variant}, batch_size {batch_size}, {n_workers} workers: {len(groups)} batches {[len(g) for g in groups]}, {differ} labels differ, "
          f"{high} labels >= 256")
    assert differ == 0
    if variant == "rg16":
        assert high > 0
    assert sorted(os.listdir(tmp_path / "out")) == sorted(os.path.basename(p) for p in got["label_paths"])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_written_files_are_ground_truth_to_the_evaluator(dev, nets, images, tmp_path, variant):
    """The files predict_from_files writes, read back by evaluate_from_files as ground truth on the same groups: every pixel on the
    diagonal.  This pins the file formats to what the rest of the project reads."""
    from zutis_amd import evaluate
    n, fmt, pal, mode = VARIANTS[variant]
    got = _predict(nets, images, tmp_path / "out", variant, 4, 8, window=6)
    ev = evaluate.evaluate_from_files(nets[n], images, got["label_paths"], n, gt_format=fmt, max_size=MAX_SIZE, mean=MEAN, std=STD, batch_size=4,
                                      window=6)
    cm = ev["confusion_matrix"]
    total = sum(h * w for h, w in FILE_HW)
    print(f"{variant}: trace {np.trace(cm):.0f} of {cm.sum():.0f} counted, {total} pixels, {int((np.diag(cm) > 0).sum())} classes predicted")
    assert np.array_equal(cm, np.diag(np.diag(cm))) and np.trace(cm) == total and ev["scores"]["Pixel Acc"] == 1.0


def test_instance_predictions_and_their_json(dev, nets, images, tmp_path, monkeypatch):
    """max_size None (coco20k_eval.py: the image goes in as it is) with instance=True: the dicts are those of predict("instance") on the
    same groups, in input-path order; semantic=False writes no PNG and launches no arg-max."""
    from zutis_amd import ops, predict_files
    net = nets[N_CAT]
    ids = [1000 + 7 * i for i in range(len(images))]
    preds = {i: [] for i in range(len(images))}
    with torch.no_grad():
        for g in _groups(4, None):
            out = net(torch.stack([_host_transform(images[i], None) for i in g]).to(dev))
            for p in net.predict(dict_outputs=out, mask_type="instance", size=FILE_HW[g[0]], image_ids=[ids[i] for i in g], nms_type="hard"):
                preds[ids.index(p["image_id"])].append(p)
    want = [p for i in range(len(images)) for p in preds[i]]
    calls = {"bytes": 0, "int64": 0}
    real_bytes, real_int64 = ops.upsample_argmax_bytes, ops.upsample_argmax
    monkeypatch.setattr(ops, "upsample_argmax_bytes", lambda *a, **k: (calls.__setitem__("bytes", calls["bytes"] + 1), real_bytes(*a, **k))[1])
    monkeypatch.setattr(ops, "upsample_argmax", lambda *a, **k: (calls.__setitem__("int64", calls["int64"] + 1), real_int64(*a, **k))[1])
    pj = tmp_path / "json" / "instance_predictions.json"
    got = predict_files.predict_from_files(net, images, out_dir=str(tmp_path / "none"), semantic=False, instance=True, image_ids=ids, max_size=None,
                                           mean=MEAN, std=STD, batch_size=4, n_workers=8, nms_type="hard", predictions_json=str(pj))
    assert calls == {"bytes": 0, "int64": 0} and not os.path.exists(tmp_path / "none") and got["label_paths"] is None and got["overlay_paths"] is None
    print(f"{len(want)} instance predictions over {len(images)} images; {len(got['instance_predictions'])} from files")
    assert len(want) > 0 and len(got["instance_predictions"]) == len(want) and got["n_images"] == len(images)
    for a, b in zip(got["instance_predictions"], want):
        assert a["segmentation"]["counts"] == b["segmentation"]["counts"] and list(a["segmentation"]["size"]) == list(b["segmentation"]["size"])
        assert a["score"] == b["score"] and a["category_id"] == b["category_id"] and a["image_id"] == b["image_id"]
        assert list(a["bbox"]) == list(b["bbox"]) and tuple(a["image_size"]) == tuple(b["image_size"])
    assert [p["image_id"] for p in got["instance_predictions"]] == sorted(p["image_id"] for p in want)      # ids ascend with the path index
    back = json.load(open(pj))
    assert len(back) == len(want)
    for a, b in zip(back, want):
        counts = b["segmentation"]["counts"]
        assert "bbox" not in a and isinstance(a["segmentation"]["counts"], str)
        assert a["segmentation"]["counts"] == (counts.decode("ascii") if isinstance(counts, bytes) else counts)
        assert a["segmentation"]["size"] == list(b["segmentation"]["size"]) and a["score"] == b["score"] and a["category_id"] == b["category_id"]
        assert a["image_id"] == b["image_id"] and a["image_size"] == list(b["image_size"])
    # with the label maps as well: one byte launch per batch, the same dicts
    both = predict_files.predict_from_files(net, images, out_dir=str(tmp_path / "both"), instance=True, image_ids=ids, max_size=None, mean=MEAN, std=STD,
                                            batch_size=4, n_workers=8, nms_type="hard")
    assert calls == {"bytes": len(_groups(4, None)), "int64": 0} and len(os.listdir(tmp_path / "both")) == len(images)
    assert [(p["image_id"], p["segmentation"]["counts"]) for p in both["instance_predictions"]] == [(p["image_id"], p["segmentation"]["counts"]) for p in want]
    assert _no_threads()


def test_overlay_is_the_integer_blend_of_the_decoded_file(dev, nets, images, tmp_path):
    alpha = 96
    got = _predict(nets, images, tmp_path / "out", "u8-palette", 4, 6, overlay=True, alpha=alpha)
    pal = np.array([PALETTE[k] for k in range(N_CAT)], np.uint8)
    assert got["overlay_paths"] == [p[:-4] + "_overlay.png" for p in got["label_paths"]]
    want = _existing_labels(nets[N_CAT], dev, images, N_CAT, 4, MAX_SIZE)
    for i, (p, o) in enumerate(zip(got["label_paths"], got["overlay_paths"])):
        lab, _, _ = _decode(p, "u8", "P")
        assert np.array_equal(lab, want[i])                                              # the labels are not moved by the overlay
        img = np.asarray(Image.open(images[i]).convert("RGB")).astype(np.int64)           # the decoded file at ITS size (the 128 x 192 one too)
        blend = ((img * (256 - alpha) + pal[lab].astype(np.int64) * alpha + 128) >> 8).astype(np.uint8)
        with Image.open(o) as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), blend), o
    assert len(os.listdir(tmp_path / "out")) == 2 * len(images)


def test_failures_reach_the_caller_and_leave_the_device_usable(dev, nets, images, tmp_path):
    from zutis_amd import predict_files
    net = nets[N_CAT]
    with_missing = images[:3] + [str(tmp_path / "missing.png")] + images[3:6]
    with pytest.raises(FileNotFoundError):
        predict_files.predict_from_files(net, with_missing, out_dir=str(tmp_path / "a"), max_size=MAX_SIZE, batch_size=2, n_workers=4)
    assert _no_threads()
    (tmp_path / "plain_file").write_bytes(b"not a directory")
    with pytest.raises(OSError):                                                         # NotADirectoryError / FileExistsError
        predict_files.predict_from_files(net, images[:3], out_dir=str(tmp_path / "plain_file" / "sub"), max_size=MAX_SIZE, batch_size=2, n_workers=4)
    assert _no_threads()
    # a writer's failure (its target is a directory): raised by the call, after which nothing of it is left running
    os.makedirs(tmp_path / "b" / "im01.png")
    with pytest.raises(OSError):
        predict_files.predict_from_files(net, images[:5], out_dir=str(tmp_path / "b"), max_size=MAX_SIZE, batch_size=1, n_workers=4)
    assert _no_threads()
    torch.cuda.synchronize()
    got = predict_files.predict_from_files(net, images[:3], out_dir=str(tmp_path / "c"), max_size=MAX_SIZE, mean=MEAN, std=STD, batch_size=1, n_workers=4)
    want = _existing_labels(net, dev, images, N_CAT, 1, MAX_SIZE)
    for i, p in enumerate(got["label_paths"]):
        assert np.array_equal(_decode(p, "u8", "L")[0], want[i])
    assert _no_threads()
