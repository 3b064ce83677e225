"""-m gpu: evaluation from image files (zutis_amd/evaluate.py) on the TINY drop-in ZUTIS against the loop as it is: a host transform with
Pillow + torch, net(x), predict("semantic", size=...) to NumPy, NumPy's _fast_hist, predict("instance").  Integer / byte equality.

The existing path is fed the SAME groups the loader forms (preprocess.bucket_batches of preprocess.eval_bucket_key): how many images
share a forward can move a value (tests/test_pseudo_files_gpu.py), so identity across different groupings is not asserted."""
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
N_CAT = 7
MAX_SIZE = 96
# (H, W) of the files, mixed order, three shapes plus ONE file larger than MAX_SIZE (128 x 192 -> 64 x 96: resized on the way in, scored
# at 128 x 192); every side a multiple of the 16-pixel patch, before and after the resize
FILE_HW = [(64, 96), (80, 64), (64, 96), (128, 192), (48, 80), (80, 64), (64, 96), (48, 80), (80, 64), (64, 96)]
JPEG_INDEX = 2
IGNORE = {"u8": 255, "rg16": 1000}


def _photo(h, w, seed):
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 256, (max(2, h // 16), max(2, w // 16), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(low).resize((w, h), Image.BICUBIC), np.float32) + rng.normal(0.0, 6.0, (h, w, 3)).astype(np.float32)
    return Image.fromarray(np.clip(a, 0, 255).astype(np.uint8))


def _labels(h, w, seed, ignore):
    """A blocky label map over [0, N_CAT) with stripes of the ignore label."""
    rng = np.random.default_rng(seed)
    v = np.kron(rng.integers(0, N_CAT, (-(-h // 8), -(-w // 8))), np.ones((8, 8), np.int64))[:h, :w]
    v[::7, 1::3] = ignore
    return v


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """(image paths, {"u8": ground-truth paths, "rg16": ...}, {"u8": the label maps as int64, ...}, FILE_HW)."""
    d = tmp_path_factory.mktemp("eval")
    images, gts, values = [], {"u8": [], "rg16": []}, {"u8": [], "rg16": []}
    for i, (h, w) in enumerate(FILE_HW):
        p = str(d / (f"im{i:02d}.jpg" if i == JPEG_INDEX else f"im{i:02d}.png"))
        _photo(h, w, 900 + i).save(p, **({"quality": 90} if i == JPEG_INDEX else {"compress_level": 1}))
        images.append(p)
        for fmt in ("u8", "rg16"):
            v = _labels(h, w, 300 + i, IGNORE[fmt])
            g = str(d / f"gt_{fmt}_{i:02d}.png")
            if fmt == "u8":
                Image.fromarray(v.astype(np.uint8), "L").save(g)
            else:
                blue = np.random.default_rng(i).integers(1, 256, (h, w))                 # a non-zero B channel: ignored
                Image.fromarray(np.stack([v & 255, v >> 8, blue], axis=-1).astype(np.uint8), "RGB").save(g)
            gts[fmt].append(g)
            values[fmt].append(v)
    return images, gts, values, FILE_HW


@pytest.fixture(scope="module")
def net(dev):
    from zutis_amd import detgen
    if PC.DROPIN not in sys.path:
        sys.path.insert(0, PC.DROPIN)
    from networks.zutis import ZUTIS
    cfg = detgen.TINY
    m = ZUTIS(categories=[f"c{i}" for i in range(N_CAT)], clip_arch="ViT-B/16", n_queries=cfg.n_queries, n_decoder_layers=cfg.dec_layers,
              n_heads=cfg.dec_heads, device=dev, text_embeddings=torch.from_numpy(detgen.text_embeddings(N_CAT, cfg.embed_dim)),
              vision_config=(cfg.width, cfg.layers, cfg.patch, cfg.grid, cfg.embed_dim))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in detgen.zutis_state_dict(cfg).items()}, strict=True)
    return m.to(dev).eval().requires_grad_(False)


def _host_transform(path, max_size):
    """The validation datasets' __getitem__ on the host (imagenet_s.py:68-82; coco2017.py:126,138 with max_size None): Pillow's BILINEAR
    cap of the longer edge, then to_tensor and normalize as torch computes them."""
    im = Image.open(path).convert("RGB")
    nw, nh = P.longer_edge_size(*im.size, max_size)
    if (nw, nh) != im.size:
        im = im.resize((nw, nh), Image.BILINEAR)
    x = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return (x - torch.tensor(MEAN)[:, None, None]) / torch.tensor(STD)[:, None, None]


def _fast_hist(label_true, label_pred, n):
    """utils/running_score.py:11-16."""
    mask = (label_true >= 0) & (label_true < n)
    return np.bincount(n * label_true[mask].astype(int) + label_pred[mask], minlength=n ** 2).reshape(n, n)


def _get_scores(hist):
    """utils/running_score.py:24-49."""
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = np.diag(hist).sum() / hist.sum()
        acc_cls = np.nanmean(np.diag(hist) / hist.sum(axis=1))
        iu = np.diag(hist) / (hist.sum(axis=1) + hist.sum(axis=0) - np.diag(hist))
        mean_iu = np.nanmean(iu)
        freq = hist.sum(axis=1) / hist.sum()
        fwavacc = (freq[freq > 0] * iu[freq > 0]).sum()
    return {"Pixel Acc": acc, "Mean Acc": acc_cls, "FreqW Acc": fwavacc, "Mean IoU": mean_iu}, dict(zip(range(hist.shape[0]), iu))


def _existing_path(net, dev, images, values, hw, groups, max_size, instance=False, image_ids=None):
    """trainer.evaluate's loop body (trainer.py:316-347) over host-made tensors, one forward per group:
    (confusion matrix, {index: label map}, {index: instance predictions})."""
    hist, labels, preds = np.zeros((N_CAT, N_CAT)), {}, {i: [] for i in range(len(images))}
    with torch.no_grad():
        for g in groups:
            H, W = hw[g[0]]
            out = net(torch.stack([_host_transform(images[i], max_size) for i in g]).to(dev))
            sem = net.predict(dict_outputs=out, mask_type="semantic", size=(H, W))
            for b, i in enumerate(g):
                hist += _fast_hist(values[i].flatten(), sem[b].flatten(), N_CAT)
                labels[i] = sem[b]
            if instance:
                for p in net.predict(dict_outputs=out, mask_type="instance", size=(H, W), image_ids=[image_ids[i] for i in g], nms_type="hard"):
                    preds[image_ids.index(p["image_id"])].append(p)
    return hist, labels, preds


def _same_scores(a, b):
    return all(np.array_equal(np.float64(a[k]), np.float64(b[k]), equal_nan=True) for k in set(a) | set(b))


def _no_decode_threads():
    return not [t for t in threading.enumerate() if t.name.startswith("zutis-decode")]


@pytest.mark.parametrize("fmt", ["u8", "rg16"])
@pytest.mark.parametrize("batch_size,n_workers", [(4, 16), (3, 2)])
def test_files_in_scores_out_equals_the_existing_loop(dev, net, corpus, fmt, batch_size, n_workers):
    from zutis_amd import _lib, evaluate
    images, gts, values, hw = corpus
    groups = P.bucket_batches([P.eval_bucket_key(w, h, w, h, MAX_SIZE) for h, w in hw], batch_size, 512)
    assert max(len(g) for g in groups) > 1 and len(groups) >= 4 and [3] in groups        # the large file has a shape of its own
    counts = {}
    _lib.COUNTER = counts
    try:
        got = evaluate.evaluate_from_files(net, images, gts[fmt], N_CAT, gt_format=fmt, max_size=MAX_SIZE, mean=MEAN, std=STD,
                                           batch_size=batch_size, n_workers=n_workers, return_labels=True)
    finally:
        _lib.COUNTER = None
    assert counts.get("zh_upsample_argmax_score") == len(groups) == counts.get("zh_resize_normalize_u8")      # one launch of each per batch
    assert "zh_upsample_argmax" not in counts and "zh_confusion_hist" not in counts
    hist, labels, _ = _existing_path(net, dev, images, values[fmt], hw, groups, MAX_SIZE)
    counted = sum(int((v < N_CAT).sum()) for v in values[fmt])
    print(f"{fmt}, batch_size {batch_size}: {len(groups)} batches {[len(g) for g in groups]}, {counted} pixels counted, "
          f"{int((got['confusion_matrix'] != hist).sum())} of {hist.size} bins differ")
    assert got["confusion_matrix"].dtype == np.float64 and np.array_equal(got["confusion_matrix"], hist) and hist.sum() == counted
    scores, cls_iu = _get_scores(hist)
    assert _same_scores(got["scores"], scores) and _same_scores(got["cls_iu"], cls_iu) and set(got["scores"]) == set(scores)
    assert sorted(got["labels"]) == list(range(len(images)))
    for i in range(len(images)):
        assert got["labels"][i].shape == hw[i] and got["labels"][i].dtype == np.int64 and np.array_equal(got["labels"][i], labels[i]), i
    assert got["instance_predictions"] == [] and _no_decode_threads()
    plain = evaluate.evaluate_from_files(net, images, gts[fmt], N_CAT, gt_format=fmt, max_size=MAX_SIZE, batch_size=batch_size, n_workers=n_workers)
    assert plain["labels"] is None and np.array_equal(plain["confusion_matrix"], hist)    # no label map asked for: the same counts


def test_native_size_and_instance_predictions(dev, net, corpus):
    """max_size None (coco2017.py / coco20k.py: the image goes in as it is) with the instance predict of trainer.py:337-345: the prediction
    dicts are those of the existing loop, in input-path order."""
    from zutis_amd import evaluate
    images, gts, values, hw = corpus
    ids = [1000 + 7 * i for i in range(len(images))]
    groups = P.bucket_batches([P.eval_bucket_key(w, h, w, h, None) for h, w in hw], 4, 512)
    got = evaluate.evaluate_from_files(net, images, gts["u8"], N_CAT, max_size=None, mean=MEAN, std=STD, batch_size=4, n_workers=8, instance=True,
                                       image_ids=ids, nms_type="hard")
    hist, _, preds = _existing_path(net, dev, images, values["u8"], hw, groups, None, instance=True, image_ids=ids)
    assert np.array_equal(got["confusion_matrix"], hist)
    want = [p for i in range(len(images)) for p in preds[i]]
    print(f"{len(want)} instance predictions over {len(images)} images; {len(got['instance_predictions'])} from files")
    assert len(want) > 0 and len(got["instance_predictions"]) == len(want)
    for a, b in zip(got["instance_predictions"], want):
        assert a["segmentation"]["counts"] == b["segmentation"]["counts"] and list(a["segmentation"]["size"]) == list(b["segmentation"]["size"])
        assert a["score"] == b["score"] and a["category_id"] == b["category_id"] and a["image_id"] == b["image_id"]
        assert list(a["bbox"]) == list(b["bbox"]) and tuple(a["image_size"]) == tuple(b["image_size"])
    assert [p["image_id"] for p in got["instance_predictions"]] == sorted(p["image_id"] for p in want)      # ids ascend with the path index
    assert _no_decode_threads()


def test_batch_size_one_equals_the_plain_one_image_loop(dev, net, corpus):
    from zutis_amd import evaluate
    images, gts, values, hw = corpus
    got = evaluate.evaluate_from_files(net, images, gts["rg16"], N_CAT, gt_format="rg16", max_size=MAX_SIZE, batch_size=1, n_workers=4, return_labels=True)
    hist, labels, _ = _existing_path(net, dev, images, values["rg16"], hw, [[i] for i in range(len(images))], MAX_SIZE)
    assert np.array_equal(got["confusion_matrix"], hist)
    assert all(np.array_equal(got["labels"][i], labels[i]) for i in range(len(images)))


def test_failures_reach_the_caller_and_leave_the_device_usable(dev, net, corpus, tmp_path):
    from zutis_amd import evaluate
    images, gts, values, hw = corpus
    with_missing = images[:3] + [str(tmp_path / "missing.png")] + images[3:6]
    with pytest.raises(FileNotFoundError):
        evaluate.evaluate_from_files(net, with_missing, gts["u8"][:7], N_CAT, max_size=MAX_SIZE, batch_size=2, n_workers=4)
    assert _no_decode_threads()
    with pytest.raises(ValueError, match="gt_u8_01"):                                    # an 80 x 64 mask for the third image, 64 x 96
        evaluate.evaluate_from_files(net, images[:3], [gts["u8"][0], gts["u8"][1], gts["u8"][1]], N_CAT, max_size=MAX_SIZE, batch_size=2, n_workers=4)
    with pytest.raises(ValueError, match="gt_rg16_00"):                                  # an RGB mask where the byte is the label
        evaluate.evaluate_from_files(net, images[:1], gts["rg16"][:1], N_CAT, gt_format="u8", batch_size=2, n_workers=4)
    with pytest.raises(ValueError):
        evaluate.evaluate_from_files(net, images[:2], gts["u8"][:2], N_CAT + 1)           # the network holds N_CAT text embeddings
    assert _no_decode_threads()
    torch.cuda.synchronize()
    got = evaluate.evaluate_from_files(net, images[:3], gts["u8"][:3], N_CAT, max_size=MAX_SIZE, batch_size=1, n_workers=4)
    hist, _, _ = _existing_path(net, dev, images[:3], values["u8"][:3], hw[:3], [[0], [1], [2]], MAX_SIZE)
    assert np.array_equal(got["confusion_matrix"], hist)
    empty = evaluate.evaluate_from_files(net, [], [], N_CAT)
    assert empty["confusion_matrix"].sum() == 0 and empty["instance_predictions"] == []


def test_running_score_update_device_equals_update_with_host_arrays(dev, net, corpus):
    """The drop-in meter: update_device (and ZUTIS.score_semantic, which calls it) leaves the histogram and the scores that update() leaves
    when it is handed the ground truth and predict()'s label map as NumPy arrays (trainer.py:347)."""
    from utils.running_score import RunningScore
    images, gts, values, hw = corpus
    a, b, c = RunningScore(N_CAT, dev), RunningScore(N_CAT, dev), RunningScore(N_CAT, dev)
    with torch.no_grad():
        for i in (0, 1, 3):
            H, W = hw[i]
            out = net(_host_transform(images[i], MAX_SIZE)[None].to(dev))
            a.update(values["u8"][i][None], net.predict(dict_outputs=out, mask_type="semantic", size=(H, W)))
            b.update_device(net, out, torch.from_numpy(np.asarray(Image.open(gts["u8"][i]))[None].copy()).to(dev), gt_format="u8", size=(H, W))
            net.score_semantic(out, torch.from_numpy(np.asarray(Image.open(gts["rg16"][i]))[None].copy()).to(dev), c, size=(H, W), gt_format="rg16")
    assert a.confusion_matrix.sum() > 0 and np.array_equal(a.confusion_matrix, b.confusion_matrix)
    # "rg16" drops 1000 where "u8" drops 255: the same pixels of the same label maps
    assert np.array_equal(a.confusion_matrix, c.confusion_matrix)
    sa, sb = a.get_scores(), b.get_scores()
    assert _same_scores(sa[0], sb[0]) and _same_scores(sa[1], sb[1])
    b.reset()
    assert b.confusion_matrix.sum() == 0
