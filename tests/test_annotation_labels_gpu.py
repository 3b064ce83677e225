"""-m gpu: semantic ground truth painted on the device (zutis_amd/annotation_labels.py, csrc/label_paint.hip: zh_runs_label_maps) against
labels_np, the host definition, byte for byte; the PNG directory of both routes; and evaluate_from_annotations against
evaluate_from_files fed those PNGs.  Shapes: tests/_label_paint_case.py."""
import os

import numpy as np
import pytest
import torch

from tests import _cocoeval_case as CC
from tests import _label_paint_case as LC
from tests import test_evaluate_gpu as TE
from zutis_amd import annotation_labels as AL

pytestmark = pytest.mark.gpu
net = TE.net                                                           # the TINY drop-in ZUTIS of tests/test_evaluate_gpu.py


@pytest.fixture(scope="module")
def edge():
    """(the edge dict, {(overlap, crowd): labels_np}) — the reference, computed once."""
    gt = LC.edge_dict()
    return gt, {(o, c): AL.labels_np(AL.paint_plan(gt, overlap=o, crowd=c)) for o in AL.OVERLAPS for c in AL.CROWDS}


@pytest.fixture(scope="module")
def same_size():
    gt = LC.same_size_dict()
    return gt, AL.labels_np(AL.paint_plan(gt, crowd="ignore"))


def _ragged(painter, idx):
    buf, off = painter.paint_ragged(idx)
    flat = buf.cpu().numpy()
    return [flat[off[k]:off[k + 1]].reshape(painter.plan.images[i]["h"], painter.plan.images[i]["w"]) for k, i in enumerate(idx)]


@pytest.mark.parametrize("overlap", AL.OVERLAPS)
@pytest.mark.parametrize("crowd", AL.CROWDS)
def test_edge_set_alone_and_in_one_ragged_launch(dev, edge, overlap, crowd):
    from zutis_amd import _lib
    gt, want = edge
    plan = AL.paint_plan(gt, overlap=overlap, crowd=crowd)
    painter = AL.LabelPainter(plan, dev)
    n = len(plan)
    assert painter.stats["host_fallback"] == 1 and painter.stats["images"] == n == 8        # the zigzag, and nothing else
    assert painter.stats["rle_annotations"] > 0 and painter.stats["polygon_annotations"] > 300
    for i in range(n):                                                                    # each image alone: B = 1
        got = painter.paint([i])
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + want[(overlap, crowd)][i].shape
        assert np.array_equal(got[0].cpu().numpy(), want[(overlap, crowd)][i]), (i, plan.images[i])
    order = np.random.default_rng(2).permutation(n).tolist()
    counts = {}
    _lib.COUNTER = counts
    try:
        got = _ragged(painter, order)                                                     # all of them, shuffled, in ONE launch
    finally:
        _lib.COUNTER = None
    assert counts == {"zh_runs_label_maps": 1}
    for i, g in zip(order, got):
        assert np.array_equal(g, want[(overlap, crowd)][i]), (i, plan.images[i])
    twice = _ragged(painter, [3, 3, 0, 3])                                                # an image may be asked for more than once
    assert all(np.array_equal(g, want[(overlap, crowd)][i]) for g, i in zip(twice, [3, 3, 0, 3]))


def test_empty_batches_and_mixed_sizes(dev, edge):
    gt, want = edge
    painter = AL.LabelPainter(AL.paint_plan(gt, image_ids=[im["id"] for im in gt["images"][:5]]), dev)
    assert tuple(painter.paint([]).shape) == (0, 0, 0)
    buf, off = painter.paint_ragged([])
    assert buf.numel() == 0 and off.tolist() == [0]
    with pytest.raises(ValueError):
        painter.paint([0, 1])                                                             # 1 x 1 and 1 x 7
    with pytest.raises(IndexError):
        painter.paint([5])
    out = torch.full((1, 20, 24), 9, dtype=torch.uint8, device=dev)                       # the image without annotations, into the caller's buffer
    assert painter.paint([4], out=out).data_ptr() == out.data_ptr() and not out.any()
    none = AL.LabelPainter(AL.paint_plan(gt, image_ids=[gt["images"][4]["id"]]), dev)      # a plan that paints no annotation at all
    assert none.stats["annotations"] == 0 and not none.paint([0]).any()


def test_same_size_batches(dev, same_size):
    gt, want = same_size
    painter = AL.LabelPainter(AL.paint_plan(gt, crowd="ignore"), dev)
    assert painter.stats["host_fallback"] == 0
    four = painter.paint([5, 6, 7, 8])
    assert tuple(four.shape) == (4, 40, 56) and four.is_contiguous()
    assert np.array_equal(four.cpu().numpy(), np.stack(want[5:9]))
    every = painter.paint(range(40)).cpu().numpy()                                        # 40 images, 0 - 12 annotations each
    assert np.array_equal(every, np.stack(want))
    assert len({len(e) for e in painter.plan.lists}) > 6 and (every == 255).any() and (every == 0).any()
    one = painter.paint([39])
    assert np.array_equal(one.cpu().numpy()[0], want[39])


def test_damaged_counts_are_reported_not_painted(dev, edge):
    gt, want = edge
    ids = [gt["images"][3]["id"]]                                                         # the 9 x 11 image
    plan = AL.paint_plan(gt, image_ids=ids)
    painter = AL.LabelPainter(plan, dev)
    j = plan.lists[0][1][0]                                                               # its second annotation
    m = painter.mask_of[j]
    o = int(painter.run_off[m].item())
    painter.counts[o] += 1                                                                # after the upload: the counts no longer sum to 99
    with pytest.raises(ValueError, match=f"annotation {gt['annotations'][j]['id']}"):
        painter.prefix()
    painter.prefix(check=False)
    got = painter.paint([0]).cpu().numpy()[0]
    rest = AL.paint_plan(gt, image_ids=ids)
    rest.lists[0] = [e for e in rest.lists[0] if e[0] != j]
    assert np.array_equal(got, AL.labels_np(rest)[0]) and not np.array_equal(got, want[("last", "label")][3])
    painter.counts[o] -= 1
    painter.prefix()
    assert np.array_equal(painter.paint([0]).cpu().numpy()[0], want[("last", "label")][3])


def test_chunks_of_seven_annotations_give_the_same_bytes(dev, edge, monkeypatch):
    from zutis_amd import polygons
    gt, want = edge
    monkeypatch.setattr(polygons, "CHUNK_ANNOTATIONS", 7)
    painter = AL.LabelPainter(AL.paint_plan(gt), dev)
    assert painter.stats["host_fallback"] == 1
    idx = list(range(len(painter.plan)))
    for i, g in zip(idx, _ragged(painter, idx)):
        assert np.array_equal(g, want[("last", "label")][i]), i


def test_device_route_writes_the_host_routes_files(dev, edge, tmp_path):
    from PIL import Image
    gt, want = edge
    host = AL.write_semantic_masks(gt, str(tmp_path / "host"), route="host", overlap="ignore")
    device = AL.write_semantic_masks(gt, str(tmp_path / "device"), overlap="ignore", n_workers=4, paint_bytes=4096, device=dev)      # "device" is the default
    assert device["stats"]["launches"] > 2 and device["stats"]["host_fallback"] == 1
    assert [os.path.basename(p) for p in host["paths"]] == [os.path.basename(p) for p in device["paths"]]
    for a, b, m in zip(host["paths"], device["paths"], want[("ignore", "label")]):
        assert open(a, "rb").read() == open(b, "rb").read(), b                            # byte for byte
        with Image.open(b) as f:
            assert f.mode == "L" and np.array_equal(np.asarray(f), m)
    assert not [t for t in __import__("threading").enumerate() if t.name.startswith("zutis-write")]


# ---- evaluation straight from the annotations
@pytest.fixture(scope="module")
def eval_corpus(tmp_path_factory):
    """(image paths, the annotation dict over categories 0 .. N_CAT - 1, image ids): tests/test_evaluate_gpu.py's ten files of three sizes
    (and one larger), with rectangles, stars and a crowd per image."""
    d = tmp_path_factory.mktemp("eval_ann")
    rng = np.random.default_rng(21)
    b, images = LC.Builder(), []
    from tests import _polygon_case as PC
    for k, (h, w) in enumerate(TE.FILE_HW):
        p = str(d / f"im{k:02d}.png")
        TE._photo(h, w, 900 + k).save(p, compress_level=1)
        images.append(p)
        i = b.image(h, w, file_name=f"im{k:02d}.jpg")
        for _ in range(int(rng.integers(2, 6))):
            x0, y0 = int(rng.integers(0, w - 8)), int(rng.integers(0, h - 8))
            b.add(i, int(rng.integers(0, TE.N_CAT)), [LC.rect(x0, y0, x0 + int(rng.integers(8, 50)), y0 + int(rng.integers(8, 40)))],
                  area=float(rng.integers(64, 2000)))
        b.add(i, int(rng.integers(0, TE.N_CAT)), [PC.star(rng, h, w)], area=500.0)
        b.add(i, int(rng.integers(0, TE.N_CAT)), LC.rle_segmentation(CC.box(h, w, 4, 4, 20, 30) & (rng.random((h, w)) > .2), "str"), iscrowd=1,
              area=300.0)
    gt = b.done(categories=range(TE.N_CAT))
    return images, gt, [im["id"] for im in gt["images"]]


@pytest.mark.parametrize("batch_size", [1, 4])
def test_evaluate_from_annotations_equals_evaluate_from_files_on_the_written_pngs(dev, net, eval_corpus, tmp_path, batch_size):  # noqa: F811
    from zutis_amd import _lib, evaluate
    images, gt, ids = eval_corpus
    rules = dict(crowd="ignore", order="area")
    written = AL.write_semantic_masks(gt, str(tmp_path / "semantic_segmentation_masks"), device=dev, **rules)
    kw = dict(max_size=TE.MAX_SIZE, mean=TE.MEAN, std=TE.STD, batch_size=batch_size, n_workers=4)
    files = evaluate.evaluate_from_files(net, images, written["paths"], TE.N_CAT, gt_format="u8", **kw)
    counts = {}
    _lib.COUNTER = counts
    try:
        anns = evaluate.evaluate_from_annotations(net, images, gt, TE.N_CAT, image_ids=ids, **kw, **rules)
    finally:
        _lib.COUNTER = None
    assert counts["zh_runs_label_maps"] == counts["zh_upsample_argmax_score"] == counts["zh_resize_normalize_u8"]       # one paint per batch
    assert counts.get("zh_polygon_runs") == 1 and counts.get("zh_rle_prefix") == 1                                  # the file is converted once
    print(f"batch_size {batch_size}: {counts['zh_runs_label_maps']} batches, {int(files['confusion_matrix'].sum())} pixels counted")
    assert files["confusion_matrix"].sum() > 0 and np.array_equal(anns["confusion_matrix"], files["confusion_matrix"])
    assert TE._same_scores(anns["scores"], files["scores"]) and TE._same_scores(anns["cls_iu"], files["cls_iu"])
    assert sorted(anns) == sorted(files) and anns["instance_predictions"] == [] and TE._no_decode_threads()


def test_evaluate_from_annotations_with_instances_gains_coco_metrics(dev, net, eval_corpus, tmp_path):  # noqa: F811
    from zutis_amd import coco_eval, evaluate
    images, gt, ids = eval_corpus
    kw = dict(max_size=None, mean=TE.MEAN, std=TE.STD, batch_size=4, n_workers=4)
    got = evaluate.evaluate_from_annotations(net, images, gt, TE.N_CAT, image_ids=ids, instance=True, nms_type="hard", **kw)
    assert len(got["instance_predictions"]) > 0 and {p["image_id"] for p in got["instance_predictions"]} <= set(ids)
    own = coco_eval.mask_ap(gt, got["instance_predictions"], image_ids=ids, device=dev)
    assert sorted(got["coco_metrics"]) == sorted(own)
    for key in ("stats", "precision", "recall"):
        assert np.array_equal(got["coco_metrics"][key], own[key]), key
    written = AL.write_semantic_masks(gt, str(tmp_path / "m"), device=dev)
    files = evaluate.evaluate_from_files(net, images, written["paths"], TE.N_CAT, **kw)
    assert np.array_equal(got["confusion_matrix"], files["confusion_matrix"]) and "coco_metrics" not in files
    assert TE._no_decode_threads()
    with pytest.raises(ValueError):
        evaluate.evaluate_from_annotations(net, images, gt, TE.N_CAT, image_ids=ids[:-1])
    with pytest.raises(ValueError, match="im01"):                                         # an 80 x 64 file under the id of a 64 x 96 image
        evaluate.evaluate_from_annotations(net, images[:2], gt, TE.N_CAT, image_ids=[ids[0], ids[2]], batch_size=1, n_workers=2)
    assert TE._no_decode_threads()
