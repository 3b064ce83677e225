"""-m gpu: the instance pictures of predict_from_files (instance_map / instance_overlay), ZUTIS.predict_instances_painted behind them and
the Visualiser binding, on the TINY drop-in ZUTIS over the seeded photo corpus of tests/test_predict_files_gpu.py.  The id map is checked
against the returned predictions themselves (their decoded RLEs, scores and ids), the overlay against instance_paint.paint_reference on
the decoded file; byte equality throughout.

TINY's five queries are near copies of each other, so hard NMS keeps one mask per image: the main call runs nms_type="gaussian" (a predict
argument), whose decayed scores keep up to four heavily overlapping masks per image — the device NMS path with overlap to resolve —, at a
min_score that leaves some of them unpainted.  One image of the corpus (48 x 80, index 7) has no prediction at all."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests.test_predict_files_gpu import FILE_HW, MAX_SIZE, MEAN, N_CAT, PALETTE, STD, _build, _no_threads, images  # noqa: F401  (images: the corpus fixture)
from zutis_amd import rle

pytestmark = pytest.mark.gpu

ALPHA = 96
MIN_SCORE = 0.05                   # between the second and the third kept score of most images (~0.06 / ~0.01): two painted, two not


@pytest.fixture(scope="module")
def net(dev):
    return _build(dev, N_CAT)


def _call(net, images, out_dir, batch_size, n_workers=8, **kw):
    from zutis_amd import predict_files
    got = predict_files.predict_from_files(net, images, out_dir=str(out_dir), max_size=MAX_SIZE, mean=MEAN, std=STD, batch_size=batch_size,
                                           n_workers=n_workers, instance=True, image_ids=list(range(len(images))), **kw)
    assert _no_threads()
    return got


def _by_image(got, n):
    """[[(id, score, category, mask u8 [H,W]) ...] per image] from the result's predictions and their instance_ids."""
    assert len(got["instance_ids"]) == len(got["instance_predictions"])
    per = [[] for _ in range(n)]
    for p, pid in zip(got["instance_predictions"], got["instance_ids"]):
        per[p["image_id"]].append((pid, p["score"], p["category_id"], rle.decode_np(p["segmentation"])))
    for ps in per:
        assert len({pid for pid, *_ in ps}) == len(ps) and all(pid >= 1 for pid, *_ in ps)      # ids are unique inside an image
    return per


def _expected_ids(preds, H, W, min_score):
    """Per pixel the id of the highest-score prediction (ties: the lower id) with score > min_score that covers it; 0 for none."""
    ids = np.zeros((H, W), np.int64)
    for pid, _, _, m in sorted((p for p in preds if p[1] > min_score), key=lambda p: (-p[1], p[0])):
        ids[(ids == 0) & (m != 0)] = pid
    return ids


def _reference(image, preds, colour_of, min_score, alpha=ALPHA, outline=True):
    """paint_reference on the decoded RLEs in id order (an id no prediction carries: an empty mask that is never painted)."""
    from zutis_amd.instance_paint import paint_reference
    H, W = image.shape[:2]
    n = max([pid for pid, *_ in preds], default=0)
    masks, scores, colours = np.zeros((n, H, W), np.uint8), np.full((n,), -np.inf), np.zeros((n, 3), np.uint8)
    for pid, s, c, m in preds:
        masks[pid - 1], scores[pid - 1], colours[pid - 1] = m, s, colour_of(pid, c)
    return paint_reference(image, masks, scores, colours, alpha=alpha, outline=outline, min_score=min_score)


def _read(path, mode):
    with Image.open(path) as im:
        assert im.mode == mode, (path, im.mode)
        return np.asarray(im).copy()


@pytest.mark.parametrize("batch_size,n_workers", [(4, 16), (3, 2)])
def test_id_map_overlay_and_unchanged_outputs(dev, net, images, tmp_path, batch_size, n_workers):
    from zutis_amd.instance_paint import instance_colours
    common = dict(palette=PALETTE, overlay=True, alpha=ALPHA, nms_type="gaussian")
    got = _call(net, images, tmp_path / "new", batch_size, n_workers, instance_map=True, instance_overlay=True, instance_min_score=MIN_SCORE, **common)
    base = _call(net, images, tmp_path / "base", batch_size, n_workers, **common)
    # what the call gave before is what it gives now
    assert sorted(base) == ["instance_predictions", "label_paths", "n_images", "overlay_paths"]
    assert got["instance_predictions"] == base["instance_predictions"] and len(base["instance_predictions"]) > 0
    for a, b in zip(got["label_paths"] + got["overlay_paths"], base["label_paths"] + base["overlay_paths"]):
        assert os.path.basename(a) == os.path.basename(b) and open(a, "rb").read() == open(b, "rb").read(), a
    stems = [os.path.splitext(os.path.basename(p))[0] for p in images]
    assert got["instance_map_paths"] == [str(tmp_path / "new" / f"{s}_instances.png") for s in stems]
    assert got["instance_overlay_paths"] == [str(tmp_path / "new" / f"{s}_instances_overlay.png") for s in stems]
    assert len(os.listdir(tmp_path / "new")) == 4 * len(images) and len(os.listdir(tmp_path / "base")) == 2 * len(images)
    per = _by_image(got, len(images))
    from zutis_amd import detgen
    table = instance_colours(detgen.TINY.n_queries)                               # the default colours: entry id - 1
    overlapping, unpainted, with_unpainted_predictions = 0, 0, 0
    for i, preds in enumerate(per):
        H, W = FILE_HW[i]
        ids = _read(got["instance_map_paths"][i], "L").astype(np.int64)          # five queries: one byte per pixel
        assert ids.shape == (H, W)
        want = _expected_ids(preds, H, W, MIN_SCORE)
        assert np.array_equal(ids, want), got["instance_map_paths"][i]
        assert set(np.unique(ids).tolist()) - {0} <= {pid for pid, s, _, _ in preds if s > MIN_SCORE}
        image = np.asarray(Image.open(images[i]).convert("RGB"))                  # the decoded file at ITS size (the 128 x 192 one too)
        ref_ids, ref_overlay = _reference(image, preds, lambda pid, c: table[pid - 1], MIN_SCORE)
        assert np.array_equal(ref_ids, want)
        assert np.array_equal(_read(got["instance_overlay_paths"][i], "RGB"), ref_overlay), got["instance_overlay_paths"][i]
        painted = [p for p in preds if p[1] > MIN_SCORE]
        overlapping += any(((a[3] != 0) & (b[3] != 0)).any() for k, a in enumerate(painted) for b in painted[k + 1:])
        unpainted += not painted
        with_unpainted_predictions += len(painted) < len(preds)
    print(f"batch_size {batch_size}: {len(got['instance_predictions'])} predictions, {overlapping} images with overlapping painted masks, "
          f"{unpainted} with nothing painted, {with_unpainted_predictions} with predictions at or under min_score")
    assert overlapping >= 1 and unpainted >= 1 and with_unpainted_predictions >= 1          # the corpus exercises what the test is about


def test_stand_alone_with_category_colours_and_a_score_filter(dev, net, images, tmp_path):
    """semantic=False: only the two instance files are written, beside where the label maps would go; hard NMS (one mask per image), the
    colour the palette gives the prediction's category, and a min_score that leaves several images unpainted."""
    min_score = 0.35
    got = _call(net, images, tmp_path / "out", 4, semantic=False, palette=PALETTE, instance_map=True, instance_overlay=True, instance_colours="category",
                instance_min_score=min_score, alpha=256, instance_outline=False, nms_type="hard")
    assert got["label_paths"] is None and got["overlay_paths"] is None
    stems = [os.path.splitext(os.path.basename(p))[0] for p in images]
    assert sorted(os.listdir(tmp_path / "out")) == sorted([f"{s}_instances.png" for s in stems] + [f"{s}_instances_overlay.png" for s in stems])
    per = _by_image(got, len(images))
    painted = 0
    for i, preds in enumerate(per):
        image = np.asarray(Image.open(images[i]).convert("RGB"))
        ref_ids, ref_overlay = _reference(image, preds, lambda pid, c: PALETTE[c], min_score, alpha=256, outline=False)
        assert np.array_equal(_read(got["instance_map_paths"][i], "L"), ref_ids)
        assert np.array_equal(_read(got["instance_overlay_paths"][i], "RGB"), ref_overlay)
        painted += bool(ref_ids.any())
    assert 0 < painted < len(images) and sum(len(p) for p in per) > painted               # some images painted, some predictions filtered out


def test_without_nms_the_uploaded_kept_list_is_painted(dev, net, images, tmp_path):
    """nms_type=None: every query with a category is a prediction, the slot table is built on the host and uploaded.  Colours from an array."""
    colours = np.array([[250, 10, 10], [10, 250, 10], [10, 10, 250], [250, 250, 10], [10, 250, 250]], np.uint8)
    got = _call(net, images[:4], tmp_path / "out", 2, semantic=False, instance_map=True, instance_overlay=True, instance_colours=colours, alpha=ALPHA,
                nms_type=None)
    per = _by_image(got, 4)
    assert max(len(p) for p in per) >= 2
    for i, preds in enumerate(per):
        image = np.asarray(Image.open(images[i]).convert("RGB"))
        ref_ids, ref_overlay = _reference(image, preds, lambda pid, c: colours[pid - 1], 0.0)
        assert np.array_equal(_read(got["instance_map_paths"][i], "L"), ref_ids)
        assert np.array_equal(_read(got["instance_overlay_paths"][i], "RGB"), ref_overlay)
    too_few = colours[:3]
    with pytest.raises(ValueError, match="queries"):
        _call(net, images[:2], tmp_path / "few", 2, semantic=False, instance_overlay=True, instance_colours=too_few)
    assert _no_threads()


def test_the_visualiser_binding(dev, net, images, tmp_path):
    """visualise_instance_predictions bound as a method, on one image's dicts: paint_reference with label_id_to_rgb's colours and the
    confidence threshold as min_score; from a PIL image and from the normalised float array; the file decodes to the returned array."""
    from zutis_amd import predict_files
    from zutis_amd.instance_paint import instance_colours, visualise_instance_predictions

    class Visualiser:
        pass
    Visualiser.visualise_instance_predictions = visualise_instance_predictions
    got = predict_files.predict_from_files(net, images[:1], semantic=False, instance=True, max_size=None, mean=MEAN, std=STD, nms_type="gaussian")
    preds = got["instance_predictions"]
    assert len(preds) >= 3
    threshold = sorted(p["score"] for p in preds)[-2]                              # strict: the second-best score itself is not drawn
    pil = Image.open(images[0]).convert("RGB")
    image = np.asarray(pil)
    rows = [(k + 1, p["score"], p["category_id"], rle.decode_np(p["segmentation"])) for k, p in enumerate(preds)]
    fp = str(tmp_path / "vis.png")
    out = Visualiser().visualise_instance_predictions(pil, preds, label_id_to_rgb=PALETTE, confidence_threshold=threshold, fp=fp)
    want_ids, want = _reference(image, rows, lambda pid, c: PALETTE[c], threshold, alpha=128)
    assert out.dtype == np.uint8 and np.array_equal(out, want) and len(np.unique(want_ids)) == 2
    assert np.array_equal(_read(fp, "RGB"), out)
    # the default colours, every prediction drawn, from the tensor the dataset yields
    x = ((image.transpose(2, 0, 1).astype(np.float32) / 255 - np.array(MEAN, np.float32)[:, None, None]) / np.array(STD, np.float32)[:, None, None])
    from zutis_amd.instance_paint import _image_bytes
    table = instance_colours(len(preds))
    out = Visualiser().visualise_instance_predictions(x, preds, confidence_threshold=0.0)
    _, want = _reference(_image_bytes(x), rows, lambda pid, c: table[pid - 1], 0.0, alpha=128)
    assert np.array_equal(out, want)
    assert np.array_equal(Visualiser().visualise_instance_predictions(pil, []), image)          # nothing to draw: the image


def test_a_writer_failure_reaches_the_caller_and_the_next_call_works(dev, net, images, tmp_path):
    (tmp_path / "plain_file").write_bytes(b"not a directory")
    with pytest.raises(OSError):                                                   # the output directory cannot be made
        _call(net, images[:3], tmp_path / "plain_file" / "sub", 2, semantic=False, instance_map=True)
    assert _no_threads()
    os.makedirs(tmp_path / "b" / "im01_instances_overlay.png")                     # a writer's target is a directory
    with pytest.raises(OSError):
        _call(net, images[:5], tmp_path / "b", 1, n_workers=4, instance_map=True, instance_overlay=True)
    assert _no_threads()
    torch.cuda.synchronize()
    got = _call(net, images[:3], tmp_path / "c", 1, n_workers=4, semantic=False, instance_map=True, nms_type="gaussian")
    for i, preds in enumerate(_by_image(got, 3)):
        assert np.array_equal(_read(got["instance_map_paths"][i], "L"), _expected_ids(preds, *FILE_HW[i], 0.0))
    assert sorted(os.listdir(tmp_path / "c")) == [f"im{i:02d}_instances.png" for i in range(3)]
