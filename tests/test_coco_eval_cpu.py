"""CPU: the host layers of COCO mask AP (zutis_amd/coco_eval.py: prepare, accumulate, summarize; rle.from_polygons, rle.counts_np) and
the test reference itself (tests/_cocoeval_ref.py) on cases computable by hand.  The device part (IoU and matching kernels) is stood in
for by the reference's own functions (tests/_cocoeval_case.numpy_matches); tests/test_coco_eval_gpu.py runs the kernels."""
import ctypes
import json

import numpy as np
import pytest

from tests import _cocoeval_case as CC
from tests import _cocoeval_ref as R
from zutis_amd import _lib, build, coco_eval, rle

NAMES = ["AP", "AP_50", "AP_75", "AP_small", "AP_medium", "AP_large", "AR_1", "AR_10", "AR_100", "AR_small", "AR_medium", "AR_large"]


def host_mask_ap(ann, preds, **kw):
    """mask_ap with the device part replaced by the reference's functions."""
    prob = coco_eval.prepare(ann, preds, **kw)
    return coco_eval.result_dict(*coco_eval.accumulate(prob, CC.numpy_matches(prob)), prob.max_dets)


def both(sizes, cats, gts, dets, **kw):
    """(host layers, reference) on the same corpus, after asserting that every array of the two agrees exactly."""
    got = host_mask_ap(*CC.to_coco(sizes, cats, gts, dets), **kw)
    ref = R.mask_ap(list(sizes), cats, gts, dets, **kw)
    for key in ("stats", "precision", "recall"):
        assert got[key].dtype == np.float64 and got[key].shape == ref[key].shape and np.array_equal(got[key], ref[key]), key
    names = coco_eval.metric_names(kw.get("max_dets", (1, 10, 100)))
    assert [got[n] for n in names] == [ref[n] for n in names] == list(got["stats"])
    return got, ref


def test_shapes_thresholds_and_key_names():
    assert np.array_equal(coco_eval.IOU_THRS, np.linspace(.5, .95, 10)) and np.array_equal(coco_eval.REC_THRS, np.linspace(0, 1, 101))
    assert np.array_equal(coco_eval.AREA_RANGES, np.array(R.AREA_RANGES, np.float64))
    assert coco_eval.metric_names((1, 10, 100)) == NAMES and coco_eval.metric_names((1, 5, 7))[6:9] == ["AR_1", "AR_5", "AR_7"]
    got, _ = both({1: (12, 12)}, [1, 2], [CC.gt(1, 1, CC.box(12, 12, 0, 0, 4, 4))], [CC.det(1, 1, .5, CC.box(12, 12, 0, 0, 4, 4))])
    assert got["precision"].shape == (10, 101, 2, 4, 3) and got["recall"].shape == (10, 2, 4, 3) and got["stats"].shape == (12,)


def test_higher_scored_miss_then_exact_hit_is_half():
    """One ground truth (16 pixels: small).  Detections in score order: a miss (9 pixels elsewhere), then the exact mask.  tp = [0, 1],
    fp = [1, 1], recall = [0, 1], precision = [0, 1 / (2 + spacing(1))] = [0, 0.5] (2 + 2^-52 rounds to 2), made monotone: [0.5, 0.5];
    every recall threshold samples 0.5.  With one detection allowed only the miss is seen: AR_1 = 0."""
    g = [CC.gt(1, 1, CC.box(20, 20, 2, 2, 6, 6))]
    d = [CC.det(1, 1, .9, CC.box(20, 20, 10, 10, 13, 13)), CC.det(1, 1, .4, CC.box(20, 20, 2, 2, 6, 6))]
    got, _ = both({1: (20, 20)}, [1], g, d)
    assert 1 / (2 + np.spacing(1)) == 0.5
    assert got["AP"] == got["AP_50"] == got["AP_75"] == got["AP_small"] == 0.5
    assert got["AP_medium"] == got["AP_large"] == got["AR_medium"] == got["AR_large"] == -1.0
    assert got["AR_1"] == 0.0 and got["AR_10"] == got["AR_100"] == got["AR_small"] == 1.0
    assert np.all(got["precision"][:, :, 0, 0, 2] == 0.5) and np.all(got["precision"][:, 1:, 0, 0, 0] == 0.0)


def test_perfect_predictions_are_one_and_unpopulated_area_rows_minus_one():
    """Two images with one small and one medium object each, predicted exactly: cumulative tp = [1, 2] per (category, range), precision
    [1 / (1 + 2^-52), 2 / 2] made monotone from the right = [1, 1]."""
    sizes = {1: (50, 50), 2: (50, 50)}
    g = [CC.gt(i, 1, CC.box(50, 50, 0, 0, 5, 5 + i)) for i in sizes] + [CC.gt(i, 2, CC.box(50, 50, 10, 10, 45, 44 + i)) for i in sizes]
    d = [CC.det(x["image_id"], x["category_id"], .5 + .1 * j, x["mask"]) for j, x in enumerate(g)]
    got, _ = both(sizes, [1, 2], g, d)
    assert [got[n] for n in NAMES] == [1.0, 1.0, 1.0, 1.0, 1.0, -1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -1.0]
    assert set(np.unique(got["precision"])) == {-1.0, 1.0} and np.all(got["precision"][:, :, :, 3, :] == -1.0)


def test_no_predictions():
    """accumulate with no detection: recall 0 and an all-zero precision row where the range holds a ground truth, -1 elsewhere."""
    got, _ = both({1: (20, 20)}, [1], [CC.gt(1, 1, CC.box(20, 20, 2, 2, 6, 6))], [])
    assert [got[n] for n in NAMES] == [0.0, 0.0, 0.0, 0.0, -1.0, -1.0, 0.0, 0.0, 0.0, 0.0, -1.0, -1.0]


@pytest.mark.parametrize("name", sorted(CC.RULES))
def test_matching_rules_of_the_reference_by_hand(name):
    """The crowd rule, the ignore-ordering break and "the later equal IoU wins", each on a 2 x 3 IoU matrix (tests/_cocoeval_case.RULES
    states the walk)."""
    case = CC.RULES[name]
    match, ignore, _ = R.match_group(np.array(case["iou"]), case["gt_ignore"], case["crowd"], CC.DET_AREA, R.AREA_RANGES[0])
    for t, (m, ig) in case["expect"].items():
        assert match[t].tolist() == m and ignore[t].astype(int).tolist() == ig, (name, t)


def test_without_categories_a_detection_of_another_category_matches():
    g = [CC.gt(1, 1, CC.box(20, 20, 2, 2, 6, 6)), CC.gt(1, 2, CC.box(20, 20, 10, 10, 16, 16))]
    d = [CC.det(1, 2, .9, CC.box(20, 20, 2, 2, 6, 6)), CC.det(1, 1, .8, CC.box(20, 20, 10, 10, 16, 16))]
    with_c, _ = both({1: (20, 20)}, [1, 2], g, d, use_categories=True)
    without, _ = both({1: (20, 20)}, [1, 2], g, d, use_categories=False)
    assert with_c["AP"] == 0.0 and with_c["precision"].shape[2] == 2
    assert without["AP"] == 1.0 and without["precision"].shape[2] == 1 and without["AR_1"] == 0.5


def test_image_ids_restrict_the_evaluation():
    sizes = {1: (20, 20), 2: (20, 20), 3: (20, 20)}
    g = [CC.gt(i, 1, CC.box(20, 20, 2, 2, 6, 6)) for i in sizes]
    d = [CC.det(1, 1, .9, CC.box(20, 20, 2, 2, 6, 6)), CC.det(2, 1, .8, CC.box(20, 20, 10, 10, 13, 13))]
    all_, _ = both(sizes, [1], g, d)
    one, _ = both(sizes, [1], g, d, image_ids=[1])
    two, _ = both(sizes, [1], g, d, image_ids=[2, 1, 2])
    assert one["AR_100"] == 1.0 and two["AR_100"] == 0.5 and all_["AR_100"] == float(np.mean([1 / 3] * 10))
    ann, preds = CC.to_coco(sizes, [1], g, d)
    with pytest.raises(ValueError, match="image 9"):
        coco_eval.prepare(ann, preds + [dict(preds[0], image_id=9)])
    with pytest.raises(ValueError, match="max_dets"):
        coco_eval.prepare(ann, preds, max_dets=(1, 10))


def test_synthetic_corpus_host_layers_equal_the_reference():
    sizes, cats, g, d = CC.synthetic_corpus()
    for use in (True, False):
        got, ref = both(sizes, cats, g, d, use_categories=use)
        assert got["AP_small"] > -1 and got["AP_medium"] > -1 and got["AP_large"] == -1.0 and 0 < got["AP"] < 1
    got, _ = both(sizes, cats, g, d, max_dets=(1, 2, 3))
    assert "AR_3" in got and "AR_100" not in got


def test_detections_are_ordered_cut_and_numbered_as_loadres_does():
    h = w = 16
    d = [CC.det(1, 1, s, CC.box(h, w, 0, 0, 2, 2 + j)) for j, s in enumerate([.3, .9, .3, .5])]
    ann, preds = CC.to_coco({1: (h, w)}, [1], [CC.gt(1, 1, CC.box(h, w, 0, 0, 2, 2))], d)
    prob = coco_eval.prepare(ann, preds, max_dets=(1, 2, 3))
    (grp,) = prob.groups
    assert grp.det_id.tolist() == [2, 4, 1] and grp.det_score.tolist() == [.9, .5, .3]          # stable among the equal scores, cut to 3
    assert [int(prob.masks[m][0][1::2].sum()) for m in grp.det_mask] == [6, 10, 4]


def test_the_three_forms_of_counts_decode_alike(tmp_path):
    sizes, cats, g, d = CC.synthetic_corpus(seed=3, n_images=2)
    res = [host_mask_ap(*CC.to_coco(sizes, cats, g, d, counts_form=f)) for f in ("bytes", "str", "list")]
    assert np.array_equal(res[0]["precision"], res[1]["precision"]) and np.array_equal(res[0]["precision"], res[2]["precision"])
    m = g[0]["mask"]
    e = rle.encode_py(m)
    assert np.array_equal(rle.counts_np(e["counts"]), rle._counts(m)) and np.array_equal(rle.counts_np(e["counts"].decode()), rle._counts(m))
    assert np.array_equal(rle.counts_np(rle._counts(m).tolist()), rle._counts(m)) and rle.counts_np(b"").size == 0
    assert rle.counts_np(e["counts"]).tolist() == rle._from_string(e["counts"])
    with pytest.raises(ValueError):
        rle.counts_np(b"0" + bytes([48 + 0x20]))                          # the last character announces another one
    # both arguments as the paths of JSON files, as trainer.py:393-398 writes the predictions (bytes -> str, no bbox)
    ann, preds = CC.to_coco(sizes, cats, g, d, counts_form="str")
    for p in preds:
        p.pop("bbox")
    (tmp_path / "ann.json").write_text(json.dumps(ann))
    (tmp_path / "pred.json").write_text(json.dumps(preds))
    from_files = host_mask_ap(str(tmp_path / "ann.json"), str(tmp_path / "pred.json"))
    assert np.array_equal(from_files["precision"], res[0]["precision"])


def test_from_polygons_by_hand():
    """rleFrPoly by hand.  Corners are scaled by 5; walking an edge, a step from column u - 1 to u of the fine grid crosses a pixel-column
    centre when (u - 1 + .5) / 5 - .5 is an integer c (u = 5 c + 3), and the row bound there is ceil((v + .5) / 5 - .5).
    An integer-cornered rectangle x0 <= x < x1, y0 <= y < y1 therefore fills exactly the pixels [y0, y1) x [x0, x1)."""
    assert np.array_equal(rle.decode(rle.from_polygons([[1, 1, 4, 1, 4, 3, 1, 3]], 5, 6)), CC.box(5, 6, 1, 1, 3, 4))
    assert np.array_equal(rle.decode(rle.from_polygons([1.0, 1.0, 4.0, 1.0, 4.0, 3.0, 1.0, 3.0], 5, 6)), CC.box(5, 6, 1, 1, 3, 4))    # one flat list
    assert np.array_equal(rle.decode(rle.from_polygons([[0, 0, 6, 0, 6, 5, 0, 5]], 5, 6)), np.ones((5, 6), bool))
    # right triangle (0,0), (6,0), (0,6) on 6 x 6: the hypotenuse is walked with u falling; it enters column c at u = 5 c + 2, where
    # v = 30 - u and the smaller neighbour row is 27 - 5 c: bound ceil((27.5 - 5 c) / 5 - .5) = 5 - c.  Column c holds rows 0 .. 4 - c.
    tri = np.array([[c + r < 5 for c in range(6)] for r in range(6)])
    assert np.array_equal(rle.decode(rle.from_polygons([[0, 0, 6, 0, 0, 6]], 6, 6)), tri)
    # a polygon leaving the image: columns left of 0 are dropped, rows past the height are clamped
    assert np.array_equal(rle.decode(rle.from_polygons([[-2, 1, 4, 1, 4, 9, -2, 9]], 5, 6)), CC.box(5, 6, 1, 0, 5, 4))
    # two overlapping polygons are united
    two = rle.from_polygons([[0, 0, 3, 0, 3, 3, 0, 3], [2, 2, 5, 2, 5, 4, 2, 4]], 5, 6)
    assert np.array_equal(rle.decode(two), CC.box(5, 6, 0, 0, 3, 3) | CC.box(5, 6, 2, 2, 4, 5)) and two["size"] == [5, 6]
    assert rle.from_polygons([[1, 1, 4, 1, 4, 3, 1, 3]], 5, 6) == rle.encode_py(CC.box(5, 6, 1, 1, 3, 4))


def test_polygon_ground_truth_is_rasterised_at_the_image_size():
    sizes, h, w = {1: (20, 24)}, 20, 24
    m = CC.box(h, w, 3, 4, 11, 15)
    ann, preds = CC.to_coco(sizes, [1], [CC.gt(1, 1, m)], [CC.det(1, 1, .9, m)])
    ann["annotations"][0]["segmentation"] = [[4, 3, 15, 3, 15, 11, 4, 11]]
    prob = coco_eval.prepare(ann, preds)
    assert np.array_equal(prob.masks[prob.groups[0].gt_mask[0]][0], rle._counts(m)) and prob.masks[0][1] == h * w


def test_compute_coco_metrics_binds_as_the_trainer_method_and_accepts_dicts_without_bbox(monkeypatch):
    """trainer.py:393 pops bbox from every prediction before trainer.py:402 calls the method."""
    monkeypatch.setattr(coco_eval, "match_on_device", lambda prob, device, chunk_bytes=0: CC.numpy_matches(prob))
    sizes, cats, g, d = CC.synthetic_corpus(seed=5, n_images=3)
    ann, preds = CC.to_coco(sizes, cats, g, d)
    [p.pop("bbox") for p in preds]

    class Trainer:
        device = "cuda:0"
        compute_coco_metrics = coco_eval.compute_coco_metrics

    got = Trainer().compute_coco_metrics(p_annotations=ann, instance_predictions=preds)
    ref = R.mask_ap(list(sizes), cats, g, d)
    assert list(got) == NAMES and [got[n] for n in NAMES] == [ref[n] for n in NAMES] and all(isinstance(v, float) for v in got.values())
    got = Trainer().compute_coco_metrics(ann, preds, False, (1, 5, 7))
    assert list(got)[6:9] == ["AR_1", "AR_5", "AR_7"] and got["AP"] == R.mask_ap(list(sizes), cats, g, d, False, (1, 5, 7))["AP"]


def test_there_is_no_cpu_fallback():
    sizes, cats, g, d = CC.synthetic_corpus(seed=5, n_images=1)
    with pytest.raises(_lib.ZutisHipError, match="no CPU fallback"):
        coco_eval.mask_ap(*CC.to_coco(sizes, cats, g, d), device="cpu")


def test_evaluate_from_files_takes_coco_annotations_keyword_only():
    import inspect
    from zutis_amd import evaluate
    p = inspect.signature(evaluate.evaluate_from_files).parameters["coco_annotations"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    sig = inspect.signature(coco_eval.mask_ap)
    assert list(sig.parameters) == ["ground_truth", "predictions", "use_categories", "max_dets", "image_ids", "device"]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in sig.parameters.items() if k not in ("ground_truth", "predictions"))
    assert list(inspect.signature(coco_eval.compute_coco_metrics).parameters) == ["self", "p_annotations", "instance_predictions",
                                                                                 "use_categories", "n_max_detections"]


def test_header_declares_the_entries_and_the_abi_bump():
    build.build(verbose=False)
    lib = _lib.load()
    vp, i, l, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_size_t
    e = _lib.entries()
    assert (e["zh_rle_prefix"].restype, e["zh_rle_prefix"].argtypes) == (i, [vp, vp, vp, i, vp, vp, vp, vp, vp])
    assert (e["zh_rle_pair_iou"].restype, e["zh_rle_pair_iou"].argtypes) == (i, [vp, vp, vp, vp, vp, vp, i, vp, vp, vp, l, vp, vp, vp])
    assert (e["zh_coco_match"].restype, e["zh_coco_match"].argtypes) == (i, [vp, vp, i, vp, vp, vp, vp, vp, l, vp, i, vp, i, vp, vp, vp, z, vp])
    assert (e["zh_coco_match_workspace_size"].restype, e["zh_coco_match_workspace_size"].argtypes) == (z, [l, i, i])
    for name in ("zh_rle_prefix", "zh_rle_pair_iou", "zh_coco_match", "zh_coco_match_workspace_size", "zh_rle_iou_lds_runs"):
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == e[name].argtypes
    assert all(e[n].plannable for n in ("zh_rle_prefix", "zh_rle_pair_iou", "zh_coco_match"))
    assert _lib.header_abi_version() >= 234
    assert lib.zh_rle_iou_lds_runs() == _lib.constants()["ZH_RLE_IOU_LDS_RUNS"] == coco_eval.LDS_RUNS == 1024       # the library was compiled with the header's value
    assert lib.zh_coco_match_workspace_size(7, 10, 4) == 280
    # argument checks come before any launch, and empty calls launch nothing
    assert lib.zh_rle_prefix(None, None, None, 0, None, None, None, None, None) == 0
    assert lib.zh_rle_pair_iou(None, None, None, None, None, None, 3, None, None, None, 0, None, None, None) == 0
    assert lib.zh_rle_pair_iou(16, 16, 16, 16, 16, 16, 1, 16, 16, 16, 1 << 31, 16, 16, None) == -1 and b"pairs" in lib.zh_last_error()
    assert lib.zh_coco_match(16, 16, 1, 16, 16, 16, 16, 16, 1, 16, 10, 16, 7, 16, 16, 16, 70, None) == -1 and b"problems" in lib.zh_last_error()
    assert lib.zh_coco_match(16, 16, 1, 16, 16, 16, 16, 16, 1, 16, 10, 16, 4, 16, 16, 16, 39, None) == -3 and b"workspace" in lib.zh_last_error()


def test_against_pycocotools_when_it_imports(tmp_path):
    pytest.importorskip("pycocotools")
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    sizes, cats, g, d = CC.synthetic_corpus(seed=7)
    ann, preds = CC.to_coco(sizes, cats, g, d, counts_form="str")
    (tmp_path / "ann.json").write_text(json.dumps(ann))
    coco_gt = COCO(str(tmp_path / "ann.json"))
    ev = COCOeval(coco_gt, coco_gt.loadRes(preds), iouType="segm")
    ev.evaluate(), ev.accumulate(), ev.summarize()
    got = host_mask_ap(ann, preds)
    assert np.array_equal(got["stats"], ev.stats) and np.array_equal(got["precision"], ev.eval["precision"])
    assert np.array_equal(got["recall"], ev.eval["recall"])
    import pycocotools.mask as M
    poly = [[3.2, 4.7, 40.1, 6.3, 35.5, 30.9, 8.8, 25.2]]
    assert rle.from_polygons(poly, 48, 64)["counts"] == M.merge(M.frPyObjects(poly, 48, 64))["counts"]
