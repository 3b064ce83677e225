"""Semantic ground truth from COCO annotations on the host (zutis_amd/annotation_labels.py): paint_plan's rules and labels_np, the
definition, against label maps written out by hand; the default label numbering; and the NumPy restatement of the walk the kernel runs
(tests/_label_paint_case.walk_np) against labels_np on the edge set.  No GPU."""
import ast
import inspect
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from tests import _label_paint_case as LC
from zutis_amd import annotation_labels as AL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_COCO = os.path.join(os.environ.get("ZUTIS_REFERENCE_DIR") or os.path.join(os.path.dirname(ROOT), "reference"), "datasets", "coco2017.py")
COCO_IDS = [i for i in range(1, 91) if i not in (12, 26, 29, 30, 45, 66, 68, 69, 71, 83)]      # the 80 public category ids


@pytest.fixture(scope="module")
def edge():
    return LC.edge_dict()


@pytest.mark.parametrize("key,want", LC.hand_cases(), ids=lambda v: "-".join(v) if isinstance(v, tuple) else "")
def test_labels_np_equals_the_maps_worked_out_by_hand(key, want):
    order, overlap, crowd = key
    plan = AL.paint_plan(LC.hand_dict(), order=order, overlap=overlap, crowd=crowd)
    got = AL.labels_np(plan)
    assert len(got) == 1 and got[0].dtype == np.uint8 and got[0].shape == (4, 6)
    assert np.array_equal(got[0], want), (key, got[0])


def test_every_rule_combination_is_covered_by_hand():
    assert {k for k, _ in LC.hand_cases()} == set(itertools.product(AL.ORDERS, AL.OVERLAPS, AL.CROWDS))


def test_plan_lists_images_and_orders():
    gt = LC.hand_dict()
    (i,) = [im["id"] for im in gt["images"]]
    plan = AL.paint_plan(gt)
    assert plan.lists == [[(0, 2), (1, 1), (2, 4)]] and plan.images[0]["h"] == 4 and plan.images[0]["w"] == 6
    assert plan.images[0]["file_name"] == gt["images"][0]["file_name"]
    assert AL.paint_plan(gt, order="area").lists == [[(0, 2), (2, 4), (1, 1)]]          # the crowd has no `area`: its 6 pixels count
    assert AL.paint_plan(gt, crowd="ignore", ignore_value=200).lists == [[(0, 2), (2, 4), (1, 200)]]
    assert AL.paint_plan(gt, crowd="skip").lists == [[(0, 2), (2, 4)]]
    assert AL.paint_plan(gt, [i, i]).lists == plan.lists * 2                            # image_ids: those images, in that order
    assert AL.paint_plan(gt, label_of={1: 9, 3: 8, 90: 7}).lists == [[(0, 8), (1, 9), (2, 7)]]
    with pytest.raises(ValueError):
        AL.paint_plan(gt, [i + 1])
    for bad in (dict(order="size"), dict(overlap="first"), dict(crowd="paint"), dict(ignore_value=256), dict(label_of={1: 0, 3: 1, 90: 2}),
                dict(label_of={1: 255, 3: 1, 90: 2})):
        with pytest.raises(ValueError):
            AL.paint_plan(gt, **bad)


def test_an_image_without_annotations_is_all_zero(edge):
    plan = AL.paint_plan(edge)
    empty = [k for k, e in enumerate(plan.lists) if not e]
    assert len(empty) == 1 and not AL.labels_np(plan)[empty[0]].any() and AL.labels_np(plan)[empty[0]].shape == (20, 24)


def test_default_labels_of_the_public_coco_ids_are_their_ranks():
    got = AL.default_label_of(COCO_IDS)
    assert len(COCO_IDS) == 80 and [got[c] for c in COCO_IDS] == list(range(1, 81))
    assert AL.default_label_of(reversed(COCO_IDS)) == got
    plan = AL.paint_plan(LC.edge_dict(zigzags=0))
    assert {lab for e in plan.lists for _, lab in e} == {1, 2, 3, 4}                      # ids 1, 3, 7, 90


@pytest.mark.skipif(not os.path.exists(REFERENCE_COCO), reason="no reference checkout next to the repository (ZUTIS_REFERENCE_DIR)")
def test_default_labels_equal_the_reference_dict_literal():
    tree = ast.parse(open(REFERENCE_COCO).read())
    found = None
    for node in ast.walk(tree):
        targets = node.targets if isinstance(node, ast.Assign) else [node.target] if isinstance(node, ast.AnnAssign) else []
        if any("old_label_id_to_new_label_id" in ast.unparse(t) for t in targets) and isinstance(node.value, ast.Dict):
            found = ast.literal_eval(node.value)
    assert found is not None and len(found) >= 80
    want = {k: v for k, v in found.items() if k != 0}                                    # background, if the literal lists it
    assert want == AL.default_label_of(want)


def test_a_missing_category_raises():
    gt = LC.hand_dict()
    with pytest.raises(ValueError, match="category"):
        AL.paint_plan(gt, label_of={1: 1, 3: 2})                                         # 90 is painted and missing
    assert AL.paint_plan(gt, label_of={3: 2, 90: 4}, crowd="skip").lists == [[(0, 2), (2, 4)]]       # 1 is only the skipped crowd's


@pytest.mark.parametrize("overlap", AL.OVERLAPS)
@pytest.mark.parametrize("crowd", AL.CROWDS)
def test_the_kernels_walk_in_numpy_equals_labels_np_on_the_edge_set(edge, overlap, crowd):
    plan = AL.paint_plan(edge, overlap=overlap, crowd=crowd)
    want, got = AL.labels_np(plan), LC.walk_np(plan)
    assert len(want) == len(edge["images"]) == 8
    for k, (a, b) in enumerate(zip(want, got)):
        assert a.shape == (plan.images[k]["h"], plan.images[k]["w"]) and np.array_equal(a, b), (k, plan.images[k])
    assert any((m == AL.paint_plan(edge).ignore_value).any() for m in want) == (overlap == "ignore" or crowd == "ignore")


def test_the_walk_fails_when_it_is_stated_wrongly(edge):
    """The restatement is a test of something: the list walked first-to-last under "last", the parity flipped and the row-major position
    each give other maps."""
    plan = AL.paint_plan(edge)
    want = AL.labels_np(plan)
    differs = lambda got: sum(not np.array_equal(a, b) for a, b in zip(want, got))
    assert differs(LC.walk_np(plan)) == 0
    assert differs(LC.walk_np(plan, forward=True)) > 0
    assert differs(LC.walk_np(plan, parity=0)) > 0
    assert differs(LC.walk_np(plan, row_major=True)) > 0
    same = AL.paint_plan(edge, overlap="ignore")                                         # "ignore" counts the hits: the direction is free
    assert all(np.array_equal(a, b) for a, b in zip(AL.labels_np(same), LC.walk_np(same, forward=True)))


def test_write_semantic_masks_on_the_host_route(edge, tmp_path):
    res = AL.write_semantic_masks(edge, str(tmp_path / "semantic_segmentation_masks"), route="host", crowd="ignore")
    want = AL.labels_np(AL.paint_plan(edge, crowd="ignore"))
    assert len(res["paths"]) == len(want) and res["stats"]["images"] == len(want)
    for p, im, m in zip(res["paths"], edge["images"], want):
        assert os.path.basename(p) == im["file_name"].split("/")[-1].split(".jpg")[0] + ".png"    # coco2017.py:133-134
        with Image.open(p) as f:
            assert f.mode == "L" and np.array_equal(np.asarray(f), m)
    some = AL.write_semantic_masks(edge, str(tmp_path / "some"), image_ids=[edge["images"][3]["id"]], route="host")
    assert len(some["paths"]) == 1 and sorted(os.listdir(tmp_path / "some")) == [os.path.basename(some["paths"][0])]
    with pytest.raises(ValueError):
        AL.write_semantic_masks(edge, str(tmp_path / "x"), route="pillow")


def test_rle_of_the_wrong_size_or_sum_is_named():
    gt = LC.hand_dict()
    gt["annotations"][1]["segmentation"] = {"size": [4, 6], "counts": [3, 5]}
    with pytest.raises(ValueError, match="1001"):
        AL.labels_np(AL.paint_plan(gt))
    gt["annotations"][1]["segmentation"] = {"size": [6, 4], "counts": [3, 21]}
    with pytest.raises(ValueError, match="1001"):
        AL.labels_np(AL.paint_plan(gt))


def test_public_signatures():
    from zutis_amd import evaluate, ops, polygons
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(AL.paint_plan) == ["ground_truth", "image_ids", "label_of", "order", "overlap", "crowd", "ignore_value"]
    p = inspect.signature(AL.paint_plan).parameters
    assert [p[k].default for k in ("image_ids", "label_of", "order", "overlap", "crowd", "ignore_value")] == [None, None, "file", "last", "label", 255]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("label_of", "order", "overlap", "crowd", "ignore_value"))
    assert sig(AL.labels_np) == ["plan"]
    assert sig(AL.LabelPainter.__init__)[:3] == ["self", "plan", "device"]
    assert sig(AL.LabelPainter.paint) == ["self", "image_indices", "out"] and sig(AL.LabelPainter.paint_ragged)[:2] == ["self", "image_indices"]
    w = inspect.signature(AL.write_semantic_masks).parameters
    assert list(w)[:2] == ["ground_truth", "out_dir"]
    assert {k: w[k].default for k in ("image_ids", "route", "n_workers", "compress_level", "device")} == \
        {"image_ids": None, "route": "device", "n_workers": 16, "compress_level": 1, "device": None}
    assert all(w[k].kind is inspect.Parameter.KEYWORD_ONLY and w[k].default == p[k].default for k in ("label_of", "order", "overlap", "crowd", "ignore_value"))
    e, f = inspect.signature(evaluate.evaluate_from_annotations).parameters, inspect.signature(evaluate.evaluate_from_files).parameters
    assert list(e)[:4] == ["network", "p_images", "coco_annotations", "n_categories"]
    assert e["image_ids"].kind is inspect.Parameter.KEYWORD_ONLY and e["image_ids"].default is inspect.Parameter.empty
    shared = [k for k in f if k not in ("network", "p_images", "p_gts", "n_categories", "gt_format", "image_ids", "coco_annotations")]
    assert all(k in e and e[k].default == f[k].default for k in shared) and "p_gts" not in e and "gt_format" not in e
    assert all(k in e and e[k].default == p[k].default for k in ("label_of", "order", "overlap", "crowd", "ignore_value"))
    assert list(f) == ["network", "p_images", "p_gts", "n_categories", "gt_format", "max_size", "mean", "std", "batch_size", "n_workers", "window",
                       "instance", "image_ids", "new_label_id_to_old_label_id", "nms_type", "return_labels", "coco_annotations"]      # as it was
    assert sig(evaluate.eval_annotations_of) == ["dataset"]
    assert sig(ops.runs_label_maps)[:9] == ["run_end", "run_off", "status", "list_off", "list_mask", "list_label", "hw", "out_off", "out"]
    assert sig(polygons.runs_resident) == sig(polygons.runs_device)


def test_eval_annotations_of():
    from zutis_amd import evaluate

    class D:
        def __init__(self, name):
            self.name, self.dir_dataset, self.image_ids, self.p_annotations = name, "/d", [9, 4], "/d/annotations/instances_val2017.json"

        def get_image_path(self, i):
            return f"/d/val2017/{i:012d}.jpg"

    for name in ("coco2017", "coco20k"):
        assert evaluate.eval_annotations_of(D(name)) == (["/d/val2017/000000000009.jpg", "/d/val2017/000000000004.jpg"],
                                                         "/d/annotations/instances_val2017.json", [9, 4])
    for name in ("coca", "voc2012", "imagenet-s50", None):
        with pytest.raises(TypeError):
            evaluate.eval_annotations_of(D(name))


def test_the_module_imports_without_torch():
    code = "import sys; import zutis_amd.annotation_labels; assert 'torch' not in sys.modules, 'torch was imported'"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True).returncode == 0
