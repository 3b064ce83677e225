"""-m gpu: the COCO mask AP kernels (csrc/cocoeval.hip: zh_rle_prefix, zh_rle_pair_iou, zh_coco_match) and zutis_amd/coco_eval.mask_ap
against the dense-mask float64 reference of tests/_cocoeval_ref.py, for EQUALITY: integers equal, float64 IoUs bit-equal, match indices
and flags equal, stats / precision / recall equal.  Shapes are the smallest at which each kernel can go wrong."""
import numpy as np
import pytest

from tests import _cocoeval_case as CC
from tests import _cocoeval_ref as R
from tests.test_evaluate_gpu import MEAN, N_CAT, STD, _labels, _photo, net  # noqa: F401  (net: the TINY drop-in ZUTIS fixture)
from zutis_amd import coco_eval, rle

pytestmark = pytest.mark.gpu

A, T = 4, 10
LIMIT = coco_eval.LDS_RUNS


def counts_of(flat):
    return rle._counts(np.asarray(flat, np.uint8).reshape(-1, 1))


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def group(dets, gts, crowd):
    """run_groups' group with the ground truths walked in their own order, the crowds ignored."""
    c = np.asarray(crowd, np.int32)
    order = np.argsort(c, kind="mergesort").astype(np.int32)
    return (list(dets), list(gts), c, np.tile(order, (A, 1)), np.tile(c[order], (A, 1)))


def check_against_reference(masks, groups, res):
    """masks: flat bool arrays; every group's inter / iou / match / ignore against the reference on the pixels."""
    for gi, (dets, gts, crowd, _, _) in enumerate(groups):
        inter, iou = R.pair_iou([masks[m] for m in dets], [masks[m] for m in gts], crowd)
        assert res["inter"][gi].dtype == np.int32 and np.array_equal(res["inter"][gi], inter), gi
        assert res["iou"][gi].dtype == np.float64 and bits_equal(res["iou"][gi], iou), gi
        for a in range(A):
            m, ig, _ = R.match_group(iou, crowd, crowd, [int(masks[d].sum()) for d in dets], R.AREA_RANGES[a])
            assert np.array_equal(res["match"][gi][:, a, :], m.T) and np.array_equal(res["ignore"][gi][:, a, :], ig.T), (gi, a)


@pytest.mark.parametrize("h,w", [(7, 5), (37, 53), (64, 64)])
def test_prefix_and_iou_kernels_on_edge_masks(dev, h, w):
    hw = h * w
    rng = np.random.default_rng(hw)
    empty, full = np.zeros(hw, bool), np.ones(hw, bool)
    starts_fg = rng.random(hw) > 0.5
    starts_fg[0] = True
    pixels = (np.arange(hw) & 1) == 0                                    # single-pixel runs throughout, foreground first: hw + 1 runs
    stripes = (np.arange(hw) // 3) % 2 == 1                              # ground truth of short runs ...
    span = np.zeros(hw, bool)
    span[hw // 5: hw - hw // 4] = True                                   # ... under ONE detection run that spans many of them
    rand = [rng.random(hw) > p for p in (0.3, 0.6, 0.9)]
    masks = [empty, full, starts_fg, pixels, stripes, span] + rand
    assert len(counts_of(empty)) == 1 and counts_of(full).tolist() == [0, hw] and counts_of(starts_fg)[0] == 0
    assert len(counts_of(pixels)) == hw + 1 and len(counts_of(span)) == 3
    n = len(masks)
    every = list(range(n))
    groups = [group(every, every, [i % 3 == 1 for i in every]),          # every pair, mixed crowd flags (the empty-vs-empty pair too)
              group([5], [4], [0]), group([5], [4], [1])]
    res = coco_eval.run_groups([(counts_of(m), hw) for m in masks], groups, dev, want_iou=True)
    assert not res["bad"].any() and res["area"].tolist() == [int(m.sum()) for m in masks]
    check_against_reference(masks, groups, res)
    assert res["inter"][1][0, 0] == int((span & stripes).sum()) > 0 and res["iou"][0][0, 0] == 0.0


def test_ground_truths_around_the_lds_staging_limit(dev):
    """A ground truth with LIMIT - 1, LIMIT and LIMIT + 1 runs (single-pixel runs, then the rest in one) on 37 x 53 = 1961 pixels."""
    hw = 37 * 53
    rng = np.random.default_rng(1)
    masks = []
    for n_runs in (LIMIT - 1, LIMIT, LIMIT + 1):
        m = np.zeros(hw, bool)
        m[:n_runs - 1] = (np.arange(n_runs - 1) & 1) == 1
        m[n_runs - 1:] = (n_runs - 1) & 1
        assert len(counts_of(m)) == n_runs
        masks.append(m)
    masks += [rng.random(hw) > 0.5, np.ones(hw, bool)]
    groups = [group([3, 4, 0, 1, 2], [0, 1, 2], [0, 1, 0])]
    res = coco_eval.run_groups([(counts_of(m), hw) for m in masks], groups, dev, want_iou=True)
    assert not res["bad"].any()
    check_against_reference(masks, groups, res)


def test_groups_of_every_shape_two_image_sizes_and_a_malformed_mask_in_one_call(dev):
    rng = np.random.default_rng(2)
    small, big = 7 * 5, 37 * 53
    masks = [rng.random(big) > rng.random() for _ in range(115)] + [rng.random(small) > 0.5 for _ in range(8)]
    hws = [big] * 115 + [small] * 8
    groups = [group([115], [116], [0]),                                            # 1 x 1, the small image
              group(range(0, 100), range(100, 115), [i % 4 == 0 for i in range(15)]),   # 100 x 15, the large image, mixed crowds
              group([], [117, 118, 119], [0, 1, 0]),                               # 0 x 3
              group([120, 121, 122], [], []),                                      # 3 x 0
              group([116, 117], [115, 122], [1, 0])]
    packed = [(counts_of(m), hw) for m, hw in zip(masks, hws)]
    good = coco_eval.run_groups(packed, groups, dev, want_iou=True)
    assert not good["bad"].any() and good["area"].tolist() == [int(m.sum()) for m in masks]
    assert good["iou"][2].shape == (0, 3) and good["iou"][3].shape == (3, 0) and good["match"][2].shape == (0, A, T)
    assert np.all(good["match"][3] == -1)
    check_against_reference(masks, groups, good)
    # mask 121 loses its last run: its counts no longer sum to h * w.  Its bit is set, its pairs are flagged, everything else is as before.
    broken = list(packed)
    broken[121] = (packed[121][0][:-1], small)
    broken[116] = (np.concatenate((packed[116][0], [3])), small)                    # one run too many: past the end
    res = coco_eval.run_groups(broken, groups, dev, want_iou=True)
    assert np.flatnonzero(res["bad"]).tolist() == [116, 121]
    assert np.array_equal(np.delete(res["area"], [116, 121]), np.delete(good["area"], [116, 121]))
    assert np.all(res["inter"][0] == -1) and np.all(res["iou"][0] == -1.0) and np.all(res["inter"][4][0] == -1)
    assert np.array_equal(res["inter"][4][1], good["inter"][4][1]) and bits_equal(res["iou"][1], good["iou"][1])
    assert np.array_equal(res["match"][1], good["match"][1]) and np.array_equal(res["ignore"][1], good["ignore"][1])
    with pytest.raises(ValueError, match="prediction 0"):
        ann, preds = CC.to_coco({1: (7, 5)}, [1], [CC.gt(1, 1, masks[115].reshape(7, 5))], [CC.det(1, 1, .5, masks[116].reshape(7, 5))])
        preds[0]["segmentation"] = {"size": [7, 5], "counts": [1, 2, 3]}
        coco_eval.mask_ap(ann, preds, device=dev)


def direct(dev, cases):
    """zh_coco_match alone on IoU matrices: cases = [(iou [D, G], crowd [G], gt_ignore [G], det_area [D])] -> per case (match, ignore)."""
    groups, ious, areas = [], [], []
    for iou, crowd, ign, area in cases:
        iou = np.asarray(iou, np.float64).reshape(len(area), len(ign))
        ign = np.asarray(ign, np.int32)
        order = np.argsort(ign, kind="mergesort").astype(np.int32)
        groups.append((list(range(iou.shape[0])), list(range(iou.shape[1])), np.asarray(crowd, np.int32), np.tile(order, (A, 1)),
                       np.tile(ign[order], (A, 1))))
        ious.append(iou), areas.append(area)
    res = coco_eval.run_groups([], groups, dev, ious=ious, areas=areas)
    for (iou, crowd, ign, area), m, ig in zip(cases, res["match"], res["ignore"]):
        iou = np.asarray(iou, np.float64).reshape(len(area), len(ign))
        for a in range(A):
            rm, rig, _ = R.match_group(iou, ign, crowd, area, R.AREA_RANGES[a])
            assert np.array_equal(m[:, a, :], rm.T) and np.array_equal(ig[:, a, :], rig.T), a
    return list(zip(res["match"], res["ignore"]))


def test_match_kernel_rules_thresholds_crowds_and_empty_groups(dev):
    rng = np.random.default_rng(4)
    names = sorted(CC.RULES)
    cases = [(CC.RULES[n]["iou"], CC.RULES[n]["crowd"], CC.RULES[n]["gt_ignore"], CC.DET_AREA) for n in names]
    half = [[1 / 2, 0.0], [0.0, 11 / 20]]                                        # exactly on a threshold: >= matches
    cases.append((half, [0, 0], [0, 0], (50, 2000)))
    cases.append(([[0.8], [0.7], [0.6], [0.2]], [1], [1], (10, 2000, 20000, 5)))  # a crowd matched by three detections
    cases.append((np.zeros((0, 3)), [0, 1, 0], [0, 1, 0], ()))                   # D = 0
    cases.append((np.zeros((3, 0)), [], [], (10, 2000, 20000)))                  # G = 0: ignored by their own area only
    crowd = rng.random(9) < 0.3
    cases.append((np.round(rng.random((100, 9)), 1), crowd, crowd | (rng.random(9) < 0.3), rng.integers(1, 20000, 100)))   # ties galore
    out = direct(dev, cases)
    for n, (m, ig) in zip(names, out):                                           # the hand-derived expectations, ranges all / small / medium
        for t, (em, eig) in CC.RULES[n]["expect"].items():
            for a in range(3):
                assert m[:, a, t].tolist() == em and ig[:, a, t].astype(int).tolist() == eig, (n, a, t)
            assert m[:, 3, t].tolist() == em and ig[:, 3, t].astype(int).tolist() == [e if k >= 0 else 1 for k, e in zip(em, eig)]
    m, ig = out[3]
    thr = np.linspace(.5, .95, 10)
    assert m[0, 0, :].tolist() == [0] + [-1] * 9 and m[1, 0, :].tolist() == [1, 1 if 11 / 20 >= thr[1] else -1] + [-1] * 8
    m, ig = out[4]
    assert m[:, 0, 0].tolist() == [0, 0, 0, -1] and ig[:, 0, 0].tolist() == [True, True, True, False] and m[:, 0, 5].tolist() == [0, -1, -1, -1]
    assert out[5][0].shape == (0, A, T) and np.all(out[6][0] == -1)
    assert out[6][1][:, :, 0].astype(int).tolist() == [[0, 0, 1, 1], [0, 1, 0, 1], [0, 1, 1, 0]]


@pytest.mark.parametrize("max_dets", [(1, 10, 100), (1, 5, 7)])
def test_120_detections_are_cut_to_the_largest_max_det(dev, max_dets):
    h, w = 16, 24
    rng = np.random.default_rng(6)
    gts = [CC.gt(1, 1, CC.box(h, w, 2 * j, 3 * j, 2 * j + 6, 3 * j + 8)) for j in range(4)]
    dets = [CC.det(1, 1, float(np.round(rng.random(), 1)), np.roll(gts[j % 4]["mask"], int(rng.integers(-2, 3)), 1) & (rng.random((h, w)) > 0.2))
            for j in range(120)]
    ann, preds = CC.to_coco({1: (h, w)}, [1], gts, dets)
    prob = coco_eval.prepare(ann, preds, max_dets=max_dets)
    assert len(prob.groups[0].det_mask) == max_dets[-1]
    got, ref = coco_eval.mask_ap(ann, preds, max_dets=max_dets, device=dev), R.mask_ap([1], [1], gts, dets, max_dets=max_dets)
    for key in ("stats", "precision", "recall"):
        assert np.array_equal(got[key], ref[key]), key
    assert f"AR_{max_dets[2]}" in got and 0 < got["AP"] < 1


@pytest.mark.parametrize("use_categories", [True, False])
def test_mask_ap_end_to_end_equals_the_reference(dev, use_categories):
    sizes, cats, gts, dets = CC.synthetic_corpus()
    assert len(sizes) == 6 and len(cats) == 3
    ann, preds = CC.to_coco(sizes, cats, gts, dets)
    got = coco_eval.mask_ap(ann, preds, use_categories=use_categories, device=dev)
    ref = R.mask_ap(list(sizes), cats, gts, dets, use_categories=use_categories)
    for key in ("stats", "precision", "recall"):
        assert got[key].dtype == np.float64 and np.array_equal(got[key], ref[key]), key
    assert got["AP_small"] > -1 and got["AP_medium"] > -1 and got["AP_large"] == -1.0
    assert [got[n] for n in coco_eval.metric_names()] == [ref[n] for n in coco_eval.metric_names()]
    # group by group, and the same from several small chunks as from one
    prob = coco_eval.prepare(ann, preds, use_categories=use_categories)
    one, many = coco_eval.match_on_device(prob, dev), coco_eval.match_on_device(prob, dev, chunk_bytes=4096)
    assert len(one) == len(many) == len(ref["groups"]) == len(prob.groups)
    for g, (m, ig), (m2, ig2), rg in zip(prob.groups, one, many, ref["groups"]):
        assert (g.k, g.image_id) == (rg["k"], rg["image_id"])
        assert np.array_equal(m.transpose(1, 2, 0), rg["match"]) and np.array_equal(ig.transpose(1, 2, 0), rg["ignore"])
        assert np.array_equal(m, m2) and np.array_equal(ig, ig2)


def test_evaluate_from_files_returns_coco_metrics(dev, net, tmp_path):  # noqa: F811
    from PIL import Image
    from zutis_amd import evaluate
    hw = [(64, 96), (80, 64), (64, 96), (48, 80)]
    images, gt_files, ids = [], [], [1000 + 7 * i for i in range(4)]
    for i, (h, w) in enumerate(hw):
        images.append(str(tmp_path / f"im{i}.png"))
        _photo(h, w, 900 + i).save(images[-1], compress_level=1)
        gt_files.append(str(tmp_path / f"gt{i}.png"))
        Image.fromarray(_labels(h, w, 300 + i, 255).astype(np.uint8), "L").save(gt_files[-1])
    kw = dict(max_size=None, mean=MEAN, std=STD, batch_size=4, n_workers=4, instance=True, image_ids=ids, nms_type="hard")
    plain = evaluate.evaluate_from_files(net, images, gt_files, N_CAT, **kw)
    assert sorted(plain) == ["cls_iu", "confusion_matrix", "instance_predictions", "labels", "scores"]        # today's keys, exactly
    # annotations: a few boxes, and every second mask the (random-weight) network predicts, eroded by a column — so that something matches
    rng = np.random.default_rng(8)
    gts = [CC.gt(ids[i], int(rng.integers(0, N_CAT)), CC.box(h, w, 8 * j, 8 * j, 8 * j + int(rng.integers(8, 40)), 8 * j + int(rng.integers(8, 40))))
           for i, (h, w) in enumerate(hw) for j in range(3)]
    for p in plain["instance_predictions"][::2]:
        m = rle.decode(p["segmentation"]).astype(bool)
        m[:, ::7] = False
        gts.append(CC.gt(p["image_id"], int(p["category_id"]), m))
    ann, _ = CC.to_coco({ids[i]: s for i, s in enumerate(hw)}, list(range(N_CAT)), gts, [])
    got = evaluate.evaluate_from_files(net, images, gt_files, N_CAT, coco_annotations=ann, **kw)
    assert sorted(got) == sorted(list(plain) + ["coco_metrics"]) and len(got["instance_predictions"]) > 0
    assert np.array_equal(got["confusion_matrix"], plain["confusion_matrix"])
    assert "coco_metrics" not in evaluate.evaluate_from_files(net, images, gt_files, N_CAT, coco_annotations=ann, **dict(kw, instance=False))
    own = coco_eval.mask_ap(ann, got["instance_predictions"], image_ids=ids, device=dev)
    dets = [CC.det(p["image_id"], int(p["category_id"]), p["score"], rle.decode(p["segmentation"]).astype(bool)) for p in got["instance_predictions"]]
    ref = R.mask_ap(ids, list(range(N_CAT)), gts, dets, image_ids=ids)
    assert sorted(got["coco_metrics"]) == sorted(own)
    for key in ("stats", "precision", "recall"):
        assert np.array_equal(got["coco_metrics"][key], own[key]) and np.array_equal(own[key], ref[key]), key
    assert got["coco_metrics"]["AP"] > 0
    print("coco_metrics of the TINY network on 4 files:", {k: v for k, v in got["coco_metrics"].items() if isinstance(v, float)})
