"""Shared inputs of tests/test_coco_eval_cpu.py and tests/test_coco_eval_gpu.py: dense-mask corpora in the two forms the tests need (the
lists tests/_cocoeval_ref.py reads, and the COCO annotation dict + prediction dicts zutis_amd/coco_eval.py reads), the three matching
rules on IoU matrices written out by hand, and a NumPy stand-in for the device part built from the reference's own functions."""
import numpy as np

from tests import _cocoeval_ref as R
from zutis_amd import rle

A, T = 4, 10


def to_coco(sizes, categories, gts, dets, counts_form="bytes"):
    """(annotation dict, prediction dicts) of the reference's lists.  sizes = {image id: (h, w)}."""
    def seg(mask):
        e = rle.encode_py(mask)
        if counts_form == "str":
            e["counts"] = e["counts"].decode("ascii")
        elif counts_form == "list":
            e["counts"] = rle._counts(mask).tolist()
        return e
    ann = {"images": [{"id": i, "height": h, "width": w} for i, (h, w) in sizes.items()],
           "categories": [{"id": c, "name": f"c{c}"} for c in categories],
           "annotations": [{"id": j + 1, "image_id": g["image_id"], "category_id": g["category_id"], "segmentation": seg(g["mask"]),
                            "area": g["area"], "iscrowd": int(g.get("iscrowd", 0)), **({"ignore": 1} if g.get("ignore") else {})}
                           for j, g in enumerate(gts)]}
    preds = [{"image_id": d["image_id"], "category_id": d["category_id"], "score": d["score"], "segmentation": seg(d["mask"]),
              "bbox": [0.0, 0.0, 1.0, 1.0], "image_size": list(d["mask"].shape)} for d in dets]
    return ann, preds


def box(h, w, y0, x0, y1, x1):
    m = np.zeros((h, w), bool)
    m[y0:y1, x0:x1] = True
    return m


def gt(image_id, category_id, mask, **kw):
    return {"image_id": image_id, "category_id": category_id, "mask": mask, "area": float(mask.sum()), **kw}


def det(image_id, category_id, score, mask):
    return {"image_id": image_id, "category_id": category_id, "score": score, "mask": mask}


def synthetic_corpus(seed=0, n_images=6, n_categories=3, max_det=12, h=48, w=64):
    """Jittered copies of the ground truth plus noise masks: small (< 32^2) and medium objects, no large one (48 x 64 < 96^2); one crowd."""
    rng = np.random.default_rng(seed)
    sizes = {10 + 3 * i: (h, w) for i in range(n_images)}
    gts, dets = [], []
    for n, i in enumerate(sizes):
        for j in range(int(rng.integers(1, 5))):
            bh, bw = (int(rng.integers(34, 44)), int(rng.integers(34, 56))) if j == 0 else (int(rng.integers(3, 20)), int(rng.integers(3, 24)))
            y0, x0 = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
            m = box(h, w, y0, x0, y0 + bh, x0 + bw) & (rng.random((h, w)) > 0.05)
            c = int(rng.integers(1, n_categories + 1))
            gts.append(gt(i, c, m, iscrowd=int(n == 1 and j == 1)))
            for _ in range(int(rng.integers(0, 3))):                                   # jittered copies, sometimes of another category
                dy, dx = (int(v) for v in rng.integers(-3, 4, 2))
                dm = np.roll(np.roll(m, dy, 0), dx, 1) & (rng.random((h, w)) > 0.1)
                dets.append(det(i, c if rng.random() < 0.8 else 1 + c % n_categories, float(np.round(rng.random(), 2)), dm))
        for _ in range(int(rng.integers(1, 4))):                                       # noise
            dets.append(det(i, int(rng.integers(1, n_categories + 1)), float(np.round(rng.random(), 2)), rng.random((h, w)) > 0.7))
        mine = [d for d in dets if d["image_id"] == i]
        assert 0 < len(mine) <= max_det
    return sizes, list(range(1, n_categories + 1)), gts, dets


# ---- the three matching rules, each on a 2 x 3 IoU matrix (2 detections in score order, 3 ground truths); detections of 32^2 pixels: inside 'all', 'small', 'medium' ----
# expected: {threshold index: (match [2], ignore [2])}; thresholds are 0.5, 0.55, ..., 0.95 (index 0 .. 9)
RULES = {
    # ground truth 1 is a crowd (so ignored, so walked last).  Both detections overlap only the crowd: a crowd may be matched again, so
    # both match it and both are ignored; above its IoU a detection is an unmatched, counted false positive.
    "crowd": dict(iou=[[0.0, 0.82, 0.0], [0.0, 0.72, 0.0]], crowd=[0, 1, 0], gt_ignore=[0, 1, 0],
                  expect={0: ([1, 1], [1, 1]), 4: ([1, 1], [1, 1]), 5: ([1, -1], [1, 0]), 6: ([1, -1], [1, 0]), 7: ([-1, -1], [0, 0])}),
    # ground truths 0 and 2 are ignored (not crowds): walk order 1, 0, 2.  At 0.5 detection 0 takes 1 (IoU 0.6) and the walk stops at the
    # first ignored one although both overlap more; detection 1 finds 1 taken, takes 0 (0.9), then 2 (0.95 >= 0.9): ignored.  At 0.65
    # detection 0 cannot take 1, takes 0 then 2; detection 1 finds 2 taken and keeps 0.
    "ignore_break": dict(iou=[[0.9, 0.6, 0.95], [0.9, 0.6, 0.95]], crowd=[0, 0, 0], gt_ignore=[1, 0, 1],
                         expect={0: ([1, 2], [0, 1]), 1: ([1, 2], [0, 1]), 3: ([2, 0], [1, 1]), 9: ([2, -1], [1, 0])}),
    # equal IoUs: the later ground truth of the walk wins, the next detection gets the earlier one
    "later_equal": dict(iou=[[0.6, 0.6, 0.1], [0.6, 0.6, 0.1]], crowd=[0, 0, 0], gt_ignore=[0, 0, 0],
                        expect={0: ([1, 0], [0, 0]), 1: ([1, 0], [0, 0]), 3: ([-1, -1], [0, 0])}),
}


DET_AREA = (1024, 1024)


def rule_group(case):
    """A RULES entry as run_groups' direct-mode group: (dets, gts, crowd, order [A, G], ignore-in-walk-order [A, G]), the same in all A."""
    ign = np.asarray(case["gt_ignore"])
    order = np.argsort(ign, kind="mergesort")
    return (list(range(len(case["iou"]))), list(range(len(ign))), np.asarray(case["crowd"], np.int32),
            np.tile(order.astype(np.int32), (A, 1)), np.tile(ign[order].astype(np.int32), (A, 1)))


def numpy_matches(prob):
    """match_on_device's result from the reference's functions on the masks' pixels (flat, column-major): the host layers of
    zutis_amd/coco_eval.py can then run, and be checked, without a GPU."""
    out = []
    flat = lambda m: np.repeat((np.arange(len(prob.masks[m][0])) & 1).astype(bool), prob.masks[m][0])
    for g in prob.groups:
        dm, gm = [flat(m) for m in g.det_mask], [flat(m) for m in g.gt_mask]
        _, iou = R.pair_iou(dm, gm, g.gt_crowd)
        D, G = len(dm), len(gm)
        match, ignore = np.zeros((D, A, T), np.int32), np.zeros((D, A, T), bool)
        for a in range(A):
            ign = np.zeros(G, bool)
            ign[g.gt_order[a]] = g.gt_ignore[a] != 0
            m, ig, _ = R.match_group(iou, ign, g.gt_crowd, [int(x.sum()) for x in dm], R.AREA_RANGES[a])
            match[:, a, :], ignore[:, a, :] = m.T, ig.T
        out.append((match, ignore))
    return out
