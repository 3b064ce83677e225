"""COCO mask AP without pycocotools: trainer.compute_coco_metrics (trainer.py:255-292, called at :400-405) and the tail of
coco20k_eval.py (:280-308), i.e. pycocotools' COCO.loadRes + COCOeval(iouType="segm").evaluate / accumulate / summarize, restated from
the published definition.

Where the time of COCOeval.evaluate goes — the IoU of every (detection, ground truth) pair of every (image, category) group and the
greedy matching per (group, area range, IoU threshold) — runs on the device in three launches per call (csrc/cocoeval.hip:
zh_rle_prefix, zh_rle_pair_iou, zh_coco_match) on the masks' run lengths, which is what the prediction dicts already carry: no mask is
ever rasterised.  Grouping, the score sorts, accumulate and summarize are NumPy float64 on the host (prepare / accumulate / summarize):
they touch flags and scores only.  There is no CPU path for the device part: mask_ap needs a GPU.

Polygon segmentations (what annotation files carry for everything but crowds) are converted to run counts for the whole file in one
more launch before prepare (zutis_amd/polygons.py, csrc/polygon.hip: zh_polygon_runs), with rle.from_polygons' counts exactly;
mask_ap_route(..., polygons="host") keeps the per-annotation host conversion.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib, rle

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)       # cocoeval.Params.setDetParams
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RANGES = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
AREA_LABELS = ("all", "small", "medium", "large")
CHUNK_BYTES = 64 << 20        # device bytes one chunk of groups may take (match_on_device's default)
LDS_RUNS = _lib.constants()["ZH_RLE_IOU_LDS_RUNS"]               # ground truths of up to this many runs are searched in LDS
GROUP_WORDS = 8


class Group:
    """One (image, category) — or, without categories, one (image) — of an evaluation: its detections in score order, cut to the
    largest max-det, and its ground truths.  det_mask / gt_mask index Problem.masks."""
    __slots__ = ("image_id", "k", "det_mask", "det_score", "det_id", "gt_mask", "gt_crowd", "gt_ignore", "gt_order")

    def __init__(self, image_id, k):
        self.image_id, self.k = image_id, k


class Problem:
    """What prepare() leaves: masks = [(int64 run counts, h * w)], groups in (category, image) order, K categories."""

    def __init__(self):
        self.masks: List[tuple] = []
        self.mask_names: List[str] = []
        self.groups: List[Group] = []
        self.K = 0
        self.max_dets = (1, 10, 100)


def _load(x):
    if isinstance(x, (str, bytes, os.PathLike)):
        with open(x) as f:
            return json.load(f)
    return x


def _segmentation_counts(seg, image, counts=None):
    """(run counts, h, w) of a segmentation in any form annotation files carry: compressed RLE (counts bytes / str), uncompressed RLE
    (counts a list), or a list of polygons (rasterised by rle.from_polygons at the image's size, unless the caller already holds its
    `counts`: zutis_amd/polygons.py converts a file's polygons in one launch)."""
    if isinstance(seg, dict):
        h, w = (int(v) for v in seg["size"])
        return rle.counts_np(seg["counts"]), h, w
    if image is None:
        raise ValueError("a polygon segmentation needs its image's height and width")
    h, w = int(image["height"]), int(image["width"])
    if counts is not None:
        return np.asarray(counts, dtype=np.int64), h, w
    return rle.counts_np(rle.from_polygons(seg, h, w)["counts"]), h, w


def polygon_segmentations(ground_truth, predictions, image_ids: Optional[Sequence] = None):
    """The polygon segmentations prepare() would rasterise: ([key], [(polygons, h, w)]) with key = ("annotation", j) or ("prediction",
    j), j the position in the annotations' / predictions' list — the keys of prepare's polygon_counts.  One whose image is not listed
    is left out (prepare raises for it if it is ever read)."""
    gt, preds = _load(ground_truth), _load(predictions)
    images = {im["id"]: im for im in gt["images"]}
    chosen = None if image_ids is None else set(np.asarray(list(image_ids)).tolist())
    keys, items = [], []
    for kind, rows in (("annotation", gt["annotations"]), ("prediction", preds)):
        for j, a in enumerate(rows):
            im = images.get(a["image_id"])
            if isinstance(a["segmentation"], dict) or im is None or (chosen is not None and a["image_id"] not in chosen):
                continue
            keys.append((kind, j))
            items.append((a["segmentation"], int(im["height"]), int(im["width"])))
    return keys, items


def prepare(ground_truth, predictions, *, use_categories: bool = True, max_dets: Sequence[int] = (1, 10, 100),
            image_ids: Optional[Sequence] = None, polygon_counts: Optional[Dict] = None) -> Problem:
    """COCO.loadRes + COCOeval._prepare + the per-group ordering of computeIoU / evaluateImg, on the host.

    Groups are (image, category) with use_categories, else (image) with its annotations in category order, as COCOeval gathers them.
    Detections get the ids 1, 2, ... in input order (loadRes); a group's detections are ordered by -score (stable) and cut to
    max_dets[-1]; a ground truth is ignored in an area range when it is a crowd, when its `ignore` is set, or when its `area` field lies
    outside the range; per range the ground truths are ordered ignored-last (stable).  polygon_counts: {("annotation", j) / ("prediction",
    j): run counts} of polygon segmentations converted beforehand (polygon_segmentations' keys); any other polygon goes through
    rle.from_polygons here."""
    gt, preds = _load(ground_truth), _load(predictions)
    polygon_counts = polygon_counts or {}
    max_dets = tuple(int(m) for m in max_dets)
    if len(max_dets) < 3:
        raise ValueError("max_dets: the summary reads three entries (AR at max_dets[0], [1], [2]; every AP row at max_dets[2])")
    images = {im["id"]: im for im in gt["images"]}
    for p in preds:
        if p["image_id"] not in images:
            raise ValueError(f"prediction for image {p['image_id']!r}, which the annotations do not list (loadRes refuses it too)")
    img_ids = np.unique(np.asarray(list(images) if image_ids is None else list(image_ids))).tolist()
    cat_ids = sorted(c["id"] for c in gt["categories"])
    anns_by, dets_by = {}, {}
    for j, a in enumerate(gt["annotations"]):
        anns_by.setdefault((a["image_id"], a["category_id"]), []).append(j)
    for j, p in enumerate(preds):
        dets_by.setdefault((p["image_id"], p["category_id"]), []).append(j)
    prob = Problem()
    prob.K, prob.max_dets = (len(cat_ids) if use_categories else 1), max_dets
    for k in range(prob.K):
        cats = [cat_ids[k]] if use_categories else cat_ids
        for i in img_ids:
            a_idx = [j for c in cats for j in anns_by.get((i, c), ())]
            d_idx = [j for c in cats for j in dets_by.get((i, c), ())]
            if not a_idx and not d_idx:
                continue                                                      # evaluateImg returns None
            g = Group(i, k)
            score = np.asarray([preds[j]["score"] for j in d_idx], dtype=np.float64)
            order = np.argsort(-score, kind="mergesort")[:max_dets[-1]]
            g.det_score = score[order]
            g.det_id = np.asarray([d_idx[o] + 1 for o in order], dtype=np.int64)
            g.det_mask = []
            for o in order:
                c, h, w = _segmentation_counts(preds[d_idx[o]]["segmentation"], images.get(i), polygon_counts.get(("prediction", d_idx[o])))
                g.det_mask.append(len(prob.masks))
                prob.masks.append((c, h * w))
                prob.mask_names.append(f"prediction {d_idx[o]}")
            g.gt_mask, crowd, base, area = [], [], [], []
            for j in a_idx:
                a = gt["annotations"][j]
                c, h, w = _segmentation_counts(a["segmentation"], images.get(i), polygon_counts.get(("annotation", j)))
                g.gt_mask.append(len(prob.masks))
                prob.masks.append((c, h * w))
                prob.mask_names.append(f"annotation {a.get('id', j)}")
                crowd.append(int(bool(a.get("iscrowd", 0))))
                base.append(bool(a.get("iscrowd", 0)) or bool(a.get("ignore", 0)))
                area.append(float(a["area"]) if "area" in a else float(c[1::2].sum()))
            g.gt_crowd = np.asarray(crowd, dtype=np.int32)
            area, base = np.asarray(area, dtype=np.float64), np.asarray(base, dtype=bool)
            ign = base[None, :] | (area[None, :] < AREA_RANGES[:, :1]) | (area[None, :] > AREA_RANGES[:, 1:])      # [A, G]
            g.gt_order = np.stack([np.argsort(ign[a].astype(np.uint8), kind="mergesort") for a in range(len(AREA_RANGES))]).astype(np.int32) \
                if len(a_idx) else np.zeros((len(AREA_RANGES), 0), np.int32)
            g.gt_ignore = np.take_along_axis(ign, g.gt_order.astype(np.int64), axis=1).astype(np.int32)              # in sorted order
            prob.groups.append(g)
    return prob


# ---- the device part ----------------------------------------------------------------------------------------------------------------
def _sections(parts):
    """{name: (byte offset, array)} and one uint8 host buffer holding `parts` = [(name, array)], each 16-byte aligned and at least 16
    bytes long (no section has a null address)."""
    off, lay = 0, {}
    for name, a in parts:
        lay[name] = (off, a)
        off += max(16, (a.nbytes + 15) // 16 * 16)
    buf = np.zeros(off, dtype=np.uint8)
    for name, (o, a) in lay.items():
        buf[o:o + a.nbytes] = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)
    return buf, lay


def _layout(parts):
    """The same for buffers that exist on the device only: parts = [(name, bytes)] -> (total bytes, {name: offset})."""
    off, lay = 0, {}
    for name, n in parts:
        lay[name] = off
        off += max(16, (int(n) + 15) // 16 * 16)
    return off, lay


def run_groups(masks, groups, device, *, thresholds=IOU_THRS, area_ranges=AREA_RANGES, want_iou: bool = False, ious=None,
               areas=None, events=None) -> dict:
    """One chunk on the device: ONE host-to-device copy of the counts and descriptors, zh_rle_prefix + zh_rle_pair_iou + zh_coco_match,
    ONE copy back.  masks = [(run counts, h * w)]; groups = [(det_mask, gt_mask, gt_crowd, gt_order [A, G], gt_ignore [A, G])] with mask
    indices into `masks`.  Returns {"area" int32 [n_masks], "bad" bool [n_masks] (counts that do not sum to h * w), "match" [per group:
    int32 [D, A, T]], "ignore" [per group: bool [D, A, T]]} and, with want_iou, "inter" / "iou" [per group: [D, G]].
    ious (a list of float64 [D, G], with areas = int [D] per group and masks empty): the matcher alone, fed IoU matrices directly.
    events (a list, tools/coco_ap_bench.py): gets (entry name, start, end) HIP events around each launch."""
    import torch
    from . import ops
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.ZutisHipError("COCO mask AP runs its IoU and matching kernels on the GPU (no CPU fallback)")
    thr = np.ascontiguousarray(thresholds, dtype=np.float64)
    rng = np.ascontiguousarray(area_ranges, dtype=np.float64).reshape(-1, 2)
    T, A = len(thr), len(rng)
    direct = ious is not None
    D = [len(g[0]) for g in groups]
    G = [len(g[1]) for g in groups]
    det_off = np.concatenate(([0], np.cumsum(D))).astype(np.int64)
    gt_off = np.concatenate(([0], np.cumsum(G))).astype(np.int64)
    pair_off = np.concatenate(([0], np.cumsum([d * g for d, g in zip(D, G)]))).astype(np.int64)
    n_det, n_gt, n_pairs, n_groups = int(det_off[-1]), int(gt_off[-1]), int(pair_off[-1]), len(groups)
    if direct:                                                   # every detection is a "mask" of its own that only carries an area
        masks = []
        area_in = np.concatenate([np.asarray(a, dtype=np.int32).reshape(-1) for a in areas] + [np.zeros(0, np.int32)])
        det_mask = np.arange(n_det, dtype=np.int32)
        gt_mask = np.zeros(n_gt, np.int32)
    else:
        det_mask = np.asarray([m for g in groups for m in g[0]], dtype=np.int32)
        gt_mask = np.asarray([m for g in groups for m in g[1]], dtype=np.int32)
    n_masks = len(masks)
    if n_pairs > 0x7fffffff or sum(len(c) for c, _ in masks) > 0x7fffffff:
        raise ValueError("run_groups: more than 2^31 - 1 pairs or runs in one chunk")
    for c, hw in masks:
        if hw > 0x7fffffff:
            raise ValueError("run_groups: a mask of more than 2^31 - 1 pixels")
    counts = np.concatenate([np.clip(c, -1, 0x7fffffff) for c, _ in masks] + [np.zeros(0, np.int64)]).astype(np.int32)
    run_off = np.concatenate(([0], np.cumsum([len(c) for c, _ in masks]))).astype(np.int32)
    desc = np.zeros((n_groups, GROUP_WORDS), np.int32)
    desc[:, 0], desc[:, 1], desc[:, 2], desc[:, 3], desc[:, 4] = det_off[:-1], D, gt_off[:-1], G, pair_off[:-1]
    cat = lambda k, shape: np.concatenate([np.asarray(g[k], dtype=np.int32).reshape(shape) for g in groups]
                                          + [np.zeros(tuple(max(v, 0) for v in shape), np.int32)], axis=-1)
    parts = [("thr", thr), ("rng", rng), ("counts", counts), ("run_off", run_off), ("hw", np.asarray([hw for _, hw in masks], dtype=np.int32)),
             ("groups", desc), ("det_mask", det_mask), ("gt_mask", gt_mask), ("gt_crowd", cat(2, (-1,))),
             ("gt_order", cat(3, (A, -1))), ("gt_ignore", cat(4, (A, -1)))]
    if direct:
        parts += [("iou", np.concatenate([np.asarray(m, dtype=np.float64).reshape(-1) for m in ious] + [np.zeros(0)])), ("area", area_in)]
    host, lay = _sections(parts)
    L = _lib.load(raw=True)
    ws_match = int(L.zh_coco_match_workspace_size(n_gt, T, A))
    n_status = (max(n_masks, 1) + 31) // 32
    work_bytes, wl = _layout([("iou", 8 * n_pairs), ("run_end", 4 * len(counts)), ("run_fg", 4 * len(counts)), ("inter", 4 * n_pairs),
                              ("taken", ws_match)])
    out_bytes, ol = _layout([("status", 4 * n_status), ("area", 4 * n_masks), ("match", 4 * n_det * A * T), ("ignore", n_det * A * T)])
    with torch.cuda.device(device):
        dbuf = torch.from_numpy(host).to(device, non_blocking=False)                     # the one host-to-device copy
        work = torch.empty(work_bytes, dtype=torch.uint8, device=device)
        out = torch.zeros(out_bytes, dtype=torch.uint8, device=device)                   # the status bits start clear
        base_in, base_w, base_o = dbuf.data_ptr(), work.data_ptr(), out.data_ptr()
        pin = lambda name: base_in + lay[name][0]
        s = ops._stream()

        def launch(name, *args):
            if events is None:
                return ops._call(name, *args)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops._call(name, *args)
            e1.record()
            events.append((name, e0, e1))
        if not direct and n_masks:
            launch("zh_rle_prefix", pin("counts"), pin("run_off"), pin("hw"), n_masks, base_w + wl["run_end"], base_w + wl["run_fg"],
                      base_o + ol["area"], base_o + ol["status"], s)
        if not direct and n_pairs:
            launch("zh_rle_pair_iou", base_w + wl["run_end"], base_w + wl["run_fg"], pin("run_off"), base_o + ol["area"],
                      base_o + ol["status"], pin("groups"), n_groups, pin("det_mask"), pin("gt_mask"), pin("gt_crowd"), n_pairs,
                      base_w + wl["inter"], base_w + wl["iou"], s)
        if n_det:
            launch("zh_coco_match", pin("iou") if direct else base_w + wl["iou"], pin("groups"), n_groups, pin("det_mask"),
                      pin("area") if direct else base_o + ol["area"], pin("gt_order"), pin("gt_ignore"), pin("gt_crowd"), n_gt,
                      pin("thr"), T, pin("rng"), A, base_o + ol["match"], base_o + ol["ignore"], base_w + wl["taken"], ws_match, s)
        h_out = out.cpu().numpy()                                                        # the one copy back
        res = {}
        if want_iou and not direct:
            h_work = work[:wl["run_end"]].cpu().numpy() if n_pairs else np.zeros(16, np.uint8)
            h_int = work[wl["inter"]:wl["inter"] + 4 * n_pairs].cpu().numpy().view(np.int32) if n_pairs else np.zeros(0, np.int32)
            iou = h_work[:8 * n_pairs].view(np.float64)
            res["iou"] = [iou[pair_off[i]:pair_off[i + 1]].reshape(D[i], G[i]).copy() for i in range(n_groups)]
            res["inter"] = [h_int[pair_off[i]:pair_off[i + 1]].reshape(D[i], G[i]).copy() for i in range(n_groups)]
    status = h_out[ol["status"]:ol["status"] + 4 * n_status].view(np.uint32)
    res["bad"] = ((status[np.arange(n_masks) >> 5] >> (np.arange(n_masks) & 31).astype(np.uint32)) & 1).astype(bool)
    res["area"] = h_out[ol["area"]:ol["area"] + 4 * n_masks].view(np.int32).copy()
    match = h_out[ol["match"]:ol["match"] + 4 * n_det * A * T].view(np.int32).reshape(n_det, A, T)
    ignore = h_out[ol["ignore"]:ol["ignore"] + n_det * A * T].reshape(n_det, A, T) != 0
    res["match"] = [match[det_off[i]:det_off[i + 1]].copy() for i in range(n_groups)]
    res["ignore"] = [ignore[det_off[i]:det_off[i + 1]].copy() for i in range(n_groups)]
    return res


def match_on_device(prob: Problem, device, chunk_bytes: int = CHUNK_BYTES, events=None):
    """The matches of every group of `prob`: [(match int32 [D, A, T], ignore bool [D, A, T])] in the order of prob.groups.  The groups
    go to the device in chunks of about chunk_bytes of device memory each (three launches per chunk; one chunk for a corpus that fits)."""
    A, T = len(AREA_RANGES), len(IOU_THRS)
    out, chunk, used, seen = [], [], 0, {}

    def flush():
        nonlocal chunk, used, seen
        if not chunk:
            return
        local = sorted(seen, key=seen.get)
        res = run_groups([prob.masks[m] for m in local],
                         [([seen[m] for m in g.det_mask], [seen[m] for m in g.gt_mask], g.gt_crowd, g.gt_order, g.gt_ignore) for g in chunk],
                         device, events=events)
        if res["bad"].any():
            bad = [prob.mask_names[local[j]] for j in np.flatnonzero(res["bad"])]
            raise ValueError(f"RLE counts that do not sum to height * width: {', '.join(bad[:8])}" + (" ..." if len(bad) > 8 else ""))
        out.extend(zip(res["match"], res["ignore"]))
        chunk, used, seen = [], 0, {}

    for g in prob.groups:
        need = 12 * sum(len(prob.masks[m][0]) + 4 for m in list(g.det_mask) + list(g.gt_mask)) + 12 * len(g.det_mask) * len(g.gt_mask) \
            + 5 * A * T * len(g.det_mask) + (8 * A + 8 + A * T) * len(g.gt_mask) + 4 * GROUP_WORDS
        if chunk and used + need > chunk_bytes:
            flush()
        for m in list(g.det_mask) + list(g.gt_mask):
            seen.setdefault(m, len(seen))
        chunk.append(g)
        used += need
    flush()
    return out


# ---- accumulate and summarize (host, float64) ---------------------------------------------------------------------------------------
def accumulate(prob: Problem, matches):
    """COCOeval.accumulate: (precision float64 [T, R, K, A, M], recall float64 [T, K, A, M]), -1 where a cell has no ground truth that
    counts.  matches = [(match [D, A, T] with -1 for none, ignore [D, A, T])] per group of prob."""
    T, R, A, M, K = len(IOU_THRS), len(REC_THRS), len(AREA_RANGES), len(prob.max_dets), prob.K
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    by_k = [[] for _ in range(K)]
    for g, (mt, ig) in zip(prob.groups, matches):
        by_k[g.k].append((g, np.asarray(mt), np.asarray(ig)))
    for k in range(K):
        E = by_k[k]
        if not E:
            continue
        for a in range(A):
            npig = int(sum(np.count_nonzero(g.gt_ignore[a] == 0) for g, _, _ in E))
            if npig == 0:
                continue
            for m, max_det in enumerate(prob.max_dets):
                scores = np.concatenate([g.det_score[:max_det] for g, _, _ in E])
                inds = np.argsort(-scores, kind="mergesort")
                dtm = np.concatenate([mt[:max_det, a, :].T for _, mt, _ in E], axis=1)[:, inds]           # [T, nd]
                dtig = np.concatenate([ig[:max_det, a, :].T for _, _, ig in E], axis=1)[:, inds]
                tps = np.logical_and(dtm >= 0, np.logical_not(dtig))
                fps = np.logical_and(dtm < 0, np.logical_not(dtig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    if nd:
                        pr = np.maximum.accumulate(pr[::-1])[::-1]                                         # monotone from the right
                        at = np.searchsorted(rc, REC_THRS, side="left")
                        ok = at < nd
                        q[ok] = pr[at[ok]]
                    precision[t, :, k, a, m] = q
    return precision, recall


def summarize(precision, recall, max_dets=(1, 10, 100)) -> np.ndarray:
    """COCOeval.summarize's twelve numbers (_summarizeDets): the mean of the entries above -1 of a slice, -1 when there are none."""
    max_dets = list(max_dets)

    def one(ap, iou_thr=None, area="all", max_det=100):
        a, m = AREA_LABELS.index(area), [i for i, v in enumerate(max_dets) if v == max_det]
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))

    md = max_dets[2]
    return np.array([one(1, max_det=md), one(1, .5, max_det=md), one(1, .75, max_det=md), one(1, area="small", max_det=md),
                     one(1, area="medium", max_det=md), one(1, area="large", max_det=md), one(0, max_det=max_dets[0]),
                     one(0, max_det=max_dets[1]), one(0, max_det=md), one(0, area="small", max_det=md), one(0, area="medium", max_det=md),
                     one(0, area="large", max_det=md)], dtype=np.float64)


def metric_names(max_dets=(1, 10, 100)):
    """The keys of trainer.compute_coco_metrics' dict (trainer.py:278-291), in the order of `stats`."""
    return ["AP", "AP_50", "AP_75", "AP_small", "AP_medium", "AP_large", f"AR_{max_dets[0]}", f"AR_{max_dets[1]}", f"AR_{max_dets[2]}",
            "AR_small", "AR_medium", "AR_large"]


def result_dict(precision, recall, max_dets) -> dict:
    stats = summarize(precision, recall, max_dets)
    out = {name: float(v) for name, v in zip(metric_names(max_dets), stats)}
    out.update(stats=stats, precision=precision, recall=recall)
    return out


def mask_ap(ground_truth, predictions, *, use_categories: bool = True, max_dets: Sequence[int] = (1, 10, 100),
            image_ids: Optional[Sequence] = None, device=None) -> dict:
    """COCO-style mask AP of instance predictions: COCOeval(cocoGt, cocoGt.loadRes(predictions), iouType="segm") with params.useCats =
    use_categories, params.maxDets = max_dets and, when image_ids is given, params.imgIds = image_ids (coco20k_eval.py:282), then
    evaluate / accumulate / summarize.

    ground_truth: a COCO annotation dict (images, annotations, categories) or the path of its JSON; an annotation's segmentation may be
    a compressed RLE, an uncompressed RLE or a list of polygons (converted on the device: mask_ap_route).  predictions: the dicts
    predict(mask_type="instance") / predict_from_files produce, or the path of the JSON trainer.py:393-398 dumps (image_id, category_id, score, segmentation
    {"size", "counts" bytes or str}; anything else, bbox included, is not read).  device: the GPU to run on (None: the current one).
    Returns the twelve entries of trainer.compute_coco_metrics under its key names, "stats" float64 [12], "precision" float64
    [T = 10, R = 101, K, A = 4, M] and "recall" float64 [T, K, A, M] (K categories, or 1 without; M = len(max_dets))."""
    return mask_ap_route(ground_truth, predictions, polygons="device", use_categories=use_categories, max_dets=max_dets,
                         image_ids=image_ids, device=device)


def mask_ap_route(ground_truth, predictions, *, polygons: str = "device", use_categories: bool = True,
                  max_dets: Sequence[int] = (1, 10, 100), image_ids: Optional[Sequence] = None, device=None, timings=None) -> dict:
    """mask_ap with the route of its polygon segmentations spelled out.  polygons="device" (what mask_ap takes): every polygon
    segmentation of the annotations, and of the predictions should any carry one, is converted to run counts in ONE
    polygons.runs_device call on `device` and handed to prepare; polygons="host": prepare rasterises each with rle.from_polygons.  The
    two return the same dict, bit for bit.  timings (a dict, tools/coco_ap_bench.py): gets "polygon_s", the polygon stage's
    "stats" and its launch's HIP "events"."""
    import time
    import torch
    if polygons not in ("device", "host"):
        raise ValueError(f"polygons = {polygons!r}: \"device\" or \"host\"")
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.ZutisHipError("mask_ap runs its IoU and matching kernels on the GPU (no CPU fallback)")
        device = torch.device("cuda", torch.cuda.current_device())
    gt, preds = _load(ground_truth), _load(predictions)
    t0 = time.perf_counter()
    keys, items = polygon_segmentations(gt, preds, image_ids)
    if polygons == "device" and items:
        from . import polygons as _polygons
        events = [] if timings is not None else None
        counts, stats = _polygons.runs_device(items, device, events=events)
        polygon_counts = dict(zip(keys, counts))
    else:                                                    # the host route converts here what prepare would, to be timed alike
        stats, events = {"annotations": len(items), "polygons": None, "host_fallback": len(items)}, []
        polygon_counts = {k: rle.counts_np(rle.from_polygons(*it)["counts"]) for k, it in zip(keys, items)} if timings is not None else None
    if timings is not None:
        timings.update(polygon_s=time.perf_counter() - t0, stats=stats, events=events)
    prob = prepare(gt, preds, use_categories=use_categories, max_dets=max_dets, image_ids=image_ids, polygon_counts=polygon_counts)
    precision, recall = accumulate(prob, match_on_device(prob, device))
    return result_dict(precision, recall, prob.max_dets)


def compute_coco_metrics(self, p_annotations, instance_predictions, use_categories: bool = True,
                         n_max_detections=(1, 10, 100)) -> Dict[str, float]:
    """Trainer.compute_coco_metrics (trainer.py:255-292) over mask_ap, to bind in its place:
        Trainer.compute_coco_metrics = zutis_amd.coco_eval.compute_coco_metrics
    The list may have lost its bbox entries (trainer.py:393)."""
    device = getattr(self, "device", None)
    res = mask_ap(p_annotations, instance_predictions, use_categories=use_categories, max_dets=tuple(n_max_detections),
                  device=device if device is not None and str(device) != "cpu" else None)
    return {name: res[name] for name in metric_names(tuple(n_max_detections))}
