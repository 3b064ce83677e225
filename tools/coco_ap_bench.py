"""COCO mask AP as its caller gets it — annotation dict + prediction dicts in, the twelve numbers out — on a seeded synthetic corpus
(default: 500 images at 480 x 640, 100 detections and up to 15 ground truths each, 80 categories): zutis_amd.coco_eval.mask_ap end to
end (arm D), its three kernels alone by HIP events, and the dense-mask NumPy reference of tests/_cocoeval_ref.py on the same corpus
(arm R: the only other implementation available without pycocotools), alternated in one process, medians and spreads over the rounds.
The two arms' stats are compared for equality.

    python tools/coco_ap_bench.py [--images N] [--rounds R] [--arm D|R ...] [--chunk-mb M ...] [--out profiles/coco_ap_ab.json]

--gt polygons: the ground truth as annotation files carry it — seeded star-shaped polygons (8 - 80 vertices, radius 10 - 120 px, 1 - 3
per annotation, 1 - 15 annotations per image, default 400 images) — and mask_ap's two routes for them, polygons="host"
(rle.from_polygons per annotation: the parent's only route) and polygons="device" (zh_polygon_runs for the whole file), alternated in
one process: mask_ap end to end, the polygon stage alone, the kernel by HIP events, the annotations left to the host.

    python tools/coco_ap_bench.py --gt polygons [--images N] [--rounds R] [--out profiles/coco_polygon_ab.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _cocoeval_ref as R  # noqa: E402
from zutis_amd import coco_eval, rle  # noqa: E402

H, W, N_CAT, N_DET, MAX_GT = 480, 640, 80, 100, 15


def blob_counts(rng, cy, cx, ry, rx):
    """Run counts of a ragged ellipse: one column interval per column, jittered by a pixel or two (the run statistics of a real mask)."""
    xs = np.arange(max(0, int(cx - rx)), min(W, int(cx + rx) + 1))
    half = ry * np.sqrt(np.clip(1 - ((xs - cx) / max(rx, 1)) ** 2, 0, 1)) + rng.integers(-2, 3, xs.size)
    top = np.clip(np.round(cy - half), 0, H).astype(np.int64)
    bot = np.clip(np.round(cy + half), 0, H).astype(np.int64)
    keep = bot > top
    edges = np.stack([xs[keep] * H + top[keep], xs[keep] * H + bot[keep]], axis=1).reshape(-1)
    if edges.size > 2:                                          # a column filled to the bottom runs on into the next one's top
        same = np.flatnonzero(edges[1:-1:2] == edges[2::2]) * 2 + 1
        edges = np.delete(edges, np.concatenate((same, same + 1)))
    return np.diff(np.concatenate(([0], edges, [H * W])))


def corpus(n_images, seed=0):
    rng = np.random.default_rng(seed)
    import ctypes
    from zutis_amd import _lib
    lib, buf = _lib.load(raw=True), ctypes.create_string_buffer(1 << 16)

    def seg(c):                                                  # the C host helper: rle._to_string is a Python loop per character
        c = np.ascontiguousarray(c, dtype=np.int64)
        n = lib.zh_rle_counts_to_string_host(c.ctypes.data, c.size, ctypes.addressof(buf), len(buf))
        assert n >= 0
        return {"size": [H, W], "counts": buf.raw[:n]}
    ann = {"images": [{"id": i + 1, "height": H, "width": W} for i in range(n_images)],
           "categories": [{"id": c + 1, "name": f"c{c}"} for c in range(N_CAT)], "annotations": []}
    preds = []
    for i in range(n_images):
        shapes = []
        for _ in range(int(rng.integers(1, MAX_GT + 1))):
            ry, rx = (rng.integers(4, 20, 2) if rng.random() < 0.4 else rng.integers(20, 160, 2))
            s = (int(rng.integers(0, H)), int(rng.integers(0, W)), int(ry), int(rx), int(rng.integers(1, N_CAT + 1)))
            shapes.append(s)
            c = blob_counts(rng, *s[:4])
            ann["annotations"].append({"id": len(ann["annotations"]) + 1, "image_id": i + 1, "category_id": s[4], "segmentation": seg(c),
                                       "area": float(c[1::2].sum()), "iscrowd": int(rng.random() < 0.05)})
        for _ in range(N_DET):
            if rng.random() < 0.6:                               # a jittered copy of a ground truth, mostly of its category
                cy, cx, ry, rx, cat = shapes[int(rng.integers(0, len(shapes)))]
                cy, cx, ry, rx = cy + int(rng.integers(-6, 7)), cx + int(rng.integers(-6, 7)), max(2, ry + int(rng.integers(-4, 5))), max(2, rx + int(rng.integers(-4, 5)))
                cat = cat if rng.random() < 0.9 else int(rng.integers(1, N_CAT + 1))
            else:
                cy, cx, ry, rx, cat = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(4, 120)), int(rng.integers(4, 120)), int(rng.integers(1, N_CAT + 1))
            c = blob_counts(rng, cy, cx, ry, rx)
            if c.size < 2:
                c = np.asarray([0, 1, H * W - 1], dtype=np.int64)
            preds.append({"image_id": i + 1, "category_id": cat, "score": float(rng.random()), "segmentation": seg(c)})
    return ann, preds


def star(rng):
    k = int(rng.integers(8, 81))
    r = float(rng.uniform(10, 120))
    cx, cy = float(rng.uniform(0, W)), float(rng.uniform(0, H))
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = r * rng.uniform(.6, 1.0, k)
    return np.round(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1), 2).reshape(-1).tolist(), (cy, cx, r)


def polygon_corpus(n_images, seed=0, n_det=20):
    """Polygon ground truth (no `area` field: COCOeval's comes from the mask, so does prepare's), RLE detections around it."""
    rng = np.random.default_rng(seed)
    import ctypes
    from zutis_amd import _lib
    lib, buf = _lib.load(raw=True), ctypes.create_string_buffer(1 << 16)
    ann = {"images": [{"id": i + 1, "height": H, "width": W} for i in range(n_images)],
           "categories": [{"id": c + 1, "name": f"c{c}"} for c in range(N_CAT)], "annotations": []}
    preds = []
    for i in range(n_images):
        shapes = []
        for _ in range(int(rng.integers(1, MAX_GT + 1))):
            stars = [star(rng) for _ in range(int(rng.integers(1, 4)))]
            cat = int(rng.integers(1, N_CAT + 1))
            shapes.append((stars[0][1], cat))
            ann["annotations"].append({"id": len(ann["annotations"]) + 1, "image_id": i + 1, "category_id": cat,
                                       "segmentation": [p for p, _ in stars], "iscrowd": 0})
        for _ in range(n_det):
            (cy, cx, r), cat = shapes[int(rng.integers(0, len(shapes)))]
            c = np.ascontiguousarray(blob_counts(rng, int(cy) + int(rng.integers(-6, 7)), int(cx) + int(rng.integers(-6, 7)), max(2, int(.8 * r)), max(2, int(.8 * r))), dtype=np.int64)
            if c.size < 2:
                c = np.asarray([0, 1, H * W - 1], dtype=np.int64)
            n = lib.zh_rle_counts_to_string_host(c.ctypes.data, c.size, ctypes.addressof(buf), len(buf))
            assert n >= 0
            preds.append({"image_id": i + 1, "category_id": cat, "score": float(rng.random()), "segmentation": {"size": [H, W], "counts": buf.raw[:n]}})
    return ann, preds


def polygon_main(a):
    import torch
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    ann, preds = polygon_corpus(a.images)
    n_poly = sum(len(x["segmentation"]) for x in ann["annotations"])
    print(f"corpus: {a.images} images, {len(ann['annotations'])} polygon annotations of {n_poly} polygons, {len(preds)} detections "
          f"({time.perf_counter() - t0:.1f} s)", flush=True)
    coco_eval.mask_ap_route({**ann, "annotations": ann["annotations"][:8]}, [p for p in preds if p["image_id"] == 1], device=dev)     # warm-up
    rec = {r: {"mask_ap_s": [], "polygon_s": [], "kernel_ms": [], "host_fallback": []} for r in ("host", "device")}
    stats = {}
    for r in range(a.rounds):
        for route in ("host", "device"):
            tm = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = coco_eval.mask_ap_route(ann, preds, polygons=route, device=dev, timings=tm)
            rec[route]["mask_ap_s"].append(time.perf_counter() - t0)
            rec[route]["polygon_s"].append(tm["polygon_s"])
            rec[route]["kernel_ms"].append(sum(e0.elapsed_time(e1) for _, e0, e1 in tm["events"]))
            rec[route]["host_fallback"].append(tm["stats"]["host_fallback"])
            for k in ("stats", "precision", "recall"):
                assert np.array_equal(stats.setdefault(k, res[k]), res[k]), (route, r, k)        # both routes, every round: the same bits
        print(f"round {r}: " + ", ".join(f"{rt} {rec[rt]['mask_ap_s'][-1]:.3f} s (polygons {rec[rt]['polygon_s'][-1]:.3f} s)" for rt in rec), flush=True)
    assert rec["device"]["host_fallback"] == [0] * a.rounds, rec["device"]["host_fallback"]
    out = {"tool": "tools/coco_ap_bench.py --gt polygons", "images": a.images, "size": [H, W], "annotations": len(ann["annotations"]),
           "polygons": n_poly, "detections": len(preds), "rounds": a.rounds, "stats": [float(s) for s in stats["stats"]],
           "routes_equal_in_every_bit": True}
    for rt, d in rec.items():
        out[rt] = {"mask_ap_s": med(d["mask_ap_s"]), "polygon_stage_s": med(d["polygon_s"]), "host_fallback": d["host_fallback"]}
    out["device"]["zh_polygon_runs_ms"] = med(rec["device"]["kernel_ms"])
    out["mask_ap_host_over_device"] = out["host"]["mask_ap_s"]["median"] / out["device"]["mask_ap_s"]["median"]
    out["polygon_stage_host_over_device"] = out["host"]["polygon_stage_s"]["median"] / out["device"]["polygon_stage_s"]["median"]
    out["device_ahead_in_every_round"] = bool(all(d < h for d, h in zip(rec["device"]["mask_ap_s"], rec["host"]["mask_ap_s"])))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def reference_arm(ann, preds):
    """tests/_cocoeval_ref.py on the corpus: the masks of one image at a time are decoded to pixels (the whole corpus would be 17 GB)."""
    cats = [c["id"] for c in ann["categories"]]
    by_img_g, by_img_d = {}, {}
    for a in ann["annotations"]:
        by_img_g.setdefault(a["image_id"], []).append(a)
    for p in preds:
        by_img_d.setdefault(p["image_id"], []).append(p)
    groups = []
    for im in ann["images"]:
        i = im["id"]
        gts = [{"image_id": i, "category_id": a["category_id"], "mask": rle.decode_np(a["segmentation"]).astype(bool), "iscrowd": a["iscrowd"],
                "area": a["area"]} for a in by_img_g.get(i, [])]
        dets = [{"image_id": i, "category_id": p["category_id"], "score": p["score"], "mask": rle.decode_np(p["segmentation"]).astype(bool)}
                for p in by_img_d.get(i, [])]
        groups += R.evaluate([i], cats, gts, dets)
    groups.sort(key=lambda g: (g["k"], g["image_id"]))
    precision, recall = R.accumulate(groups, len(cats), (1, 10, 100))
    return R.summarize(precision, recall, (1, 10, 100))


def device_arm(ann, preds, dev, chunk_bytes):
    import torch
    t0 = time.perf_counter()
    prob = coco_eval.prepare(ann, preds)
    t1 = time.perf_counter()
    events = []
    matches = coco_eval.match_on_device(prob, dev, chunk_bytes=chunk_bytes, events=events)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    res = coco_eval.result_dict(*coco_eval.accumulate(prob, matches), prob.max_dets)
    t3 = time.perf_counter()
    kern = {}
    for name, e0, e1 in events:
        kern[name] = kern.get(name, 0.0) + e0.elapsed_time(e1)
    return res["stats"], {"total_s": t3 - t0, "prepare_s": t1 - t0, "device_s": t2 - t1, "accumulate_s": t3 - t2, "kernel_ms": kern,
                          "launches": len(events), "pairs": int(sum(len(g.det_mask) * len(g.gt_mask) for g in prob.groups)),
                          "groups": len(prob.groups), "masks": len(prob.masks)}


def med(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "rounds": [float(x) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gt", default="rle", choices=["rle", "polygons"])
    ap.add_argument("--images", type=int, default=None, help="default: 500 (--gt rle), 400 (--gt polygons)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--arm", nargs="+", default=["D", "R"], choices=["D", "R"])
    ap.add_argument("--chunk-mb", type=int, nargs="+", default=[coco_eval.CHUNK_BYTES >> 20])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.gt == "polygons":
        a.images = 400 if a.images is None else a.images
        return polygon_main(a)
    a.images = 500 if a.images is None else a.images
    import torch
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    ann, preds = corpus(a.images)
    print(f"corpus: {a.images} images, {len(ann['annotations'])} ground truths, {len(preds)} detections ({time.perf_counter() - t0:.1f} s)", flush=True)
    stats_d = coco_eval.mask_ap(ann, preds, device=dev)["stats"]                       # warm-up: library load, first launches
    times = {f"D_chunk{m}": [] for m in a.chunk_mb} if "D" in a.arm else {}
    detail, ref_t, stats_r = {}, [], None
    for r in range(a.rounds):
        for m in (a.chunk_mb if "D" in a.arm else []):
            s, d = device_arm(ann, preds, dev, m << 20)
            assert np.array_equal(s, stats_d)
            times[f"D_chunk{m}"].append(d["total_s"])
            detail.setdefault(f"D_chunk{m}", []).append(d)
        if "R" in a.arm:
            t0 = time.perf_counter()
            stats_r = reference_arm(ann, preds)
            ref_t.append(time.perf_counter() - t0)
        print(f"round {r}: " + ", ".join(f"{k} {v[-1]:.3f} s" for k, v in times.items()) + (f", R {ref_t[-1]:.1f} s" if ref_t else ""), flush=True)
    out = {"tool": "tools/coco_ap_bench.py", "images": a.images, "size": [H, W], "detections_per_image": N_DET, "max_ground_truths": MAX_GT,
           "categories": N_CAT, "rounds": a.rounds, "stats": [float(s) for s in stats_d]}
    for k, v in times.items():
        d = detail[k]
        out[k] = {"mask_ap_s": med(v), "prepare_s": med([x["prepare_s"] for x in d]), "device_s": med([x["device_s"] for x in d]),
                  "accumulate_s": med([x["accumulate_s"] for x in d]), "launches": d[0]["launches"], "pairs": d[0]["pairs"],
                  "groups": d[0]["groups"], "masks": d[0]["masks"],
                  "kernel_ms": {n: med([x["kernel_ms"].get(n, 0.0) for x in d]) for n in d[0]["kernel_ms"]}}
    if ref_t:
        out["R_numpy_reference_s"] = med(ref_t)
        out["stats_equal_to_reference"] = bool(np.array_equal(stats_r, stats_d))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
