"""Developer tool: semantic ground truth from COCO annotations (zutis_amd/annotation_labels.py) on the corpus of
tools/coco_ap_bench.py --gt polygons (default 400 images at 480 x 640, 3216 polygon annotations), arms ALTERNATED in one process, medians
and min - max over the rounds, a device synchronise in every window.

    python tools/label_paint_bench.py [--images N] [--rounds R] [--workers W] [--model vitb16|tiny] [--batch B] [--no-eval]
                                      [--corpus DIR] [--out profiles/label_paint_ab.json]

Writing the directory:
  write host     write_semantic_masks(route="host"): labels_np (rle.from_polygons per annotation, then paint) + Image.save, one thread
  write device   write_semantic_masks(route="device"): LabelPainter (zh_polygon_runs, zh_rle_prefix), ragged launches of
                 zh_runs_label_maps, one copy back per launch, PNG encoding in the writer threads
  paint host / paint device   the same without the PNGs: labels_np alone; LabelPainter + every map painted + the copies back
  kernels        zh_polygon_runs / zh_rle_prefix / zh_runs_label_maps by HIP events, summed over a run's launches
The two routes' files are compared byte for byte.
Evaluation (images/s): evaluate_from_files on the written PNGs against evaluate_from_annotations on the same image files (seeded JPEGs
written here), the random-weight drop-in ZUTIS of tools/eval_files_bench.py with 81 classes, semantic scoring only."""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "zutis_amd", "dropin"))
import coco_ap_bench  # noqa: E402
import eval_files_bench  # noqa: E402
from zutis_amd import annotation_labels as AL, evaluate  # noqa: E402

H, W, N_CLASSES = coco_ap_bench.H, coco_ap_bench.W, coco_ap_bench.N_CAT + 1


def med(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "rounds": [float(x) for x in v]}


def write_photo(k, path):
    rng = np.random.default_rng(70_000 + k)
    low = rng.integers(0, 256, (H // 24, W // 24, 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(low).resize((W, H), Image.BICUBIC), np.float32)
    a += rng.normal(0.0, 6.0, a.shape).astype(np.float32)
    Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(path, quality=90)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def paint_device(plan, dev, events):
    """LabelPainter and every map, in write_semantic_masks' launches, copied back: the device route without PNG encoding."""
    painter = AL.LabelPainter(plan, dev, events)
    per = max(1, AL.PAINT_BYTES // (H * W))
    host = torch.empty(per * H * W, dtype=torch.uint8, pin_memory=True)
    for lo in range(0, len(plan), per):
        buf, _ = painter.paint_ragged(range(lo, min(lo + per, len(plan))))
        host[:buf.numel()].copy_(buf, non_blocking=True)
        torch.cuda.synchronize()
    return painter.stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--model", default="vitb16", choices=["vitb16", "tiny"])
    ap.add_argument("--no-eval", action="store_true")
    ap.add_argument("--corpus", default=os.path.join(tempfile.gettempdir(), "zutis_label_paint_corpus"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    workers = max(1, min(a.workers, 16))
    t0 = time.perf_counter()
    ann, _ = coco_ap_bench.polygon_corpus(a.images)                                     # the detections are drawn and dropped: the same stars
    for im in ann["images"]:
        im["file_name"] = f"{im['id']:012d}.jpg"
    n_poly = sum(len(x["segmentation"]) for x in ann["annotations"])
    print(f"corpus: {a.images} images of {H} x {W}, {len(ann['annotations'])} polygon annotations of {n_poly} polygons ({time.perf_counter() - t0:.1f} s)", flush=True)
    d_host, d_dev = os.path.join(a.corpus, "masks_host"), os.path.join(a.corpus, "masks_device")
    plan = AL.paint_plan(ann)
    small = AL.paint_plan(ann, [im["id"] for im in ann["images"][:4]])
    AL.LabelPainter(small, dev).paint(range(4))                                        # warm-up: library load, first launches
    AL.write_semantic_masks(ann, d_dev, image_ids=[im["id"] for im in ann["images"][:4]], device=dev, n_workers=workers)
    rec = {k: [] for k in ("write_host_s", "write_device_s", "paint_host_s", "paint_device_s")}
    kern = {}
    stats = None
    for r in range(a.rounds):
        rec["write_host_s"].append(timed(lambda: AL.write_semantic_masks(ann, d_host, route="host"))[0])
        dt, res = timed(lambda: AL.write_semantic_masks(ann, d_dev, route="device", device=dev, n_workers=workers))
        rec["write_device_s"].append(dt)
        rec["paint_host_s"].append(timed(lambda: AL.labels_np(plan))[0])
        events = []
        dt, stats = timed(lambda: paint_device(plan, dev, events))
        rec["paint_device_s"].append(dt)
        per = {}
        for name, e0, e1 in events:
            per[name] = per.get(name, 0.0) + e0.elapsed_time(e1)
        for name, ms in per.items():
            kern.setdefault(name, []).append(ms)
        print(f"round {r}: " + ", ".join(f"{k} {v[-1]:.3f}" for k, v in rec.items()) + " | " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in kern.items()), flush=True)
    paths_h = [os.path.join(d_host, AL.stem_of(im["file_name"]) + ".png") for im in ann["images"]]
    equal = all(open(p, "rb").read() == open(q, "rb").read() for p, q in zip(paths_h, res["paths"]))
    out = {"tool": "tools/label_paint_bench.py", "images": a.images, "size": [H, W], "annotations": len(ann["annotations"]), "polygons": n_poly,
           "rounds": a.rounds, "n_workers": workers, "compress_level": 1, "paint_bytes": AL.PAINT_BYTES,
           "cpus_in_use": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None, "painter_stats": stats,
           "files_equal_byte_for_byte": bool(equal), **{k: med(v) for k, v in rec.items()}, "kernel_ms": {k: med(v) for k, v in kern.items()}}
    out["write_host_over_device"] = out["write_host_s"]["median"] / out["write_device_s"]["median"]
    out["paint_host_over_device"] = out["paint_host_s"]["median"] / out["paint_device_s"]["median"]
    out["device_ahead_in_every_round"] = bool(all(d < h for d, h in zip(rec["write_device_s"], rec["write_host_s"])))
    out["encoding_share_of_write_device"] = 1.0 - out["paint_device_s"]["median"] / out["write_device_s"]["median"]
    if not a.no_eval:
        d_img = os.path.join(a.corpus, "images")
        os.makedirs(d_img, exist_ok=True)
        p_images = [os.path.join(d_img, im["file_name"]) for im in ann["images"]]
        with ThreadPoolExecutor(max_workers=workers) as pool:
            list(pool.map(lambda k: write_photo(k, p_images[k]), [k for k in range(a.images) if not os.path.exists(p_images[k])]))
        net, _ = eval_files_bench.network_of(a.model, N_CLASSES, dev)
        ids = [im["id"] for im in ann["images"]]
        kw = dict(max_size=None, batch_size=a.batch, n_workers=workers)
        arms = {"files": lambda: evaluate.evaluate_from_files(net, p_images, res["paths"], N_CLASSES, **kw),
                "annotations": lambda: evaluate.evaluate_from_annotations(net, p_images, ann, N_CLASSES, image_ids=ids, **kw)}
        cms = {}
        for k, fn in arms.items():                                                      # warm-up: graph captures, allocator
            fn()
        secs = {k: [] for k in arms}
        for r in range(a.rounds):
            for k, fn in arms.items():
                dt, got = timed(fn)
                secs[k].append(dt)
                cms[k] = got["confusion_matrix"]
            print(f"eval round {r}: " + ", ".join(f"{k} {a.images / v[-1]:.1f} images/s" for k, v in secs.items()), flush=True)
        rates = {k: [a.images / s for s in v] for k, v in secs.items()}
        out["evaluation"] = {"model": a.model, "classes": N_CLASSES, "batch": a.batch, "instance": False,
                             "confusion_matrices_equal": bool(np.array_equal(cms["files"], cms["annotations"])),
                             "pixels_counted": int(cms["files"].sum()),
                             **{f"{k}_images_per_s": med(v) for k, v in rates.items()}}
        f, g = out["evaluation"]["files_images_per_s"], out["evaluation"]["annotations_images_per_s"]
        out["evaluation"]["annotations_over_files"] = g["median"] / f["median"]
        out["evaluation"]["verdict"] = "annotations ahead" if g["min"] > f["max"] else "files ahead" if f["min"] > g["max"] else "tie (inside the arms' spread)"
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
