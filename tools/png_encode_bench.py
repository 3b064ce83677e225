"""Developer tool: the device PNG encoder (png_encoder="device": zh_png_deflate, zutis_amd/png_device.py) against the writer threads'
Pillow encoder (png_encoder="host", the default) on the three file drivers' set-ups that write pictures.

    python tools/png_encode_bench.py [--setup a|b|c ...] [--rounds R] [--images N] [--mask-images M] [--batch B] [--workers W]
                                     [--model vitb16|tiny] [--compress-level C] [--corpus DIR] [--out profiles/png_encode_ab.json]

Set-ups:
  a  tools/instance_paint_bench.py's F1: predict_from_files(semantic=False, instance=True, instance_map=True, instance_overlay=True) over
     N (64) coco-like JPEGs of 640 x 480 / 480 x 640 — an id map (mode L) and a photographic overlay (RGB) per image
  b  tools/predict_files_bench.py's F arm on its coco config: the semantic label map as a mode L PNG (81 classes, "u8"), instance predict on
  c  tools/label_paint_bench.py's write_semantic_masks(route="device") over M (400) images of 480 x 640 with polygon annotations
Arms "host" and "device", ALTERNATED in one process (round r runs both), one untimed pass per arm first, a device synchronise in every
window; medians and min - max over the rounds, every round kept.  Per arm: images/s (seconds for c) and the bytes of the files written; for
"device" also the HIP-event time of zh_png_deflate's launches summed over a run, and the seconds the writer threads spend inside
png_device.frame (the IDAT's CRC-32 is what is left of the encoding on the host), summed over the threads.  A difference counts when the
two arms' ranges of rounds do not overlap.  The two arms' files are decoded and compared once at the end."""
import argparse
import json
import os
import statistics
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
from eval_files_bench import CONFIGS, MEAN, STD, network_of, write_pair          # noqa: E402
from zutis_amd import annotation_labels as AL, ops, png_device, predict_files     # noqa: E402

ARMS = ("host", "device")


class Probes:
    """Wraps ops.png_deflate in HIP events and png_device.frame in a clock; read() returns and clears what a run gathered."""

    def __init__(self):
        self.events, self.frame_s = [], []
        real_deflate, real_frame = ops.png_deflate, png_device.frame

        def deflate(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = real_deflate(*a, **k)
            e1.record()
            self.events.append((e0, e1))
            return r

        def frame(*a, **k):
            t = time.perf_counter()
            r = real_frame(*a, **k)
            self.frame_s.append(time.perf_counter() - t)               # list.append: safe from the writer threads
            return r

        ops.png_deflate, png_device.frame = deflate, frame

    def read(self):
        torch.cuda.synchronize()
        out = {"deflate_calls": len(self.events), "deflate_ms": round(sum(a.elapsed_time(b) for a, b in self.events), 4),
               "frame_calls": len(self.frame_s), "frame_thread_s": round(sum(self.frame_s), 5)}
        self.events, self.frame_s = [], []
        return out


def files_bytes(paths):
    return int(sum(os.path.getsize(p) for p in paths))


def same_pixels(a_paths, b_paths):
    differ = 0
    for a, b in zip(a_paths, b_paths):
        with Image.open(a) as x, Image.open(b) as y:
            differ += int(x.mode != y.mode or x.size != y.size or not np.array_equal(np.asarray(x), np.asarray(y)))
    return differ


def ab(run, rounds, probes, unit_count):
    """run(arm) -> (seconds, [paths written]).  One untimed pass per arm, then `rounds` alternated rounds."""
    rec = {a: {"seconds_rounds": [], "device_rounds": []} for a in ARMS}
    paths = {}
    for a in ARMS:
        run(a)
        probes.read()
    for r in range(rounds):
        for a in ARMS:
            s, paths[a] = run(a)
            got = probes.read()
            rec[a]["seconds_rounds"].append(round(s, 5))
            if a == "device":
                rec[a]["device_rounds"].append(got)
            print(f"round {r} {a}: {s:.4f} s = {unit_count / s:.1f} images/s", flush=True)
    out = {}
    for a in ARMS:
        s = rec[a]["seconds_rounds"]
        out[a] = {"seconds": round(statistics.median(s), 5), "seconds_min": min(s), "seconds_max": max(s), "seconds_rounds": s,
                  "images_per_s": round(unit_count / statistics.median(s), 1), "images_per_s_min": round(unit_count / max(s), 1),
                  "images_per_s_max": round(unit_count / min(s), 1), "files": len(paths[a]), "bytes_written": files_bytes(paths[a])}
    d = rec["device"]["device_rounds"]
    out["device"].update(deflate_ms=round(statistics.median(x["deflate_ms"] for x in d), 4), deflate_calls=d[0]["deflate_calls"],
                         frame_thread_s=round(statistics.median(x["frame_thread_s"] for x in d), 5), frame_calls=d[0]["frame_calls"],
                         device_rounds=d)
    out["device_over_host"] = round(out["host"]["seconds"] / out["device"]["seconds"], 3)
    out["bytes_device_over_host"] = round(out["device"]["bytes_written"] / max(1, out["host"]["bytes_written"]), 3)
    out["ranges_overlap"] = bool(out["device"]["seconds_min"] <= out["host"]["seconds_max"] and out["host"]["seconds_min"] <= out["device"]["seconds_max"])
    out["verdict"] = "no difference (the arms' ranges overlap)" if out["ranges_overlap"] else \
        ("device faster" if out["device"]["seconds_max"] < out["host"]["seconds_min"] else "device slower")
    out["files_differing_in_pixels"] = same_pixels(paths["host"], paths["device"])
    return out


def corpus_images(args, workers):
    cfg = CONFIGS["coco"]
    d = os.path.join(args.corpus, "coco")
    os.makedirs(d, exist_ok=True)
    p_images = [os.path.join(d, f"img_{k:05d}.jpg") for k in range(args.images)]
    p_gts = [os.path.join(d, f"gt_{k:05d}.png") for k in range(args.images)]
    todo = [k for k in range(args.images) if not (os.path.exists(p_images[k]) and os.path.exists(p_gts[k]))]
    with ThreadPoolExecutor(max_workers=workers) as pool:
        list(pool.map(lambda k: write_pair(cfg, k, p_images[k], p_gts[k]), todo))
    return cfg, d, p_images


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setup", nargs="+", default=["a", "b", "c"], choices=["a", "b", "c"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--mask-images", type=int, default=400)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--model", default="vitb16", choices=["vitb16", "tiny"])
    ap.add_argument("--compress-level", type=int, default=1)
    ap.add_argument("--corpus", default=os.path.join(tempfile.gettempdir(), "zutis_eval_corpus"))
    ap.add_argument("--out", help="also write the result object to this JSON file")
    args = ap.parse_args()
    workers = max(1, min(args.workers, 16))
    dev = torch.device("cuda:0")
    probes = Probes()
    res = {"tool": "png_encode_bench", "model": args.model, "images": args.images, "mask_images": args.mask_images, "batch": args.batch,
           "n_workers": workers, "rounds": args.rounds, "compress_level": args.compress_level, "pillow": Image.__version__,
           "segment_bytes": png_device.SEGMENT_BYTES, "cpus_in_use": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None,
           "setups": {}}
    if "a" in args.setup or "b" in args.setup:
        cfg, d, p_images = corpus_images(args, workers)
        net, _ = network_of(args.model, cfg["n"], dev)
        ids = list(range(args.images))
        if "a" in args.setup:
            def run_a(arm):
                s, r = timed(lambda: predict_files.predict_from_files(
                    net, p_images, out_dir=os.path.join(d, f"png_a_{arm}"), semantic=False, instance=True, image_ids=ids, max_size=cfg["max_size"],
                    mean=MEAN, std=STD, batch_size=args.batch, n_workers=workers, compress_level=args.compress_level, instance_map=True,
                    instance_overlay=True, png_encoder=arm))
                return s, r["instance_map_paths"] + r["instance_overlay_paths"]
            res["setups"]["a"] = dict(ab(run_a, args.rounds, probes, args.images), what="instance id map (L) + instance overlay (RGB) per image")
            for arm in ARMS:                                               # the two kinds of picture apart: the overlay is where the size trade is
                root = os.path.join(d, f"png_a_{arm}")
                names = sorted(os.listdir(root))
                res["setups"]["a"][arm]["bytes_id_maps"] = files_bytes(os.path.join(root, n) for n in names if n.endswith("_instances.png"))
                res["setups"]["a"][arm]["bytes_overlays"] = files_bytes(os.path.join(root, n) for n in names if n.endswith("_instances_overlay.png"))
        if "b" in args.setup:
            def run_b(arm):
                s, r = timed(lambda: predict_files.predict_from_files(
                    net, p_images, out_dir=os.path.join(d, f"png_b_{arm}"), label_format=cfg["fmt"], max_size=cfg["max_size"], mean=MEAN, std=STD,
                    batch_size=args.batch, n_workers=workers, compress_level=args.compress_level, instance=cfg["instance"], image_ids=ids,
                    png_encoder=arm))
                return s, r["label_paths"]
            res["setups"]["b"] = dict(ab(run_b, args.rounds, probes, args.images), what="semantic label map (L) per image, instance predict on")
        del net
        torch.cuda.empty_cache()
    if "c" in args.setup:
        ann, _ = coco_ap_bench.polygon_corpus(args.mask_images)
        for im in ann["images"]:
            im["file_name"] = f"{im['id']:012d}.jpg"
        dm = os.path.join(args.corpus, "png_masks")

        def run_c(arm):
            s, r = timed(lambda: AL.write_semantic_masks(ann, os.path.join(dm, arm), route="device", device=dev, n_workers=workers,
                                                         compress_level=args.compress_level, png_encoder=arm))
            return s, r["paths"]
        res["setups"]["c"] = dict(ab(run_c, args.rounds, probes, args.mask_images), what="write_semantic_masks: one label map (L) per image",
                                  annotations=len(ann["annotations"]))
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
