"""Developer tool: what a picture of the instance predictions costs — on the coco-like corpus of tools/eval_files_bench.py (640x480 /
480x640 JPEGs, 81 classes) and as a kernel.

    python tools/instance_paint_bench.py [--rounds R] [--images N] [--batch B] [--workers W] [--model vitb16|tiny] [--compress-level C]
                                         [--no-kernel | --kernel-only] [--corpus DIR] [--out FILE.json]

Arms, ALTERNATED in one process (round r runs every arm once), medians and spreads over the rounds, a device synchronise in every window:
  F0 predict_from_files(semantic=False, instance=True): the predictions alone
  F1 the same with instance_map=True, instance_overlay=True: the two PNGs per image painted on the device, encoded by the writer ring
  H  the loop a user writes without them: F0's call, then per image the RLEs decoded (rle.decode_np), instance_paint.paint_reference and two
     Image.save on the calling thread
Kernel (HIP events, us per call): zh_instance_paint at 480 x 640 with 100 slots, B in {1, batch}, count in {17, 100}, masks as bits and as
bytes, id map + overlay with outline (three launches).  The compiler's register / occupancy / scratch figures of the three kernels are
recorded when hipcc is at hand.  --kernel-only runs nothing else: the form to put behind `rocprofv3 --kernel-trace --stats --`."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
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
from eval_files_bench import CONFIGS, MEAN, STD, network_of, write_pair          # noqa: E402
from zutis_amd import instance_paint, ops, predict_files, rle                     # noqa: E402


def paint_on_the_host(p_images, predictions, map_paths, overlay_paths, compress_level):
    """Arm H's tail: per image the pictures from the prediction dicts, on the calling thread."""
    per = [[] for _ in p_images]
    for p in predictions:
        per[p["image_id"]].append(p)
    for i, preds in enumerate(per):
        image = np.asarray(Image.open(p_images[i]).convert("RGB"))
        H, W = image.shape[:2]
        masks = np.stack([rle.decode_np(p["segmentation"]) for p in preds]) if preds else np.zeros((0, H, W), np.uint8)
        got_ids, overlay = instance_paint.paint_reference(image, masks, [p["score"] for p in preds], instance_paint.instance_colours(len(preds)))
        Image.fromarray(got_ids.astype(np.uint8)).save(map_paths[i], compress_level=compress_level)
        Image.fromarray(overlay).save(overlay_paths[i], compress_level=compress_level)


def blob_masks(dev, B, Q, H, W, seed):
    """u8 [B,Q,H,W] on the device: smooth blobs (a thresholded up-sampled noise field), ~15 % of the image per mask."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn((B * Q, 1, 6, 8), generator=g).to(dev)
    field = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=False)
    return (field > 1.0).to(torch.uint8).view(B, Q, H, W).contiguous()


def kernel_times(dev, B, Q, H, W, count, iters=50, repeats=5):
    g = torch.Generator().manual_seed(5)
    masks = blob_masks(dev, B, Q, H, W, 11)
    bits = torch.empty((B, Q, (H * W + 63) // 64), dtype=torch.int64, device=dev)
    inter = torch.empty((Q, Q), dtype=torch.int32, device=dev)
    for b in range(B):
        ops.mask_iou_counts(masks[b], Q, H * W, inter, torch.empty_like(inter), workspace=bits[b])
    index = torch.stack([torch.randperm(Q, generator=g) for _ in range(B)]).to(torch.int32).to(dev)
    score = torch.rand((B, Q), generator=g, dtype=torch.float64).to(dev)
    cnt = torch.full((B,), count, dtype=torch.int32, device=dev)
    colours = torch.from_numpy(instance_paint.instance_colours(Q)).to(dev).unsqueeze(0).expand(B, Q, 3).contiguous()
    per = -(-3 * H * W // 16)
    packed = torch.randint(0, 256, (B * per * 16,), dtype=torch.uint8, generator=g).to(dev)
    desc_host = torch.tensor([[b * per, W, H, W, H, 0, 0, 0] for b in range(B)], dtype=torch.int32)
    desc = desc_host.to(dev)
    ids = {f: torch.empty((B, H, W), dtype=torch.uint8, device=dev) for f in ("bits", "bytes")}
    ovl = {f: torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) for f in ("bits", "bytes")}
    ws = torch.empty(ops.instance_paint_workspace_size(B, Q, H, W), dtype=torch.uint8, device=dev)

    def run(form):
        ops.instance_paint(index, score, cnt, H, W, masks=masks if form == "bytes" else None, bits=bits if form == "bits" else None, colours=colours,
                           packed=packed, desc=desc, desc_host=desc_host, ids_out=ids[form], overlay_out=ovl[form], workspace=ws)

    out = {"B": B, "Q": Q, "count": count, "size": [H, W]}
    for form in ("bits", "bytes"):
        run(form)
        ts = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                run(form)
            b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1000.0 / iters)
        out[form] = {"median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)}
    out["outputs_equal"] = bool(torch.equal(ids["bits"], ids["bytes"]) and torch.equal(ovl["bits"], ovl["bytes"]))
    out["painted_fraction"] = round(float((ids["bits"] != 0).float().mean()), 4)
    return out


def kernel_resources():
    """{kernel: {vgprs, sgprs, occupancy_waves_per_simd, scratch_bytes_per_lane, lds_bytes}} from hipcc's resource remarks, or None."""
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        return None
    src = os.path.join(ROOT, "zutis_amd", "csrc", "instance_paint.hip")
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([hipcc, "-Rpass-analysis=kernel-resource-usage", "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-c", src, "-o",
                            os.path.join(d, "x.o")], stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        return None
    res, name = {}, None
    keys = {"VGPRs:": "vgprs", "TotalSGPRs:": "sgprs", "Occupancy [waves/SIMD]:": "occupancy_waves_per_simd",
            "ScratchSize [bytes/lane]:": "scratch_bytes_per_lane", "LDS Size [bytes/block]:": "lds_bytes"}
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            res[name] = {}
        for k, v in keys.items():
            if name and " " + k in ln:
                res[name][v] = int(ln.split(k)[1].split()[0])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--model", default="vitb16", choices=["vitb16", "tiny"])
    ap.add_argument("--compress-level", type=int, default=1)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--corpus", default=os.path.join(tempfile.gettempdir(), "zutis_eval_corpus"))
    ap.add_argument("--out", help="also write the result object to this JSON file")
    args = ap.parse_args()
    cfg = CONFIGS["coco"]
    workers = max(1, min(args.workers, 16))
    dev = torch.device("cuda:0")
    res = {"tool": "instance_paint_bench", "model": args.model, "images": args.images, "batch": args.batch, "n_workers": workers, "rounds": args.rounds,
           "compress_level": args.compress_level, "pillow": Image.__version__, "classes": cfg["n"], "sizes_wh": sorted(set(cfg["sizes"])),
           "cpus_in_use": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None}
    if not args.kernel_only:
        net, _ = network_of(args.model, cfg["n"], dev)
        d = os.path.join(args.corpus, "coco")
        os.makedirs(d, exist_ok=True)
        p_images = [os.path.join(d, f"img_{k:05d}.jpg") for k in range(args.images)]
        p_gts = [os.path.join(d, f"gt_{k:05d}.png") for k in range(args.images)]
        todo = [k for k in range(args.images) if not (os.path.exists(p_images[k]) and os.path.exists(p_gts[k]))]
        with ThreadPoolExecutor(max_workers=workers) as pool:
            list(pool.map(lambda k: write_pair(cfg, k, p_images[k], p_gts[k]), todo))
        outs = {a: os.path.join(d, f"paint_{a}") for a in ("F1", "H")}
        for o in outs.values():
            os.makedirs(o, exist_ok=True)
        h_maps = [os.path.join(outs["H"], f"img_{k:05d}_instances.png") for k in range(args.images)]
        h_ovls = [os.path.join(outs["H"], f"img_{k:05d}_instances_overlay.png") for k in range(args.images)]
        common = dict(semantic=False, instance=True, image_ids=list(range(args.images)), max_size=cfg["max_size"], mean=MEAN, std=STD,
                      batch_size=args.batch, n_workers=workers, compress_level=args.compress_level)
        last = {}

        def run(arm):
            torch.cuda.synchronize(); t = time.perf_counter()
            if arm == "F1":
                r = predict_files.predict_from_files(net, p_images, out_dir=outs["F1"], instance_map=True, instance_overlay=True, **common)
            else:
                r = predict_files.predict_from_files(net, p_images, **common)
                if arm == "H":
                    paint_on_the_host(p_images, r["instance_predictions"], h_maps, h_ovls, args.compress_level)
            torch.cuda.synchronize()
            last[arm] = r
            return time.perf_counter() - t

        order = ["F0", "F1", "H"]
        for a in order:                                                 # warm-up: one untimed pass per arm (graph captures, allocator, page cache)
            run(a)
        secs = {a: [] for a in order}
        for r in range(args.rounds):
            for a in order:
                secs[a].append(run(a))
                print(f"round {r} arm {a}: {secs[a][-1]:.3f} s = {args.images / secs[a][-1]:.1f} images/s", flush=True)
        res["arms"] = {}
        for a in order:
            rates = [args.images / s for s in secs[a]]
            res["arms"][a] = {"images_per_s": round(args.images / statistics.median(secs[a]), 1),
                              "ms_per_image": round(1000 * statistics.median(secs[a]) / args.images, 3),
                              "seconds_rounds": [round(v, 4) for v in secs[a]], "images_per_s_min": round(min(rates), 1),
                              "images_per_s_max": round(max(rates), 1), "instance_predictions": len(last[a]["instance_predictions"])}
        F0, F1, H = (res["arms"][a] for a in order)
        res["F1_over_F0"] = round(F1["images_per_s"] / F0["images_per_s"], 3)
        res["F0_spread"] = round(F0["images_per_s_max"] / F0["images_per_s_min"], 3)
        res["F1_spread"] = round(F1["images_per_s_max"] / F1["images_per_s_min"], 3)
        # inside the spread: the two arms' ranges of rounds overlap
        res["F1_inside_F0_spread"] = bool(F1["images_per_s_max"] >= F0["images_per_s_min"] and F0["images_per_s_max"] >= F1["images_per_s_min"])
        res["F1_over_H"] = round(F1["images_per_s"] / H["images_per_s"], 3)
        res["F1_clears_H"] = bool(F1["images_per_s_min"] > H["images_per_s_max"])
        # the pictures of the two paths: F1's ids are slots of the kept list, H numbers the predictions in order, so compare the overlays' shapes
        # and the painted area, not the ids
        differ = 0
        for k in range(args.images):
            a = np.asarray(Image.open(last["F1"]["instance_map_paths"][k])) != 0
            b = np.asarray(Image.open(h_maps[k])) != 0
            differ += int((a != b).sum())
        res["painted_pixels_differing_F1_vs_H"] = differ
        del net
        torch.cuda.empty_cache()
    if not args.no_kernel:
        w0, h0 = cfg["sizes"][0]
        res["kernel"] = [kernel_times(dev, B, 100, h0, w0, count) for B in sorted({1, args.batch}) for count in (17, 100)]
        res["kernel_resources"] = kernel_resources()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
