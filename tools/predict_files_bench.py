"""Developer tool: predictions as their caller gets them — image files in, label PNGs (and instance predictions) out — on the seeded
corpora of tools/eval_files_bench.py.

    python tools/predict_files_bench.py [--config coco|imagenet ...] [--arm L|F|T ...] [--rounds R] [--images N] [--batch B] [--workers W]
                                        [--model vitb16|tiny] [--compress-level C] [--no-kernel-ab | --kernel-ab-only] [--corpus DIR] [--out FILE.json]

Configs (eval_files_bench.CONFIGS): coco = 640x480 JPEGs, 81 classes, "u8" label PNGs, instance predict on; imagenet = JPEGs capped at
1024 on the longer edge, 920 classes, "rg16" label PNGs, predicted at the file's own size.
Arms, ALTERNATED in one process (round r runs every arm once), medians and spreads over the rounds, a device synchronise in every window:
  L  the loop a user writes on the public API without predict_from_files: per image Image.open + cap + to_tensor + normalize on the
     calling thread, network(image[None]), predict("semantic") to int64 NumPy, Image.fromarray(bytes).save(compress_level=C) on the
     calling thread, predict("instance") (coco)
  F  zutis_amd.predict_files.predict_from_files
  T  the host ceiling: decoding every image and encoding every label PNG (F's own output, re-encoded) in W threads, no device work
Kernel A/B (per config, HIP events): zh_upsample_argmax_bytes against zh_upsample_argmax + the torch cast of its int64 map to the u8 /
RG bytes.  --kernel-ab-only runs nothing else: the form to put behind `rocprofv3 --kernel-trace --stats --`."""
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
from eval_files_bench import CONFIGS, MEAN, STD, network_of, write_pair          # noqa: E402
from zutis_amd import ops, predict_files, preprocess                              # noqa: E402


def host_transform(path, max_size):
    im = Image.open(path).convert("RGB")
    W, H = im.size
    size = preprocess.longer_edge_size(W, H, max_size)
    if size != im.size:
        im = im.resize(size, Image.BILINEAR)
    x = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return (x - torch.tensor(MEAN)[:, None, None]) / torch.tensor(STD)[:, None, None], (H, W)


def loop_by_hand(net, dev, p_images, out_paths, fmt, max_size, instance, compress_level):
    preds = []
    with torch.no_grad():
        for i, (p, o) in enumerate(zip(p_images, out_paths)):
            x, (H, W) = host_transform(p, max_size)
            out = net(x[None].to(dev))
            sem = net.predict(dict_outputs=out, mask_type="semantic", size=(H, W))[0]
            Image.fromarray(predict_files.encode_labels(sem, fmt)).save(o, compress_level=compress_level)
            if instance:
                preds.extend(net.predict(dict_outputs=out, mask_type="instance", size=(H, W), image_ids=[i], nms_type="hard"))
    return preds


def host_ceiling(p_images, label_paths, out_paths, workers, compress_level):
    def one(k):
        np.asarray(Image.open(p_images[k]).convert("RGB"))
        Image.fromarray(np.asarray(Image.open(label_paths[k]))).save(out_paths[k], compress_level=compress_level)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        list(pool.map(one, range(len(p_images))))


def kernel_ab(cfg, dev, B, h, w, H, W, iters=50, repeats=5):
    """us per call of the byte kernel (labels only; labels + overlay) and of the int64 kernel + the casts, medians of `repeats` timings."""
    n, fmt = cfg["n"], cfg["fmt"]
    g = torch.Generator().manual_seed(3)
    coarse = torch.randn((B, n, max(2, h // 6), max(2, w // 6)), generator=g)
    lo = (torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear") * 4 + torch.randn((B, n, h, w), generator=g) * 0.1).to(dev).contiguous()
    ch = predict_files.LABEL_CHANNELS[fmt]
    raw = torch.empty((B, H, W) if ch == 1 else (B, H, W, 3), dtype=torch.uint8, device=dev)
    ovl = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    per = -(-3 * H * W // 16)
    packed = torch.randint(0, 256, (B * per * 16,), dtype=torch.uint8, generator=g).to(dev)
    desc_host = torch.tensor([[b * per, W, H, W, H, 0, 0, 0] for b in range(B)], dtype=torch.int32)
    desc, pal = desc_host.to(dev), torch.randint(0, 256, (n, 3), dtype=torch.uint8, generator=g).to(dev)
    labels = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    cast = torch.empty_like(raw)

    def fused():
        ops.upsample_argmax_bytes(lo, B, n, h, w, H, W, label_format=fmt, labels_out=raw)

    def fused_overlay():
        ops.upsample_argmax_bytes(lo, B, n, h, w, H, W, label_format=fmt, labels_out=raw, overlay_out=ovl, packed=packed, desc=desc, palette=pal,
                                  alpha=128, desc_host=desc_host)

    def chain():
        ops.upsample_argmax(lo, labels, B, n, h, w, H, W)
        if ch == 1:
            cast.copy_(labels)
        else:
            cast[..., 0] = labels & 255
            cast[..., 1] = labels >> 8
            cast[..., 2] = 0

    fused(); chain()
    torch.cuda.synchronize()
    equal = bool(torch.equal(raw, cast))
    us = {}
    for name, fn in (("bytes", fused), ("bytes_overlay", fused_overlay), ("int64_cast", chain)):
        fn()
        ts = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1000.0 / iters)
        us[name] = {"median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)}
    return {"B": B, "n": n, "label_format": fmt, "lowres": [h, w], "size": [H, W], **us, "bytes_equal": equal,
            "int64_cast_over_bytes": round(us["int64_cast"]["median_us"] / us["bytes"]["median_us"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--arm", action="append", choices=["L", "F", "T"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--images", type=int, default=96)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--model", default="vitb16", choices=["vitb16", "tiny"])
    ap.add_argument("--compress-level", type=int, default=1)
    ap.add_argument("--no-kernel-ab", action="store_true")
    ap.add_argument("--kernel-ab-only", action="store_true")
    ap.add_argument("--corpus", default=os.path.join(tempfile.gettempdir(), "zutis_eval_corpus"))
    ap.add_argument("--out", help="also write the result object to this JSON file")
    args = ap.parse_args()
    configs, arms = list(dict.fromkeys(args.config or sorted(CONFIGS))), list(dict.fromkeys(args.arm or ["L", "F", "T"]))
    if "T" in arms and "F" not in arms:
        ap.error("arm T re-encodes arm F's label maps: run F as well")
    workers = max(1, min(args.workers, 16))
    dev = torch.device("cuda:0")
    res = {"tool": "predict_files_bench", "model": args.model, "images": args.images, "batch": args.batch, "n_workers": workers, "rounds": args.rounds,
           "compress_level": args.compress_level, "pillow": Image.__version__,
           "cpus_in_use": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None, "configs": {}}
    for name in configs:
        cfg = CONFIGS[name]
        net, mcfg = network_of(args.model, cfg["n"], dev)
        out = {"classes": cfg["n"], "label_format": cfg["fmt"], "max_size": cfg["max_size"], "instance": cfg["instance"], "sizes_wh": sorted(set(cfg["sizes"]))}
        if not args.kernel_ab_only:
            d = os.path.join(args.corpus, name)
            os.makedirs(d, exist_ok=True)
            p_images = [os.path.join(d, f"img_{k:05d}.jpg") for k in range(args.images)]
            p_gts = [os.path.join(d, f"gt_{k:05d}.png") for k in range(args.images)]
            todo = [k for k in range(args.images) if not (os.path.exists(p_images[k]) and os.path.exists(p_gts[k]))]
            with ThreadPoolExecutor(max_workers=workers) as pool:
                list(pool.map(lambda k: write_pair(cfg, k, p_images[k], p_gts[k]), todo))
            outs = {a: [os.path.join(d, f"pred_{a}", f"img_{k:05d}.png") for k in range(args.images)] for a in "LFT"}
            for a in "LFT":
                os.makedirs(os.path.join(d, f"pred_{a}"), exist_ok=True)

            def run(arm):
                torch.cuda.synchronize(); t = time.perf_counter()
                if arm == "L":
                    n_preds = len(loop_by_hand(net, dev, p_images, outs["L"], cfg["fmt"], cfg["max_size"], cfg["instance"], args.compress_level))
                elif arm == "F":
                    r = predict_files.predict_from_files(net, p_images, out_paths=outs["F"], label_format=cfg["fmt"], max_size=cfg["max_size"], mean=MEAN,
                                                         std=STD, batch_size=args.batch, n_workers=workers, compress_level=args.compress_level,
                                                         instance=cfg["instance"], image_ids=list(range(args.images)))
                    n_preds = len(r["instance_predictions"])
                else:
                    host_ceiling(p_images, outs["F"], outs["T"], workers, args.compress_level)
                    n_preds = 0
                torch.cuda.synchronize()
                return time.perf_counter() - t, n_preds

            order = [a for a in ("L", "F", "T") if a in arms]           # T after F: it reads F's files
            for a in order:                                             # warm-up: one untimed pass per arm (graph captures, allocator, page cache)
                run(a)
            secs, n_preds = {a: [] for a in order}, {}
            for r in range(args.rounds):
                for a in order:
                    dt, n_preds[a] = run(a)
                    secs[a].append(dt)
                    print(f"{name} round {r} arm {a}: {dt:.3f} s = {args.images / dt:.1f} images/s", flush=True)
            out["arms"] = {}
            for a in order:
                rates = [args.images / s for s in secs[a]]
                out["arms"][a] = {"images_per_s": round(args.images / statistics.median(secs[a]), 1),
                                  "ms_per_image": round(1000 * statistics.median(secs[a]) / args.images, 3),
                                  "seconds_rounds": [round(v, 3) for v in secs[a]], "images_per_s_min": round(min(rates), 1),
                                  "images_per_s_max": round(max(rates), 1), "instance_predictions": n_preds[a]}
            if "L" in out["arms"] and "F" in out["arms"]:
                L, F = out["arms"]["L"], out["arms"]["F"]
                out["F_over_L"] = round(F["images_per_s"] / L["images_per_s"], 3)
                out["L_spread"] = round(L["images_per_s_max"] / L["images_per_s_min"], 3)              # L against itself, the same process
                out["F_clears_L"] = bool(F["images_per_s_min"] > L["images_per_s_max"])                # every round of F above every round of L
                differ = sum(int((np.asarray(Image.open(a)) != np.asarray(Image.open(b))).sum()) for a, b in zip(outs["L"], outs["F"]))
                out["label_bytes_differing"] = differ                                                  # batch 1 against batch B: reported, not required
        if not args.no_kernel_ab:
            w0, h0 = cfg["sizes"][0] if cfg["max_size"] is None else (1024, 768)
            lo_h, lo_w = 2 * (h0 // mcfg.patch), 2 * (w0 // mcfg.patch)                                # the decoder's x2-upsampled token grid
            out["kernel_ab"] = [kernel_ab(cfg, dev, B, lo_h, lo_w, h0, w0) for B in (1, args.batch)]
        res["configs"][name] = out
        del net
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
