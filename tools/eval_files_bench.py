"""Developer tool: evaluation as its caller gets it — image files and ground-truth PNGs in, scores out — on a seeded corpus written here.

    python tools/eval_files_bench.py [--config coco|imagenet ...] [--arm L|F ...] [--rounds R] [--images N] [--batch B] [--workers W]
                                     [--model vitb16|tiny] [--no-kernel-ab] [--corpus DIR] [--out FILE.json]

Configs:
  coco      640x480 / 480x640 JPEGs, 81 classes, 8-bit grey ground truth ("u8"), no resize, instance predict on (trainer.py:335-345)
  imagenet  500x375 ... 1600x1200 JPEGs capped at 1024 on the longer edge, 920 classes, RGB ground truth R + 256 G ("rg16"), scored at the
            file's own size (imagenet_s.py:63-99, trainer.py:322-325)
Arms, ALTERNATED in one process (round r runs every arm once), medians and spreads over the rounds, a device synchronise in every window:
  L  the loop as it was before evaluate_from_files: a DataLoader(batch_size=1, num_workers=W) over a restatement of the dataset (Pillow +
     torch: decode, cap, to_tensor, normalize, ground truth as int64), then network(image) -> predict("semantic") to NumPy ->
     RunningScore.update with NumPy arrays -> predict("instance") (coco)
  F  zutis_amd.evaluate.evaluate_from_files
Kernel A/B (per config, HIP events, the ground truth resident): zh_upsample_argmax_score against what it replaces on the device —
zh_upsample_argmax + the int64 conversions of ground truth and prediction + zh_confusion_hist — on a blocky (natural) and on a uniformly
random ground truth.  The host-to-device uploads and the label map's copy to the host that the loop pays are NOT in the chain's time."""
import argparse
import json
import multiprocessing.forkserver
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
sys.path.insert(0, os.path.join(ROOT, "zutis_amd", "dropin"))
from zutis_amd import detgen, evaluate, ops, preprocess          # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CONFIGS = {   # (w, h) mix, classes, ground-truth format, max_size, instance predict, ignore label
    "coco": dict(sizes=[(640, 480)] * 3 + [(480, 640)], n=81, fmt="u8", max_size=None, instance=True, ignore=255),
    "imagenet": dict(sizes=[(500, 375)] * 3 + [(375, 500)] * 2 + [(1024, 768), (1600, 1200), (800, 1066)], n=920, fmt="rg16", max_size=1024,
                     instance=False, ignore=1000),
}


def blocky_labels(rng, h, w, n, ignore, classes=4, cell=48):
    """A label map as an annotated photograph has it: a few classes in large cells, a thin ignore band between some of them."""
    pick = rng.choice(n, size=classes, replace=False)
    v = np.kron(pick[rng.integers(0, classes, (-(-h // cell), -(-w // cell)))], np.ones((cell, cell), np.int64))[:h, :w]
    v[::cell, :] = ignore
    return v


def gt_bytes(v, fmt, rng):
    if fmt == "u8":
        return v.astype(np.uint8)
    return np.stack([v & 255, v >> 8, rng.integers(0, 256, v.shape)], axis=-1).astype(np.uint8)


def write_pair(cfg, k, p_image, p_gt):
    rng = np.random.default_rng(70_000 + k)
    w, h = cfg["sizes"][int(rng.integers(len(cfg["sizes"])))]
    low = rng.integers(0, 256, (max(2, h // 24), max(2, w // 24), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(low).resize((w, h), Image.BICUBIC), np.float32)
    a += rng.normal(0.0, 6.0, a.shape).astype(np.float32)
    Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(p_image, quality=90)
    Image.fromarray(gt_bytes(blocky_labels(rng, h, w, cfg["n"], cfg["ignore"]), cfg["fmt"], rng)).save(p_gt, compress_level=1)


class ValDataset(torch.utils.data.Dataset):
    """coco2017.py:121-149 / imagenet_s.py:63-99 with Pillow + torch (torchvision is not a dependency): runs in the DataLoader's worker
    processes, on the CPU only."""

    def __init__(self, p_images, p_gts, fmt, max_size):
        self.p_images, self.p_gts, self.fmt, self.max_size = p_images, p_gts, fmt, max_size

    def __len__(self):
        return len(self.p_images)

    def __getitem__(self, i):
        im = Image.open(self.p_images[i]).convert("RGB")
        W, H = im.size
        size = preprocess.longer_edge_size(W, H, self.max_size)
        if size != im.size:
            im = im.resize(size, Image.BILINEAR)
        x = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        x = (x - torch.tensor(MEAN)[:, None, None]) / torch.tensor(STD)[:, None, None]
        gt = np.array(Image.open(self.p_gts[i])).astype(np.int64)
        if self.fmt == "rg16":
            gt = gt[..., 0] + gt[..., 1] * 256
        return {"image": x, "semantic_mask": torch.from_numpy(gt).to(torch.int64), "original_size": (H, W), "image_id": i}


def network_of(model, n, dev):
    from networks.zutis import ZUTIS
    cfg = {"tiny": detgen.TINY, "vitb16": detgen.VIT_B16}[model]
    net = ZUTIS(categories=[f"c{i}" for i in range(n)], clip_arch="ViT-B/16", n_queries=cfg.n_queries, n_decoder_layers=cfg.dec_layers,
                n_heads=cfg.dec_heads, device=dev, text_embeddings=torch.from_numpy(detgen.text_embeddings(n, cfg.embed_dim)),
                vision_config=(cfg.width, cfg.layers, cfg.patch, cfg.grid, cfg.embed_dim))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in detgen.zutis_state_dict(cfg).items()}, strict=True)
    return net.to(dev).eval().requires_grad_(False), cfg


def loop_as_it_was(net, dev, loader, n, instance):
    """trainer.evaluate's loop body, trainer.py:316-347."""
    from utils.running_score import RunningScore
    meter, preds = RunningScore(n_classes=n, device=dev), []
    with torch.no_grad():
        for d in loader:
            image, gts = d["image"], d["semantic_mask"].cpu().numpy()
            H, W = (int(v) for v in d["original_size"])
            out = net(image.to(dev))
            sem = net.predict(dict_outputs=out, mask_type="semantic", size=(H, W))
            if instance:
                preds.extend(net.predict(dict_outputs=out, mask_type="instance", size=(H, W), image_ids=[int(d["image_id"])], nms_type="hard"))
            meter.update(gts, sem)
    return meter.confusion_matrix, preds


def kernel_ab(cfg, dev, B, h, w, H, W, iters=50, repeats=5):
    """us per call of the fused kernel and of the chain it replaces, medians of `repeats` timings of `iters` calls each."""
    n, fmt, rng = cfg["n"], cfg["fmt"], np.random.default_rng(1)
    g = torch.Generator().manual_seed(3)
    coarse = torch.randn((B, n, max(2, h // 6), max(2, w // 6)), generator=g)
    lo = (torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear") * 4 + torch.randn((B, n, h, w), generator=g) * 0.1).to(dev).contiguous()
    out = {}
    for kind in ("blocky", "random"):
        v = np.stack([blocky_labels(rng, H, W, n, cfg["ignore"]) if kind == "blocky" else rng.integers(0, n, (H, W)) for _ in range(B)])
        gt = torch.from_numpy(gt_bytes(v, fmt, rng)).to(dev)
        hist_f, hist_c = torch.zeros(n * n, dtype=torch.int64, device=dev), torch.zeros(n * n, dtype=torch.int64, device=dev)
        labels = torch.empty((B, H, W), dtype=torch.int64, device=dev)

        def fused():
            ops.upsample_argmax_score(lo, gt, hist_f, B, n, h, w, H, W, gt_format=fmt)

        def chain():
            ops.upsample_argmax(lo, labels, B, n, h, w, H, W)
            t = gt.to(torch.int64) if fmt == "u8" else gt[..., 0].to(torch.int64) + gt[..., 1].to(torch.int64) * 256
            ops.confusion_hist(t.reshape(-1).contiguous(), labels.to(torch.int64).reshape(-1), hist_c, n)

        fused(); chain()
        torch.cuda.synchronize()
        equal = bool(torch.equal(hist_f, hist_c))
        us = {}
        for name, fn in (("fused", fused), ("chain", chain)):
            ts = []
            for _ in range(repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters):
                    fn()
                b.record(); b.synchronize()
                ts.append(a.elapsed_time(b) * 1000.0 / iters)
            us[name] = {"median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)}
        distinct = int(len(np.unique(v[v < n])))
        out[kind] = {"fused": us["fused"], "chain": us["chain"], "chain_over_fused": round(us["chain"]["median_us"] / us["fused"]["median_us"], 3),
                     "histograms_equal": equal, "gt_classes": distinct}
    return {"B": B, "n": n, "gt_format": fmt, "lowres": [h, w], "size": [H, W], **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--arm", action="append", choices=["L", "F"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--images", type=int, default=96)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--model", default="vitb16", choices=["vitb16", "tiny"])
    ap.add_argument("--no-kernel-ab", action="store_true")
    ap.add_argument("--corpus", default=os.path.join(tempfile.gettempdir(), "zutis_eval_corpus"))
    ap.add_argument("--out", help="also write the result object to this JSON file")
    args = ap.parse_args()
    configs, arms = list(dict.fromkeys(args.config or sorted(CONFIGS))), list(dict.fromkeys(args.arm or ["L", "F"]))
    workers = max(1, min(args.workers, 16))
    if "L" in arms:     # the DataLoader's workers come from a fork server started before this process opens the device: none ever holds it open
        torch.multiprocessing.set_start_method("forkserver")
        torch.multiprocessing.set_forkserver_preload(["torch", "numpy", "PIL.Image", "zutis_amd.preprocess"])
        multiprocessing.forkserver.ensure_running()
    dev = torch.device("cuda:0")
    res = {"tool": "eval_files_bench", "model": args.model, "images": args.images, "batch": args.batch, "n_workers": workers, "rounds": args.rounds,
           "pillow": Image.__version__, "cpus_in_use": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None, "configs": {}}
    for name in configs:
        cfg = CONFIGS[name]
        d = os.path.join(args.corpus, name)
        os.makedirs(d, exist_ok=True)
        p_images = [os.path.join(d, f"img_{k:05d}.jpg") for k in range(args.images)]
        p_gts = [os.path.join(d, f"gt_{k:05d}.png") for k in range(args.images)]
        todo = [k for k in range(args.images) if not (os.path.exists(p_images[k]) and os.path.exists(p_gts[k]))]
        with ThreadPoolExecutor(max_workers=workers) as pool:
            list(pool.map(lambda k: write_pair(cfg, k, p_images[k], p_gts[k]), todo))
        net, mcfg = network_of(args.model, cfg["n"], dev)

        # L's worker processes are started ONCE, outside the timed windows (persistent workers): a real evaluation starts them once for
        # thousands of images, and a corpus of this size must not charge that start-up to every round
        loader = None
        if "L" in arms:
            loader = torch.utils.data.DataLoader(ValDataset(p_images, p_gts, cfg["fmt"], cfg["max_size"]), batch_size=1, num_workers=workers,
                                                 pin_memory=True, persistent_workers=True)

        def run(arm):
            torch.cuda.synchronize(); t = time.perf_counter()
            if arm == "L":
                cm, preds = loop_as_it_was(net, dev, loader, cfg["n"], cfg["instance"])
            else:
                r = evaluate.evaluate_from_files(net, p_images, p_gts, cfg["n"], gt_format=cfg["fmt"], max_size=cfg["max_size"], mean=MEAN, std=STD,
                                                 batch_size=args.batch, n_workers=workers, instance=cfg["instance"], image_ids=list(range(args.images)))
                cm, preds = r["confusion_matrix"], r["instance_predictions"]
            torch.cuda.synchronize()
            return time.perf_counter() - t, cm, len(preds)

        for a in arms:                                          # warm-up: one untimed pass per arm (worker start-up, graph captures, allocator)
            run(a)
        secs, cms, n_preds = {a: [] for a in arms}, {}, {}
        for r in range(args.rounds):
            for a in arms:
                dt, cms[a], n_preds[a] = run(a)
                secs[a].append(dt)
                print(f"{name} round {r} arm {a}: {dt:.3f} s = {args.images / dt:.1f} images/s", flush=True)
        out = {"classes": cfg["n"], "gt_format": cfg["fmt"], "max_size": cfg["max_size"], "instance": cfg["instance"], "sizes_wh": sorted(set(cfg["sizes"])),
               "arms": {}}
        for a in arms:
            rates = [args.images / s for s in secs[a]]
            out["arms"][a] = {"images_per_s": round(args.images / statistics.median(secs[a]), 1), "ms_per_image": round(1000 * statistics.median(secs[a]) / args.images, 3),
                              "seconds_rounds": [round(v, 3) for v in secs[a]], "images_per_s_min": round(min(rates), 1), "images_per_s_max": round(max(rates), 1),
                              "instance_predictions": n_preds[a], "pixels_counted": int(cms[a].sum())}
        if "L" in out["arms"] and "F" in out["arms"]:
            L, F = out["arms"]["L"], out["arms"]["F"]
            out["F_over_L"] = round(F["images_per_s"] / L["images_per_s"], 3)
            out["F_clears_L"] = bool(F["images_per_s_min"] > L["images_per_s_max"])              # every round of F above every round of L
            out["confusion_bins_differing"] = int((cms["L"] != cms["F"]).sum())                  # batch 1 against batch B: reported, not required
        if not args.no_kernel_ab:
            w0, h0 = cfg["sizes"][0] if cfg["max_size"] is None else (1024, 768)
            lo_h, lo_w = 2 * (h0 // mcfg.patch), 2 * (w0 // mcfg.patch)                          # the decoder's x2-upsampled token grid
            out["kernel_ab"] = [kernel_ab(cfg, dev, B, lo_h, lo_w, h0, w0) for B in (1, args.batch)]
        res["configs"][name] = out
        del net, loader                                         # the workers end with their loader
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":       # the DataLoader's worker processes import this file for ValDataset: nothing else runs there
    main()
