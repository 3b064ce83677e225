"""Developer tool: pseudo-label generation as its caller gets it — image files in, RLE JSON files out — on a seeded corpus of JPEGs.

    python tools/pseudo_files_bench.py [--arm P4|P16|D|E|G ...] [--rounds R] [--images N] [--batch B] [--workers W] [--window N]
                                       [--parent FILE] [--corpus DIR] [--out FILE.json]

Arms, ALTERNATED in one process (round r runs every arm once), medians over the rounds, a device synchronise inside every window:
  P4, P16  `dataset_generate_pseudo_masks` of the module file given with --parent (another commit's zutis_amd/pseudo_masks.py, bound
           as a sibling module of this tree's) over a MaskDataset restatement (Pillow resize + torch normalise, as
           datasets/index_dataset.py:388-411) under its DataLoader with 4 (the reference's default) and 16 worker processes, which only
           decode on the CPU — skipped without --parent
  D        this tree's `generate_pseudo_masks_from_files` (threads decode, the device resizes, shape-bucketed batches, threaded tail)
  E        `generate_pseudo_masks_batched` on resident tensors in D's shape groups: no decoding, no resize, the tail on the caller
  G        `pseudo_masks_batch` on the same resident groups and nothing else: what the device alone needs (no file is written)
Per arm: images/s, the mean number of images per SelfMask call (counted at the call), and G's time over the arm's time — the share
of the arm's wall time the device chain alone accounts for; the rest is host time the device waits through.
The corpus (written once into --corpus): N JPEGs, quality 90, the size mix of tools/extract_bench.py (500x375 / 375x500 / 500x333 /
640x480, some 1024x768, 1600x1200 and 256x256), smooth content plus noise.  Pools are sized by --workers (at most 16), never by the
machine's CPU count."""
import argparse
import functools
import importlib.util
import json
import multiprocessing.forkserver
import os
import shutil
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
from zutis_amd import detgen, ops, preprocess, pseudo_masks          # noqa: E402
from zutis_amd.engine import SelfMaskEngine                          # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SIZES = [(500, 375)] * 6 + [(375, 500)] * 3 + [(500, 333)] * 3 + [(640, 480)] * 3 + [(1024, 768), (1600, 1200), (256, 256)]   # (w, h)


def write_image(k: int, path: str):
    rng = np.random.default_rng(50_000 + k)
    w, h = SIZES[int(rng.integers(len(SIZES)))]
    low = rng.integers(0, 256, (max(2, h // 24), max(2, w // 24), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(low).resize((w, h), Image.BICUBIC), np.float32)
    a += rng.normal(0.0, 6.0, a.shape).astype(np.float32)
    Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(path, quality=90)


class MaskDataset(torch.utils.data.Dataset):
    """datasets/index_dataset.py:388-411 with Pillow + torch (torchvision is not a dependency): runs in the DataLoader's worker processes,
    on the CPU only."""

    def __init__(self, p_images, image_size=512, mean=MEAN, std=STD):
        self.p_images, self.image_size, self.mean, self.std = p_images, image_size, mean, std

    def __len__(self):
        return len(self.p_images)

    def __getitem__(self, i):
        im = Image.open(self.p_images[i]).convert("RGB")
        size = preprocess.mask_dataset_size(*im.size, self.image_size)
        if size != im.size:
            im = im.resize(size, Image.BILINEAR)
        x = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        x = (x - torch.tensor(self.mean)[:, None, None]) / torch.tensor(self.std)[:, None, None]
        return {"image": x, "p_image": self.p_images[i]}


def main():
    ARMS = ["P4", "P16", "D", "E", "G"]
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", action="append", choices=ARMS, help="repeatable (default: all; P4 / P16 need --parent)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--images", type=int, default=768)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--window", type=int, default=512)
    ap.add_argument("--image-size", type=int, default=512)
    ap.add_argument("--precision", default="exact")
    ap.add_argument("--parent", help="module file of another commit's zutis_amd/pseudo_masks.py (arms P4, P16)")
    ap.add_argument("--corpus", default=os.path.join(tempfile.gettempdir(), "zutis_pseudo_corpus"))
    ap.add_argument("--out", help="also write the result object to this JSON file")
    args = ap.parse_args()
    arms = list(dict.fromkeys(args.arm or ARMS))
    if not args.parent:
        arms = [a for a in arms if not a.startswith("P")]
    workers = max(1, min(args.workers, 16))
    # the DataLoader's workers come from a fork server that is started before this process opens the device and has the libraries loaded:
    # as cheap to start as forked workers, and no worker process ever holds the device open
    if any(a.startswith("P") for a in arms):
        torch.multiprocessing.set_start_method("forkserver")
        torch.multiprocessing.set_forkserver_preload(["torch", "numpy", "PIL.Image", "zutis_amd.preprocess"])
        multiprocessing.forkserver.ensure_running()

    def corpus(n: int):
        os.makedirs(os.path.join(args.corpus, "images"), exist_ok=True)
        paths = [os.path.join(args.corpus, "images", f"img_{k:05d}.jpg") for k in range(n)]
        todo = [(k, p) for k, p in enumerate(paths) if not os.path.exists(p)]
        with ThreadPoolExecutor(max_workers=workers) as pool:
            list(pool.map(lambda kp: write_image(*kp), todo))
        return paths

    class Owner:
        """What dataset_generate_pseudo_masks takes from the dataset object."""

        def __init__(self, dev, arm):
            self.device, self.arm = dev, arm

        def _convert_p_image_to_p_pseudo_mask(self, p_image):
            return out_path(self.arm, p_image)

    def out_path(arm, p_image):
        return os.path.join(args.corpus, "out_" + arm, os.path.basename(p_image).replace(".jpg", ".json"))

    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    paths = corpus(args.images)
    corpus_s = time.perf_counter() - t0
    sizes_wh = [Image.open(p).size for p in paths]
    sizes_hw = [(h, w) for w, h in sizes_wh]
    engine = SelfMaskEngine({k: torch.from_numpy(v).to(dev) for k, v in detgen.selfmask_state_dict().items()}, precision=args.precision)
    groups = preprocess.bucket_batches([preprocess.mask_dataset_size(w, h, args.image_size) for w, h in sizes_wh], args.batch, args.window)
    calls = []                                                            # images per SelfMask call of the arm that is running

    def counted(fn):
        def wrapper(eng, images, *a, **k):
            calls.append(int(images.shape[0]))
            return fn(eng, images, *a, **k)
        return wrapper

    pseudo_masks._device_masks_batch = counted(pseudo_masks._device_masks_batch)
    parent = None
    if any(a.startswith("P") for a in arms):
        spec = importlib.util.spec_from_file_location("zutis_amd._parent_pseudo_masks", args.parent)      # its relative imports find this package
        parent = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = parent
        spec.loader.exec_module(parent)
        parent.pseudo_masks_batch = counted(parent.pseudo_masks_batch)

    resident = None
    if "E" in arms or "G" in arms:                                        # D's groups as tensors on the device, made by the product kernel
        lut = torch.from_numpy(preprocess.normalise_table(MEAN, STD)).to(dev)
        by_first = {}
        for b in preprocess.ShapeBucketLoader(paths, args.image_size, args.batch, workers, window=args.window):
            packed, desc = preprocess.split_staging(b.staging.to(dev), len(b.paths))
            by_first[b.indices[0]] = ops.resize_normalize(packed, desc, *b.out_hw, lut, kmax=b.kmax)
        resident = [by_first[g[0]] for g in groups]
        torch.cuda.synchronize()

    def run(arm, some=None):
        """One timed pass of `arm` over the corpus (or over the first `some` images: warm-up)."""
        n = len(paths) if some is None else some
        ps = paths[:n]
        shutil.rmtree(os.path.join(args.corpus, "out_" + arm), ignore_errors=True)
        calls.clear()
        torch.cuda.synchronize(); t = time.perf_counter()
        if arm.startswith("P"):
            parent.dataset_generate_pseudo_masks(Owner(dev, arm), ps, args.corpus, int(arm[1:]), True, batch_size=args.batch, network=engine,
                                                 mask_dataset_cls=functools.partial(MaskDataset, image_size=args.image_size))
        elif arm == "D":
            pseudo_masks.generate_pseudo_masks_from_files(engine, ps, [out_path(arm, p) for p in ps], image_size=args.image_size, mean=MEAN, std=STD,
                                                          batch_size=args.batch, n_workers=workers, window=args.window)
        else:
            for g, x in zip(groups, resident):
                if g[0] >= n:
                    continue
                if arm == "E":
                    pseudo_masks.generate_pseudo_masks_batched(engine, list(x), [sizes_hw[i] for i in g], [out_path(arm, paths[i]) for i in g],
                                                               batch_size=args.batch)
                else:
                    pseudo_masks.pseudo_masks_batch(engine, x, [sizes_hw[i] for i in g], True)
        torch.cuda.synchronize()
        return time.perf_counter() - t, list(calls)

    engine.to = lambda d: engine                                          # the adapter's network.to(device) / .eval(): the engine is in place
    engine.eval = lambda: None
    secs, per_call = {a: [] for a in arms}, {}
    for a in arms:                                                        # warm-up: every shape of the corpus once per arm
        run(a, some=min(len(paths), 8 * args.batch))
    for r in range(args.rounds):
        for a in arms:
            dt, c = run(a)
            secs[a].append(dt)
            per_call[a] = c
            print(f"round {r} arm {a}: {dt:.3f} s = {len(paths) / dt:.1f} images/s, {len(c)} SelfMask calls", flush=True)

    res = {"tool": "pseudo_files_bench", "images": len(paths), "batch": args.batch, "window": args.window, "image_size": args.image_size,
           "precision": args.precision, "n_workers": workers, "dataloader_start_method": "forkserver", "rounds": args.rounds, "pillow": Image.__version__,
           "cpus_in_use": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None,
           "corpus": {"files": len(paths), "jpeg_bytes": sum(os.path.getsize(p) for p in paths), "decoded_bytes": int(sum(3 * w * h for w, h in sizes_wh)),
                      "resized_shapes": len({tuple(x.shape[2:]) for x in resident}) if resident else None, "written_in_s": round(corpus_s, 1)},
           "arms": {}}
    for a in arms:
        med = statistics.median(secs[a])
        rates = [len(paths) / s for s in secs[a]]
        res["arms"][a] = {"images_per_s": round(len(paths) / med, 1), "seconds_rounds": [round(v, 3) for v in secs[a]],
                          "images_per_s_min": round(min(rates), 1), "images_per_s_max": round(max(rates), 1),
                          "spread_images_per_s": round(max(rates) - min(rates), 1),
                          "selfmask_calls": len(per_call[a]), "mean_images_per_selfmask_call": round(sum(per_call[a]) / max(1, len(per_call[a])), 2)}
    A = res["arms"]
    if "G" in A:
        for a in arms:
            A[a]["device_chain_share_of_wall"] = round(statistics.median(secs["G"]) / statistics.median(secs[a]), 3)
    P = [a for a in ("P4", "P16") if a in A]
    if P and "D" in A:
        best = max(P, key=lambda a: A[a]["images_per_s"])
        margin = max(A[best]["spread_images_per_s"], A["D"]["spread_images_per_s"])
        res["best_P"], res["D_minus_best_P_images_per_s"] = best, round(A["D"]["images_per_s"] - A[best]["images_per_s"], 1)
        res["margin_images_per_s"] = margin                                # the larger round-to-round spread (max - min) of the two arms
        res["D_clears_best_P"] = bool(A["D"]["images_per_s"] - A[best]["images_per_s"] > margin)
        res["D_over_best_P"] = round(A["D"]["images_per_s"] / A[best]["images_per_s"], 3)
    if "D" in A and "E" in A:
        res["D_over_E"] = round(A["D"]["images_per_s"] / A["E"]["images_per_s"], 3)
        res["D_files_equal_E_files"] = all(open(out_path("D", p), "rb").read() == open(out_path("E", p), "rb").read() for p in paths)
    if "D" in A and "G" in A:
        res["D_over_G"] = round(A["D"]["images_per_s"] / A["G"]["images_per_s"], 3)
    if P and "D" in A:                                                     # different groupings: reported, not required (the key split depends on the batch)
        res["files_equal_D_vs_" + P[0]] = sum(open(out_path("D", p), "rb").read() == open(out_path(P[0], p), "rb").read() for p in paths)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":       # the DataLoader's worker processes import this file for MaskDataset: nothing else runs there
    main()
