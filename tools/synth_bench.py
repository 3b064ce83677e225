"""Developer tool: training samples as the training loop gets them — image + pseudo-mask files in, collate_fn batches out — on a
seeded corpus of JPEGs, with the reference's defaults (crop 384, 1 - 10 objects per sample, batch 8).

    python tools/synth_bench.py [--arm H|P|D|T ...] [--rounds R] [--images N] [--batches K] [--batch B] [--workers W]
                                [--corpus DIR] [--out FILE.json]

Arms, ALTERNATED in one process (round r runs every arm once on the SAME recipes), medians and spread over the rounds:
  H  the host restatement chain (zutis_amd.synth.sample_np, NumPy; the resize by Pillow itself) in W worker PROCESSES, whole samples
     sent back to the parent.  torchvision and cv2 are not installed, so this is the closest available stand-in for the reference's
     DataLoader over IndexDataset.__getitem__ — it is NOT the reference: its photometric ops and its float64 blur are NumPy where the
     reference runs Pillow's and OpenCV's C code.
  P  the same chain with Pillow's own C routines wherever the reference calls them (Image.resize, ImageEnhance, convert("HSV"));
     the blur is ImageFilter.GaussianBlur as a COST stand-in for cv2.GaussianBlur (other pixels).  Also a stand-in, a cheaper one.
  D  the new path end to end: TrainBatchLoader (W threads decode one batch ahead) + one copy + csrc/synth.hip, a device synchronise
     per batch.
  T  decode only: the same loader, nothing copied or launched — the ceiling of any path that decodes these files in W threads.
The worker processes come from a fork server started before the device is opened and never touch it.  Pools are sized by --workers
(at most 16), never by the machine's CPU count.  `--arm D --rounds 1` is the `rocprofv3 --kernel-trace --stats` target."""
import argparse
import json
import multiprocessing
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(500, 375)] * 6 + [(375, 500)] * 3 + [(500, 333)] * 3 + [(640, 480)] * 3 + [(1024, 768), (1600, 1200), (256, 256)]   # (w, h)
IGNORE = 255


def write_pair(k: int, corpus: str):
    from PIL import Image
    from zutis_amd import rle
    rng = np.random.default_rng(70_000 + k)
    w, h = SIZES[int(rng.integers(len(SIZES)))]
    low = rng.integers(0, 256, (max(2, h // 24), max(2, w // 24), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(low).resize((w, h), Image.BICUBIC), np.float32)
    a += rng.normal(0.0, 6.0, a.shape).astype(np.float32)
    p_image, p_mask = os.path.join(corpus, f"{k:05d}.jpg"), os.path.join(corpus, f"{k:05d}.json")
    Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(p_image, quality=90)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    cy, cx, ry, rx = h * rng.uniform(0.3, 0.7), w * rng.uniform(0.3, 0.7), h * rng.uniform(0.1, 0.35), w * rng.uniform(0.1, 0.35)
    r = rle.encode_py(((((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2) < 1.0).astype(np.uint8))
    with open(p_mask, "w") as f:
        json.dump({"size": r["size"], "counts": r["counts"].decode("ascii")}, f)
    return p_image, p_mask


def make_fields(corpus: str, n: int):
    from zutis_amd import synth
    os.makedirs(corpus, exist_ok=True)
    pairs = []
    for k in range(n):
        p = (os.path.join(corpus, f"{k:05d}.jpg"), os.path.join(corpus, f"{k:05d}.json"))
        pairs.append(p if all(os.path.exists(q) for q in p) else write_pair(k, corpus))
    p_images = [p for p, _ in pairs]
    labels = {p: 1 + i % 20 for i, p in enumerate(p_images)}
    cats = {}
    for p, l in labels.items():
        cats.setdefault(f"category{l}", []).append(p)
    return synth.DatasetFields(p_images, [m for _, m in pairs], labels, cats, IGNORE)      # the reference's defaults: 384, (0.1, 1.0), 10


# ---------------------------------------------------------------------------------------------------- host arms (worker processes)
def _pil_resize(a, nw, nh):
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((nw, nh), Image.BILINEAR))


def host_sample(recipe):
    from zutis_amd import synth
    out = synth.sample_np(recipe, resize=_pil_resize)
    return out["image"], out["semantic_mask"], out["instance_mask"]


def pillow_sample(recipe):
    """sample_np's chain with Pillow's C routines for the photometric stage and the blur (see the module docstring)."""
    from PIL import Image, ImageEnhance, ImageFilter
    from zutis_amd import preprocess, synth
    C = recipe.crop_size
    imgs, masks = [], []
    for sub in recipe.subs:
        image, mask = synth.load_files(sub)
        img, m = synth.geometry_np(image, mask, sub, C, recipe.ignore_index, _pil_resize)
        im = Image.fromarray(img)
        if sub.jitter:
            for op in sub.order:
                if op == 0:
                    im = ImageEnhance.Brightness(im).enhance(sub.brightness)
                elif op == 1:
                    im = ImageEnhance.Contrast(im).enhance(sub.contrast)
                elif op == 2:
                    im = ImageEnhance.Color(im).enhance(sub.saturation)
                else:
                    h, s, v = im.convert("HSV").split()
                    np_h = np.array(h, dtype=np.uint8)
                    np_h += np.uint8(sub.hue_shift)
                    im = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
        if sub.grey:
            im = im.convert("L").convert("RGB")
        if sub.blur:
            im = im.filter(ImageFilter.GaussianBlur(sub.sigma))
        imgs.append(np.asarray(im))
        masks.append(m)
    u8, semantic, onehot = synth.compose_np(imgs, masks, recipe)
    return synth.normalise_np(u8, preprocess.normalise_table(synth.MEAN, synth.STD)), semantic, onehot


def run_host(pool, fn, batches):
    t0 = time.perf_counter()
    n = 0
    for _ in pool.imap(fn, [r for recipes in batches for r in recipes]):     # in order, every worker busy (a DataLoader keeps 2 batches per
        n += 1                                                               # worker in flight); a sample counts once it is back in the parent
    return n / (time.perf_counter() - t0)


# --------------------------------------------------------------------------------------------------------------------- device arms
def run_device(fields, args, seed):
    import torch
    from zutis_amd import synth
    dev = torch.device("cuda:0")
    loader = synth.TrainBatchLoader(fields, args.batch, args.workers, seed, n_batches=args.batches)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    n = 0
    for out in loader.batches(dev):
        torch.cuda.synchronize(dev)
        n += out["image"].shape[0]
    return n / (time.perf_counter() - t0)


def run_decode(fields, args, seed):
    from zutis_amd import synth
    loader = synth.TrainBatchLoader(fields, args.batch, args.workers, seed, n_batches=args.batches)
    t0 = time.perf_counter()
    n = sum(len(b.recipes) for b in loader)
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", nargs="+", default=["H", "P", "D", "T"], choices=["H", "P", "D", "T"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--corpus", default=os.path.join(tempfile.gettempdir(), "zutis_synth_corpus"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.workers = max(1, min(args.workers, 16))

    pool = None
    if {"H", "P"} & set(args.arm):              # before anything opens the device: the children never see it
        pool = multiprocessing.get_context("forkserver").Pool(args.workers)
    from zutis_amd import synth
    fields = make_fields(args.corpus, args.images)
    if {"D"} & set(args.arm):
        import torch
        assert torch.cuda.is_available(), "arm D needs the GPU: there is no fallback"
        run_device(fields, argparse.Namespace(batch=args.batch, workers=args.workers, batches=2), seed=999)     # warm-up: code objects, pinned buffers
    if pool is not None:
        pool.map(host_sample, [synth.draw_recipe(random.Random(998), fields)] * args.workers)                  # warm-up: imports in every child

    rates = {a: [] for a in args.arm}
    for r in range(args.rounds):
        seed = 1000 + r
        rng = random.Random(seed)
        sizes = {}

        def size_of(p):
            if p not in sizes:
                sizes[p] = synth.image_size(p)
            return sizes[p]

        batches = [[synth.draw_recipe(rng, fields, size_of) for _ in range(args.batch)] for _ in range(args.batches)]   # the loader's own draws for this seed
        for a in args.arm:
            if a == "H":
                rates[a].append(run_host(pool, host_sample, batches))
            elif a == "P":
                rates[a].append(run_host(pool, pillow_sample, batches))
            elif a == "D":
                rates[a].append(run_device(fields, args, seed))
            else:
                rates[a].append(run_decode(fields, args, seed))
            print(f"round {r} arm {a}: {rates[a][-1]:.1f} samples/s", flush=True)
    if pool is not None:
        pool.close()
        pool.join()
    names = {"H": "host restatement chain (NumPy) in worker processes — stand-in for the reference's DataLoader, not the reference",
             "P": "the same chain on Pillow's C routines, ImageFilter blur as a cost stand-in — also a stand-in",
             "D": "TrainBatchLoader + csrc/synth.hip, end to end", "T": "decode only in threads (ceiling)"}
    result = {"tool": "synth_bench", "crop_size": fields.crop_size, "max_n_masks": fields.max_n_masks, "batch": args.batch,
              "batches_per_round": args.batches, "images": args.images, "workers": args.workers, "rounds": args.rounds,
              "arms": {a: {"what": names[a], "samples_per_s_median": statistics.median(v), "min": min(v), "max": max(v),
                           "rounds": [round(x, 2) for x in v]} for a, v in rates.items()}}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
