"""Developer tool: what a caller of the extraction drop-in gets — files in, embeddings out — on a seeded corpus of JPEGs.

    python tools/extract_bench.py [--arm P|H|D|E ...] [--rounds R] [--images N] [--batch B] [--workers W] [--precision MODE]
                                  [--parent FILE] [--corpus DIR] [--out FILE.json]

Arms, ALTERNATED in one process (round r runs every arm once), medians over the rounds, a device synchronise inside every window:
  P  `extract_image_embeddings` of the module file given with --parent (an earlier commit's drop-in: pre-processing one image after
     the other on the calling thread) — skipped without --parent
  H  the host pre-processing (`_preprocess`) of every image on a pool of W threads, then `encode_image`: what threads alone buy
  D  this tree's `extract_image_embeddings` (threads decode, the device resizes / crops / normalises)
  E  `encode_image` on a resident batch: the ceiling
P and D are whole calls, so they include building and packing the tower; that part is measured on a one-image call of the same
function and the rate net of it is reported next to the gross one (H and E run on a tower that is already packed).
The corpus (written once into --corpus, default a directory under the system's temporary directory): N JPEGs, quality 90, sizes
drawn from a fixed list weighted towards 500x375 / 375x500 / 500x333 / 640x480 with some 1024x768, 1600x1200 and 256x256, smooth
content plus noise.  Tower and weights are those of `bench.py --workload c5` (ViT-L/14@336, fp16-valued GEMM tensors).
The pool is sized by --workers (at most 16), never by the machine's CPU count."""
import argparse
import importlib.util
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
from zutis_amd import detgen, preprocess                            # noqa: E402
from zutis_amd.engine import ClipImageEncoder                       # noqa: E402
from utils import extract_image_embeddings as DROPIN                # noqa: E402
from extract_corpus import corpus, tower                            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--arm", action="append", choices=["P", "H", "D", "E"], help="repeatable (default: all four; P needs --parent)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--images", type=int, default=2048)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--workers", type=int, default=16)
ap.add_argument("--precision", default="fast")
ap.add_argument("--layers", type=int, default=24)
ap.add_argument("--parent", help="module file of another commit's utils/extract_image_embeddings.py (arm P)")
ap.add_argument("--corpus", default=os.path.join(tempfile.gettempdir(), "zutis_extract_corpus"))
ap.add_argument("--out", help="also write the result object to this JSON file")
args = ap.parse_args()
arms = list(dict.fromkeys(args.arm or ["P", "H", "D", "E"]))
if "P" in arms and not args.parent:
    arms.remove("P")
workers = max(1, min(args.workers, 16))

dev = torch.device("cuda:0")
t0 = time.perf_counter()
paths = corpus(args.corpus, args.images, workers)
corpus_s = time.perf_counter() - t0
sizes = [Image.open(p).size for p in paths]
file_bytes = sum(os.path.getsize(p) for p in paths)
sd, patch = tower(dev, args.layers)
n_px = 336
parent = None
if "P" in arms:
    spec = importlib.util.spec_from_file_location("parent_extract_image_embeddings", args.parent)
    parent = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(parent)


def whole_call(mod, some_paths):
    torch.cuda.synchronize(); t = time.perf_counter()
    out = mod.extract_image_embeddings(some_paths, model_name="ViT-L/14@336px", device=dev, batch_size=args.batch, n_workers=workers,
                                       state_dict=sd, precision=args.precision)
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


enc = ClipImageEncoder(sd, patch, prefix="visual.", precision=args.precision)
resident = torch.randn((args.batch, 3, n_px, n_px), generator=torch.Generator(device="cpu").manual_seed(2000)).to(dev)
enc.encode_image(resident)
torch.cuda.synchronize()


def arm_H():
    torch.cuda.synchronize(); t = time.perf_counter()
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for i in range(0, len(paths), args.batch):
            x = torch.from_numpy(np.stack(list(pool.map(lambda p: DROPIN._preprocess(p, n_px), paths[i:i + args.batch])))).to(dev)
            enc.encode_image(x).cpu()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def arm_E():
    steps = (len(paths) + args.batch - 1) // args.batch
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(steps):
        enc.encode_image(resident)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * len(paths) / (steps * args.batch)


secs = {a: [] for a in arms}
setup = {a: [] for a in arms if a in "PD"}
ref_out = {}
for a in setup:                                        # warm-up of both functions + the part of a call that is not the loop
    for _ in range(2):
        setup[a].append(whole_call(parent if a == "P" else DROPIN, paths[:1])[0])
for r in range(args.rounds):
    for a in arms:
        if a in "PD":
            dt, out = whole_call(parent if a == "P" else DROPIN, paths)
            ref_out[a] = out
        else:
            dt = arm_H() if a == "H" else arm_E()
        secs[a].append(dt)
        print(f"round {r} arm {a}: {dt:.3f} s = {len(paths) / dt:.1f} images/s", flush=True)

res = {"tool": "extract_bench", "images": len(paths), "batch": args.batch, "precision": args.precision, "layers": args.layers,
       "n_workers": workers, "cpus_in_use": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None,
       "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "rounds": args.rounds, "pillow": Image.__version__,
       "corpus": {"files": len(paths), "jpeg_bytes": file_bytes, "decoded_bytes": int(sum(3 * w * h for w, h in sizes)),
                  "written_in_s": round(corpus_s, 1)}, "arms": {}}
for a in arms:
    med = statistics.median(secs[a])
    e = {"images_per_s": round(len(paths) / med, 1), "seconds_rounds": [round(v, 3) for v in secs[a]],
         "images_per_s_min": round(len(paths) / max(secs[a]), 1), "images_per_s_max": round(len(paths) / min(secs[a]), 1),
         "spread_pct": round((max(secs[a]) - min(secs[a])) / med * 100, 2)}
    if a in setup:
        s = min(setup[a])
        e["setup_s"] = round(s, 3)
        e["images_per_s_net_of_setup"] = round(len(paths) / (med - s), 1)
    res["arms"][a] = e
if "P" in ref_out and "D" in ref_out:
    res["D_equals_P_bitwise"] = bool(list(ref_out["P"]) == list(ref_out["D"]) and
                                     all(torch.equal(ref_out["P"][k], ref_out["D"][k]) for k in ref_out["P"]))
A = res["arms"]
for x, y in (("D", "P"), ("D", "E"), ("D", "H")):
    if x in A and y in A:
        res[f"{x}_over_{y}"] = round(A[x]["images_per_s"] / A[y]["images_per_s"], 3)
        if "images_per_s_net_of_setup" in A[x]:
            res[f"{x}_over_{y}_net_of_setup"] = round(A[x]["images_per_s_net_of_setup"] / A[y].get("images_per_s_net_of_setup", A[y]["images_per_s"]), 3)
print(json.dumps(res), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
