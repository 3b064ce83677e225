"""Developer tool: the mask post-processing of bilateral_solver_output (utils/bilateral_solver.py:185-193) on the host and on the device.

    python tools/components_bench.py [--rounds R] [--reps N] [--images N] [--batch B] [--workers W] [--corpus DIR]
                                     [--out profiles/components_ab.json]

Arms ALTERNATED in one process (round r runs every arm once), medians and ranges over the rounds, a device synchronise inside every window:
  (a) the post-processing alone at 512 x 683 for B = 1 and 8, on the soft output of a solve of detgen.selfmask_like_rgb ("blob") and on
      the same output with 0.1 % of its pixels flipped across the threshold ("flips"):
        host    the float64 soft output copied back + the drop-in's _postprocess (scipy.ndimage), image by image
        device  ops.second_largest_component on the resident soft output + the 1-byte mask copied back
  (b) the drop-in's bilateral_solver_output end to end (PIL image and target in, soft output and mask out) with postprocess="host" / "device"
  (c) generate_pseudo_masks_from_files on the corpus of tools/pseudo_files_bench.py (--images of it) without and with
      component="second_largest": what the option costs the driver
Per pair: both medians, both ranges, whether the device arm was ahead in every round, and whether the ranges are disjoint."""
import argparse
import json
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
sys.path.insert(0, os.path.join(ROOT, "zutis_amd", "dropin"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from zutis_amd import components, detgen, ops, pseudo_masks          # noqa: E402
from zutis_amd.engine import SelfMaskEngine                          # noqa: E402
from utils import bilateral_solver as dropin                         # noqa: E402
import pseudo_files_bench as corpus_tool                             # noqa: E402

H, W = 512, 683


def pair(secs_a, secs_b, name_a, name_b, unit_scale=1e3):
    """The record of two alternated arms: medians, ranges (ms), b ahead in every round, ranges disjoint."""
    ra, rb = [s * unit_scale for s in secs_a], [s * unit_scale for s in secs_b]
    return {name_a + "_ms": round(statistics.median(ra), 4), name_a + "_range_ms": [round(min(ra), 4), round(max(ra), 4)],
            name_b + "_ms": round(statistics.median(rb), 4), name_b + "_range_ms": [round(min(rb), 4), round(max(rb), 4)],
            name_b + "_ahead_every_round": all(b < a for a, b in zip(ra, rb)), "ranges_disjoint": max(rb) < min(ra) or max(ra) < min(rb),
            name_a + "_over_" + name_b: round(statistics.median(ra) / statistics.median(rb), 2)}


def timed(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed window of (a) and (b)")
    ap.add_argument("--images", type=int, default=256, help="files of the corpus used in (c)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--corpus", default=os.path.join(tempfile.gettempdir(), "zutis_pseudo_corpus"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_ab.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    workers = max(1, min(args.workers, 16))
    res = {"tool": "components_bench", "H": H, "W": W, "rounds": args.rounds, "reps_per_window": args.reps, "postprocess_alone": {}}

    # ---- (a) the post-processing alone
    rgb = detgen.selfmask_like_rgb(H, W, seed=3)
    yy, xx = np.mgrid[:H, :W]
    target = ((((yy - 250) / 150.0) ** 2 + ((xx - 340) / 220.0) ** 2) < 1.0).astype(np.uint8)
    soft, _ = ops.bilateral_solve(torch.from_numpy(rgb).to(dev), torch.from_numpy(target).to(dev))
    blob = soft.cpu().numpy()
    flips = blob.copy()
    flip = np.random.default_rng(11).random((H, W)) < 0.001
    flips[flip] = 1.0 - flips[flip]                                       # across the threshold of 0.5
    for name, img in (("blob", blob), ("flips", flips)):
        _, _, _, st = components.components_np(img)
        for B in (1, 8):
            x = torch.from_numpy(np.stack([img] * B)).to(dev)
            ws = torch.empty(B * ops.components_workspace_size(H, W), dtype=torch.uint8, device=dev)
            out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)

            def host():
                s = x.cpu().numpy()
                return [dropin._postprocess(s[b]) for b in range(B)]

            def device():
                return ops.second_largest_component(x, workspace=ws, out=out).cpu().numpy()

            same = all(np.array_equal(h, d.astype(bool)) for h, d in zip(host(), device()))
            device()
            hs, ds = [], []
            for _ in range(args.rounds):
                hs.append(timed(host, 1 if name == "flips" else args.reps))
                ds.append(timed(device, args.reps))
            rec = pair(hs, ds, "host", "device")
            rec.update({"components_after_filling": int(st[0]), "tie": components.has_tie(img), "masks_equal": same})
            res["postprocess_alone"][f"{name}_B{B}"] = rec
            print(name, B, rec, flush=True)

    # ---- (b) the drop-in end to end
    img = Image.fromarray(rgb)
    for p in ("host", "device"):
        dropin.bilateral_solver_output(img, target, postprocess=p)
    hs, ds = [], []
    for _ in range(args.rounds):
        hs.append(timed(lambda: dropin.bilateral_solver_output(img, target, postprocess="host"), args.reps))
        ds.append(timed(lambda: dropin.bilateral_solver_output(img, target, postprocess="device"), args.reps))
    res["bilateral_solver_output"] = pair(hs, ds, "host", "device")
    print("dropin", res["bilateral_solver_output"], flush=True)

    # ---- (c) the file driver without / with the option
    os.makedirs(os.path.join(args.corpus, "images"), exist_ok=True)
    paths = [os.path.join(args.corpus, "images", f"img_{k:05d}.jpg") for k in range(args.images)]
    with ThreadPoolExecutor(max_workers=workers) as pool:
        list(pool.map(lambda kp: corpus_tool.write_image(*kp), [(k, p) for k, p in enumerate(paths) if not os.path.exists(p)]))
    engine = SelfMaskEngine({k: torch.from_numpy(v).to(dev) for k, v in detgen.selfmask_state_dict().items()})

    def files(component, n=None):
        ps = paths[:n]
        d = os.path.join(args.corpus, "out_components_" + str(component))
        shutil.rmtree(d, ignore_errors=True)
        outs = [os.path.join(d, os.path.basename(p).replace(".jpg", ".json")) for p in ps]
        torch.cuda.synchronize()
        t = time.perf_counter()
        pseudo_masks.generate_pseudo_masks_from_files(engine, ps, outs, mean=corpus_tool.MEAN, std=corpus_tool.STD, batch_size=args.batch,
                                                      n_workers=workers, component=component)
        torch.cuda.synchronize()
        return time.perf_counter() - t

    for c in (None, "second_largest"):
        files(c, n=min(len(paths), 8 * args.batch))
    ns, cs = [], []
    for _ in range(args.rounds):
        ns.append(files(None))
        cs.append(files("second_largest"))
    rec = pair(ns, cs, "plain", "component", unit_scale=1.0)
    rec = {k.replace("_ms", "_s"): v for k, v in rec.items()}
    rec.update({"images": len(paths), "plain_images_per_s": round(len(paths) / statistics.median(ns), 1),
                "component_images_per_s": round(len(paths) / statistics.median(cs), 1),
                "option_costs_percent": round(100.0 * (statistics.median(cs) / statistics.median(ns) - 1.0), 2)})
    res["generate_pseudo_masks_from_files"] = rec
    print("files", rec, flush=True)
    a = list(res["postprocess_alone"].values()) + [res["bilateral_solver_output"]]
    res["device_ahead_every_round_everywhere"] = all(r["device_ahead_every_round"] for r in a)
    res["ranges_disjoint_everywhere"] = all(r["ranges_disjoint"] for r in a)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
