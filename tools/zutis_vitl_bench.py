"""ZUTIS over the full-depth ViT-L/14@336px tower (24 + 6 layers, width 1024, decoder head dim 128) on the HIP engine (developer tool):
forward + semantic predict of a batch of 336 x 336 images in images/s, `exact` and `fast`, against benchlib.baselines.torch_gpu_baseline
— the reference's op sequence in stock PyTorch fp32 eager on the same GPU and weights, the baseline the headline figures are quoted
against.

    python tools/zutis_vitl_bench.py [--batch 8] [--classes 81] [--rounds 5] [--steps 5] [--out profiles/zutis_vitl_ab.json]

Per round: the baseline, `exact`, `fast`, in that order (alternated over the rounds); the JSON holds every round, the medians and the
spreads.  Outside the timed region the engine's outputs for the first image are checked against the CPU oracle (oracle/zutis_ref.py) once
per precision.  Weights and inputs are zutis_amd.detgen draws (VIT_L14_336); nothing outside the repository is read."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from benchlib.baselines import torch_gpu_baseline
from zutis_amd import detgen
from zutis_amd.engine import ZutisEngine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--classes", type=int, default=81)
    ap.add_argument("--size", type=int, default=336)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=None, help="encoder depth (default: the full 24; 6 decoder layers either way)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = detgen.VIT_L14_336 if a.layers is None else detgen.ZutisConfig(width=1024, layers=a.layers, patch=14, grid=24, embed_dim=768)
    dev = torch.device("cuda:0")
    B, S, n = a.batch, a.size, a.classes
    t0 = time.perf_counter()
    sd = detgen.zutis_state_dict(cfg)
    P = {k: torch.from_numpy(v).to(dev) for k, v in sd.items()}
    print(f"{sum(v.size for v in sd.values()) / 1e6:.0f} M parameters drawn in {time.perf_counter() - t0:.1f} s", flush=True)
    x = torch.from_numpy(detgen.images(B, S, S)).to(dev)
    text = torch.from_numpy(detgen.text_embeddings(n, cfg.embed_dim)).to(dev)

    # the oracle for image 0 (CPU, fp32), once
    from oracle import zutis_ref as O
    from oracle.parity import unexplained_label_mismatches
    with torch.no_grad():
        ref = O.zutis_forward(O.to_torch_params(sd), x[:1].cpu(), cfg.patch, cfg.dec_heads)
        lo_ref = O.semantic_logits_lowres(ref["patch_tokens"], text.cpu()).numpy()
        lab_ref = O.predict_semantic(ref["patch_tokens"], text.cpu(), (S, S))
    del sd

    engines, parity = {}, {}
    for precision in ("exact", "fast"):
        eng = engines[precision] = ZutisEngine(P, cfg.patch, cfg.dec_heads, precision=precision)
        out = eng.forward(x[:1])
        lo = eng.semantic_logits_lowres(out["patch_tokens"], text).cpu().numpy()
        lab = eng.predict_semantic(out["patch_tokens"], text, (S, S)).cpu().numpy()
        err = float(np.abs(lo - lo_ref).max())
        e_mp = float(np.abs(out["mask_proposals"].cpu().numpy() - ref["mask_proposals"].numpy()).max())
        n_mis, n_bad, worst = unexplained_label_mismatches(lab, lab_ref, lo_ref, err, (S, S))
        parity[precision] = dict(logit_max_abs_err=err, mask_proposal_max_abs_err=e_mp, label_mismatches=n_mis, unexplained_label_mismatches=n_bad,
                                 tolerance=1e-3, against="fp32 CPU oracle, image 0 at batch 1")
        print(precision, parity[precision], flush=True)

    def hip_rate(eng):
        def step():
            out = eng.forward(x)
            return eng.predict_semantic(out["patch_tokens"], text, (S, S))
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        return B * a.steps / (time.perf_counter() - t)

    rounds = []
    for r in range(a.rounds):
        legs = [("baseline", lambda: torch_gpu_baseline(P, cfg, x, text, S, B)["value"]),
                ("exact", lambda: hip_rate(engines["exact"])), ("fast", lambda: hip_rate(engines["fast"]))]
        legs = legs[r % 3:] + legs[:r % 3]
        rec = {name: round(float(f()), 1) for name, f in legs}
        rec["order"] = [name for name, _ in legs]
        rounds.append(rec)
        print(f"round {r}: {rec}", flush=True)
    summary = {}
    for name in ("baseline", "exact", "fast"):
        v = [r[name] for r in rounds]
        summary[name] = dict(images_per_s_median=statistics.median(v), spread=round(max(v) - min(v), 1))
    summary["exact_over_baseline_rounds"] = [round(r["exact"] / r["baseline"], 2) for r in rounds]
    summary["fast_over_baseline_rounds"] = [round(r["fast"] / r["baseline"], 2) for r in rounds]
    summary["exact_faster_than_baseline_in_every_round"] = all(r["exact"] > r["baseline"] for r in rounds)
    print(summary)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/zutis_vitl_bench.py", device=torch.cuda.get_device_name(0), config=dict(width=cfg.width, layers=cfg.layers,
                           dec_layers=cfg.dec_layers, patch=cfg.patch, grid=cfg.grid, embed_dim=cfg.embed_dim, batch=B, size=S, classes=n, steps=a.steps),
                           baseline="benchlib.baselines.torch_gpu_baseline (the reference's op sequence, stock PyTorch fp32 eager, SDPA in the encoder)",
                           rounds=rounds, summary=summary, parity=parity), f, indent=1)
            f.write("\n")
    return 0 if summary["exact_faster_than_baseline_in_every_round"] else 1


if __name__ == "__main__":
    sys.exit(main())
