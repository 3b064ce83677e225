"""Forward + backward of the training criterion at the shipped training shape (batch 8, 384^2, 6 decoder layers x 100 queries on
48x48, seeded 1-10 instances per image, 48x48x512 tokens): HipCriterion against the stock-torch op sequence of the reference's
criterion.py (fp32, same GPU), for 81 and 920 classes.  Reports the median wall time per step (both paths synchronise on their
host Hungarian solve) and torch.cuda.max_memory_allocated above the inputs.

    python tools/criterion_bench.py [--steps 10] [--warmup 3] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests._criterion_case import make_case  # noqa: E402
from zutis_amd.criterion import HipCriterion  # noqa: E402


def stock_step(props, gts, tok, sem, te, ignore_index=255):
    """The reference's op sequence (criterion.py:63-161) with stock torch ops, default weights."""
    B = len(props)
    H, W = gts[0].shape[-2:]
    up_tok = F.interpolate(tok.permute(0, 3, 1, 2), size=(H, W), mode="bilinear")
    logits = torch.einsum("nc,bchw->bnhw", te, up_tok)
    ce = F.cross_entropy(logits, sem.to(tok.device), ignore_index=ignore_index)
    mask_loss = torch.zeros((), device=props.device)
    for b in range(B):
        g = gts[b].to(device=props.device, dtype=torch.float32).flatten(1)
        if g.sum() == 0:
            continue
        p = F.interpolate(props[b], size=(H, W), mode="bilinear").flatten(2)
        for pl in p:
            n, Q = g.shape[0], pl.shape[0]
            dice = 1 - (2 * torch.einsum("nc,mc->nm", pl, g) + 1) / (pl.sum(-1)[:, None] + g.sum(-1)[None, :] + 1)
            bce = F.binary_cross_entropy(pl[:, None].repeat(1, n, 1), g[None].repeat(Q, 1, 1), reduction="none").mean(-1)
            cost = (dice + bce).permute(1, 0)
            r, c = linear_sum_assignment(cost.detach().cpu().numpy())
            for i, q in zip(r, c):
                mask_loss = mask_loss + cost[i, q]
    loss = mask_loss / B + ce
    loss.backward()
    return float(ce), float(mask_loss / B)


def measure(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for n_cat in (81, 920):
        props, gts, tok, te, sem = make_case(8, 6, 100, 48, 48, 384, 384, n_cat, 512, 48, 48, seed=11)
        props, tok, te = props.to(dev), tok.to(dev), te.to(dev)
        crit = HipCriterion(te)
        row = {"n_cat": n_cat, "instances": [int(g.shape[0]) for g in gts]}
        for name in ("hip", "stock"):
            p = props.clone().requires_grad_(True)
            t = tok.clone().requires_grad_(True)

            def step():
                p.grad = t.grad = None
                if name == "hip":
                    crit(p, gts, None, t, sem)["loss"].backward()
                else:
                    stock_step(p, gts, t, sem, te)

            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            step()                                           # first call: warm and measure the peak
            torch.cuda.synchronize()
            p.grad = t.grad = None
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            med, best = measure(step, a.steps, a.warmup)
            row[name] = {"median_ms": med * 1e3, "min_ms": best * 1e3, "peak_extra_bytes": int(peak)}
            del p, t
            torch.cuda.empty_cache()
        row["speedup"] = row["stock"]["median_ms"] / row["hip"]["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "shape": "b=8 L=6 Q=100 48x48 -> 384x384, tokens 48x48x512",
           "steps": a.steps, "warmup": a.warmup, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
