"""Forward + backward of the training criterion at the shipped training shape (batch 8, 384^2, 6 decoder layers x 100 queries on
48x48, seeded 1-10 instances per image, 48x48x512 tokens): HipCriterion against the stock-torch op sequence of the reference's
criterion.py (fp32, same GPU), for 81 and 920 classes.  Reports the median wall time per step (both paths synchronise on their
host Hungarian solve) and torch.cuda.max_memory_allocated above the inputs.

Then HipCriterion(assignment="host") against assignment="device" in the same process, with the ground truth on the CPU (what the
reference's DataLoader hands over) and on the device (bool views of one allocation, what zutis_amd.synth delivers): the arms are
ALTERNATED (round r runs every arm once), each round's value is the median step of that round, and the result is the median over the
rounds with every round's value — the spread of an arm against itself is what a difference between two arms has to exceed.

    python tools/criterion_bench.py [--steps 10] [--warmup 3] [--rounds 5] [--no-stock] [--arm NAME ...] [--out FILE.json] [--ab-out FILE.json]

`--no-stock --rounds 1 --arm device_gt_dev` is the `rocprofv3 --kernel-trace --stats` target.
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


ARMS = ("host", "device", "host_gt_dev", "device_gt_dev")       # assignment mode, ground truth on the CPU / on the device


def assignment_arms(props, gts, tok, te, sem, dev, arms, rounds, steps, warmup):
    """{arm: {median_ms, rounds_ms, spread_ms}} of forward + backward, the arms alternated."""
    gts_dev = list(torch.split(torch.cat(gts, 0).to(dev).bool(), [int(g.shape[0]) for g in gts], 0))
    crits = {"host": HipCriterion(te), "device": HipCriterion(te, assignment="device")}
    p = props.clone().requires_grad_(True)
    t = tok.clone().requires_grad_(True)
    sem_d = sem.to(dev)

    def step_of(arm):
        crit, g = crits[arm.split("_")[0]], gts_dev if arm.endswith("_gt_dev") else gts

        def step():
            p.grad = t.grad = None
            crit(p, g, None, t, sem_d)["loss"].backward()
        return step

    ms = {arm: [] for arm in arms}
    for r in range(rounds):
        for arm in arms:
            ms[arm].append(measure(step_of(arm), steps, warmup if r == 0 else 1)[0] * 1e3)
    return {arm: {"median_ms": round(float(np.median(v)), 4), "rounds_ms": [round(x, 4) for x in v],
                  "spread_ms": round(max(v) - min(v), 4)} for arm, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the assignment arms")
    ap.add_argument("--no-stock", action="store_true", help="skip the stock-torch comparison")
    ap.add_argument("--arm", action="append", choices=ARMS, help="assignment arms to run (default: all)")
    ap.add_argument("--ab-out", default=None, help="JSON file for the assignment arms")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for n_cat in (81, 920):
        props, gts, tok, te, sem = make_case(8, 6, 100, 48, 48, 384, 384, n_cat, 512, 48, 48, seed=11)
        props, tok, te = props.to(dev), tok.to(dev), te.to(dev)
        crit = HipCriterion(te)
        row = {"n_cat": n_cat, "instances": [int(g.shape[0]) for g in gts]}
        for name in ("hip",) if a.no_stock else ("hip", "stock"):
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
        if not a.no_stock:
            row["speedup"] = row["stock"]["median_ms"] / row["hip"]["median_ms"]
        arms = tuple(a.arm) if a.arm else ARMS
        ab = assignment_arms(props, gts, tok, te, sem, dev, arms, a.rounds, a.steps, a.warmup)
        for host, device in (("host", "device"), ("host_gt_dev", "device_gt_dev")):
            if host in ab and device in ab:
                ab[f"{device}_over_{host}"] = round(ab[device]["median_ms"] / ab[host]["median_ms"], 4)
        row["assignment"] = ab
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "shape": "b=8 L=6 Q=100 48x48 -> 384x384, tokens 48x48x512",
           "steps": a.steps, "warmup": a.warmup, "rows": rows}
    if a.ab_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.ab_out)), exist_ok=True)
        with open(a.ab_out, "w") as f:
            json.dump({k: res[k] for k in ("device", "shape", "steps", "warmup")} | {
                "rounds": a.rounds, "protocol": "arms alternated in one process; per round the median step, then the median over the rounds",
                "rows": [{"n_cat": r["n_cat"], "instances": r["instances"], **r["assignment"]} for r in rows]}, f, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
