"""Records tests/golden/criterion.npz from the REAL reference criterion.py (CPU, fp32): the inputs of a small seeded case and
the reference's cost matrices, assignments, losses and autograd gradients, with default and with non-default weights, plus the
signatures of Criterion.__init__ / __call__.  Data only: nothing of the reference's program text is stored.

    python tools/gen_criterion_golden.py --reference PATH_TO_REFERENCE_CHECKOUT [--out tests/golden/criterion.npz]
"""
from __future__ import annotations

import argparse
import importlib.util
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, L, Q, h, w, H, W, NCAT, D, h2, w2 = 3, 2, 12, 40, 48, 67, 101, 7, 16, 20, 24
COUNTS = (3, 2, 5)                         # image 1's two GT masks are all zero (skipped by the criterion)
WEIGHTS = {"default": {}, "custom": dict(weight_ce_loss=0.7, weight_mask_loss=1.3, weight_dice_loss=0.6, weight_bce_loss=1.7)}


def make_inputs(seed: int = 5):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    props = torch.empty(B, L, Q, h, w)
    for b in range(B):
        for q in range(Q):
            y0, x0 = (torch.rand(2, generator=g) * torch.tensor([h * 0.6, w * 0.6])).tolist()
            hh, ww = (torch.rand(2, generator=g) * torch.tensor([h * 0.5, w * 0.5]) + 4).tolist()
            box = ((yy >= y0) & (yy < y0 + hh) & (xx >= x0) & (xx < x0 + ww)).float()
            for l in range(L):
                props[b, l, q] = torch.sigmoid(5.0 * (box - 0.5) + 0.8 * torch.randn(h, w, generator=g))
    props = (props * 1024).round().clamp(1, 1023) / 1024        # 10-bit values: the fixture stays small
    Y, X = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    gts = []
    for b, n in enumerate(COUNTS):
        m = torch.zeros(n, H, W, dtype=torch.uint8)
        if b != 1:
            for i in range(n):
                y0, x0 = int(torch.randint(0, H - 20, (1,), generator=g)), int(torch.randint(0, W - 20, (1,), generator=g))
                hh, ww = int(torch.randint(8, 40, (1,), generator=g)), int(torch.randint(8, 50, (1,), generator=g))
                m[i] = ((Y >= y0) & (Y < y0 + hh) & (X >= x0) & (X < x0 + ww)).to(torch.uint8)
        gts.append(m)
    tok = torch.randn(B, h2, w2, D, generator=g)
    tok = tok / tok.norm(dim=-1, keepdim=True)
    te = torch.randn(NCAT, D, generator=g)
    te = te / te.norm(dim=-1, keepdim=True)
    sem = torch.randint(0, NCAT, (B, H, W), generator=g)
    sem[torch.rand(B, H, W, generator=g) < 0.05] = 255
    return props, gts, tok, te, sem


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="reference checkout (holds criterion.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "criterion.npz"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_criterion", os.path.join(a.reference, "criterion.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    props, gts, tok, te, sem = make_inputs()
    rec = {"props": props.numpy(), "gt_u8": torch.cat(gts).numpy(), "gt_counts": np.array(COUNTS, np.int32), "tokens": tok.numpy(),
           "te": te.numpy(), "sem": sem.numpy().astype(np.int32)}
    sig = {}
    for fn in ("__init__", "__call__"):
        ps = inspect.signature(getattr(mod.Criterion, fn)).parameters.values()
        sig[fn] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)] for p in ps]
    rec["signatures"] = np.array(json.dumps(sig))
    real_lsa = mod.linear_sum_assignment
    for tag, kw in WEIGHTS.items():
        seen = []

        def lsa(cost_matrix):
            r, c = real_lsa(cost_matrix=cost_matrix)
            seen.append((cost_matrix.copy(), r, c))
            return r, c

        mod.linear_sum_assignment = lsa
        p = props.clone().requires_grad_(True)
        t = tok.clone().requires_grad_(True)
        crit = mod.Criterion(te, **kw)
        out = crit(p, gts, [[0] * n for n in COUNTS], t, sem)
        out["loss"].backward()
        mod.linear_sum_assignment = real_lsa
        k = 0
        for b in range(B):
            if gts[b].sum() == 0:
                continue
            for l in range(L):
                cm, r, c = seen[k]
                k += 1
                rec[f"{tag}_cost_{b}_{l}"] = cm.astype(np.float32)
                rec[f"{tag}_rows_{b}_{l}"] = np.asarray(r, np.int64)
                rec[f"{tag}_cols_{b}_{l}"] = np.asarray(c, np.int64)
                # the optimum must be unique by a margin that fp32 reorderings cannot bridge
                best = cm[r, c].sum()
                for i, q in zip(r, c):
                    alt = cm.astype(np.float64).copy()
                    alt[i, q] = 1e9
                    r2, c2 = real_lsa(alt)
                    assert alt[r2, c2].sum() - best > 1e-4, (tag, b, l)
        assert k == len(seen)
        rec[f"{tag}_ce_loss"] = np.float64(out["ce_loss"])
        rec[f"{tag}_mask_loss"] = np.float64(out["mask_loss"])
        rec[f"{tag}_loss"] = np.float64(out["loss"].item())
        rec[f"{tag}_grad_props"] = p.grad.numpy()
        rec[f"{tag}_grad_tokens"] = t.grad.numpy()
    np.savez_compressed(a.out, **rec)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
