"""Developer tool: config-5 throughput — CLIP ViT-L/14@336 image-embedding extraction (ClipImageEncoder), random-init weights.

    python tools/embed_bench.py [--precision MODE ...] [--batch B ...] [--rounds R] [--steps K] [--warmup W] [--layers L] [--fp32-weights]

The given precisions (default: exact) run ALTERNATELY in one process — round r times K steps of every mode in turn, so that clock
and thermal drift fall on all of them alike — and one JSON line per (batch, mode) is printed: images/s and ms per step as the median
over the rounds (with every round's value, min and max: the spread of a mode against itself is what a difference between two modes
has to beat), and max |e_mode - e_exact| of the unit-norm embeddings.  Weights are those of `bench.py --workload c5`: fp16-VALUED
conv / Linear / attention / proj tensors (what the reference's convert_weights leaves) unless --fp32-weights."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zutis_amd import detgen                        # noqa: E402
from zutis_amd.engine import ClipImageEncoder       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--precision", action="append", help="exact | fast | f16 | half; repeatable (default: exact)")
ap.add_argument("--batch", action="append", type=int, help="images per step; repeatable (default: 32 64 128)")
ap.add_argument("--rounds", type=int, default=3, help="alternations of the modes after the warm-up")
ap.add_argument("--steps", type=int, default=5, help="timed steps per mode and round")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--layers", type=int, default=24)
ap.add_argument("--fp32-weights", action="store_true", help="generic fp32 values in every tensor (a fine-tuned tower)")
ap.add_argument("--no-exact", action="store_true", help="skip the `exact` run the embeddings are compared with (profiling runs)")
args = ap.parse_args()
modes = args.precision or ["exact"]
batches = args.batch or [32, 64, 128]

dev = torch.device("cuda:0")
D, L, p, g, E = 1024, args.layers, 14, 24, 768
def w(name, shape, std, mean=0.0): return torch.from_numpy(detgen.det_normal("c5." + name, shape, std, mean, 5)).to(dev)
P = {"visual.class_embedding": w("cls", (D,), D ** -0.5), "visual.positional_embedding": w("pos", (g * g + 1, D), D ** -0.5),
     "visual.proj": w("proj", (D, E), D ** -0.5), "visual.conv1.weight": w("conv", (D, 3, p, p), (3 * p * p) ** -0.5)}
for ln in ("ln_pre", "ln_post"):
    P[f"visual.{ln}.weight"] = w(ln + "w", (D,), 0.1, 1.0); P[f"visual.{ln}.bias"] = w(ln + "b", (D,), 0.1)
for i in range(L):
    q = f"visual.transformer.resblocks.{i}."
    P[q + "attn.in_proj_weight"] = w(q + "a", (3 * D, D), D ** -0.5); P[q + "attn.in_proj_bias"] = w(q + "ab", (3 * D,), 0.02)
    P[q + "attn.out_proj.weight"] = w(q + "o", (D, D), D ** -0.5 * (2 * L) ** -0.5); P[q + "attn.out_proj.bias"] = w(q + "ob", (D,), 0.02)
    P[q + "mlp.c_fc.weight"] = w(q + "f", (4 * D, D), (2 * D) ** -0.5); P[q + "mlp.c_fc.bias"] = w(q + "fb", (4 * D,), 0.02)
    P[q + "mlp.c_proj.weight"] = w(q + "p", (D, 4 * D), D ** -0.5 * (2 * L) ** -0.5); P[q + "mlp.c_proj.bias"] = w(q + "pb", (D,), 0.02)
    for ln in ("ln_1", "ln_2"):
        P[q + ln + ".weight"] = w(q + ln + "w", (D,), 0.1, 1.0); P[q + ln + ".bias"] = w(q + ln + "b", (D,), 0.1)
if not args.fp32_weights:
    for k in list(P):
        if k.endswith(("conv1.weight", "in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias", "c_fc.weight", "c_fc.bias",
                       "c_proj.weight", "c_proj.bias")) or k == "visual.proj":
            P[k] = P[k].to(torch.float16).to(torch.float32)
T = g * g + 1
flop = L * (2 * T * (D * 3 * D + D * D + 2 * D * 4 * D) + 4 * T * T * D) + 2 * g * g * 3 * p * p * D
for B in batches:
    x = torch.randn((B, 3, 336, 336), generator=torch.Generator(device="cpu").manual_seed(2000)).to(dev)
    e_exact = None
    if not args.no_exact:
        ex = ClipImageEncoder(P, p, prefix="visual.", precision="exact")
        e_exact = ex.encode_image(x).clone()
        ex.check_finite()
        del ex
    encs = {m: ClipImageEncoder(P, p, prefix="visual.", precision=m) for m in dict.fromkeys(modes)}
    emb = {}
    for m, enc in encs.items():
        for _ in range(max(1, args.warmup)):
            emb[m] = enc.encode_image(x)
        enc.check_finite()
    ms = {m: [] for m in encs}
    for r in range(args.rounds):
        for m, enc in encs.items():
            torch.cuda.synchronize(); t = time.perf_counter()
            for _ in range(args.steps):
                emb[m] = enc.encode_image(x)
            torch.cuda.synchronize()
            ms[m].append((time.perf_counter() - t) / args.steps * 1e3)
    for m in encs:
        med = statistics.median(ms[m])
        print(json.dumps({"tool": "embed_bench", "batch": B, "layers": L, "precision": m, "images_per_s": round(B / med * 1e3, 1),
                          "ms_per_step": round(med, 3), "ms_per_step_rounds": [round(v, 3) for v in ms[m]],
                          "images_per_s_min": round(B / max(ms[m]) * 1e3, 1), "images_per_s_max": round(B / min(ms[m]) * 1e3, 1),
                          "spread_pct": round((max(ms[m]) - min(ms[m])) / med * 100, 2), "rounds": args.rounds, "steps": args.steps,
                          "tflops": round(B * flop / med / 1e9, 1),
                          "max_abs_diff_vs_exact": None if e_exact is None else float((emb[m] - e_exact).abs().max()),
                          "embedding_norm": round(float(emb[m].norm(dim=1).mean()), 6),
                          "weights": "generic fp32" if args.fp32_weights else "fp16-valued GEMM tensors"}), flush=True)
    del encs, emb
