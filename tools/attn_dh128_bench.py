"""Attention at head dim 128 beside its dh = 96 sibling (developer tool): the same (batch, heads, Tq, Tk), fp16 and split pairs, for the
decoder's self-attention, its cross-attention at batch 32 and the batch-1 key-split form.  The work ratio 128 : 96 is 4/3.

    python tools/attn_dh128_bench.py [--rounds 5] [--iters 50] [--out profiles/attn_dh128_ab.json]

Per round the rows are timed in alternation (every row once per round: dh 96, dh 128, next shape, ...), a round's figure is the mean of
`iters` launches between two events behind a warm-up; the JSON holds every round, the medians, the spread (max - min over the rounds) and
the dh 128 / dh 96 time ratio per shape and operand mode."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from zutis_amd import ops, shape_rules

SHAPES = [("self", 32, 8, 100, 100, 1), ("cross", 32, 8, 100, 2304, 1), ("cross_b1_split12", 1, 8, 100, 6120, 12)]   # name, B, heads, Tq, Tk, key split


def make(dev, B, H, dh, Tq, Tk, x3, ksplit):
    D = H * dh
    g = torch.Generator(device="cpu").manual_seed(dh * 7 + Tk)
    def operand(T):
        x = torch.randn(B, T, D, generator=g)
        hi = x.half()
        t = torch.stack([hi, (x - hi.float()).half()]) if x3 else hi[None]
        return ops.Act(t.to(dev).contiguous())
    q, k, v = operand(Tq), operand(Tk), operand(Tk)
    o = ops.Act.empty((B, Tq, D), x3, dev)
    ksplit = shape_rules.fit_key_split(ksplit, shape_rules.key_tiles(Tk, x3))
    ws = torch.empty(ops.attention_splitk_workspace_size(B, H, Tq, dh, ksplit), dtype=torch.uint8, device=dev) if ksplit > 1 else None
    arg = (lambda a: a) if x3 else (lambda a: a.hi)
    return lambda: ops.attention(arg(q), arg(k), arg(v), arg(o), batch=B, heads=H, Tq=Tq, Tk=Tk, head_dim=dh, ldq=D, ldk=D, ldv=D, ldo=D,
                                 strideQ=Tq * D, strideK=Tk * D, strideV=Tk * D, strideO=Tq * D, x3=x3, ksplit=ksplit, workspace=ws)


def timed(run, iters):
    for _ in range(5):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = {}
    for name, B, H, Tq, Tk, S in SHAPES:
        for x3 in (False, True):
            for dh in (96, 128):
                rows[(name, x3, dh)] = dict(run=make(dev, B, H, dh, Tq, Tk, x3, S), flops=4.0 * B * H * Tq * Tk * dh, us=[])
    for _ in range(a.rounds):
        for r in rows.values():
            r["us"].append(timed(r["run"], a.iters))
    result = []
    for name, B, H, Tq, Tk, S in SHAPES:
        for x3 in (False, True):
            rec = dict(shape=name, batch=B, heads=H, Tq=Tq, Tk=Tk, ksplit=S, operands="split pair" if x3 else "fp16")
            for dh in (96, 128):
                r = rows[(name, x3, dh)]
                med = statistics.median(r["us"])
                rec[f"dh{dh}"] = dict(us_rounds=[round(u, 2) for u in r["us"]], us_median=round(med, 2), us_spread=round(max(r["us"]) - min(r["us"]), 2),
                                      tflops=round(r["flops"] / med / 1e6, 1))
            rec["time_ratio_128_over_96"] = round(rec["dh128"]["us_median"] / rec["dh96"]["us_median"], 3)
            rec["ratio_rounds"] = [round(x / y, 3) for x, y in zip(rows[(name, x3, 128)]["us"], rows[(name, x3, 96)]["us"])]
            result.append(rec)
            print(f"{name:17s} {rec['operands']:10s} dh96 {rec['dh96']['us_median']:8.1f} us ({rec['dh96']['tflops']:6.1f} TF/s)  dh128 "
                  f"{rec['dh128']['us_median']:8.1f} us ({rec['dh128']['tflops']:6.1f} TF/s)  ratio {rec['time_ratio_128_over_96']:.3f} (work 1.333)")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/attn_dh128_bench.py", device=torch.cuda.get_device_name(0), rounds=a.rounds, iters=a.iters, rows=result), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
