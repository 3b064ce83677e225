"""Fused bilinear upsample + argmax (networks/zutis.py:366-372): us per launch of the product kernel, random logits and spatially
smooth ones (its comparison with the round-2 kernel: profiles/r06_argmax_bench.txt).
usage: argmax_bench.py"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from zutis_amd import ops

dev = torch.device("cuda:0")
CASES = ((32, 81, 42, 336), (8, 920, 74, 518), (16, 920, 64, 518), (1, 81, 60, 480), (4, 21, 42, 336))


def logits(B, n, h, smooth):
    g = torch.Generator(device=dev).manual_seed(n + h)
    lo = torch.randn(B, n, h, h, device=dev, generator=g)
    if smooth:       # neighbouring pixels share their leading classes, as on images
        lo = torch.nn.functional.avg_pool2d(lo, 5, stride=1, padding=2) * 3
    return lo.contiguous()


for (B, n, h, H) in CASES:
    for smooth in (False, True):
        lo = logits(B, n, h, smooth)
        lab = torch.empty(B, H, H, dtype=torch.int64, device=dev)
        for _ in range(3):
            ops.upsample_argmax(lo, lab, B, n, h, h, H, H)
        torch.cuda.synchronize(); t = time.perf_counter()
        for _ in range(10):
            ops.upsample_argmax(lo, lab, B, n, h, h, H, H)
        torch.cuda.synchronize(); dt = (time.perf_counter() - t) / 10
        byts = B * n * h * h * 4 + B * H * H * 8
        print(f"B={B} n={n} {h}->{H} {'smooth' if smooth else 'random'}: {dt * 1e6:8.1f} us; "
              f"{byts / 1e6:.0f} MB compulsory -> {byts / dt / 1e12:.2f} TB/s; {B * H * H * n / dt / 1e12:.2f} T pixel-classes/s")
