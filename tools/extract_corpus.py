"""The seeded JPEG corpus and the ViT-L/14@336 tower of the embedding-extraction benchmarks (tools/extract_bench.py,
tools/jpeg_decode_bench.py): importable, runs nothing."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from zutis_amd import detgen

SIZES = [(500, 375)] * 6 + [(375, 500)] * 3 + [(500, 333)] * 3 + [(640, 480)] * 3 + [(1024, 768), (1600, 1200), (256, 256)]   # (w, h)


def write_image(k: int, path: str):
    rng = np.random.default_rng(50_000 + k)
    w, h = SIZES[int(rng.integers(len(SIZES)))]
    low = rng.integers(0, 256, (max(2, h // 24), max(2, w // 24), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(low).resize((w, h), Image.BICUBIC), np.float32)
    a += rng.normal(0.0, 6.0, a.shape).astype(np.float32)
    Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(path, quality=90)


def corpus(directory: str, n: int, workers: int):
    """The paths of the n files, written once."""
    os.makedirs(directory, exist_ok=True)
    paths = [os.path.join(directory, f"img_{k:05d}.jpg") for k in range(n)]
    todo = [(k, p) for k, p in enumerate(paths) if not os.path.exists(p)]
    with ThreadPoolExecutor(max_workers=workers) as pool:
        list(pool.map(lambda kp: write_image(*kp), todo))
    return paths


def tower(dev, layers: int = 24):
    """(state dict, patch) of a ViT-L/14@336 visual tower with seeded weights, fp16-valued where CLIP's convert_weights leaves them so."""
    D, L, p, g, E = 1024, layers, 14, 24, 768
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
    for k in list(P):
        if k.endswith(("conv1.weight", "in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias", "c_fc.weight", "c_fc.bias",
                       "c_proj.weight", "c_proj.bias")) or k == "visual.proj":
            P[k] = P[k].to(torch.float16).to(torch.float32)
    return P, p
