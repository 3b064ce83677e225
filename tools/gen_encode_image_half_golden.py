"""Records tests/golden/encode_image_half.npz from the REAL reference VisionTransformer (networks/clip_arch.py), on the CPU:
per case the unit-norm `encode_image` embeddings in fp32 and in half precision — the run the reference itself makes of this
tower (third-party clip.load leaves the model in fp16 on a GPU; utils/extract_image_embeddings.py:43,72-78).  Outputs only:
weights and images are regenerated from zutis_amd/detgen.py by the tests (tests/_half_stream_case.py holds the cases).

For each case the reference's own VisionTransformer is built from detgen weights whose conv / Linear / attention / proj tensors
were first rounded through fp16 (what convert_weights leaves), its submodules are run in the order of CLIP's original forward
(the order oracle/gen_golden.py::gen_encode_image uses) once in fp32 -> `{tag}_f32`, and once after the reference's
convert_weights with a half input -> `{tag}_ref_half`; `{tag}_shape` = [B, R, width, layers, patch, grid, embed_dim].

    python tools/gen_encode_image_half_golden.py --reference PATH_TO_REFERENCE_CHECKOUT [--out tests/golden/encode_image_half.npz]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _half_stream_case as HC                      # noqa: E402  (the cases; never the other way round: no test imports this tool)


def run(vt, x):
    """The submodules in the order of CLIP's original VisionTransformer.forward (clip_arch.py:413-431) + the L2 normalisation of
    utils/extract_image_embeddings.py:73, in the dtype of `x`."""
    with torch.no_grad():
        t = vt.conv1(x)
        t = t.reshape(t.shape[0], t.shape[1], -1).permute(0, 2, 1)
        t = torch.cat([vt.class_embedding.to(t.dtype) + torch.zeros(t.shape[0], 1, t.shape[-1], dtype=t.dtype), t], dim=1)
        t = t + vt.positional_embedding.to(t.dtype)
        t = vt.ln_pre(t)
        t = vt.transformer(t.permute(1, 0, 2)).permute(1, 0, 2)
        e = vt.ln_post(t[:, 0, :]) @ vt.proj
        e = e / torch.linalg.norm(e, ord=2, dim=1, keepdim=True)
    return e.to(torch.float32).numpy()                  # :78 float16 -> float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="reference checkout (holds networks/clip_arch.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "encode_image_half.npz"))
    ap.add_argument("--cases", nargs="*", default=list(HC.CASES))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from networks.clip_arch import VisionTransformer, convert_weights
    rec = {}
    for tag in a.cases:
        cfg, sd, x = HC.case(tag)
        R = cfg.patch * cfg.grid
        vt = VisionTransformer(input_resolution=R, patch_size=cfg.patch, width=cfg.width, layers=cfg.layers, heads=cfg.width // 64,
                               output_dim=cfg.embed_dim)
        vt.load_state_dict({k[len("encoder."):]: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        vt.eval().requires_grad_(False)
        f32 = run(vt, x)
        convert_weights(vt)
        half = run(vt, x.half())
        rec[f"{tag}_shape"] = np.array([x.shape[0], R, cfg.width, cfg.layers, cfg.patch, cfg.grid, cfg.embed_dim])
        rec[f"{tag}_f32"], rec[f"{tag}_ref_half"] = f32, half
        d = half.astype(np.float64) - f32
        print(f"{tag}: {f32.shape} max |ref_half - f32| {np.abs(d).max():.3e} rms {np.sqrt((d * d).mean()):.3e}", flush=True)
    np.savez_compressed(a.out, **rec)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
