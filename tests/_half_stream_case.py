"""Cases of the fp16 residual stream (precision "half") and a CPU restatement of its rounding points.

tests/golden/encode_image_half.npz (tools/gen_encode_image_half_golden.py) holds, per case, the reference VisionTransformer's
embeddings in fp32 (`{tag}_f32`) and in half precision after the reference's convert_weights (`{tag}_ref_half`).  Weights and
images are regenerated here from zutis_amd/detgen.py; the conv / Linear / attention / proj tensors are rounded through fp16 first
(what convert_weights leaves, networks/clip_arch.py:566-587), so the fp32 run and the half run see the same weight values."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from zutis_amd import detgen

PATCH = 14
# tag -> (width, layers, grid, batch, embed_dim, detgen seed)
CASES = {
    "small": (128, 2, 3, 3, 64, 1234),
    "l14_336": (1024, 2, 24, 2, 768, 1234),         # ViT-L/14@336 geometry, 2 layers
    "deep": (256, 12, 8, 4, 128, 1234),
    "full": (1024, 24, 24, 2, 768, 5),              # ViT-L/14@336, every layer
}
# the tensors convert_weights rounds to fp16 (nn.Conv2d / nn.Linear weight and bias, the attention in_proj tensors, `proj`)
F16_VALUED = ("conv1.weight", "in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias", "c_fc.weight", "c_fc.bias",
              "c_proj.weight", "c_proj.bias")


def f16_valued(k: str) -> bool:
    return k.endswith(F16_VALUED) or k.endswith(".proj") or k == "proj"


@functools.lru_cache(maxsize=1)
def case(tag):
    """(cfg, encoder state dict [numpy fp32, `encoder.` keys, fp16-valued GEMM tensors], images torch fp32 [B,3,R,R]).
    The last case is kept (24 layers of ViT-L are 1.2 GB of generated weights): callers do not modify what they get."""
    width, layers, grid, B, embed, seed = CASES[tag]
    cfg = detgen.ZutisConfig(width=width, layers=layers, patch=PATCH, grid=grid, embed_dim=embed)
    shapes = detgen.zutis_param_shapes(cfg)
    sd = {}
    for k, (shp, std, mean) in shapes.items():
        if not k.startswith("encoder."):
            continue
        v = detgen.det_normal(k, shp, std, mean, seed)
        sd[k] = v.astype(np.float16).astype(np.float32) if f16_valued(k) else v
    R = PATCH * grid
    return cfg, sd, torch.from_numpy(detgen.images(B, R, R, seed=5))


def visual_params(sd, device):
    """The case's weights under the CLIP `visual.` prefix, on `device` (ClipImageEncoder's params)."""
    return {"visual." + k[len("encoder."):]: torch.from_numpy(v).to(device) for k, v in sd.items()}


def h(t: torch.Tensor) -> torch.Tensor:
    """One rounding to fp16 (round to nearest even), carried on in fp32."""
    return t.half().float()


def restate_half(sd, x: torch.Tensor, patch: int, two_roundings: bool = True) -> torch.Tensor:
    """Precision "half" restated with torch on the CPU: fp32 compute, an explicit rounding through fp16 at every rounding point.

    1. X after ln_pre is rounded once.
    2. X <- X + (O W^T + b): X read as fp16, the sum in fp32; two_roundings: f16(f16(O W^T + b) + X) (the form the engine takes),
       else one rounding of the fp32 sum.
    3. The im2col'd image, Y16 (LayerNorm outputs), QKV16, O16 and H16 (QuickGELU(c_fc)) are rounded where "fast" rounds them; the
       `embed` projection is fp32-class (x3): cls16 is a split pair there, i.e. not rounded to one fp16 value.
    LayerNorm statistics, accumulators, softmax and QuickGELU stay fp32."""
    P = {k: torch.from_numpy(v) for k, v in sd.items()}
    pre = "encoder."
    B = x.shape[0]
    D = P[pre + "class_embedding"].shape[0]
    heads, dh = D // 64, 64
    ln = lambda t, n: F.layer_norm(t, (D,), P[n + ".weight"], P[n + ".bias"], 1e-5)
    t = F.conv2d(h(x), P[pre + "conv1.weight"], None, stride=patch)                   # conv site: fp16 operands (the im2col'd image)
    t = t.reshape(B, D, -1).permute(0, 2, 1)
    t = torch.cat([P[pre + "class_embedding"][None, None].expand(B, 1, D), t], dim=1) + P[pre + "positional_embedding"][None]
    X = h(ln(t, pre + "ln_pre"))                                                      # rounding point 1
    T = X.shape[1]

    def update(X, lin):
        return h(h(lin) + X) if two_roundings else h(lin + X)                         # rounding point 2

    n_layers = 1 + max(int(k.split(".")[3]) for k in P if k.startswith(pre + "transformer.resblocks."))
    for i in range(n_layers):
        p = f"{pre}transformer.resblocks.{i}."
        y = h(ln(X, p + "ln_1"))                                                      # Y16
        qkv = h(F.linear(y, P[p + "attn.in_proj_weight"], P[p + "attn.in_proj_bias"]))    # QKV16
        q, k, v = (z.view(B, T, heads, dh).transpose(1, 2) for z in qkv.split(D, dim=-1))
        s = torch.matmul(q, k.transpose(-1, -2)) * (1.0 / math.sqrt(dh))
        o = h(torch.matmul(torch.softmax(s, dim=-1), v).transpose(1, 2).reshape(B, T, D))   # O16 (probabilities: fp32 here)
        X = update(X, F.linear(o, P[p + "attn.out_proj.weight"], P[p + "attn.out_proj.bias"]))
        y = h(ln(X, p + "ln_2"))                                                      # Y16
        f = F.linear(y, P[p + "mlp.c_fc.weight"], P[p + "mlp.c_fc.bias"])
        hh = h(f * torch.sigmoid(1.702 * f))                                          # H16
        X = update(X, F.linear(hh, P[p + "mlp.c_proj.weight"], P[p + "mlp.c_proj.bias"]))
    e = ln(X[:, 0], pre + "ln_post") @ P[pre + "proj"]                                # embed site: fp32-class (x3)
    return e / e.norm(dim=-1, keepdim=True)


def errors(got: np.ndarray, f32: np.ndarray, ref_half: np.ndarray):
    """(e, e_ref, rms, rms_ref): max / rms of (got - f32) and of the reference's own half run against its fp32 run."""
    d, dr = got.astype(np.float64) - f32, ref_half.astype(np.float64) - f32
    return float(np.abs(d).max()), float(np.abs(dr).max()), float(np.sqrt((d * d).mean())), float(np.sqrt((dr * dr).mean()))


def check_envelope(tag, got, g):
    """The acceptance envelope of precision "half": e < 1e-3 (the project's north-star tolerance) and, against the reference's own
    half-precision run, e <= 1.5 e_ref and rms <= 1.25 rms_ref.  Prints both ratios."""
    e, e_ref, rms, rms_ref = errors(got, g[f"{tag}_f32"], g[f"{tag}_ref_half"])
    print(f"half-stream {tag}: e {e:.3e} e_ref {e_ref:.3e} max ratio {e / e_ref:.3f} rms {rms:.3e} rms_ref {rms_ref:.3e} rms ratio {rms / rms_ref:.3f}")
    assert e < 1e-3, (tag, e)
    assert e <= 1.5 * e_ref, (tag, e, e_ref)
    assert rms <= 1.25 * rms_ref, (tag, rms, rms_ref)
    return e / e_ref, rms / rms_ref
