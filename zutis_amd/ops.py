"""Thin torch-tensor -> raw-pointer wrappers over the C ABI (include/zutis_hip.h).

PyTorch is plumbing here: device memory, the current HIP stream.  Every op launches a hand-written HIP
kernel from libzutis_hip.so; a missing library or a non-GPU tensor is an error, never a fallback.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib

_ZH = _lib.constants()     # the ZH_* constants of include/zutis_hip.h: the values the kernels were compiled with
ACT_NONE, ACT_QUICKGELU, ACT_RELU, ACT_SIGMOID, ACT_GELU_ERF = (_ZH["ZH_ACT_" + a] for a in ("NONE", "QUICKGELU", "RELU", "SIGMOID", "GELU_ERF"))
f16, f32 = torch.float16, torch.float32


# Optional per-launch profiler (bench.py): PROFILER(name, work, launch) must call launch() and may bracket it with
# HIP events on the current stream.  None in production: zero overhead.
PROFILER = None


def _call(entry: str, *args):
    """Call the C entry point `entry` and raise on a non-zero return code.  Looked up through _lib.load(), so that an active
    plan recorder or launch counter sees the call."""
    _lib.check(getattr(_lib.load(), entry)(*args), entry)


def _launch(name, work, entry: str, args):
    """_call(entry, *args), the call itself bracketed by PROFILER as launch `name` doing `work`."""
    fn = getattr(_lib.load(), entry)
    _lib.check(fn(*args) if PROFILER is None else PROFILER(name, work, lambda: fn(*args)), entry)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """Raw handle of torch's current HIP stream.  torch.cuda.current_stream() costs ~8 us of Python per call (half of the
    per-launch host overhead, tools/py_overhead.py); the private raw getter is ~0.3 us and returns the same handle."""
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.ZutisHipError("zutis_amd ops need GPU tensors (no CPU fallback)")
    if _raw_device is not None and t.device.index != _raw_device():
        raise _lib.ZutisHipError(f"tensor on cuda:{t.device.index} but the current device (whose stream is used) is "
                                 f"cuda:{_raw_device()}: wrap the call in torch.cuda.device(...)")
    if _lib.RECORDER is not None:
        _lib.RECORDER.keepalive.append(t)        # a launch plan owns every tensor whose address it recorded
    return t.data_ptr()


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


def _workspace(size_entry: str, device, *dims):
    """(uint8 tensor of `size_entry`(*dims) bytes on `device`, that size).  A size query launches nothing: it goes to the library
    itself, not through a recorder or counter."""
    need = int(getattr(_lib.load(raw=True), size_entry)(*dims))
    return torch.empty(need, dtype=torch.uint8, device=device), need


def _workspace_or(ws, name: str, size_entry: str, device, *dims):
    """_workspace, or the caller's own `ws` (any dtype) checked against that size."""
    if ws is None:
        return _workspace(size_entry, device, *dims)
    need = int(getattr(_lib.load(raw=True), size_entry)(*dims))
    if _nbytes(ws) < need:
        raise _lib.ZutisHipError(f"{name}: workspace holds {_nbytes(ws)} bytes, {need} needed")
    return ws, need


def _chk(t: torch.Tensor, dtype, name: str):
    if t.dtype != dtype or not t.is_contiguous():
        raise _lib.ZutisHipError(f"{name}: expected contiguous {dtype}, got {t.dtype} contiguous={t.is_contiguous()}")


class Act:
    """An fp16 activation (or weight) tensor, optionally stored as a split pair for the f16x3 precision (zutis_hip.h):
    `t` has shape [P, ...] with P = 1 (plain fp16) or 2 (hi, lo); `hi` = t[0] is the plain fp16 tensor every fp16 consumer
    reads; `plane` = element offset hi -> lo (0 when not split); `out_scale` = 2^-s for weights packed as W * 2^s; `x2`: a
    split_weight() pack whose lo plane would be all zeros, stored as its hi plane alone."""
    __slots__ = ("t", "hi", "plane", "out_scale", "x2")

    def __init__(self, t: torch.Tensor, out_scale: float = 1.0):
        assert t.dtype == f16 and t.shape[0] in (1, 2)
        self.t, self.hi = t, t[0]
        self.plane = t.stride(0) if t.shape[0] == 2 else 0
        self.out_scale = float(out_scale)
        self.x2 = False      # set by split_weight(): one plane that IS the fp32 weight (times 2^s) exactly — the f16x2 operand form

    @staticmethod
    def empty(shape, split: bool, device) -> "Act":
        return Act(torch.empty((2 if split else 1,) + tuple(shape), dtype=f16, device=device))

    def view(self, t_hi: torch.Tensor) -> "Act":
        """The same pair seen through a view of the hi plane (column / row slices keep the plane offset)."""
        a = Act.__new__(Act)
        a.t, a.hi, a.plane, a.out_scale, a.x2 = self.t, t_hi, self.plane, self.out_scale, self.x2
        return a


ALLOW_X2 = True     # developer switch (tests / A-B): False packs every weight as two planes, zero lo plane or not


def split_weight(w32: torch.Tensor, allow_x2: Optional[bool] = None) -> Act:
    """Pack-time split of an fp32 weight for zh_gemm_f16x3: W * 2^s with s chosen so that max|W| lands in [2^13, 2^14)
    (hi far from overflow, lo = f16(W*2^s - hi) a normal fp16 number); out_scale = 2^-s is exact.  A weight whose lo plane
    would be all zeros is packed as ONE plane (the "f16x2" form of zh_gemm_f16x3) unless allow_x2 (default: ALLOW_X2) is False."""
    w = w32.detach().to(f32)
    m = float(w.abs().max()) if w.numel() else 0.0
    s = 0 if m == 0.0 or not math.isfinite(m) else 13 - math.floor(math.log2(m))
    s = max(-14, min(60, s))                        # 2^-60 is still a normal fp32 out_scale
    ws = w * (2.0 ** s)
    hi = ws.to(f16)
    lo = (ws - hi.to(f32)).to(f16)
    if (ALLOW_X2 if allow_x2 is None else allow_x2) and not bool(lo.any()):
        # every value of W * 2^s is an fp16 number: the released CLIP towers, whose Linear / conv / attention weights the
        # reference's constructor rounds to fp16 (convert_weights, clip_arch.py:566-587,625) before they are cast back to fp32
        # (zutis.py:55).  One plane, plane = 0: zh_gemm_f16x3 then skips the product with the zero lo plane (bit-identical).
        a = Act(hi.unsqueeze(0).contiguous(), out_scale=2.0 ** -s)
        a.x2 = True
        return a
    return Act(torch.stack([hi, lo]).contiguous(), out_scale=2.0 ** -s)


def _hp(a):
    """(hi tensor, lo-plane offset) of an Act or a plain fp16 tensor."""
    return (a.hi, a.plane) if isinstance(a, Act) else (a, 0)


def _gemm_bytes(M, N, K, batch, strideA, strideW, op_bytes, out_bytes, has_residual, res_bytes: int = 4) -> float:
    """Compulsory (algorithmic) bytes of one GEMM launch: each operand once (a batch-shared operand once), the output once,
    the residual once (res_bytes per element: 4 for fp32, 2 for the fp16 stream).  op_bytes = 2 for fp16 operands, 4 for split pairs."""
    a = M * K * op_bytes * (batch if strideA else 1)
    w = N * K * op_bytes * (batch if (strideW or batch == 1) else 1)
    return float(a + w + M * N * batch * (out_bytes + (res_bytes if has_residual else 0)))


def _pos(pos, N):
    """Argument words of the optional separable row bias: pos = (pos_y [h, >=N], pos_x [w, >=N]), both fp32 or both fp16 ->
    rows are pixels m = img * h*w + y * w + x and pos_y[y] + pos_x[x] is added before the activation."""
    if pos is None:
        return (None, None, 0, 0, 0, 0)
    ty, tx = pos
    assert ty.dtype == tx.dtype and ty.dtype in (f32, f16) and ty.dim() == 2 and tx.dim() == 2 and ty.stride(1) == 1 and tx.stride(1) == 1
    assert ty.stride(0) == tx.stride(0) and ty.shape[1] >= N and tx.shape[1] >= N
    return (_p(ty), _p(tx), ty.stride(0), ty.shape[0], tx.shape[0], int(ty.dtype == f16))


def gemm_x3(A: Act, W: Act, out, bias=None, residual=None, res_rows: int = 0, act: int = ACT_NONE, *, M=None, N=None, K=None,
            lda=None, ldw=None, ldc=None, batch: int = 1, strideA: int = 0, strideW: int = 0, strideC: int = 0, ldr=None,
            strideR: int = 0, pos=None, fixed_k_order: bool = False):
    """fixed_k_order: results of calls with different M / N are compared bit for bit (sharded retrieval): ring kernels only.
    out = act((A @ W^T) * W.out_scale + bias + pos) + residual[m % res_rows] at the reference's fp32-class precision: A and W
    are split pairs (Act with plane != 0); out is an f32 tensor, an fp16 tensor / plain Act, or a split Act (then the residual is
    added in fp32 before the one rounding, act must be none).  pos: see _pos()."""
    if not (isinstance(A, Act) and isinstance(W, Act) and A.plane and (W.plane or W.x2)):
        raise _lib.ZutisHipError("gemm_x3: A must be a split pair, W a split pair or a one-plane split_weight() pack")
    a, w = A.hi, W.hi
    M = a.shape[-2] if M is None else M
    K = a.shape[-1] if K is None else K
    N = w.shape[-2] if N is None else N
    lda = a.stride(-2) if lda is None else lda
    ldw = w.stride(-2) if ldw is None else ldw
    o, planeC = _hp(out)
    kind = 0 if o.dtype == f32 else (2 if planeC else 1)
    ldc = o.stride(-2) if ldc is None else ldc
    if residual is not None:
        assert residual.dtype == f32 and (kind == 0 or act == ACT_NONE)
        ldr = residual.stride(-2) if ldr is None else ldr
        res_rows = res_rows or M
    if bias is not None:
        assert bias.dtype == f32 and bias.numel() >= N
    args = (_p(a), lda, strideA, A.plane, _p(w), ldw, strideW, W.plane, _p(o), ldc, strideC, planeC, kind,
            float(A.out_scale * W.out_scale), _p(bias), _p(residual), ldr or 0, strideR, res_rows, *_pos(pos, N),
            act, M, N, K, batch, _ZH["ZH_GEMM_FIXED_K_ORDER"] if fixed_k_order else 0, _stream())
    nbytes = _gemm_bytes(M, N, K, batch, strideA, strideW, 4, 4 if kind == 0 else (4 if kind == 2 else 2), residual is not None)
    if not W.plane:                                  # one-plane weight: 2 bytes per element instead of 4
        nbytes -= N * K * 2.0 * (batch if (strideW or batch == 1) else 1)
    name = "gemm_f16x3" if W.plane else "gemm_f16x2"
    _launch(name, (2.0 * M * N * K * batch, nbytes, (M, N, K, batch)), "zh_gemm_f16x3", args)
    return out


def gemm(A: torch.Tensor, W: torch.Tensor, out: torch.Tensor, bias=None, residual=None, res_rows: int = 0,
         act: int = ACT_NONE, *, M=None, N=None, K=None, lda=None, ldw=None, ldc=None, batch: int = 1,
         strideA: int = 0, strideW: int = 0, strideC: int = 0, ldr=None, strideR: int = 0, pos=None):
    """out = act(A @ W^T + bias + pos) + residual[m % res_rows].  A [M,K] f16, W [N,K] f16, out f32|f16 [M,N]; pos: see _pos().
    Act operands / outputs are read / written through their hi plane (plain fp16).
    An fp16 residual (the half-precision residual stream) goes with an fp16 `out`, no activation and no pos tables:
    out = f16(f16(A @ W^T + bias) + residual[m % res_rows]), both additions in fp32 (zh_gemm_f16_res16); it may alias `out`."""
    for t in (A, W):
        if isinstance(t, Act) and t.out_scale != 1.0:   # a weight packed for the x3 mode is W * 2^s: its hi plane alone is not W
            raise _lib.ZutisHipError("gemm: operand packed with out_scale != 1 (split_weight) reached the fp16-operand GEMM")
    A, W, out_ret = _hp(A)[0], _hp(W)[0], out
    if isinstance(out, Act):
        if out.plane:
            raise _lib.ZutisHipError("gemm: an fp16-operand GEMM cannot fill a split-pair output (its lo plane would be stale)")
        out = out.hi
    M = A.shape[-2] if M is None else M
    K = A.shape[-1] if K is None else K
    N = W.shape[-2] if N is None else N
    lda = A.stride(-2) if lda is None else lda
    ldw = W.stride(-2) if ldw is None else ldw
    ldc = out.stride(-2) if ldc is None else ldc
    assert A.dtype == f16 and W.dtype == f16 and out.dtype in (f16, f32)
    if residual is not None:
        if residual.dtype == f16 and (out.dtype != f16 or act != ACT_NONE or pos is not None):
            raise _lib.ZutisHipError("gemm: an fp16 residual needs an fp16 out, no activation and no pos tables")
        assert residual.dtype in (f16, f32)
        ldr = residual.stride(-2) if ldr is None else ldr
        res_rows = res_rows or M
    if bias is not None:
        assert bias.dtype == f32 and bias.numel() >= N
    if residual is not None and residual.dtype == f16:
        args = (_p(A), lda, strideA, _p(W), ldw, strideW, _p(out), ldc, strideC, _p(bias), _p(residual), ldr, strideR, res_rows,
                M, N, K, batch, _stream())
        nbytes = _gemm_bytes(M, N, K, batch, strideA, strideW, 2, 2, True, res_bytes=2)
        _launch("gemm_f16", (2.0 * M * N * K * batch, nbytes, (M, N, K, batch)), "zh_gemm_f16_res16", args)
        return out_ret
    args = (_p(A), lda, strideA, _p(W), ldw, strideW, _p(out), ldc, strideC, int(out.dtype == f16),
            _p(bias), _p(residual), ldr or 0, strideR, res_rows, *_pos(pos, N), act, M, N, K, batch, _stream())
    nbytes = _gemm_bytes(M, N, K, batch, strideA, strideW, 2, 2 if out.dtype == f16 else 4, residual is not None)
    _launch("gemm_f16", (2.0 * M * N * K * batch, nbytes, (M, N, K, batch)), "zh_gemm_f16", args)
    return out_ret


def attention_splitk_workspace_size(batch, heads, Tq, head_dim, ksplit) -> int:
    return int(_lib.load(raw=True).zh_attention_splitk_workspace_size(batch, heads, Tq, head_dim, ksplit))


def attention(Q, K, V, O, *, batch, heads, Tq, Tk, head_dim, ldq, ldk, ldv, ldo, strideQ, strideK, strideV, strideO,
              scale=None, causal=False, x3=False, ksplit: int = 1, workspace=None):
    """x3: Q, K and V are split-pair Acts; scores and P.V get the three-product fp32-class form; a split O is filled as a pair.
    ksplit > 1: the keys are split over ksplit workgroups per (image, head, query block) and merged by a second launch; workspace =
    a uint8 CUDA tensor of attention_splitk_workspace_size() bytes."""
    scale = 1.0 / math.sqrt(head_dim) if scale is None else scale
    (Q, pq), (K, pk), (V, pv), (O, po) = _hp(Q), _hp(K), _hp(V), _hp(O)
    if x3 and not (pq and pk and pv):
        raise _lib.ZutisHipError("attention(x3): Q, K and V must be split pairs")
    if not x3:
        pq = pk = pv = 0
    name = "attention_f16x3" if x3 else "attention_f16"
    if causal:
        if Tq != Tk:
            raise _lib.ZutisHipError("causal attention needs Tq == Tk")
        ksplit = 1                               # the causal kernel has no split form
    if ksplit > 1:
        need = attention_splitk_workspace_size(batch, heads, Tq, head_dim, ksplit)
        if workspace is None or _nbytes(workspace) < need:
            raise _lib.ZutisHipError(f"attention(ksplit={ksplit}): workspace of {need} bytes required")
    head = (_p(Q), ldq, strideQ, _p(K), ldk, strideK, _p(V), ldv, strideV, _p(O), ldo, strideO, batch, heads, Tq)
    tail = (head_dim, float(scale), pq, pk, pv, po)
    if causal:
        entry, args = "zh_attention_causal_f16", head + tail
    elif ksplit > 1:
        entry, args = "zh_attention_f16_splitk", head + (Tk,) + tail + (ksplit, _p(workspace), _nbytes(workspace))
    else:
        entry, args = "zh_attention_f16", head + (Tk,) + tail
    _launch(name, (2.0 if causal else 4.0) * batch * heads * Tq * Tk * head_dim, entry, args + (_stream(),))
    return O


def embed_tokens(tokens, table, pos, out):
    """tokens int64 [n,ctx] -> out f32 [n*ctx, D] = table[tokens] + pos (clip_arch.py:535-537)."""
    n, ctx = tokens.shape
    _chk(table, f32, "token table"); _chk(pos, f32, "positional embedding"); _chk(out, f32, "embed out")
    if tokens.dtype != torch.int64 or not tokens.is_contiguous():
        raise _lib.ZutisHipError("embed_tokens: tokens must be contiguous int64")
    _call("zh_embed_tokens_f32", _p(tokens), _p(table), _p(pos), _p(out), n, ctx, table.shape[1], table.shape[0], _stream())


def eot_rows(tokens, x, out):
    n, ctx = tokens.shape
    _chk(x, f32, "eot x"); _chk(out, f32, "eot out")
    _call("zh_eot_rows_f32", _p(tokens), _p(x), _p(out), n, ctx, out.shape[1], _stream())


def group_mean_l2norm(x, out, groups, T, E):
    _chk(x, f32, "group mean x"); _chk(out, f32, "group mean out")
    _call("zh_group_mean_l2norm", _p(x), _p(out), groups, T, E, _stream())


STATUS_RANGE, STATUS_NONFINITE, STATUS_LABEL = _ZH["ZH_STATUS_RANGE"], _ZH["ZH_STATUS_NONFINITE"], _ZH["ZH_STATUS_LABEL"]     # bits of the status word
UNIT_NORM_SCALE = 1024.0                     # f16_scale of the unit-norm producers (2^10): see zutis_hip.h


def _group_map(rows, group_rows, group_stride):
    """Defaults of a row-group mapping (zutis_hip.h): one group of all `rows`, groups packed back to back."""
    group_rows = rows if group_rows is None else group_rows
    return group_rows, group_rows if group_stride is None else group_stride


def layernorm(x, gamma, beta, eps, rows, D, *, out_f32=None, out_f16=None, out_f16_plus=None, out_f32_plus=None,
              add=None, add_rows=0, in_group_rows=None, in_group_stride=None, in_offset=0,
              out_group_rows=None, out_group_stride=None, out_offset=0, status=None):
    in_group_rows, in_group_stride = _group_map(rows, in_group_rows, in_group_stride)
    out_group_rows, out_group_stride = _group_map(rows, out_group_rows, out_group_stride)
    (out_f16, p1), (out_f16_plus, p2) = _hp(out_f16), _hp(out_f16_plus)
    if out_f16 is not None and out_f16_plus is not None and p1 != p2:
        raise _lib.ZutisHipError("layernorm: both fp16 outputs must be split pairs of the same shape, or both plain")
    lo_plane = p1 or p2
    # an fp16 x is the half-precision residual stream: same addressing and outputs, fp32 statistics
    _call("zh_layernorm_f16" if x.dtype == f16 else "zh_layernorm_f32", _p(x), in_group_rows, in_group_stride, in_offset,
          out_group_rows, out_group_stride, out_offset, _p(gamma), _p(beta), float(eps),
          _p(out_f32), _p(out_f16), _p(out_f16_plus), _p(out_f32_plus), _p(add), add_rows,
          rows, D, lo_plane, _p(status), _stream())


def sum_layernorm(parts, n_parts, rows, D, *, part_stride=None, bias=None, residual=None, out_sum=None, gamma=None, beta=None, eps=1e-5,
                  out_f32=None, out_f16=None, out_group_rows=None, out_group_stride=None, out_offset=0, skip_first_in_group=False,
                  gamma2=None, beta2=None, eps2=1e-5, out2_f32=None, out2_f16=None, out2_group_rows=None, out2_group_stride=None, out2_offset=0,
                  status=None):
    """x = sum of the n_parts fp32 planes of `parts` + bias + residual -> out_sum; LN(x) -> out_f32 / out_f16 (row-mapped); LN(LN(x)) with
    gamma2 / beta2 -> out2_* (zh_sum_layernorm_f32).  n_parts = 1 with no bias / residual is a plain (or chained) LayerNorm."""
    part_stride = rows * D if part_stride is None else part_stride
    ogr, ogs = _group_map(rows, out_group_rows, out_group_stride)
    ogr2, ogs2 = _group_map(rows, out2_group_rows, out2_group_stride)
    (out_f16, lo1), (out2_f16, lo2) = _hp(out_f16), _hp(out2_f16)
    _call("zh_sum_layernorm_f32", _p(parts), n_parts, part_stride, _p(bias), _p(residual), _p(out_sum), _p(gamma), _p(beta), float(eps),
          _p(out_f32), _p(out_f16), lo1, ogr, ogs, out_offset, int(skip_first_in_group),
          _p(gamma2), _p(beta2), float(eps2), _p(out2_f32), _p(out2_f16), lo2, ogr2, ogs2, out2_offset,
          rows, D, _p(status), _stream())


def assemble_tokens_ln(patch_emb, cls, pos, gamma, beta, eps, out, B, T, D):
    """out f32 [B,T,D], or f16 (the half-precision residual stream: rounded once from the fp32 result)."""
    _call("zh_assemble_tokens_ln_f16" if out.dtype == f16 else "zh_assemble_tokens_ln", _p(patch_emb), _p(cls), _p(pos), _p(gamma), _p(beta),
          float(eps), _p(out), B, T, D, _stream())


def _f16_scale(a) -> float:
    """The factor a producer stores into Act `a` with: 1 / a.out_scale (a plain tensor or an unscaled Act: 1)."""
    return 1.0 / a.out_scale if isinstance(a, Act) else 1.0


def l2norm_rows(x, rows, D, out_f32=None, out_f16=None, eps=0.0):
    """out_f16 may be an Act with out_scale = 2^-s: the fp16 / split-pair copy is then stored times 2^s (unit-norm rows: UNIT_NORM_SCALE)."""
    sc = _f16_scale(out_f16)
    out_f16, lo = _hp(out_f16)
    _call("zh_l2norm_rows", _p(x), _p(out_f32), _p(out_f16), float(eps), rows, D, lo, sc, _stream())


def global_ln_l2_workspace_size(B, M, Cc) -> int:
    return int(_lib.load(raw=True).zh_global_ln_l2_workspace_size(B, M, Cc))


def global_ln_l2(x, B, M, Cc, out_f32=None, out_f16=None, eps=1e-5, l2_eps=1e-7, workspace=None, status=None):
    need = global_ln_l2_workspace_size(B, M, Cc)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
    sc = _f16_scale(out_f16)
    out_f16, lo = _hp(out_f16)
    _call("zh_global_ln_l2", _p(x), _p(out_f32), _p(out_f16), float(eps), float(l2_eps), B, M, Cc, _p(workspace),
          _nbytes(workspace), lo, sc, _p(status), _stream())


def im2col(x, out, patch, Kpad, pad_to_patch=False):
    B, Cin, H, W = x.shape
    _chk(x, f32, "im2col x")
    out, lo = _hp(out)
    _call("zh_im2col_f16", _p(x), _p(out), B, Cin, H, W, patch, Kpad, int(pad_to_patch), lo, _stream())


def posembed_bicubic(pos, out, grid, h, w, D, scale_h, scale_w, has_cls=True):
    _call("zh_posembed_bicubic", _p(pos), _p(out), grid, h, w, D, float(np.float32(scale_h)), float(np.float32(scale_w)), int(has_cls), _stream())


def upsample2x_cl(x, B, h, w, D, out_f32=None, out_f16=None, relu=False):
    out_f16, lo = _hp(out_f16)
    _call("zh_upsample2x_bilinear_cl", _p(x), _p(out_f32), _p(out_f16), B, h, w, D, lo, int(relu), _stream())


def sine_pe(out, h, w, D, temperature=10000.0):
    _call("zh_sine_pe", _p(out), h, w, D, float(temperature), _stream())


def add_rowperiodic_f16(a, add, out, rows, D, add_rows):
    (a, la), (out, lo) = _hp(a), _hp(out)
    _call("zh_add_rowperiodic_f16", _p(a), _p(add), _p(out), rows, D, add_rows, la, lo, _stream())


def fill_f32(x, value=0.0):
    _chk(x, f32, "fill x")
    _call("zh_fill_f32", _p(x), float(value), x.numel(), _stream())


def cast_f16(x, out, rows, D, add=None, add_rows=0):
    sc = _f16_scale(out)
    out, lo = _hp(out)
    _call("zh_cast_f32_f16", _p(x), _p(add), add_rows, _p(out), rows, D, lo, sc, _stream())


def lin_scale(in_size: int, out_size: int) -> float:
    """ATen area_pixel_compute_scale for size= calls: float32(in)/float32(out)."""
    return float(np.float32(in_size) / np.float32(out_size))


def upsample_argmax(logits_lo, labels, B, n, h, w, H, W):
    _call("zh_upsample_argmax", _p(logits_lo), _p(labels), B, n, h, w, H, W, lin_scale(h, H), lin_scale(w, W), _stream())


GT_FORMATS = {"u8": _ZH["ZH_GT_U8"], "rg16": _ZH["ZH_GT_RG16"]}


def upsample_argmax_score(logits_lo, gt, hist, B, n, h, w, H, W, gt_format: str = "u8", labels=None):
    """upsample_argmax with RunningScore._fast_hist fused in (zutis.py:366-372 + utils/running_score.py:11-16): hist int64 [n * n] +=
    bincount(n * gt + label) over the pixels with gt < n.  gt u8 [B,H,W] ("u8") or [B,H,W,3] ("rg16": R + 256 G, imagenet_s.py:93);
    labels: None (no label map is made) or int64 [B,H,W]."""
    _chk(logits_lo, f32, "upsample_argmax_score logits"); _chk(gt, torch.uint8, "upsample_argmax_score gt"); _chk(hist, torch.int64, "upsample_argmax_score hist")
    if gt_format not in GT_FORMATS:
        raise _lib.ZutisHipError(f"upsample_argmax_score: gt_format {gt_format!r} is not one of {sorted(GT_FORMATS)}")
    want = (B, H, W) if gt_format == "u8" else (B, H, W, 3)
    if tuple(logits_lo.shape) != (B, n, h, w) or tuple(gt.shape) != want or hist.numel() != n * n:
        raise _lib.ZutisHipError(f"upsample_argmax_score: logits {(B, n, h, w)}, gt {want}, hist [{n * n}] expected, got "
                                 f"{tuple(logits_lo.shape)}, {tuple(gt.shape)}, {tuple(hist.shape)}")
    if labels is not None:
        _chk(labels, torch.int64, "upsample_argmax_score labels")
        if tuple(labels.shape) != (B, H, W):
            raise _lib.ZutisHipError(f"upsample_argmax_score: labels {tuple(labels.shape)}, expected {(B, H, W)}")
    _call("zh_upsample_argmax_score", _p(logits_lo), _p(gt), GT_FORMATS[gt_format], _p(hist), _p(labels), B, n, h, w, H, W,
          lin_scale(h, H), lin_scale(w, W), _stream())


def _chk_overlay(name: str, overlay_out, packed, desc, desc_host, table_name: str, table, table_shape, alpha, B, H, W):
    """The overlay arguments of `name` (colour table `table_name`, u8 of `table_shape`) and, on desc_host when given (else on a blocking
    read of desc), every descriptor row's image of the overlay's size and inside packed: the kernels trust packed / desc."""
    _chk(overlay_out, torch.uint8, f"{name} overlay_out"); _chk(packed, torch.uint8, f"{name} packed")
    _chk(desc, torch.int32, f"{name} desc"); _chk(table, torch.uint8, f"{name} {table_name}")
    if tuple(overlay_out.shape) != (B, H, W, 3) or packed.dim() != 1 or tuple(desc.shape) != (B, 8) or tuple(table.shape) != table_shape:
        raise _lib.ZutisHipError(f"{name}: overlay_out {(B, H, W, 3)}, packed [bytes], desc {(B, 8)}, {table_name} {table_shape} expected, got "
                                 f"{tuple(overlay_out.shape)}, {tuple(packed.shape)}, {tuple(desc.shape)}, {tuple(table.shape)}")
    if int(alpha) != alpha or not 0 <= int(alpha) <= 256:
        raise _lib.ZutisHipError(f"{name}: alpha {alpha!r} is not an integer in 0..256")
    rows = (desc if desc_host is None else desc_host).cpu().numpy().reshape(B, 8)
    for b, (off, iw, ih) in enumerate(rows[:, :3].tolist()):
        if (iw, ih) != (W, H):
            raise _lib.ZutisHipError(f"{name}: descriptor row {b} holds a {iw} x {ih} image, the overlay is {W} x {H}")
        if off < 0 or off * 16 + 3 * W * H > packed.numel():
            raise _lib.ZutisHipError(f"{name}: descriptor row {b} places its image outside packed ({packed.numel()} bytes)")


def upsample_argmax_bytes(logits_lo, B, n, h, w, H, W, label_format: str = "u8", labels_out=None, overlay_out=None, packed=None, desc=None,
                          palette=None, alpha: int = 128, desc_host=None):
    """upsample_argmax with the label leaving as the bytes of the file it becomes (zutis.py:366-372; imagenet_s.py:93 read backwards):
    labels_out None or u8 [B,H,W] ("u8": the byte is the label, n <= 256) / u8 [B,H,W,3] ("rg16": R = label & 255, G = label >> 8, B = 0,
    n <= 65536); overlay_out None or u8 [B,H,W,3] = (img * (256 - alpha) + palette[label] * alpha + 128) >> 8, alpha an integer in 0..256,
    palette u8 [n,3], img the decoded images of a loader's staging buffer (packed u8 [bytes], desc int32 [B,8]: offset / 16, w, h, ...)
    at the output's own size.  Not both None.  The kernel trusts packed / desc: every row's (w, h) must be (W, H) and its image lie
    inside packed, which is checked HERE, on desc_host (the loader's host copy of the rows) when given, else on a blocking read of desc."""
    _chk(logits_lo, f32, "upsample_argmax_bytes logits")
    if label_format not in GT_FORMATS:
        raise _lib.ZutisHipError(f"upsample_argmax_bytes: label_format {label_format!r} is not one of {sorted(GT_FORMATS)}")
    if tuple(logits_lo.shape) != (B, n, h, w):
        raise _lib.ZutisHipError(f"upsample_argmax_bytes: logits {(B, n, h, w)} expected, got {tuple(logits_lo.shape)}")
    if labels_out is None and overlay_out is None:
        raise _lib.ZutisHipError("upsample_argmax_bytes: labels_out and overlay_out are both None")
    limit = 256 if label_format == "u8" else 65536
    if n > limit:
        raise _lib.ZutisHipError(f"upsample_argmax_bytes: {n} classes do not fit the label format {label_format!r} (at most {limit})")
    if labels_out is not None:
        _chk(labels_out, torch.uint8, "upsample_argmax_bytes labels_out")
        want = (B, H, W) if label_format == "u8" else (B, H, W, 3)
        if tuple(labels_out.shape) != want:
            raise _lib.ZutisHipError(f"upsample_argmax_bytes: labels_out {tuple(labels_out.shape)}, expected {want}")
    if overlay_out is not None:
        if packed is None or desc is None or palette is None:
            raise _lib.ZutisHipError("upsample_argmax_bytes: an overlay needs packed, desc and palette")
        _chk_overlay("upsample_argmax_bytes", overlay_out, packed, desc, desc_host, "palette", palette, (n, 3), alpha, B, H, W)
    else:
        packed = desc = palette = None
    _call("zh_upsample_argmax_bytes", _p(logits_lo), _p(labels_out), GT_FORMATS[label_format], _p(overlay_out), _p(packed), _p(desc), _p(palette),
          int(alpha), B, n, h, w, H, W, lin_scale(h, H), lin_scale(w, W), _stream())


def upsample_bilinear_nchw(x, planes, h, w, H, W, out=None, mask_u8=None, threshold=0.5, scale_h=None, scale_w=None):
    """scale_* default to in/out (size= form); pass 1/scale_factor for the scale_factor form with a cropped output."""
    sh = lin_scale(h, H) if scale_h is None else float(np.float32(scale_h))
    sw = lin_scale(w, W) if scale_w is None else float(np.float32(scale_w))
    _call("zh_upsample_bilinear_nchw", _p(x), _p(out), _p(mask_u8), float(threshold), planes, h, w, H, W, sh, sw, _stream())


def confusion_hist(label_true, label_pred, hist, n_class):
    _chk(label_true, torch.int64, "label_true")
    _chk(label_pred, torch.int64, "label_pred")
    _chk(hist, torch.int64, "hist")
    _call("zh_confusion_hist", _p(label_true), _p(label_pred), _p(hist), label_true.numel(), n_class, _stream())


def instance_mask_stats(mask_proposals_last, stride_image, threshold, B, Q, M, sizes, conf, binary, range_flag=None):
    """range_flag: int32 [1] (zeroed by the caller): bit 0 set when a proposal lies outside [0, 1] (zutis.py:385-386)."""
    _call("zh_instance_mask_stats", _p(mask_proposals_last), stride_image, float(threshold), B, Q, M, _p(sizes), _p(conf),
          _p(binary), _p(range_flag), _stream())


def masked_mean_tokens(tokens, binary, sizes, avg, B, Q, M, E):
    ws, need = _workspace("zh_masked_mean_workspace_size", tokens.device, B, Q, M, E)
    _call("zh_masked_mean_tokens", _p(tokens), _p(binary), _p(sizes), _p(avg), B, Q, M, E, _p(ws), need, _stream())


def instance_classify(avg, text, conf, temperature, rows, n, E, category, score):
    _call("zh_instance_classify", _p(avg), _p(text), _p(conf), float(temperature), rows, n, E, _p(category), _p(score), _stream())


def mask_iou_counts(masks_u8, n, pixels, inter, uni, workspace=None):
    """workspace (optional, >= zh_mask_iou_workspace_size bytes, any dtype): kept by the caller, it holds the masks bit-packed afterwards
    (u64 [n][(pixels + 63) // 64]: the `bits` of mask_rle_fused_kept)."""
    ws, need = _workspace_or(workspace, "mask_iou_counts", "zh_mask_iou_workspace_size", masks_u8.device, n, pixels)
    _call("zh_mask_iou_counts", _p(masks_u8), n, pixels, _p(inter), _p(uni), _p(ws), need, _stream())


NMS_TYPES = {"hard": 0, "linear": 1, "gaussian": 2}


def mask_nms(inter, uni, scores, category_ids, nms_type="hard", nms_threshold=0.3, sigma=0.5, score_threshold=0.001, packed=None,
             range_flag=None, zero_word=None):
    """Greedy per-category mask NMS on the device (zutis.py:211-299).  inter / uni int32 [B,Q,Q], scores f32 [B,Q], category_ids
    int64 [B,Q] -> (index int32 [B,Q], score f64 [B,Q], category int64 [B,Q], count int32 [B]); the first count[b] entries of
    row b are the kept queries in the reference's emission order."""
    B, Q = scores.shape
    _chk(inter, torch.int32, "nms inter"); _chk(uni, torch.int32, "nms union"); _chk(scores, f32, "nms scores")
    _chk(category_ids, torch.int64, "nms categories")
    if nms_type not in NMS_TYPES:
        raise AssertionError(nms_type)                     # reference: assert nms_type in ["hard", "linear", "gaussian"]
    dev = scores.device
    idx = torch.empty((B, Q), dtype=torch.int32, device=dev)
    sc = torch.empty((B, Q), dtype=torch.float64, device=dev)
    cat = torch.empty((B, Q), dtype=torch.int64, device=dev)
    cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    _call("zh_mask_nms", _p(inter), _p(uni), _p(scores), _p(category_ids), B, Q, NMS_TYPES[nms_type], float(nms_threshold),
          float(sigma), float(score_threshold), _p(idx), _p(sc), _p(cat), _p(cnt), _p(packed), _p(range_flag),
          None if zero_word is None else _p(zero_word), _stream())
    return idx, sc, cat, cnt


def mask_runs_kept(masks_u8, kept_index, kept_count, max_runs, pos, nr, ba, packed=False):
    """masks u8 [B,Q,H,W]; kept_index int32 [B,Q] / kept_count int32 [B] = zh_mask_nms' device outputs -> pos int32 [B*Q,max_runs], nr
    int32 [B*Q,2], ba int32 [B*Q,5] (row b*Q + j = image b's j-th kept mask; rows past the count are not written).  packed: pos is ONE
    int32 list (any length) that takes the kept masks' transitions back to back, min(#transitions, max_runs) each, as far as it reaches."""
    _chk(masks_u8, torch.uint8, "mask_runs_kept masks"); _chk(kept_index, torch.int32, "kept_index"); _chk(kept_count, torch.int32, "kept_count")
    _chk(pos, torch.int32, "mask_runs_kept pos")
    B, Q, H, W = masks_u8.shape
    if not packed and pos.numel() < B * Q * max_runs:
        raise _lib.ZutisHipError(f"mask_runs_kept: pos holds {pos.numel()} ints, the row form needs {B * Q * max_runs}")
    ws, need = _workspace("zh_mask_runs_workspace_size", masks_u8.device, B * Q, W)
    _call("zh_mask_runs_kept", _p(masks_u8), _p(kept_index), _p(kept_count), B, Q, H, W, max_runs, _p(pos), pos.numel() if packed else 0,
          _p(nr), _p(ba), _p(ws), need, _stream())


def mask_rle_kept(pos_packed, nr, kept_count, B, Q, max_runs, HW, out, out_len):
    """COCO RLE strings of the kept masks on the device from mask_runs_kept(packed=True)'s list: out u8 (any length) takes mask b*Q + j's
    string at 5 * off + 16 * rank (see include/zutis_hip.h), out_len int32 [B*Q] its length (-1: the caller encodes that mask itself)."""
    _chk(pos_packed, torch.int32, "mask_rle_kept positions"); _chk(nr, torch.int32, "mask_rle_kept nruns"); _chk(kept_count, torch.int32, "kept_count")
    _chk(out, torch.uint8, "mask_rle_kept out"); _chk(out_len, torch.int32, "mask_rle_kept out_len")
    _call("zh_mask_rle_kept", _p(pos_packed), pos_packed.numel(), _p(nr), _p(kept_count), B, Q, max_runs, HW, _p(out), out.numel(), _p(out_len),
          _stream())


def mask_rle_fused_supported(H, W, max_runs) -> bool:
    return bool(_lib.load(raw=True).zh_mask_rle_fused_supported(int(H), int(W), int(max_runs)))


def mask_rle_fused_kept(masks_u8, kept_index, kept_count, max_runs, out, cursor, info, bits=None):
    """Runs, box, area and COCO RLE string of the kept masks in one launch (include/zutis_hip.h): masks u8 [B,Q,H,W], kept_index int32
    [B,Q] / kept_count int32 [B] = zh_mask_nms' outputs; out u8 (any length) takes the strings, cursor int32 [1] (zeroed by the caller)
    places them, info int32 [B*Q, 8] = (offset, length or -1, xmin, ymin, xmax, ymax, area, transitions) per kept slot.  bits: the masks
    bit-packed by mask_iou_counts(..., workspace=) — int64 [B, Q, (H*W + 63) // 64] — read instead of the bytes."""
    _chk(masks_u8, torch.uint8, "mask_rle_fused_kept masks"); _chk(kept_index, torch.int32, "kept_index"); _chk(kept_count, torch.int32, "kept_count")
    _chk(out, torch.uint8, "mask_rle_fused_kept out"); _chk(cursor, torch.int32, "cursor"); _chk(info, torch.int32, "info")
    B, Q, H, W = masks_u8.shape
    if bits is not None:
        _chk(bits, torch.int64, "mask_rle_fused_kept bits")
        if bits.numel() != B * Q * ((H * W + 63) // 64):
            raise _lib.ZutisHipError(f"mask_rle_fused_kept: bits holds {bits.numel()} words, {B * Q * ((H * W + 63) // 64)} expected")
    _call("zh_mask_rle_fused_kept", _p(masks_u8), None if bits is None else _p(bits), _p(kept_index), _p(kept_count), B, Q, H, W, max_runs,
          _p(out), out.numel(), _p(cursor), _p(info), _stream())


PAINT_MAX_Q = _ZH["ZH_PAINT_MAX_Q"]      # zh_instance_paint: slots per image (its rank table lives in LDS)


def instance_paint_workspace_size(B, Q, H, W) -> int:
    return int(_lib.load(raw=True).zh_instance_paint_workspace_size(int(B), int(Q), int(H), int(W)))


def instance_paint(index, score, count, H, W, *, masks=None, bits=None, colours=None, alpha: int = 128, outline: bool = True,
                   min_score: float = 0.0, packed=None, desc=None, desc_host=None, id_format: str = "u8", ids_out=None, overlay_out=None,
                   workspace=None):
    """A picture of the kept instances (include/zutis_hip.h zh_instance_paint): index int32 [B,Q] / score f64 [B,Q] / count int32 [B] =
    mask_nms' outputs, read on the device; masks u8 [B,Q,H,W] or bits int64 [B,Q,(H*W + 63) // 64] (mask_iou_counts' workspace; read
    instead of the bytes when given).  ids_out None or u8 [B,H,W] ("u8", Q <= 255) / u8 [B,H,W,3] ("rg16"): slot + 1 of the painted slot
    (score > min_score) of highest score that covers the pixel, 0 for none; overlay_out None or u8 [B,H,W,3]: colours u8 [B,Q,3] (one per
    slot) blended over the decoded images of a loader's staging buffer (packed / desc as upsample_argmax_bytes takes and checks them,
    on desc_host when given) with alpha in 0..256, outline pixels in the pure colour.  Not both None.  Returns (ids_out, overlay_out)."""
    _chk(index, torch.int32, "instance_paint index"); _chk(score, torch.float64, "instance_paint score"); _chk(count, torch.int32, "instance_paint count")
    if index.dim() != 2 or tuple(score.shape) != tuple(index.shape) or tuple(count.shape) != (index.shape[0],):
        raise _lib.ZutisHipError(f"instance_paint: index [B,Q], score [B,Q], count [B] expected, got {tuple(index.shape)}, {tuple(score.shape)}, "
                                 f"{tuple(count.shape)}")
    (B, Q), H, W = index.shape, int(H), int(W)
    if id_format not in GT_FORMATS:
        raise _lib.ZutisHipError(f"instance_paint: id_format {id_format!r} is not one of {sorted(GT_FORMATS)}")
    if B < 1 or Q < 1 or H < 1 or W < 1:
        raise _lib.ZutisHipError(f"instance_paint: B, Q, H, W must be positive, got {(B, Q, H, W)}")
    if masks is None and bits is None:
        raise _lib.ZutisHipError("instance_paint: masks and bits are both None")
    if ids_out is None and overlay_out is None:
        raise _lib.ZutisHipError("instance_paint: ids_out and overlay_out are both None")
    if bits is not None:
        _chk(bits, torch.int64, "instance_paint bits")
        if bits.numel() != B * Q * ((H * W + 63) // 64):
            raise _lib.ZutisHipError(f"instance_paint: bits holds {bits.numel()} words, {B * Q * ((H * W + 63) // 64)} expected")
        masks = None
    else:
        _chk(masks, torch.uint8, "instance_paint masks")
        if tuple(masks.shape) != (B, Q, H, W):
            raise _lib.ZutisHipError(f"instance_paint: masks {tuple(masks.shape)}, expected {(B, Q, H, W)}")
    if ids_out is not None:
        _chk(ids_out, torch.uint8, "instance_paint ids_out")
        want = (B, H, W) if id_format == "u8" else (B, H, W, 3)
        if tuple(ids_out.shape) != want:
            raise _lib.ZutisHipError(f"instance_paint: ids_out {tuple(ids_out.shape)}, expected {want}")
    if overlay_out is not None:
        if packed is None or desc is None or colours is None:
            raise _lib.ZutisHipError("instance_paint: an overlay needs packed, desc and colours")
        _chk_overlay("instance_paint", overlay_out, packed, desc, desc_host, "colours", colours, (B, Q, 3), alpha, B, H, W)
    else:
        packed = desc = colours = None
    ws, need = _workspace_or(workspace, "instance_paint", "zh_instance_paint_workspace_size", index.device, B, Q, H, W)
    _call("zh_instance_paint", _p(masks), _p(bits), _p(index), _p(score), _p(count), _p(colours), int(alpha), int(bool(outline)), float(min_score),
          _p(packed), _p(desc), _p(ids_out), GT_FORMATS[id_format], _p(overlay_out), B, Q, H, W, _p(ws), need, _stream())
    return ids_out, overlay_out


# ---------------------------------------------------------------------------------------- CLIP image pre-processing
RCN_KMAX = _ZH["ZH_RCN_KMAX"]


def resize_crop_normalize(packed, desc, n_px: int, lut, out=None, kmax: Optional[int] = None):
    """utils/extract_image_embeddings.py:97-103 (Resize BICUBIC, CenterCrop, ToTensor, Normalize) for a ragged batch in one launch,
    bit-identical to Pillow + NumPy: packed u8 [bytes] (the decoded RGB images back to back at 16-byte-aligned offsets), desc int32
    [B, 8] = (offset / 16, w, h, nw, nh, left, top, 0) per image, lut f32 [3, 256] (zutis_amd.preprocess.normalise_table) ->
    f32 [B, 3, n_px, n_px].  kmax: the batch's largest tap count (zutis_amd.preprocess.ksize), which sizes the launch's LDS; None = the
    largest the kernel serves.  An image whose descriptor does not fit comes back as NaN (include/zutis_hip.h)."""
    _chk(packed, torch.uint8, "resize_crop_normalize packed"); _chk(desc, torch.int32, "resize_crop_normalize desc"); _chk(lut, f32, "resize_crop_normalize lut")
    if packed.dim() != 1 or desc.dim() != 2 or desc.shape[1] != 8 or desc.shape[0] == 0 or tuple(lut.shape) != (3, 256):
        raise _lib.ZutisHipError(f"resize_crop_normalize: packed [bytes], desc [B, 8], lut [3, 256] expected, got {tuple(packed.shape)}, {tuple(desc.shape)}, {tuple(lut.shape)}")
    B = desc.shape[0]
    if out is None:
        out = torch.empty((B, 3, n_px, n_px), dtype=f32, device=packed.device)
    _chk(out, f32, "resize_crop_normalize out")
    if tuple(out.shape) != (B, 3, n_px, n_px):
        raise _lib.ZutisHipError(f"resize_crop_normalize: out {tuple(out.shape)}, expected {(B, 3, n_px, n_px)}")
    _call("zh_resize_crop_normalize_u8", _p(packed), packed.numel(), _p(desc), B, n_px, RCN_KMAX if kmax is None else int(kmax), _p(lut), _p(out), _stream())
    return out


FILTERS = {"bilinear": _ZH["ZH_FILTER_BILINEAR"], "bicubic": _ZH["ZH_FILTER_BICUBIC"]}      # (= PIL.Image's values)


def resize_normalize(packed, desc, out_h: int, out_w: int, lut, filter: str = "bilinear", out=None, kmax: Optional[int] = None):
    """datasets/index_dataset.py:405-411 (TF.resize BILINEAR, to_tensor, normalize) for a ragged batch whose images all resize to
    out_h x out_w, in one launch and with no crop, bit-identical to Pillow + the fp32 normalisation: packed / desc / lut / kmax as for
    resize_crop_normalize, every desc row (offset / 16, w, h, out_w, out_h, 0, 0, 0) -> f32 [B, 3, out_h, out_w].  `filter`:
    "bilinear" or "bicubic" (zutis_amd.preprocess.ksize(..., filter) taps per output pixel)."""
    _chk(packed, torch.uint8, "resize_normalize packed"); _chk(desc, torch.int32, "resize_normalize desc"); _chk(lut, f32, "resize_normalize lut")
    if packed.dim() != 1 or desc.dim() != 2 or desc.shape[1] != 8 or desc.shape[0] == 0 or tuple(lut.shape) != (3, 256):
        raise _lib.ZutisHipError(f"resize_normalize: packed [bytes], desc [B, 8], lut [3, 256] expected, got {tuple(packed.shape)}, {tuple(desc.shape)}, {tuple(lut.shape)}")
    if filter not in FILTERS:
        raise _lib.ZutisHipError(f"resize_normalize: filter {filter!r} is not one of {sorted(FILTERS)}")
    B = desc.shape[0]
    if out is None:
        out = torch.empty((B, 3, out_h, out_w), dtype=f32, device=packed.device)
    _chk(out, f32, "resize_normalize out")
    if tuple(out.shape) != (B, 3, out_h, out_w):
        raise _lib.ZutisHipError(f"resize_normalize: out {tuple(out.shape)}, expected {(B, 3, out_h, out_w)}")
    _call("zh_resize_normalize_u8", _p(packed), packed.numel(), _p(desc), B, out_h, out_w, FILTERS[filter], RCN_KMAX if kmax is None else int(kmax),
          _p(lut), _p(out), _stream())
    return out


# ---------------------------------------------------------------------------------------- training samples (csrc/synth.hip)
def _synth_chk(desc, name):
    _chk(desc, torch.int32, f"{name} desc")
    if desc.dim() != 2 or desc.shape[1] != 32 or desc.shape[0] == 0:
        raise _lib.ZutisHipError(f"{name}: desc int32 [N, 32] expected, got {tuple(desc.shape)}")
    return desc.shape[0]


def synth_geometry(packed, desc, crop_size: int, ignore_index: int, kmax: int, fill_wh, work, out=None):
    """random_scale + random_crop + random_hflip of N sub-images (zutis_amd.synth): packed u8 [bytes], desc int32 [N, 32], work int32
    [N, 12] (initialised as include/zutis_hip.h says; receives the fill sums and the objects' boxes) -> u8 [N, C, C, 4] = (R, G, B, mask)."""
    N = _synth_chk(desc, "synth_geometry")
    _chk(packed, torch.uint8, "synth_geometry packed"); _chk(work, torch.int32, "synth_geometry work")
    if packed.dim() != 1 or tuple(work.shape) != (N, 12):
        raise _lib.ZutisHipError(f"synth_geometry: packed [bytes], work [N, 12] expected, got {tuple(packed.shape)}, {tuple(work.shape)}")
    C = int(crop_size)
    if out is None:
        out = torch.empty((N, C, C, 4), dtype=torch.uint8, device=packed.device)
    _chk(out, torch.uint8, "synth_geometry out")
    if tuple(out.shape) != (N, C, C, 4):
        raise _lib.ZutisHipError(f"synth_geometry: out {tuple(out.shape)}, expected {(N, C, C, 4)}")
    _call("zh_synth_geometry_u8", _p(packed), packed.numel(), _p(desc), N, C, int(ignore_index), int(kmax), int(fill_wh[0]), int(fill_wh[1]),
          _p(work), _p(out), _stream())
    return out


def synth_photometric(rgbm, desc, work):
    """ColorJitter in desc's order + RandomGrayscale on u8 [N, C, C, 4], in place."""
    N = _synth_chk(desc, "synth_photometric")
    _chk(rgbm, torch.uint8, "synth_photometric rgbm"); _chk(work, torch.int32, "synth_photometric work")
    if rgbm.dim() != 4 or rgbm.shape[0] != N or rgbm.shape[1] != rgbm.shape[2] or rgbm.shape[3] != 4 or tuple(work.shape) != (N, 12):
        raise _lib.ZutisHipError(f"synth_photometric: rgbm [N, C, C, 4], work [N, 12] expected, got {tuple(rgbm.shape)}, {tuple(work.shape)}")
    _call("zh_synth_photometric_u8", _p(rgbm), _p(desc), N, rgbm.shape[1], _p(work), _stream())
    return rgbm


def synth_blur(rgbm, desc, weights, out=None):
    """The separable Gaussian (weights f32 [N, ksize]) of the sub-images whose desc flags say blur -> a second u8 [N, C, C, 4]; the
    rows of the other sub-images are NOT written."""
    N = _synth_chk(desc, "synth_blur")
    _chk(rgbm, torch.uint8, "synth_blur rgbm"); _chk(weights, f32, "synth_blur weights")
    if rgbm.dim() != 4 or rgbm.shape[0] != N or rgbm.shape[1] != rgbm.shape[2] or rgbm.shape[3] != 4 or weights.dim() != 2 or weights.shape[0] != N:
        raise _lib.ZutisHipError(f"synth_blur: rgbm [N, C, C, 4], weights [N, ksize] expected, got {tuple(rgbm.shape)}, {tuple(weights.shape)}")
    if out is None:
        out = torch.empty_like(rgbm)
    _chk(out, torch.uint8, "synth_blur out")
    if out.shape != rgbm.shape:
        raise _lib.ZutisHipError(f"synth_blur: out {tuple(out.shape)}, expected {tuple(rgbm.shape)}")
    _call("zh_synth_blur_u8", _p(rgbm), _p(desc), _p(weights), N, rgbm.shape[1], weights.shape[1], _p(out), _stream())
    return out


def synth_compose(rgbm, blurred, desc, samples, work, lut, ignore_index: int):
    """copy_paste per output pixel + normalisation: samples int32 [B, 4] = (first sub-image, n, first one-hot row, 0) ->
    (image f32 [B, 3, C, C], semantic int64 [B, C, C], one-hot bool [sum n, C, C])."""
    N = _synth_chk(desc, "synth_compose")
    for t, name in ((rgbm, "rgbm"), (blurred, "blurred")):
        _chk(t, torch.uint8, f"synth_compose {name}")
        if t.dim() != 4 or t.shape[0] != N or t.shape[1] != t.shape[2] or t.shape[3] != 4 or t.shape != rgbm.shape:
            raise _lib.ZutisHipError(f"synth_compose: {name} [N, C, C, 4] expected, got {tuple(t.shape)}")
    _chk(samples, torch.int32, "synth_compose samples"); _chk(work, torch.int32, "synth_compose work"); _chk(lut, f32, "synth_compose lut")
    if samples.dim() != 2 or samples.shape[1] != 4 or samples.shape[0] == 0 or tuple(work.shape) != (N, 12) or tuple(lut.shape) != (3, 256):
        raise _lib.ZutisHipError(f"synth_compose: samples [B, 4], work [N, 12], lut [3, 256] expected, got {tuple(samples.shape)}, {tuple(work.shape)}, {tuple(lut.shape)}")
    B, C = samples.shape[0], rgbm.shape[1]
    image = torch.empty((B, 3, C, C), dtype=f32, device=rgbm.device)
    semantic = torch.empty((B, C, C), dtype=torch.int64, device=rgbm.device)
    onehot = torch.empty((N, C, C), dtype=torch.bool, device=rgbm.device)
    _call("zh_synth_compose", _p(rgbm), _p(blurred), _p(desc), _p(samples), _p(work), _p(lut), N, B, C, int(ignore_index), _p(image), _p(semantic),
          _p(onehot), _stream())
    return image, semantic, onehot


# ---------------------------------------------------------------------------------------- bilateral solver (float64)
def _caller_buffer(t, dtype, shape, name: str):
    """A caller's output buffer viewed as `shape`: contiguous, of `dtype`, with exactly as many elements."""
    _chk(t, dtype, name)
    n = 1
    for d in shape:
        n *= int(d)
    if t.numel() != n:
        raise _lib.ZutisHipError(f"{name}: holds {t.numel()} elements, {n} needed for {tuple(shape)}")
    return t.view(shape)


def denormalize_u8(x, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), out=None):
    """utils/utils.py:261-273 on device: x f32 [3,H,W] -> rgb u8 [H,W,3] (out: the caller's buffer of H*W*3 bytes)."""
    import ctypes as C
    _chk(x, f32, "denormalize x")
    _, H, W = x.shape
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=x.device) if out is None else _caller_buffer(out, torch.uint8, (H, W, 3), "denormalize out")
    m = (C.c_float * 3)(*[float(np.float32(v)) for v in mean])
    s = (C.c_float * 3)(*[float(np.float32(v)) for v in std])
    _call("zh_denormalize_u8", _p(x), _p(out), H, W, m, s, _stream())
    return out


def bgrid_coords(rgb_u8, sigma_spatial=16, sigma_luma=16, sigma_chroma=8, out=None):
    H, W, _ = rgb_u8.shape
    _chk(rgb_u8, torch.uint8, "rgb")
    out = torch.empty((H * W, 5), dtype=torch.int32, device=rgb_u8.device) if out is None else _caller_buffer(out, torch.int32, (H * W, 5), "bgrid_coords out")
    _call("zh_bgrid_coords", _p(rgb_u8), H, W, float(sigma_spatial), float(sigma_luma), float(sigma_chroma), _p(out), _stream())
    return out


def bilateral_workspace_size(H, W, sigma_spatial=16, sigma_luma=16, sigma_chroma=8) -> int:
    """Bytes of workspace ONE H x W image needs (a batch needs B times that)."""
    return int(_lib.load(raw=True).zh_bilateral_workspace_size(H, W, float(sigma_spatial), float(sigma_luma), float(sigma_chroma)))


def bilateral_solve(rgb_u8, target, sigma_spatial=16, sigma_luma=16, sigma_chroma=8, confidence=0.999, lam=256.0,
                    a_diag_min=1e-5, cg_tol=1e-5, cg_maxiter=25, debug=False, workspace=None, out=None, stats=None):
    """rgb u8 [H,W,3] + target u8|f64 [H,W] (device) -> soft f64 [H,W] (device), stats int32 [2] (device)
    [, n, m f64 [H*W] when debug].  A batch ([B,H,W,3] + [B,H,W]) returns [B,H,W], [B,2] (, [B,H*W] x 2): one sequence of
    launches for all B images.
    Caller buffers (optional; each contiguous, of the dtype and element count of what it replaces, and returned viewed at that
    shape): `workspace` (any dtype, >= B * bilateral_workspace_size(...) bytes; whatever it holds is overwritten), `out` f64,
    `stats` int32, and `debug=(n, m)`, a pair of f64 buffers of B*H*W elements of which the first V of each image's row are written."""
    batched = rgb_u8.dim() == 4
    r4 = rgb_u8 if batched else rgb_u8[None]
    t3 = target if batched else target[None]
    B, H, W, _ = r4.shape
    _chk(r4, torch.uint8, "rgb")
    assert t3.shape == (B, H, W) and t3.is_contiguous() and t3.dtype in (torch.uint8, torch.float64)
    need = B * bilateral_workspace_size(H, W, sigma_spatial, sigma_luma, sigma_chroma)
    dev = r4.device
    ws = workspace if workspace is not None else torch.empty(need, dtype=torch.uint8, device=dev)
    if not ws.is_contiguous() or _nbytes(ws) < need:
        raise _lib.ZutisHipError(f"bilateral_solve: workspace holds {_nbytes(ws)} bytes (contiguous={ws.is_contiguous()}), {need} needed")
    out = torch.empty((B, H, W), dtype=torch.float64, device=dev) if out is None else _caller_buffer(out, torch.float64, (B, H, W), "bilateral_solve out")
    stats = torch.zeros((B, 2), dtype=torch.int32, device=dev) if stats is None else _caller_buffer(stats, torch.int32, (B, 2), "bilateral_solve stats")
    if debug is True:
        n = torch.zeros((B, H * W), dtype=torch.float64, device=dev)
        m = torch.zeros((B, H * W), dtype=torch.float64, device=dev)
    elif debug:
        n, m = (_caller_buffer(d, torch.float64, (B, H * W), "bilateral_solve debug") for d in debug)
    else:
        n = m = None
    t8 = t3 if t3.dtype == torch.uint8 else None
    t64 = t3 if t3.dtype == torch.float64 else None
    _call("zh_bilateral_solve_batch", _p(r4), _p(t8), _p(t64), B, H, W, float(sigma_spatial), float(sigma_luma), float(sigma_chroma),
          float(confidence), float(lam), float(a_diag_min), float(cg_tol), int(cg_maxiter), _p(out),
          _p(stats), _p(n), _p(m), _p(ws), need, _stream())
    if not batched:
        out, stats = out[0], stats[0]
        n, m = (n[0], m[0]) if debug else (None, None)
    return (out, stats, n, m) if debug else (out, stats)


def threshold_f64_u8(x, threshold=0.5, out=None):
    """x f64 (device, contiguous) -> u8 {0,1} of the same shape: x > threshold (out: the caller's buffer of x.numel() bytes)."""
    _chk(x, torch.float64, "threshold x")
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if out is None else _caller_buffer(out, torch.uint8, tuple(x.shape), "threshold out")
    _call("zh_threshold_f64_u8", _p(x), float(threshold), _p(out), x.numel(), _stream())
    return out


def components_workspace_size(H, W) -> int:
    """Bytes of workspace ONE H x W image needs in second_largest_component (a batch needs B times that)."""
    return int(_lib.load(raw=True).zh_components_workspace_size(int(H), int(W)))


def second_largest_component(x, threshold=0.5, *, filled=None, labels=None, stats=None, workspace=None, out=None):
    """utils/bilateral_solver.py:185-193 on the device (zutis_amd/components.py is the definition): x f64 (foreground = x > threshold,
    NaN is background) or u8 (non-zero), [H,W] or [B,H,W] -> u8 {0,1} mask of the same shape: holes filled, 4-connected components,
    the second largest under the key (count, label), all ones without an object.  One sequence of launches for all B images.
    Caller buffers, as in bilateral_solve (each contiguous, of the dtype and element count of what it fills, returned viewed at its
    shape): `out` u8 (the mask), `stats` int32 [B,4] = {nr_objects, chosen label, chosen count, fallback}, `workspace` (any dtype,
    >= B * components_workspace_size(H, W) bytes) and the optional outputs `filled` u8 (the filled foreground) and `labels` int32
    (scipy's numbering) — pass True to have one allocated.  Returns the mask, or (mask, stats[, filled][, labels]) when any of
    stats / filled / labels was asked for."""
    batched = x.dim() == 3
    x3 = x if batched else x[None]
    if x3.dim() != 3 or x3.dtype not in (torch.float64, torch.uint8) or not x3.is_contiguous():
        raise _lib.ZutisHipError(f"second_largest_component: expected contiguous f64 or u8 [H,W] / [B,H,W], got {x.dtype} {tuple(x.shape)}")
    B, H, W = x3.shape
    dev = x3.device
    need = B * components_workspace_size(H, W)
    ws = workspace if workspace is not None else torch.empty(need, dtype=torch.uint8, device=dev)
    if not ws.is_contiguous() or _nbytes(ws) < need:
        raise _lib.ZutisHipError(f"second_largest_component: workspace holds {_nbytes(ws)} bytes (contiguous={ws.is_contiguous()}), {need} needed")
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if out is None else _caller_buffer(out, torch.uint8, (B, H, W), "second_largest_component out")
    want_stats = stats is not None
    st = torch.empty((B, 4), dtype=torch.int32, device=dev) if stats is None or stats is True else _caller_buffer(stats, torch.int32, (B, 4), "second_largest_component stats")
    fl = lb = None
    if filled is not None:
        fl = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if filled is True else _caller_buffer(filled, torch.uint8, (B, H, W), "second_largest_component filled")
    if labels is not None:
        lb = torch.empty((B, H, W), dtype=torch.int32, device=dev) if labels is True else _caller_buffer(labels, torch.int32, (B, H, W), "second_largest_component labels")
    soft = x3 if x3.dtype == torch.float64 else None
    binary = x3 if x3.dtype == torch.uint8 else None
    _call("zh_second_largest_component", _p(soft), _p(binary), float(threshold), B, H, W, _p(mask), _p(fl), _p(lb), _p(st), _p(ws), _nbytes(ws), _stream())
    if not batched:
        mask, st, fl, lb = mask[0], st[0], (None if fl is None else fl[0]), (None if lb is None else lb[0])
    if not (want_stats or fl is not None or lb is not None):
        return mask
    return (mask, st) + ((fl,) if fl is not None else ()) + ((lb,) if lb is not None else ())


def select_upsample_mask(obj, masks, out_u8, index, B, Q, h, w, H, W, scale_h, scale_w, threshold=0.5):
    _chk(obj, f32, "objectness"); _chk(masks, f32, "masks"); _chk(out_u8, torch.uint8, "mask out")
    _call("zh_select_upsample_mask", _p(obj), _p(masks), _p(out_u8), _p(index), B, Q, h, w, H, W, float(scale_h), float(scale_w),
          float(threshold), _stream())


def resize_nearest_u8(x_u8, H, W, out=None):
    """F.interpolate(x[None,None], size=(H,W), mode="nearest")[0,0] for a u8 [h,w] mask on the GPU (into `out` u8 [H,W] when given)."""
    _chk(x_u8, torch.uint8, "resize_nearest x")
    h, w = x_u8.shape
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint8, device=x_u8.device)
    _chk(out, torch.uint8, "resize_nearest out")
    if tuple(out.shape) != (H, W):
        raise _lib.ZutisHipError(f"resize_nearest: out {tuple(out.shape)}, expected {(H, W)}")
    _call("zh_resize_nearest_u8", _p(x_u8), _p(out), h, w, H, W, lin_scale(h, H), lin_scale(w, W), _stream())
    return out


def topk_rows(scores, k, N=None, with_values=False, idx_map=None, idx_add=0, out_idx=None, out_val=None):
    """scores f32 [R, ld] on the GPU -> int64 [R,k] indices of the k largest of the first N columns: NaNs of either sign first, then
    score descending with -0.0 == +0.0, ties by ascending column (torch.sort(descending=True, stable=True)); values as stored.
    Reported index of column i = idx_map[r, i] (int64 [R, ld]) if given, else i + idx_add.  out_idx / out_val may be column
    blocks [R, k] of wider row-major tables (same row stride for both)."""
    _chk(scores, f32, "topk scores")
    R, ld = scores.shape
    N = ld if N is None else N
    if idx_map is not None:
        _chk(idx_map, torch.int64, "topk idx_map")
        if tuple(idx_map.shape) != (R, ld):
            raise _lib.ZutisHipError("topk_rows: idx_map must have the shape of scores")
    idx = torch.empty((R, k), dtype=torch.int64, device=scores.device) if out_idx is None else out_idx
    val = (torch.empty((R, k), dtype=f32, device=scores.device) if out_val is None else out_val) if with_values else None
    if idx.dtype != torch.int64 or idx.stride(1) != 1 or (val is not None and (val.dtype != f32 or val.stride() != idx.stride())):
        raise _lib.ZutisHipError("topk_rows: outputs must be int64 / f32 row-major blocks with equal row strides")
    _call("zh_topk_rows", _p(scores), ld, R, N, k, _p(idx_map), int(idx_add), _p(idx), _p(val), idx.stride(0), _stream())
    return (idx, val) if with_values else idx


def mask_runs(masks_u8, sel, max_runs=8192):
    """masks u8 [n,H,W] (device), sel int32 [m] (device) -> (positions int32 [m,max_runs], nruns int32 [m,2], box_area int32 [m,5])."""
    _chk(masks_u8, torch.uint8, "mask_runs masks")
    _chk(sel, torch.int32, "mask_runs sel")
    n, H, W = masks_u8.shape
    m = sel.numel()
    pos = torch.empty((m, max_runs), dtype=torch.int32, device=masks_u8.device)
    nr = torch.empty((m, 2), dtype=torch.int32, device=masks_u8.device)
    ba = torch.empty((m, 5), dtype=torch.int32, device=masks_u8.device)
    ws, need = _workspace("zh_mask_runs_workspace_size", masks_u8.device, m, W)
    _call("zh_mask_runs", _p(masks_u8), _p(sel), m, H, W, max_runs, _p(pos), _p(nr), _p(ba), _p(ws), need, _stream())
    return pos, nr, ba


POLYGON_LDS_CROSSINGS = _ZH["ZH_POLYGON_LDS_CROSSINGS"]     # crossings of one annotation's polygons the kernel sorts in LDS


def polygon_runs(xs, ys, step_pref, vert_off, poly_off, hw, out_off, flags, counts, n_runs):
    """zutis_amd/polygons.pack's arrays as int32 device tensors (xs, ys [V]; step_pref [V + P]; vert_off [P + 1]; poly_off, out_off
    [A + 1]; hw [A, 2] or [2 A]; flags [A]) -> counts int32 [>= out_off[-1], the caller's figure] and n_runs int32 [A] (-1: left to
    the host), written in place."""
    for name, t in (("xs", xs), ("ys", ys), ("step_pref", step_pref), ("vert_off", vert_off), ("poly_off", poly_off), ("hw", hw),
                    ("out_off", out_off), ("flags", flags), ("counts", counts), ("n_runs", n_runs)):
        _chk(t, torch.int32, f"polygon_runs {name}")
    A, P, V = n_runs.numel(), vert_off.numel() - 1, xs.numel()
    if (P < 0 or ys.numel() != V or step_pref.numel() != V + P or poly_off.numel() != A + 1 or out_off.numel() != A + 1
            or hw.numel() != 2 * A or flags.numel() != A):
        raise _lib.ZutisHipError("polygon_runs: the arrays' lengths do not describe one packed batch (zutis_amd/polygons.pack)")
    _call("zh_polygon_runs", _p(xs), _p(ys), _p(step_pref), _p(vert_off), _p(poly_off), _p(hw), _p(flags), _p(out_off), A, _p(counts),
          _p(n_runs), _stream())


def rle_prefix(counts, run_off, hw, run_end, run_fg, area, status):
    """zh_rle_prefix of n masks whose run counts lie on the device: counts int32 [R] (mask m's at run_off[m] .. run_off[m + 1] - 1,
    run_off int32 [n + 1]), hw int32 [n] = h * w -> run_end, run_fg int32 [R], area int32 [n], and the masks' bits ORed into status int32
    [(n + 31) // 32] (zeroed by the caller), written in place."""
    for name, t in (("counts", counts), ("run_off", run_off), ("hw", hw), ("run_end", run_end), ("run_fg", run_fg), ("area", area),
                    ("status", status)):
        _chk(t, torch.int32, f"rle_prefix {name}")
    n = hw.numel()
    if (run_off.numel() != n + 1 or area.numel() != n or status.numel() < (n + 31) // 32 or run_end.numel() != counts.numel()
            or run_fg.numel() != counts.numel()):
        raise _lib.ZutisHipError("rle_prefix: the arrays' lengths do not describe n masks and their runs")
    if n:
        _call("zh_rle_prefix", _p(counts), _p(run_off), _p(hw), n, _p(run_end), _p(run_fg), _p(area), _p(status), _stream())


OVERLAP_MODES = {"last": _ZH["ZH_OVERLAP_LAST"], "ignore": _ZH["ZH_OVERLAP_IGNORE"]}
LABEL_TILE_W, LABEL_TILE_H = _ZH["ZH_LABEL_TILE_W"], _ZH["ZH_LABEL_TILE_H"]


def label_tiles(h: int, w: int) -> int:
    """Workgroups zh_runs_label_maps spends on an h x w image."""
    return -(-int(w) // LABEL_TILE_W) * -(-int(h) // LABEL_TILE_H) if h > 0 and w > 0 else 0


def runs_label_maps(run_end, run_off, status, list_off, list_mask, list_label, hw, out_off, out, max_tiles, overlap="last",
                    ignore_value=255):
    """The label maps of B images in one launch (zh_runs_label_maps).  run_end int32 [R], run_off int32 [n + 1], status int32 [>= (n + 31)
    // 32]: n masks as rle_prefix leaves them; list_off int32 [B + 1], list_mask int32 [N], list_label u8 [N]: the images' paint lists;
    hw int32 [B, 2] = (h, w); out_off int64 [B + 1]; out u8 (any shape, contiguous): image b's [h, w] map at out_off[b] of its bytes;
    max_tiles: the largest label_tiles(h, w) of the batch (the caller holds hw on the host).  Everything on the device; nothing is
    copied.  Returns out."""
    for name, t in (("run_end", run_end), ("run_off", run_off), ("status", status), ("list_off", list_off), ("list_mask", list_mask),
                    ("hw", hw)):
        _chk(t, torch.int32, f"runs_label_maps {name}")
    _chk(list_label, torch.uint8, "runs_label_maps list_label")
    _chk(out_off, torch.int64, "runs_label_maps out_off")
    _chk(out, torch.uint8, "runs_label_maps out")
    if overlap not in OVERLAP_MODES:
        raise _lib.ZutisHipError(f"runs_label_maps: overlap {overlap!r} is not one of {sorted(OVERLAP_MODES)}")
    if not 0 <= int(ignore_value) <= 255:
        raise _lib.ZutisHipError(f"runs_label_maps: ignore_value {ignore_value!r} is not a byte")
    B, n, N = list_off.numel() - 1, run_off.numel() - 1, list_mask.numel()
    if B < 0 or n < 0 or hw.numel() != 2 * B or out_off.numel() != B + 1 or list_label.numel() != N or status.numel() < (n + 31) // 32:
        raise _lib.ZutisHipError("runs_label_maps: the arrays' lengths do not describe B images, their lists and n masks")
    if B > 65535:
        raise _lib.ZutisHipError(f"runs_label_maps: {B} images in one launch, at most 65535")
    if B and int(max_tiles) > 0:
        _call("zh_runs_label_maps", _p(run_end) if run_end.numel() else None, _p(run_off), _p(status), n, run_end.numel(), _p(list_off),
              _p(list_mask) if N else None, _p(list_label) if N else None, N, _p(hw), _p(out_off), B, int(max_tiles), OVERLAP_MODES[overlap],
              int(ignore_value), _p(out), out.numel(), _stream())
    return out


PNG_SEGMENT_BYTES = _ZH["ZH_PNG_SEGMENT_BYTES"]


def png_deflate(images, img_off, hw, c, out, out_off, lengths, max_segments, workspace=None):
    """The zlib streams of the PNGs of B images in one call (zh_png_deflate; png_device.deflate_np byte for byte).  images u8 (any shape,
    contiguous): image b is [h, w, c] at img_off[b] of its bytes; img_off int64 [B], hw int32 [B, 2] = (h, w), c 1 or 3; out u8: image b's
    stream at out_off[b] (int64 [B]), laid out by the caller at png_device.stream_bound strides; lengths int32 [B]: the streams' lengths
    (-1: the image does not fit, see zutis_hip.h); max_segments: the largest png_device.segments(h, w, c) of the batch (the caller holds
    the sizes on the host).  Everything on the device; nothing is copied.  Returns lengths."""
    _chk(images, torch.uint8, "png_deflate images"); _chk(out, torch.uint8, "png_deflate out")
    _chk(img_off, torch.int64, "png_deflate img_off"); _chk(out_off, torch.int64, "png_deflate out_off")
    _chk(hw, torch.int32, "png_deflate hw"); _chk(lengths, torch.int32, "png_deflate lengths")
    if c not in (1, 3):
        raise _lib.ZutisHipError(f"png_deflate: c {c!r} is not 1 or 3")
    B = img_off.numel()
    if hw.numel() != 2 * B or out_off.numel() != B or lengths.numel() != B:
        raise _lib.ZutisHipError("png_deflate: img_off [B], hw [B, 2], out_off [B] and lengths [B] do not describe one batch")
    if B > 65535:
        raise _lib.ZutisHipError(f"png_deflate: {B} images in one call, at most 65535")
    if B and int(max_segments) < 1:
        raise _lib.ZutisHipError(f"png_deflate: max_segments {max_segments!r} for {B} images")
    if B:
        ws, need = _workspace_or(workspace, "png_deflate", "zh_png_deflate_workspace_size", images.device, B, int(max_segments))
        _call("zh_png_deflate", _p(images), images.numel(), _p(img_off), _p(hw), int(c), B, int(max_segments), _p(out_off), _p(out), out.numel(),
              _p(lengths), _p(ws), need, _stream())
    return lengths


def jpeg_encode(images, img_off, hw, subsampling, quant, out, out_off, slot_bytes, lengths, max_mcus, workspace=None):
    """The entropy-coded scans of the baseline JPEGs of B RGB images in one call (zh_jpeg_encode; jpeg_device.scan_np byte for byte).
    images u8 (any shape, contiguous): image b is [h, w, 3] at img_off[b] of its bytes; img_off int64 [B], hw int32 [B, 2] = (h, w);
    subsampling 0 (4:4:4) or 2 (4:2:0); quant u16 / int16 [2, 64]: jpeg_device.quant_tables on the device; out u8: image b's scan at
    out_off[b] (int64 [B]), at most slot_bytes of it; lengths int32 [B]: the TRUE lengths (above slot_bytes: the scan did not fit and the
    caller encodes that image another way; -1: the image does not fit, see zutis_hip.h); max_mcus: the most MCUs of an image of the
    batch (the caller holds the sizes on the host).  Everything on the device; nothing is copied.  Returns lengths."""
    _chk(images, torch.uint8, "jpeg_encode images"); _chk(out, torch.uint8, "jpeg_encode out")
    _chk(img_off, torch.int64, "jpeg_encode img_off"); _chk(out_off, torch.int64, "jpeg_encode out_off")
    _chk(hw, torch.int32, "jpeg_encode hw"); _chk(lengths, torch.int32, "jpeg_encode lengths")
    if quant.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)):
        raise _lib.ZutisHipError(f"jpeg_encode quant: a 16-bit integer tensor expected, got {quant.dtype}")
    _chk(quant, quant.dtype, "jpeg_encode quant")
    if subsampling not in (0, 2):
        raise _lib.ZutisHipError(f"jpeg_encode: subsampling {subsampling!r} is not 0 (4:4:4) or 2 (4:2:0)")
    B = img_off.numel()
    if hw.numel() != 2 * B or out_off.numel() != B or lengths.numel() != B or quant.numel() != 128:
        raise _lib.ZutisHipError("jpeg_encode: img_off [B], hw [B, 2], out_off [B], lengths [B] and quant [2, 64] do not describe one batch")
    if B > 65535:
        raise _lib.ZutisHipError(f"jpeg_encode: {B} images in one call, at most 65535")
    if B and (int(max_mcus) < 1 or int(slot_bytes) < 0):
        raise _lib.ZutisHipError(f"jpeg_encode: max_mcus {max_mcus!r} / slot_bytes {slot_bytes!r} for {B} images")
    if B:
        ws, need = _workspace_or(workspace, "jpeg_encode", "zh_jpeg_encode_workspace_size", images.device, B, int(max_mcus), int(subsampling))
        _call("zh_jpeg_encode", _p(images), images.numel(), _p(img_off), _p(hw), B, int(subsampling), int(max_mcus), _p(quant), _p(out_off), _p(out),
              out.numel(), int(slot_bytes), _p(lengths), _p(ws), need, _stream())
    return lengths


def jpeg_decode(scan, segments, images, tables, n_blocks, max_image_blocks, max_image_pixels, out, status, workspace=None):
    """B baseline JPEG files to interleaved RGB in one call (zh_jpeg_decode; jpeg_device.decode_np byte for byte).  The arrays of
    jpeg_device.pack on the device: scan u8 [bytes], segments int32 [S, 4], images int32 [B, 12], tables u8 [n_sets, TABLE_SET_BYTES];
    n_blocks / max_image_blocks / max_image_pixels: the batch's 8 x 8 blocks and its largest image's blocks and pixels (the caller holds
    the plans on the host); out u8 [bytes]: image b's [h, w, 3] at 16 x its row's offset word; status int32 [B]: 0 or the OR of
    jpeg_device.STATUS bits (the image is then left to the host).  Everything on the device; nothing is copied.  Returns status."""
    _chk(scan, torch.uint8, "jpeg_decode scan"); _chk(out, torch.uint8, "jpeg_decode out"); _chk(tables, torch.uint8, "jpeg_decode tables")
    _chk(segments, torch.int32, "jpeg_decode segments"); _chk(images, torch.int32, "jpeg_decode images"); _chk(status, torch.int32, "jpeg_decode status")
    B = images.shape[0] if images.dim() == 2 else -1
    if B < 0 or images.shape[1] != _ZH["ZH_JPEG_IMAGE_WORDS"] or segments.dim() != 2 or segments.shape[1] != _ZH["ZH_JPEG_SEGMENT_WORDS"] or \
            tables.dim() != 2 or tables.shape[1] != _ZH["ZH_JPEG_TABLE_SET_BYTES"] or status.numel() != B:
        raise _lib.ZutisHipError("jpeg_decode: segments [S, 4], images [B, 12], tables [n_sets, TABLE_SET_BYTES] and status [B] do not describe one batch")
    if B:
        ws, need = _workspace_or(workspace, "jpeg_decode", "zh_jpeg_decode_workspace_size", out.device, B, int(n_blocks))
        _call("zh_jpeg_decode", _p(scan), scan.numel(), _p(segments), segments.shape[0], _p(images), B, _p(tables), tables.shape[0], int(n_blocks),
              int(max_image_blocks), int(max_image_pixels), _p(out), out.numel(), _p(status), _p(ws), need, _stream())
    return status


def jpeg_decode_split(scan, segments, chunks, images, tables, n_blocks, max_image_blocks, max_image_pixels, out, status, chunk_bytes=None, passes=None,
                      workspace=None):
    """jpeg_decode with every segment's entropy stage split among lanes (zh_jpeg_decode_split): chunks int32 [C, 4] are the rows of
    jpeg_device.chunk_rows at chunk_bytes (default: jpeg_device.CHUNK_BYTES), passes the synchronising launches (default:
    jpeg_device.SPLIT_PASSES).  An image whose chunks did not all start from verified states has the `unsynced` bit in its status and is
    left to the host like any other non-zero status; every other image's pixels are jpeg_decode's.  Returns status."""
    _chk(scan, torch.uint8, "jpeg_decode_split scan"); _chk(out, torch.uint8, "jpeg_decode_split out"); _chk(tables, torch.uint8, "jpeg_decode_split tables")
    _chk(segments, torch.int32, "jpeg_decode_split segments"); _chk(images, torch.int32, "jpeg_decode_split images")
    _chk(status, torch.int32, "jpeg_decode_split status"); _chk(chunks, torch.int32, "jpeg_decode_split chunks")
    B = images.shape[0] if images.dim() == 2 else -1
    if B < 0 or images.shape[1] != _ZH["ZH_JPEG_IMAGE_WORDS"] or segments.dim() != 2 or segments.shape[1] != _ZH["ZH_JPEG_SEGMENT_WORDS"] or \
            chunks.dim() != 2 or chunks.shape[1] != _ZH["ZH_JPEG_CHUNK_WORDS"] or tables.dim() != 2 or tables.shape[1] != _ZH["ZH_JPEG_TABLE_SET_BYTES"] or \
            status.numel() != B:
        raise _lib.ZutisHipError("jpeg_decode_split: segments [S, 4], chunks [C, 4], images [B, 12], tables [n_sets, TABLE_SET_BYTES] and status [B] do not "
                                 "describe one batch")
    chunk_bytes = _ZH["ZH_JPEG_CHUNK_BYTES"] if chunk_bytes is None else int(chunk_bytes)
    passes = _ZH["ZH_JPEG_SPLIT_PASSES"] if passes is None else int(passes)
    if B:
        ws, need = _workspace_or(workspace, "jpeg_decode_split", "zh_jpeg_decode_split_workspace_size", out.device, B, int(n_blocks), chunks.shape[0])
        _call("zh_jpeg_decode_split", _p(scan), scan.numel(), _p(segments), segments.shape[0], _p(chunks), chunks.shape[0], chunk_bytes, passes, _p(images), B,
              _p(tables), tables.shape[0], int(n_blocks), int(max_image_blocks), int(max_image_pixels), _p(out), out.numel(), _p(status), _p(ws), need, _stream())
    return status


# ---- training criterion (criterion.py::Criterion): zutis_amd/criterion.py

def mask_match_cost(proposals, gt_u8, inst_off, n_max, H, W, costs, stat_p, stat_pg, stat_g, skip, status, weight_dice=1.0, weight_bce=1.0):
    """proposals f32 [B, L, Q, h, w]; gt_u8 [n_tot, H, W]; inst_off int32 [B + 1] (device).  Writes costs / stat_pg (image b's [L, n_b, Q]
    at L * inst_off[b] * Q), stat_p [B, L, Q], stat_g [n_tot], skip int32 [B] and ORs STATUS_RANGE into status (see zutis_hip.h)."""
    _chk(proposals, f32, "mask_match_cost proposals")
    _chk(gt_u8, torch.uint8, "mask_match_cost gt_u8")
    _chk(inst_off, torch.int32, "mask_match_cost inst_off")
    B, Ly, Q, h, w = proposals.shape
    ws, need = _workspace("zh_mask_match_cost_workspace_size", proposals.device, B, Ly, Q, H, n_max)
    _call("zh_mask_match_cost", _p(proposals), _p(gt_u8) if gt_u8.numel() else None, _p(inst_off), _p(costs), _p(stat_p), _p(stat_pg),
          _p(stat_g), _p(skip), _p(status), B, Ly, Q, h, w, H, W, n_max, float(weight_dice), float(weight_bce),
          lin_scale(h, H), lin_scale(w, W), _p(ws), need, _stream())


def mask_match_grad(proposals, gt_u8, inst_off, pairs, stat_p, stat_pg, stat_g, grad_out, H, W, weight_dice, weight_bce, loss_scale, out=None):
    """pairs int32 [P, 4] = (b, l, q, i local) on the device -> grad f32 [B, L, Q, h, w] (0 outside the matched planes)."""
    _chk(proposals, f32, "mask_match_grad proposals")
    _chk(pairs, torch.int32, "mask_match_grad pairs")
    _chk(grad_out, f32, "mask_match_grad grad_out")
    B, Ly, Q, h, w = proposals.shape
    out = torch.empty_like(proposals) if out is None else out
    _chk(out, f32, "mask_match_grad out")
    n_pairs = pairs.shape[0]
    _call("zh_mask_match_grad", _p(proposals), _p(gt_u8) if gt_u8.numel() else None, _p(inst_off), _p(pairs) if n_pairs else None,
          n_pairs, _p(stat_p), _p(stat_pg), _p(stat_g), _p(grad_out), _p(out), B, Ly, Q, h, w, H, W,
          float(weight_dice), float(weight_bce), float(loss_scale), lin_scale(h, H), lin_scale(w, W), _stream())
    return out


ASSIGN_MAX_DIM = _ZH["ZH_ASSIGN_MAX_DIM"]     # cap on max(instances of an image, queries), from the solver's LDS state


def assignment_pairs_capacity(B, L, Q, n_max, n_tot) -> int:
    """Rows of the pairs buffer linear_assignment_batched asks for: a bound on sum_b L * min(n_b, Q) from the shape arguments alone."""
    return L * min(n_tot, B * min(n_max, Q))


def linear_assignment_batched(costs, inst_off, skip, B, L, Q, n_max, n_tot, pairs, n_pairs, mask_loss, status):
    """scipy.optimize.linear_sum_assignment for every (image, layer) of the costs zh_mask_match_cost wrote, in one call: pairs int32
    [assignment_pairs_capacity(), 4] = (b, l, q, i) in (b, l, i) order, n_pairs int32 [1], mask_loss f32 [1] = matched costs / B, and
    STATUS_NONFINITE OR-ed into status for a problem with a non-finite cost (which gives no pairs; scipy would accept +inf).
    max(n_max, Q) > ASSIGN_MAX_DIM is the library's argument error (see zutis_hip.h)."""
    _chk(costs, f32, "linear_assignment costs")
    _chk(inst_off, torch.int32, "linear_assignment inst_off")
    _chk(skip, torch.int32, "linear_assignment skip")
    _chk(pairs, torch.int32, "linear_assignment pairs")
    if (costs.numel() < L * n_tot * Q or pairs.numel() < 4 * assignment_pairs_capacity(B, L, Q, n_max, n_tot) or inst_off.numel() < B + 1
            or skip.numel() < B):
        raise _lib.ZutisHipError("linear_assignment: a buffer is smaller than its shape arguments say")
    ws, need = _workspace("zh_linear_assignment_workspace_size", costs.device, B, L, n_tot)
    _call("zh_linear_assignment", _p(costs) if n_tot else None, _p(inst_off), _p(skip), B, L, Q, n_max, n_tot,
          _p(pairs) if n_tot else None, _p(n_pairs), _p(mask_loss), _p(status), _p(ws), need, _stream())


def linear_assignment(cost: torch.Tensor):
    """(rows, cols) int64 arrays = scipy.optimize.linear_sum_assignment(cost) for ONE float32 [n, Q] matrix on the GPU, solved by
    the device kernel.  Every entry must be finite (ValueError otherwise; scipy would accept +inf)."""
    if cost.dim() != 2:
        raise _lib.ZutisHipError(f"linear_assignment: expected a [n, Q] matrix, got {tuple(cost.shape)}")
    _chk(cost, f32, "linear_assignment cost")
    n, Q = (int(d) for d in cost.shape)
    if n == 0 or Q == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    dev = cost.device
    inst_off = torch.tensor([0, n], dtype=torch.int32, device=dev)
    out = torch.zeros(4 + 4 * min(n, Q), dtype=torch.int32, device=dev)      # [status, n_pairs, loss, skip | pairs]
    linear_assignment_batched(cost.reshape(-1), inst_off, out[3:4], 1, 1, Q, n, n, out[4:], out[1:2], out[2:3].view(f32), out[0:1])
    h = out.cpu().numpy()
    if h[0] & STATUS_NONFINITE:
        raise ValueError("linear_assignment: the cost matrix has a non-finite entry")
    pr = h[4:4 + 4 * int(h[1])].reshape(-1, 4).astype(np.int64)
    return pr[:, 3].copy(), pr[:, 2].copy()


def pack_masks_u8(srcs, H: int, W: int):
    """[bool | uint8 | int64 [n_b, H, W] GPU tensors] -> (gt_u8 [n_tot, H, W] with non-zero -> 1, inst_off int32 [B + 1] on the
    device, counts): one zh_pack_masks_u8 launch per 32 images, nothing copied from or to the host (the pointers and counts are
    kernel arguments).  Bool sources (bytes 0 / 1 already) that lie back to back in one allocation, in order, are not copied:
    gt_u8 is then a view of that allocation and only inst_off is written."""
    import ctypes
    if _lib.RECORDER is not None:
        raise _lib.ZutisHipError("pack_masks_u8 takes host tables: it cannot be recorded into a launch plan")
    B = len(srcs)
    sizes = {g.element_size() for g in srcs if g.shape[0]}
    if any(g.dtype not in (torch.bool, torch.uint8, torch.int64) for g in srcs) or len(sizes) > 1:
        raise _lib.ZutisHipError("pack_masks_u8: the sources must be all bool / uint8 or all int64")
    es = sizes.pop() if sizes else 1
    srcs = [g.contiguous() for g in srcs]
    counts = [int(g.shape[0]) for g in srcs]
    n_tot, HW = sum(counts), H * W
    dev = srcs[0].device
    live = [g for g in srcs if g.shape[0]]
    gt_u8 = None
    if live and all(g.dtype == torch.bool for g in live):
        base, first, at = live[0].data_ptr(), live[0], 0
        for g in live:
            if g.data_ptr() != base + at or g.untyped_storage().data_ptr() != first.untyped_storage().data_ptr():
                break
            at += g.shape[0] * HW
        else:
            gt_u8 = torch.empty(0, dtype=torch.uint8, device=dev).set_(first.untyped_storage(), first.storage_offset(), (n_tot, H, W))
    if gt_u8 is None:
        gt_u8 = torch.empty((n_tot, H, W), dtype=torch.uint8, device=dev)
    inst_off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    ptrs = (ctypes.c_void_p * B)(*[_p(g) if g.shape[0] else None for g in srcs])
    _call("zh_pack_masks_u8", ptrs, (ctypes.c_int * B)(*counts), B, es, HW, _p(gt_u8) if n_tot else None, _p(inst_off), _stream())
    return gt_u8, inst_off, counts


def upsample_ce_fwd(logits_lo, labels, ignore_index, out, status, lse=None):
    """logits_lo f32 [B, n_cat, h, w], labels int64 [B, H, W] -> out f32 [2] = (mean NLL, valid count); lse f32 [B, H, W] returned."""
    _chk(logits_lo, f32, "upsample_ce logits_lo")
    _chk(labels, torch.int64, "upsample_ce labels")
    B, n, h, w = logits_lo.shape
    H, W = labels.shape[-2:]
    lse = torch.empty((B, H, W), dtype=f32, device=logits_lo.device) if lse is None else lse
    ws, need = _workspace("zh_upsample_ce_workspace_size", logits_lo.device, B, H, W)
    _call("zh_upsample_ce_fwd", _p(logits_lo), _p(labels), _p(lse), _p(out), _p(status), B, n, h, w, H, W, int(ignore_index),
          lin_scale(h, H), lin_scale(w, W), _p(ws), need, _stream())
    return lse


def upsample_ce_bwd(logits_lo, labels, lse, ce_out, grad_out, ignore_index, out=None):
    _chk(logits_lo, f32, "upsample_ce_bwd logits_lo")
    _chk(grad_out, f32, "upsample_ce_bwd grad_out")
    B, n, h, w = logits_lo.shape
    H, W = labels.shape[-2:]
    out = torch.empty_like(logits_lo) if out is None else out
    _call("zh_upsample_ce_bwd", _p(logits_lo), _p(labels), _p(lse), _p(ce_out), _p(grad_out), _p(out), B, n, h, w, H, W,
          int(ignore_index), lin_scale(h, H), lin_scale(w, W), _stream())
    return out


def gemm_f32_strided(A, a_strides, Bm, b_strides, C, c_strides, batch, M, N, K):
    """C[t](m, n) = sum_k A[t](m, k) Bm[t](n, k); *_strides = (batch, row, k) / (batch, m, n) in elements; fp32 tensors."""
    for t, nm in ((A, "A"), (Bm, "B"), (C, "C")):
        if t.dtype != f32:
            raise _lib.ZutisHipError(f"gemm_f32_strided {nm}: expected float32, got {t.dtype}")
    _call("zh_gemm_f32_strided", _p(A), *a_strides, _p(Bm), *b_strides, _p(C), *c_strides, batch, M, N, K, _stream())
