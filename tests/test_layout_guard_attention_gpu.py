"""-m gpu: zh_attention_f16, zh_attention_causal_f16 and zh_attention_f16_splitk (fp16 and split-pair "x3" operands, head_dim 64 and 96)
at the engine's layouts, inside guard bands (tests/_guard.py).

Layouts:
  packed  Q, K and V are the column blocks 0, D and 2D of ONE [B*T, 3D] buffer (ldq = ldk = ldv = 3D, strides T*3D): the encoder's and the
          decoder self-attention's calls (engine_base.py, `ops.attention(q_, k_, v_, ...)` and `ops.attention(qkv16, qkv16.view(...))`);
  slice   Q from its own buffer with ldq > D; K and V each column block l*D of a [B*M, L*D] buffer (ldk = ldv = L*D): the decoder's
          cross-attention over all layers' K / V projections.  Everything outside the slice is 0xFF = NaN, one NaN row lies between images.
In the packed layout images follow each other without a gap (the engine's strides): a K / V row past Tk of any image but the last is the
next image's finite data, so the read-overrun screen rests on the slice layout; the packed cases check values and the output guards.
O always has ldo > D and a padded batch stride; split-pair O has a padded plane offset.

Key-tile height kt (include/zutis_hip.h: ZH_ATTN_KEY_TILE_F16, ZH_ATTN_KEY_TILE_X3): 64 keys for the fp16 kernels, 32 for the split-pair ones; a
workgroup covers 128 queries (4 waves of 32), so Tq = 1 .. 127 leaves waves that only help with the tile loads, and their O rows — past
Tq — must stay untouched.  K / V rows past Tk are never part of the logical input: a key tile that reads them must not let them reach
the result (P = 0 times NaN is NaN), which the finite check shows.

Tolerances: 4e-3 (fp16, test_attention) and 2e-5 (x3, test_attention_x3_scores) against float64; guard comparisons are exact.
"""
import math

import pytest
import torch

from tests._guard import IN_FILL, OUT_FILL, Arena, assert_close, assert_untouched

pytestmark = pytest.mark.gpu

f16, f32, f64 = torch.float16, torch.float32, torch.float64
Q_BLOCK = 128                                   # queries per workgroup


def _kt(x3):
    return 32 if x3 else 64


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _put_pair(view, x32, x3):
    if x3:
        hi = x32.to(f16)
        view.put(torch.stack([hi, (x32 - hi.float()).to(f16)]))
        return x32.double()
    view.put(x32.to(f16))
    return x32.to(f16).double()                 # fp16 operands: the reference starts from the rounded values


def attn_case(dev, *, x3, dh, heads, B, Tq, Tk, layout, split_o=None, causal=False, ksplit=1, scale=None, seed=0, expect_error=False,
              inputs=None):
    """inputs = (q32, k32, v32): float32 [B, Tq, D], [B, Tk, D], [B, Tk, D] instead of the seeded randn draws (tests/_attention_case.py)."""
    from zutis_amd import _lib, ops
    D = heads * dh
    planes = 2 if x3 else 1
    split_o = x3 if split_o is None else split_o
    qs = 2.5 if x3 else 1.0                     # the input scales of test_attention_x3_scores / test_attention
    q32, k32, v32 = _randn((B, Tq, D), seed + 1, qs), _randn((B, Tk, D), seed + 2, qs), _randn((B, Tk, D), seed + 3)
    if inputs is not None:
        q32, k32, v32 = (t.detach().cpu().to(f32) for t in inputs)
        assert q32.shape == (B, Tq, D) and k32.shape == (B, Tk, D) and v32.shape == (B, Tk, D)
    ia = Arena(IN_FILL, dev)
    kt = _kt(x3)
    if layout == "packed":
        assert Tq == Tk
        T, ld = Tq, 3 * D
        inner = B * T * ld
        vqkv = ia.add("QKV", f16, T, ld, batch=B, planes=planes, plane=inner + 64, tail_rows=kt)
        hi = torch.cat([q32, k32, v32], dim=-1)
        _put_pair(vqkv, hi, x3)
        q64, k64, v64 = (t.double() if x3 else t.to(f16).double() for t in (q32, k32, v32))
        full = vqkv.hi
        if x3:
            A = vqkv.act()
            Qo, Ko, Vo = A, A.view(full[..., D:]), A.view(full[..., 2 * D:])
        else:
            Qo, Ko, Vo = full, full[..., D:], full[..., 2 * D:]
        kw = dict(ldq=ld, ldk=ld, ldv=ld, strideQ=T * ld, strideK=T * ld, strideV=T * ld)
    else:
        L, l = 3, 1
        ldq, ldk = D + 8, L * D
        vq = ia.add("Q", f16, Tq, D, ld=ldq, batch=B, bstride=Tq * ldq + 16, planes=planes, plane=B * (Tq * ldq + 16) + 24, tail_rows=Q_BLOCK)
        sk = (Tk + 1) * ldk                      # one row of NaN between images
        vk = ia.add("K", f16, Tk, D, ld=ldk, batch=B, bstride=sk, planes=planes, plane=B * sk + 8, misalign=l * D * 2, tail_rows=kt)
        vv = ia.add("V", f16, Tk, D, ld=ldk, batch=B, bstride=sk, planes=planes, plane=B * sk + 8, misalign=l * D * 2, tail_rows=kt)
        q64, k64, v64 = _put_pair(vq, q32, x3), _put_pair(vk, k32, x3), _put_pair(vv, v32, x3)
        Qo, Ko, Vo = (v.act() if x3 else v.hi for v in (vq, vk, vv))
        kw = dict(ldq=ldq, ldk=ldk, ldv=ldk, strideQ=vq.bstride, strideK=sk, strideV=sk)
    oa = Arena(OUT_FILL, dev)
    ldo = D + 4
    so = Tq * ldo + 8
    vo = oa.add("O", f16, Tq, D, ld=ldo, batch=B, bstride=so, planes=2 if split_o else 1, plane=B * so + 20, misalign=8 if seed % 2 else 0,
                tail_rows=Q_BLOCK)
    ws = None
    if ksplit > 1:
        need = ops.attention_splitk_workspace_size(B, heads, Tq, dh, ksplit)
        assert need == (ksplit * B * Tq * heads * dh + 2 * ksplit * B * heads * Tq) * 4
        ws = oa.workspace("workspace", need)
    call = dict(batch=B, heads=heads, Tq=Tq, Tk=Tk, head_dim=dh, ldo=ldo, strideO=so, scale=scale, causal=causal, x3=x3, ksplit=ksplit,
                workspace=None if ws is None else ws.t.reshape(-1), **kw)
    O = vo.act() if split_o else vo.hi
    what = f"attention x3={x3} dh={dh} heads={heads} B={B} Tq={Tq} Tk={Tk} {layout} split_o={split_o} causal={causal} ksplit={ksplit}"
    if expect_error:
        with pytest.raises(_lib.ZutisHipError):
            ops.attention(Qo, Ko, Vo, O, **call)
        assert_untouched(oa, [])                # a refused call writes nothing, not even its workspace
        return
    ops.attention(Qo, Ko, Vo, O, **call)
    sc = 1.0 / math.sqrt(dh) if scale is None else scale
    qh, kh, vh = (t.view(B, -1, heads, dh).transpose(1, 2) for t in (q64, k64, v64))
    s = qh @ kh.transpose(-1, -2) * sc
    if causal:
        s = s + torch.full((Tq, Tk), float("-inf"), dtype=f64).triu_(1)
    ref = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Tq, D)
    # a plain fp16 O holds one rounding of the result (2^-11 |o|) whichever kernel formed it: the fp16 bound
    assert_close(vo.pair(), ref, 2e-5 if (x3 and split_o) else 4e-3, 0.0, what)
    assert_untouched(oa)
    assert_untouched(ia)


TQ = [1, 31, 32, 33, 127, 128, 129]


def _tks(x3):
    kt = _kt(x3)
    return [1, kt - 1, kt, kt + 1, 2 * kt + 5]


@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("dh", [64, 96])
@pytest.mark.parametrize("heads,B", [(1, 1), (3, 1), (1, 3), (3, 3)])
def test_attention_cross_layout_every_edge(dev, x3, dh, heads, B):
    """Cross-attention layout (K / V = column block 1 of a three-block buffer, ldq > D): Tq in {1, 31, 32, 33, 127, 128, 129} x Tk in
    {1, kt - 1, kt, kt + 1, 2 kt + 5}; x3 fills a split-pair O with a padded plane offset, fp16 a plain O; O base 8- or 256-byte aligned."""
    n = 0
    for Tq in TQ:
        for Tk in _tks(x3):
            attn_case(dev, x3=x3, dh=dh, heads=heads, B=B, Tq=Tq, Tk=Tk, layout="slice", seed=Tq * 7 + Tk)
            n += 1
    # a plain fp16 O from the split-pair kernel (x3 scores, one rounding) and a non-default softmax scale, at the ragged corners
    for Tq, Tk in ((33, _kt(x3) + 1), (129, 2 * _kt(x3) + 5), (1, 1)):
        attn_case(dev, x3=x3, dh=dh, heads=heads, B=B, Tq=Tq, Tk=Tk, layout="slice", scale=0.07, seed=Tq)
        if x3:
            attn_case(dev, x3=True, dh=dh, heads=heads, B=B, Tq=Tq, Tk=Tk, layout="slice", split_o=False, seed=Tq + 1)
        n += 1 + int(x3)
    print(f"cross layout x3={x3} dh={dh} heads={heads} B={B}: {n} cases")


@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("dh", [64, 96])
@pytest.mark.parametrize("heads,B", [(1, 1), (3, 3)])
def test_attention_packed_qkv(dev, x3, dh, heads, B):
    """Packed QKV (the encoder / decoder self-attention calls: exact strides T*3D, no padding between images): T over the query-block and
    key-tile edges; non-causal, and causal (the text tower) at T in {1, 33, 77}; a non-default scale."""
    kt = _kt(x3)
    for T in sorted({1, 31, 32, 33, kt - 1, kt, kt + 1, 127, 128, 129, 2 * kt + 5}):
        attn_case(dev, x3=x3, dh=dh, heads=heads, B=B, Tq=T, Tk=T, layout="packed", seed=T)
    for T in (1, 33, 77):
        attn_case(dev, x3=x3, dh=dh, heads=heads, B=B, Tq=T, Tk=T, layout="packed", causal=True, seed=T + 100)
        attn_case(dev, x3=x3, dh=dh, heads=heads, B=B, Tq=T, Tk=T, layout="slice", causal=True, scale=0.07, seed=T + 200)


@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("dh", [64, 96])
def test_attention_key_split_workspace_exact(dev, x3, dh):
    """zh_attention_f16_splitk, ksplit in {2, 3}, key counts whose last chunk is ragged (2 kt + 5: chunks of 2 tiles + 5 keys / 1 + 1 + 5 keys;
    5 kt + 5: 3 + 3 tiles / 2 + 2 + 2), the workspace EXACTLY zh_attention_splitk_workspace_size bytes between guards; Tq of 1, 33 and 129
    (a second query block); both layouts that allow Tq != Tk.  A ksplit that leaves an empty chunk is refused and writes nothing."""
    kt = _kt(x3)
    for ksplit in (2, 3):
        for Tk in (2 * kt + 5, 5 * kt + 5):
            for Tq, heads, B in ((1, 1, 1), (33, 3, 3), (129, 3, 1)):
                attn_case(dev, x3=x3, dh=dh, heads=heads, B=B, Tq=Tq, Tk=Tk, layout="slice", ksplit=ksplit, seed=Tk + Tq)
        attn_case(dev, x3=x3, dh=dh, heads=3, B=3, Tq=2 * kt + 5, Tk=2 * kt + 5, layout="packed", ksplit=ksplit, scale=0.07, seed=9)
    # 3 key tiles over 4 chunks of one tile: the fourth is empty; 4 tiles over 3 chunks of two: the third is empty
    attn_case(dev, x3=x3, dh=dh, heads=1, B=1, Tq=33, Tk=2 * kt + 5, layout="slice", ksplit=4, expect_error=True)
    attn_case(dev, x3=x3, dh=dh, heads=1, B=1, Tq=33, Tk=3 * kt + 5, layout="slice", ksplit=3, expect_error=True)
