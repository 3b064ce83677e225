"""GPU: precision "half" of ClipImageEncoder — the fp16 residual stream — from the kernels up.

Kernel level, against float64: the GEMM epilogue with an fp16 residual and an fp16 output (every store path: the persistent
256 x 256 / 256 x 192 tiles, the tail peel, the smaller tiles, the direct 8-byte path, the scalar path; in place and out of place;
row-periodic and full residuals; with and without bias), the LayerNorm that reads fp16 rows and the token assembly that writes them.
End to end: the engine against tests/golden/encode_image_half.npz, where the yardstick is the reference's OWN half-precision run
(tools/gen_encode_image_half_golden.py), never the code under test; bitwise repeatability, batch permutation, launch-plan replay and
fork(); the range envelope; the drop-in.

The stored value of the residual GEMM is  f16( f16(sum_k a w + b) + r )  — two roundings, the reference's own for a half-precision
`x + linear(y)`.  Bound per element, with u = 2^-11 (unit roundoff of fp16; 2^-25 absolute below the normal range), g = sum a w + b
and v = g + r in float64:   u |v| + u |g| + K 2^-24 sum |a| |w|   (the last term: fp32 accumulation, Higham's recursive-summation bound).
"""
import math
import os
import pickle
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _half_stream_case as HC

pytestmark = pytest.mark.gpu

f16, f32, f64 = torch.float16, torch.float32, torch.float64
U16, U32, SUB16 = 2.0 ** -11, 2.0 ** -24, 2.0 ** -25


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _gemm_bound(A, W, bias, res_rows_tensor, K):
    """(v, bound) in float64 on the CPU for out = f16(f16(A W^T + b) + r)."""
    a, w = A.double(), W.double()
    g = a @ w.t()
    if bias is not None:
        g = g + bias.double()
    acc = (a.abs() @ w.abs().t()) * (K * U32)
    v = g + res_rows_tensor.double()
    bound = torch.clamp(v.abs() * U16, min=SUB16) + torch.clamp(g.abs() * U16, min=SUB16) + acc
    return v, bound


def _run_res16(dev, M, N, K, *, in_place, res_rows, with_bias, ldc=None, seed=0):
    """One fp16-residual GEMM through ops.gemm; returns the worst |out - v| / bound."""
    from zutis_amd import ops
    ldc = N if ldc is None else ldc
    A, W = _randn((M, K), seed + 1, 0.5).to(f16), _randn((N, K), seed + 2, 0.05).to(f16)
    bias = _randn((N,), seed + 3, 0.5) if with_bias else None
    rr = M if in_place else res_rows
    R = _randn((rr, N), seed + 4, 2.0).to(f16)
    Ad, Wd, bd = A.to(dev), W.to(dev), (bias.to(dev) if with_bias else None)
    buf = torch.full((M, ldc), float("nan"), dtype=f16, device=dev)
    out = buf[:, :N]
    if in_place:
        out.copy_(R.to(dev))
        ops.gemm(Ad, Wd, out, bias=bd, residual=out)
    else:
        ops.gemm(Ad, Wd, out, bias=bd, residual=R.to(dev), res_rows=rr)
    got = out.cpu().double()
    if ldc > N:
        assert torch.isnan(buf[:, N:]).all(), "the GEMM wrote outside its N columns"
    rfull = R if rr == M else R.repeat((M + rr - 1) // rr, 1)[:M]
    v, bound = _gemm_bound(A, W, bias, rfull, K)
    ratio = float(((got - v).abs() / bound).max())
    assert torch.isfinite(got).all()
    return ratio, out


@pytest.mark.parametrize("tile", ["256", "192", "128", "64", "2128", "2064", "3064", "7032", "7096", "7128"])
def test_gemm_f16_residual_every_tile(dev, tile):
    """Every tile / ring variant of the 16-byte (LDS slab) store path, ragged M and N, K of one slice and of many: in place with bias,
    out of place with a row-periodic residual and no bias."""
    from zutis_amd import _lib
    L = _lib.load(raw=True)
    try:
        _lib.check(L.zh_dev_set_gemm_overrides(0, int(tile), 0), "zh_dev_set_gemm_overrides")
        for K in (64, 320):
            r1, _ = _run_res16(dev, 333, 328, K, in_place=True, res_rows=333, with_bias=True, seed=10 + K)
            r2, _ = _run_res16(dev, 333, 328, K, in_place=False, res_rows=37, with_bias=False, seed=20 + K)
            r3, _ = _run_res16(dev, 333, 328, K, in_place=False, res_rows=333, with_bias=True, seed=30 + K)
            print(f"tile {tile} K {K}: worst |err| / bound {r1:.3f} {r2:.3f} {r3:.3f}")
            assert max(r1, r2, r3) <= 1.0, (tile, K, r1, r2, r3)
    finally:
        L.zh_dev_set_gemm_overrides(0, 0, 0)


@pytest.mark.parametrize("tile,N", [("256", 1024), ("192", 960)])
def test_gemm_f16_residual_persistent_walk(dev, tile, N):
    """The persistent big tiles with several tiles per workgroup (forced grids of 8 and 16 workgroups over 24 / 30 tiles, ragged last
    m-tile): the residual chunks of a pass are requested while the next tile's first K slices are in flight.  Against float64, and
    bitwise one workgroup per tile."""
    from zutis_amd import _lib
    L = _lib.load(raw=True)
    M = 5 * 256 + 77
    try:
        _lib.check(L.zh_dev_set_gemm_overrides(0, int(tile), 0), "zh_dev_set_gemm_overrides")
        for K, in_place, rr, wb in ((64, True, M, True), (192, False, 100, False), (768, False, M, True)):
            _lib.check(L.zh_dev_set_gemm_persist(0), "zh_dev_set_gemm_persist")
            r0, o0 = _run_res16(dev, M, N, K, in_place=in_place, res_rows=rr, with_bias=wb, seed=40 + K)
            assert r0 <= 1.0, (tile, K, r0)
            for g in (8, 16):
                _lib.check(L.zh_dev_set_gemm_persist(g), "zh_dev_set_gemm_persist")
                r, o = _run_res16(dev, M, N, K, in_place=in_place, res_rows=rr, with_bias=wb, seed=40 + K)
                print(f"tile {tile} K {K} grid {g}: worst |err| / bound {r:.3f}")
                assert r <= 1.0 and torch.equal(o, o0), (tile, K, g, r)
    finally:
        L.zh_dev_set_gemm_overrides(0, 0, 0)
        L.zh_dev_set_gemm_persist(-1)


def test_gemm_f16_residual_tail_peel(dev):
    """The cost model's own choice on a config-5-like row count: 257 m-tiles x 4 n-tiles of 256 x 192 = 4 rounds of the chip + 4 tiles ->
    whole rounds on the persistent walk + a second call on the last m-tile row (its residual offset counts 2-byte elements).  In place,
    against float64, and bitwise the single forced-tile launch."""
    from zutis_amd import ops, _lib
    L = _lib.load(raw=True)
    M, N, K = 257 * 256 - 37, 768, 64
    ratio, out = _run_res16(dev, M, N, K, in_place=True, res_rows=M, with_bias=True, seed=77)
    print(f"tail peel {M}x{N}x{K}: worst |err| / bound {ratio:.3f}")
    assert ratio <= 1.0
    try:
        _lib.check(L.zh_dev_set_gemm_overrides(0, 192, 0), "zh_dev_set_gemm_overrides")
        _, one = _run_res16(dev, M, N, K, in_place=True, res_rows=M, with_bias=True, seed=77)
    finally:
        L.zh_dev_set_gemm_overrides(0, 0, 0)
    assert torch.equal(out, one)


@pytest.mark.parametrize("in_place", [True, False])
def test_gemm_f16_residual_direct_and_scalar_paths(dev, in_place):
    """Rows that are not 16-byte aligned (ldc = N + 4: the direct 8-byte store path, VEC = 1) and an odd N (the scalar path)."""
    for K in (64, 256):
        r1, _ = _run_res16(dev, 150, 328, K, in_place=in_place, res_rows=50, with_bias=True, ldc=332, seed=50 + K)
        r2, _ = _run_res16(dev, 150, 327, K, in_place=in_place, res_rows=150, with_bias=False, ldc=327, seed=60 + K)
        r3, _ = _run_res16(dev, 150, 327, K, in_place=in_place, res_rows=7, with_bias=True, ldc=331, seed=70 + K)
        print(f"direct / scalar K {K}: worst |err| / bound {r1:.3f} {r2:.3f} {r3:.3f}")
        assert max(r1, r2, r3) <= 1.0, (K, r1, r2, r3)


def test_gemm_f16_residual_argument_checks(dev):
    from zutis_amd import ops, _lib
    A, W = torch.zeros((64, 64), dtype=f16, device=dev), torch.zeros((64, 64), dtype=f16, device=dev)
    r16 = torch.zeros((64, 64), dtype=f16, device=dev)
    with pytest.raises(_lib.ZutisHipError, match="fp16 residual"):
        ops.gemm(A, W, torch.empty((64, 64), dtype=f32, device=dev), residual=r16)         # fp32 out
    with pytest.raises(_lib.ZutisHipError, match="fp16 residual"):
        ops.gemm(A, W, torch.empty((64, 64), dtype=f16, device=dev), residual=r16, act=ops.ACT_QUICKGELU)


# --------------------------------------------------------------------------------------------------------------------- LayerNorm / assembly
@pytest.mark.parametrize("D", [192, 384, 768, 1024])
def test_layernorm_f16_input(dev, D):
    """zh_layernorm_f16 against float64 LayerNorm of the same (exactly representable) fp16 input, at the tolerances of
    tests/test_kernels_gpu.py::test_layernorm; in_group_* addressing, no affine, plus-forms, the status word."""
    from zutis_amd import ops
    B, T = 3, 11
    x = (_randn((B * T, D), 31) * 3 + 1).to(f16)
    g, b, add = _randn((D,), 32) * 0.1 + 1, _randn((D,), 33) * 0.1, _randn((T, D), 34)
    ref = F.layer_norm(x.double(), (D,), g.double(), b.double(), 1e-5)
    o32 = torch.empty((B * T, D), dtype=f32, device=dev)
    o16 = torch.empty((B * T, D), dtype=f16, device=dev)
    p16 = torch.empty((B * T, D), dtype=f16, device=dev)
    p32 = torch.empty((B * T, D), dtype=f32, device=dev)
    st = torch.zeros((1,), dtype=torch.int32, device=dev)
    ops.layernorm(x.to(dev), g.to(dev), b.to(dev), 1e-5, B * T, D, out_f32=o32, out_f16=o16, out_f16_plus=p16, out_f32_plus=p32,
                  add=add.to(dev), add_rows=T, status=st)
    refp = ref + add.double().repeat(B, 1)
    assert torch.allclose(o32.cpu().double(), ref, atol=2e-5, rtol=1e-5)
    assert torch.allclose(o16.cpu().double(), ref, atol=4e-3, rtol=2e-3)
    assert torch.allclose(p32.cpu().double(), refp, atol=2e-5, rtol=1e-5)
    assert torch.allclose(p16.cpu().double(), refp, atol=4e-3, rtol=2e-3)
    assert int(st.item()) == 0
    # drop-cls input mapping + stacked output mapping, no affine, eps 1e-6
    o = torch.zeros((B * 2 * (T - 1), D), dtype=f32, device=dev)
    ops.layernorm(x.to(dev), None, None, 1e-6, B * (T - 1), D, out_f32=o, in_group_rows=T - 1, in_group_stride=T, in_offset=1,
                  out_group_rows=T - 1, out_group_stride=2 * (T - 1), out_offset=T - 1)
    ref2 = F.layer_norm(x.double().view(B, T, D)[:, 1:], (D,), None, None, 1e-6)
    got = o.cpu().view(B, 2, T - 1, D)
    assert torch.allclose(got[:, 1].double(), ref2, atol=2e-5, rtol=1e-5)
    assert torch.all(got[:, 0] == 0)
    # ln_post(x[:, 0, :]): one row per image, fp16 output
    c16 = torch.empty((B, D), dtype=f16, device=dev)
    ops.layernorm(x.to(dev), g.to(dev), b.to(dev), 1e-5, B, D, out_f16=c16, in_group_rows=1, in_group_stride=T, in_offset=0)
    assert torch.allclose(c16.cpu().double(), ref.view(B, T, D)[:, 0], atol=4e-3, rtol=2e-3)
    # a split-pair output carries the fp32-class value: hi + lo
    pair = ops.Act.empty((B * T, D), True, dev)
    ops.layernorm(x.to(dev), g.to(dev), b.to(dev), 1e-5, B * T, D, out_f16=pair)
    assert torch.allclose(pair.t[0].cpu().double() + pair.t[1].cpu().double(), ref, atol=2e-5, rtol=1e-5)
    # an inf in the stream (a value beyond 65504 stored as fp16) raises the status word; so does a NaN
    for bad in (float("inf"), float("nan")):
        xb = x.clone()
        xb[4, 7] = bad
        ops.layernorm(xb.to(dev), g.to(dev), b.to(dev), 1e-5, B * T, D, out_f16=o16, status=st)
        assert int(st.item()) & ops.STATUS_NONFINITE
        st.zero_()


@pytest.mark.parametrize("D", [192, 384, 768, 1024])
def test_assemble_tokens_ln_f16_output(dev, D):
    """cls + patches + pos, ln_pre, stored as fp16: against float64 at the fp16-output tolerance of test_layernorm."""
    from zutis_amd import ops
    B, hw = 2, 35
    pe, cls, pos = _randn((B * hw, D), 41), _randn((D,), 42), _randn((1 + hw, D), 43)
    g, b = _randn((D,), 44) * 0.1 + 1, _randn((D,), 45) * 0.1
    t = torch.cat([cls[None, None].expand(B, 1, D), pe.view(B, hw, D)], 1).double() + pos[None].double()
    ref = F.layer_norm(t, (D,), g.double(), b.double(), 1e-5)
    out = torch.full((B, 1 + hw, D), float("nan"), dtype=f16, device=dev)
    ops.assemble_tokens_ln(pe.to(dev), cls.to(dev), pos.to(dev), g.to(dev), b.to(dev), 1e-5, out, B, 1 + hw, D)
    assert torch.allclose(out.cpu().double(), ref, atol=4e-3, rtol=2e-3)
    # the stored value IS the fp32 kernel's value rounded once
    o32 = torch.empty((B, 1 + hw, D), dtype=f32, device=dev)
    ops.assemble_tokens_ln(pe.to(dev), cls.to(dev), pos.to(dev), g.to(dev), b.to(dev), 1e-5, o32, B, 1 + hw, D)
    assert torch.allclose(o32.cpu().double(), ref, atol=2e-5, rtol=1e-5)
    assert float((out.float() - o32).abs().max()) <= float((o32.abs().max() * U16 * 2))
    out2 = torch.empty((B, 1 + hw, D), dtype=f16, device=dev)
    ops.assemble_tokens_ln(pe.to(dev), cls.to(dev), pos.to(dev), None, None, 1e-5, out2, B, 1 + hw, D)       # no ln_pre
    assert torch.allclose(out2.cpu().double(), t, atol=4e-3, rtol=2e-3)


# --------------------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(f"{golden_dir}/encode_image_half.npz")


def _encoder(tag, dev, precision="half"):
    from zutis_amd.engine import ClipImageEncoder
    cfg, sd, x = HC.case(tag)
    return ClipImageEncoder(HC.visual_params(sd, dev), cfg.patch, prefix="visual.", precision=precision), x.to(dev), cfg


@pytest.mark.parametrize("tag", list(HC.CASES))
def test_encode_image_half_against_the_references_half_run(dev, gold, tag):
    """e = max |got - f32| < 1e-3, e <= 1.5 e_ref and rms <= 1.25 rms_ref, with e_ref / rms_ref the error of the reference's own
    half-precision run of the same tower against its fp32 run (tests/_half_stream_case.py::check_envelope prints the ratios)."""
    enc, x, cfg = _encoder(tag, dev)
    got = enc.encode_image(x)
    enc.check_finite()
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == gold[f"{tag}_f32"].shape
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-5
    HC.check_envelope(tag, got, gold)


def test_half_is_narrower_than_fast(dev, gold):
    """The name does not silently map to `fast`: the stream buffer is fp16 and the embeddings differ."""
    enc, x, _ = _encoder("full", dev)
    e_half = enc.encode_image(x)
    xb = [b for k, b in enc._bufs.items() if k[0] == "X"]
    assert len(xb) == 1 and xb[0].dtype == torch.float16
    fast, _, _ = _encoder("full", dev, "fast")
    e_fast = fast.encode_image(x)
    assert [b for k, b in fast._bufs.items() if k[0] == "X"][0].dtype == torch.float32
    d = float((e_half - e_fast).abs().max())
    print(f"full: max |e_half - e_fast| = {d:.3e}")
    assert d > 0


def test_half_is_bitwise_reproducible_and_batch_permutable(dev):
    from zutis_amd import plan as zplan
    enc, x, _ = _encoder("deep", dev)
    a = enc.encode_image(x).clone()
    b = enc.encode_image(x).clone()
    assert torch.equal(a, b)
    perm = torch.tensor([2, 0, 3, 1], device=dev)
    assert torch.equal(enc.encode_image(x[perm].contiguous()), a[perm])
    # a recorded launch plan replays bitwise equal to the eager call
    with zplan.Recorder() as rec:
        out = enc.encode_image(x)
    plan = rec.build()
    assert any(n == "zh_gemm_f16_res16" for n, _ in rec.calls) and any(n == "zh_layernorm_f16" for n, _ in rec.calls)
    assert any(n == "zh_assemble_tokens_ln_f16" for n, _ in rec.calls)
    out.fill_(float("nan"))
    torch.cuda.synchronize()
    plan.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    # a fork on a second stream agrees bitwise
    f = enc.fork()
    assert f.half_stream and f.precision == "half"
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c = f.encode_image(x)
    s.synchronize()
    f.check_finite()
    assert torch.equal(c, a)


def test_half_refuses_to_answer_outside_the_fp16_range(dev):
    """ln_pre.bias pushes one channel of X beyond 65504: it is stored as inf, the next LayerNorm's variance is not finite and its
    status word says so — check_finite() raises, nothing faults; the same engine answers again once the bias is back."""
    from zutis_amd import _lib
    enc, x, _ = _encoder("small", dev)
    ok = enc.encode_image(x).clone()
    enc.check_finite()
    bias = enc.params["visual.ln_pre.bias"]
    b0 = bias.clone()
    with torch.no_grad():
        bias[5] = 1.0e5
    enc.encode_image(x)
    with pytest.raises(_lib.ZutisHipError, match="non-finite"):
        enc.check_finite()
    enc.check_finite()                                        # the word was cleared by the raise
    with torch.no_grad():
        bias.copy_(b0)
    again = enc.encode_image(x)
    enc.check_finite()
    assert torch.equal(again, ok)


def test_dropin_extract_image_embeddings_half(dev, tmp_path):
    """The five-image case of tests/test_configs_gpu.py::test_extract_image_embeddings_dropin_files_and_pickle with precision="half":
    fp32 CPU tensors within 1e-3 of the fp32 oracle on the fp16-valued weights; the pickle equals the dict."""
    from PIL import Image
    from oracle import zutis_ref as O
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zutis_amd", "dropin"))
    from utils.extract_image_embeddings import extract_image_embeddings, _preprocess
    cfg, esd, _ = HC.case("small")                                           # the 42 px tower of that test, fp16-valued weights
    sd = {"visual." + k[len("encoder."):]: torch.from_numpy(v) for k, v in esd.items()}
    rng = np.random.default_rng(0)
    paths = []
    for i, (w, h) in enumerate([(64, 43), (50, 75), (42, 42), (91, 60), (47, 53)]):
        p = tmp_path / f"img_{i}.png"
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p)
        paths.append(str(p))
    fp = str(tmp_path / "emb.pkl")
    out = extract_image_embeddings(paths, model_name="ViT-B/16", fp=fp, device=dev, batch_size=2, state_dict=sd, precision="half")
    assert sorted(out) == sorted(os.path.basename(p) for p in paths)
    xs = torch.from_numpy(np.stack([_preprocess(p, 42) for p in paths]))
    with torch.no_grad():
        ref = O.clip_encode_image(O.to_torch_params(esd), xs, cfg.patch).numpy()
    worst = 0.0
    for p, r in zip(paths, ref):
        e = out[os.path.basename(p)]
        assert isinstance(e, torch.Tensor) and e.dtype == torch.float32 and e.device.type == "cpu" and e.shape == (64,)
        worst = max(worst, float(np.abs(e.numpy() - r).max()))
    print(f"drop-in half: max |err| {worst:.3e}")
    assert worst < 1e-3
    disk = pickle.load(open(fp, "rb"))
    assert sorted(disk) == sorted(out) and all(torch.equal(disk[k], out[k]) for k in out)
