"""-m gpu: the MFMA GEMMs (zh_gemm_f16, zh_gemm_f16_res16, zh_gemm_f16x3 with its one-plane "x2" weights and the few-row kernel of
gemm_skinny.h) at the engine's layouts, inside guard bands (tests/_guard.py).

Every case (1) computes a float64 reference on the CPU from the LOGICAL operands only, (2) compares with the tolerance of the existing
direct test of the same kernel and output type, (3) proves with assert_untouched() that not one byte outside the logical [batch, M, N]
output (row padding, inter-batch and inter-plane space, 4 KiB in front, 256 rows behind) was written.  Operands are column slices of
wider buffers (lda, ldw > K) whose other bytes are 0xFF (NaN), with padded batch strides and plane offsets.

Store paths.  The launch records do not say which epilogue ran, so the launcher's rule (csrc/gemm_dispatch.h) is restated in
_store_path() and every case asserts the path it was built to reach — and that the library's own dispatcher, asked through
zh_dev_gemm_plan for the very arguments of the call, plans that path (the restatement stays the independent statement):
  scalar  N % 4 != 0, or ldc / strideC / ldr / strideR % 4 != 0, or C not aligned to four elements, or bias / fp32 residual not 16-byte
          aligned (fp16 residual: 8-byte) -> the element-wise epilogue of the fallback tile (fp16 operands: 128 x 128; split: 128 x 64);
  direct  vector-legal, but rows that are not 16-byte multiples or not 16-byte aligned (fp16 / split outputs with N % 8 == 4 or
          ldc % 8 == 4, C 8- but not 16-byte aligned), an fp16 output with an fp32 residual, an x3 fp16 output with any residual -> 8 / 16-byte
          stores straight from the accumulators, same fallback tile.  An fp32 output that is vector-legal always has 16-byte rows: no
          fp32 case can reach this path, which the rule below shows;
  wide    everything else: the forced / chosen tile with the LDS-slab epilogue.  Only this path depends on the tile code.
  skinny  (x3 / x2, no forced tile or tile code 32): M <= 128 rows and <= 512 blocks of 32 x 32 -> gemm_skinny.h, whose epilogue has a
          4-wide form (the scalar rule above false) and an element-wise one.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _gemm_plan_case as PC
from tests._guard import IN_FILL, OUT_FILL, Arena, assert_close, assert_untouched, assert_within

pytestmark = pytest.mark.gpu

f16, f32, f64 = torch.float16, torch.float32, torch.float64
U16, U32, SUB16 = 2.0 ** -11, 2.0 ** -24, 2.0 ** -25

# tile code -> (tile_m, tile_n), read from the plain-fp16 tile table of csrc/gemm_dispatch.h (rows = WM * TM * 16, cols = WN * TN * 16);
# test_tile_dicts_are_the_librarys_tables holds the three dicts to the library
F16_TILES = {0: (128, 128), 256: (256, 256), 192: (256, 192), 128: (128, 128), 64: (128, 64), 2128: (128, 128), 2064: (128, 64),
             3064: (64, 64), 7032: (64, 64), 7096: (128, 96), 7128: (128, 128)}
# ... and from the split-pair table (code 32: the few-row kernel's 32 x 32 blocks, forced for any M)
X3_TILES = {0: (128, 64), 64: (128, 64), 96: (128, 96), 192: (192, 128), 256: (256, 128), 512: (256, 256), 448: (192, 256), 3064: (64, 64),
            3066: (64, 64), 32: (32, 32), 1288: (128, 128), 6496: (128, 96), 6464: (128, 64), 7096: (128, 96), 7128: (128, 128)}
# the one-plane weight form has its own big tiles (test_gemm_x2_is_bitwise_the_x3_kernel_on_fp16_valued_weights)
X2_TILES = {0: (128, 64), 64: (128, 64), 96: (128, 96), 192: (192, 128), 256: (256, 128), 512: (256, 256), 448: (192, 256), 3064: (64, 64),
            5122: (256, 256), 5124: (256, 256), 4484: (192, 256), 1288: (128, 128), 32: (32, 32), 6496: (128, 96), 3066: (64, 64),
            6464: (128, 64)}

# zh_dev_gemm_plan's (family, store path) in the words of _store_path()
PLAN_PATHS = {(0, 0): "scalar", (0, 1): "direct", (0, 2): "wide", (1, 0): "skinny-scalar", (1, 1): "skinny-vec"}


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _store_path(mode, kind, M, N, batch, C, strideC, bias, R, strideR, res_f16, forced, has_pos, fixed_k=False):
    """The launcher's choice, restated: 'scalar' | 'direct' | 'wide' | 'skinny-vec' | 'skinny-scalar'.  C / R: guard views (or None)."""
    esz = 4 if kind == "f32" else 2
    cp, ldc = C.t.data_ptr(), C.ld
    vec = N % 4 == 0 and ldc % 4 == 0 and strideC % 4 == 0 and cp % (4 * esz) == 0 and (bias is None or bias.data_ptr() % 16 == 0)
    if R is not None:
        vec = vec and R.ld % 4 == 0 and strideR % 4 == 0 and R.t.data_ptr() % (8 if res_f16 else 16) == 0
    if mode in ("x3", "x2"):
        skinny_rows = (1 << 30) if forced == 32 else (0 if (forced or fixed_k) else 128)
        blocks = -(-N // 32) * -(-M // 32) * batch
        if not has_pos and M <= skinny_rows and (forced == 32 or blocks <= 512):
            return "skinny-vec" if vec else "skinny-scalar"
    if not vec:
        return "scalar"
    rows16 = cp % 16 == 0 and (ldc * esz) % 16 == 0 and (strideC * esz) % 16 == 0
    if mode in ("f16", "res16"):
        res_wide = R is None or ((R.ld % 8 == 0 and strideR % 8 == 0 and R.t.data_ptr() % 16 == 0) if res_f16 else kind == "f32")
        wide = rows16 and (N * esz) % 16 == 0 and res_wide
    else:
        wide = rows16 and (kind != "f16" or (N % 8 == 0 and R is None)) and (kind != "split" or (ldc % 8 == 0 and C.plane % 8 == 0 and N % 8 == 0))
    return "wide" if wide else "direct"


def _c_layout(kind, N, path):
    """(ldc, base misalignment in bytes) that take an N-column output of `kind` to `path` (None: N cannot reach it)."""
    if path == "scalar":
        return (N + 5, 0) if N % 4 else (N + 8, 4)            # ragged N (unaligned rows too), or a base pointer off by 4 bytes
    if N % 4:
        return None
    if path == "direct":
        if kind == "f32":
            return None
        return (N + 8, 0) if N % 8 else (N + 12, 0)           # N % 8 == 4, or ldc % 8 == 4: 8-byte rows
    if kind != "f32" and N % 8:
        return None
    return (N + 24, 0)


def gemm_case(dev, mode, kind, M, N, K, *, path, forced=0, batch=1, stride_a0=False, bias="exact", residual=None, res_rows=7, pos=None,
              act=0, seed=0, c_layout=None, misalign_c=None):
    """One guarded GEMM.  mode: 'f16' | 'res16' | 'x3' | 'x2'; kind: 'f32' | 'f16' | 'split'; residual: None | 'periodic' | 'full' |
    'inplace'; bias: None | 'exact' (N elements, NaN behind) | 'long' (the tensor handed over is 5 elements longer: they are NaN);
    pos: (h, w) of the separable tables.  Returns the store path that ran."""
    from zutis_amd import _lib, ops
    from zutis_amd.ops import Act
    x3 = mode in ("x3", "x2")
    ba = 1 if stride_a0 else batch
    A32 = _randn((ba, M, K), seed * 7 + 1, 0.5)
    W32 = _randn((batch, N, K), seed * 7 + 2, 0.2)
    if not x3:
        A32, W32 = A32.to(f16).float(), W32.to(f16).float()       # fp16 operands: the reference starts from the rounded values
    elif mode == "x2":
        W32 = W32.to(f16).float()                                 # fp16-valued weights: split_weight() packs ONE plane
    # ---- inputs: column slices of wider buffers, NaN everywhere else; a split pair's lo plane starts one 256-row tile of NaN behind the
    #      hi plane's last row, so that an over-read past row M of the hi plane meets NaN and not finite lo-plane data
    ia = Arena(IN_FILL, dev)
    lda, ldw = K + 8, K + 16
    va = ia.add("A", f16, M, K, ld=lda, batch=ba, bstride=M * lda + 24, planes=2 if x3 else 1, plane=(ba * (M * lda + 24) + 256 * lda) if x3 else None)
    pack = ops.split_weight(W32, allow_x2=(mode == "x2")) if x3 else None
    wplanes = pack.t.shape[0] if x3 else 1
    vw = ia.add("W", f16, N, K, ld=ldw, batch=batch, bstride=N * ldw + 8, planes=wplanes, plane=(batch * (N * ldw + 8) + 256 * ldw) if wplanes == 2 else None)
    vb = ia.add("bias", f32, 1, N) if bias else None
    res_f16 = mode == "res16"
    rdt = f16 if res_f16 else f32
    scalar_like = path == "scalar" and N % 4 != 0
    vr = None
    if residual == "periodic":
        vr = ia.add("R", rdt, res_rows, N, ld=N + (3 if scalar_like else 8))
    elif residual == "full":
        vr = ia.add("R", rdt, M, N, ld=N + (3 if scalar_like else 8), batch=batch, bstride=M * (N + (3 if scalar_like else 8)) + 16)
    vy = vx = None
    if pos:
        ldp = (N + 15) // 8 * 8                                   # ld_pos > N, a multiple of 8
        vy, vx = ia.add("pos_y", f32, pos[0], N, ld=ldp), ia.add("pos_x", f32, pos[1], N, ld=ldp)
    # ---- output
    ldc, mis = c_layout if c_layout is not None else _c_layout(kind, N, path)
    mis = mis if misalign_c is None else misalign_c
    oa = Arena(OUT_FILL, dev)
    sC = M * ldc + (8 if ldc % 4 == 0 else 3)
    vc = oa.add("C", f32 if kind == "f32" else f16, M, N, ld=ldc, batch=batch, bstride=sC, planes=2 if kind == "split" else 1,
                plane=(batch * sC + 31) // 8 * 8 if kind == "split" else None, misalign=mis)
    # ---- fill
    if x3:
        hi = A32.to(f16)
        va.put(torch.stack([hi, (A32 - hi.float()).to(f16)]))
        vw.put(pack.t)
        Aop = va.act()
        Wop = Act(vw.t, pack.out_scale)
        Wop.x2 = pack.x2
        assert pack.x2 == (mode == "x2")
    else:
        va.put(A32); vw.put(W32)
        Aop, Wop = va.hi, vw.hi
    bias_t = b64 = None
    if bias:
        bv = _randn((N,), seed * 7 + 3, 0.25)
        vb.put(bv)
        b64 = bv.double()
        bias_t = vb.m2.reshape(-1) if bias == "exact" else torch.as_strided(vb.m2, (N + 5,), (1,))
    r64 = None
    if residual == "inplace":
        rv = _randn((batch, M, N), seed * 7 + 4, 0.25).to(vc.dtype)
        vc.t[0].copy_(rv)
        r64, vr, rows = rv.double(), vc, M
    elif residual:
        rows = res_rows if residual == "periodic" else M
        rv = _randn((vr.batch, rows, N), seed * 7 + 4, 0.25).to(rdt)
        vr.put(rv)
        r64 = rv.double()[:, torch.arange(M) % rows]
    p64 = None
    if pos:
        ty, tx = _randn((pos[0], N), seed * 7 + 5, 0.25), _randn((pos[1], N), seed * 7 + 6, 0.25)
        vy.put(ty); vx.put(tx)
        m = torch.arange(M)
        p64 = ty.double()[(m % (pos[0] * pos[1])) // pos[1]] + tx.double()[m % pos[1]]
    # ---- the launcher's rule says which epilogue this layout takes: it must be the one the case was built for
    strideC = sC if batch > 1 else 0
    strideR = (vr.bstride if (vr is not None and vr.batch > 1) else 0)
    got_path = _store_path(mode, kind, M, N, batch, vc, strideC, bias_t, vr, strideR, res_f16, forced, pos is not None)
    want = path if not got_path.startswith("skinny") else got_path
    assert got_path == want, (mode, kind, M, N, path, got_path)
    kw = dict(M=M, N=N, K=K, lda=lda, ldw=ldw, ldc=ldc, batch=batch, strideA=0 if (stride_a0 or batch == 1) else va.bstride,
              strideW=vw.bstride if batch > 1 else 0, strideC=strideC, bias=bias_t, act=act)
    if vr is not None:
        kw.update(residual=vr.hi, res_rows=rows, ldr=vr.ld, strideR=strideR)       # 'inplace': vr IS the output view
    if pos:
        kw["pos"] = (vy.m2, vx.m2)
    out = vc.act() if kind == "split" else vc.hi
    # ... and the library's own dispatcher, asked for the very arguments about to be passed, plans that path
    plan = PC.ask_call(_lib.load(raw=True), mode, M, N, K, out_kind=("f32", "f16", "split").index(kind), C=ops._hp(out)[0].data_ptr(),
                       ldc=ldc, batch=batch, lda=lda, ldw=ldw, strideC=strideC, planeC=ops._hp(out)[1],
                       bias=bias_t.data_ptr() if bias_t is not None else 0, residual=vr.hi.data_ptr() if vr is not None else 0,
                       ldr=kw.get("ldr", 0), strideR=kw.get("strideR", 0), res_rows=kw.get("res_rows", 0), act=act, has_pos=pos is not None)
    assert PLAN_PATHS[plan.family, plan.path] == got_path, (mode, kind, M, N, got_path, plan)
    (ops.gemm_x3 if x3 else ops.gemm)(Aop, Wop, out, **kw)
    # ---- float64 reference from the logical operands
    a64, w64 = A32.double(), W32.double()
    g = torch.einsum("bmk,bnk->bmn", a64.expand(batch, M, K), w64)
    if b64 is not None:
        g = g + b64
    if p64 is not None:
        g = g + p64
    y = [g, g * torch.sigmoid(1.702 * g), F.relu(g), torch.sigmoid(g), F.gelu(g)][act]
    v = y if r64 is None else y + r64
    got = vc.pair()
    what = f"{mode} {kind} tile {forced} M={M} N={N} K={K} batch={batch} path={got_path} ldc={ldc} res={residual}"
    absprod = torch.einsum("bmk,bnk->bmn", a64.abs().expand(batch, M, K), w64.abs())
    if mode == "res16":                               # test_half_stream_gpu._gemm_bound: two fp16 roundings + fp32 accumulation
        bound = torch.clamp(v.abs() * U16, min=SUB16) + torch.clamp(g.abs() * U16, min=SUB16) + absprod * (K * U32)
        assert_within(got, v, bound, what)
    elif not x3:
        if kind == "f32":                             # test_gemm_plain (fp32 out); the every-tile test allows more
            assert_close(got, v, 1e-3, 1e-4, what)
        else:                                         # test_gemm_plain (fp16 out)
            assert_close(got, v, 2e-2 * math.sqrt(K / 64), 2e-3, what)
    elif kind == "f16":                               # test_gemm_x3_epilogues_and_outputs (fp16 out)
        assert_close(got, v, 4e-3, 1e-3, what)
    else:                                             # test_gemm_x3_matches_float64: |err| <= 2e-6 sum_k |a| |w|, element-wise
        assert_within(got, v, 2e-6 * absprod, what)
    assert_untouched(oa)
    assert_untouched(ia)                              # and the operands' padding is still NaN (nothing stored through an input pointer)
    return got_path


def _sweep(dev, mode, kind, tile, tile_m, tile_n, K=64):
    """Rows x columns x store paths for one (tile code, output kind).  Returns {path: cases}."""
    Ms = [1, tile_m - 1, tile_m, tile_m + 1, 2 * tile_m + 37]
    Ns = [1, 8, tile_n - 4, tile_n, tile_n + 4, tile_n + 1] + ([tile_n - 8, tile_n + 8] if kind != "f32" else [])
    seen = {}
    res = "full" if mode == "res16" else None
    for M in sorted(set(m for m in Ms if m > 0)):
        for N in sorted(set(n for n in Ns if n > 0)):
            # the path the column count leads to with padded, aligned rows ...
            natural = "scalar" if N % 4 else ("direct" if (kind != "f32" and N % 8) else "wide")
            paths = [natural]
            # ... and, once per column count at the row count that overhangs a tile by one, the other paths forced through ldc / the base pointer
            if M == tile_m + 1:
                paths += [p for p in ("scalar", "direct", "wide") if p != natural and _c_layout(kind, N, p) is not None]
            for path in paths:
                ran = gemm_case(dev, mode, kind, M, N, K, path=path, forced=tile, residual=res, seed=M * 1000 + N)
                seen[ran] = seen.get(ran, 0) + 1
    return seen


def _forced(tile):
    from zutis_amd import _lib
    L = _lib.load(raw=True)
    _lib.check(L.zh_dev_set_gemm_overrides(0, int(tile), 0), "zh_dev_set_gemm_overrides")
    return L


@pytest.mark.parametrize("mode,tiles", [("f16", F16_TILES), ("x3", X3_TILES), ("x2", X2_TILES)])
def test_tile_dicts_are_the_librarys_tables(mode, tiles):
    """The *_TILES dicts above against the library's own tile_m x tile_n per code (host calls only): every code forced on a wide-path
    shape (600 x 768, fp32 rows) reports itself and the dict's shape; code 0 is the base tile of a scalar-path call (N = 81)."""
    for code, shape in tiles.items():
        L = _forced(code)
        try:
            p = PC.ask_call(L, mode, 600, 768 if code else 81, 64, out_kind=0, C=1 << 20, ldc=776 if code else 89)
            assert (p.code, p.tile_m, p.tile_n) == (code,) + shape, (mode, code, p)
            assert PLAN_PATHS[p.family, p.path] == ("wide" if code not in (0, 32) else ("scalar" if code == 0 else "skinny-vec"))
        finally:
            L.zh_dev_set_gemm_overrides(0, 0, 0)


@pytest.mark.parametrize("kind", ["f32", "f16", "res16"])
@pytest.mark.parametrize("tile", sorted(F16_TILES))
def test_gemm_f16_every_tile_every_store_path(dev, tile, kind):
    """zh_gemm_f16 (fp32 / fp16 out) and zh_gemm_f16_res16 under every tile code of test_gemm_every_tile_variant_every_ring_phase and the
    cost model's own choice (0): M in {1, tile_m - 1, tile_m, tile_m + 1, 2 tile_m + 37} x N in {1, 8, tile_n - 4, tile_n, tile_n + 4,
    tile_n + 1} (fp16 outputs: tile_n -+ 8 too, their ragged wide-path columns), ldc = N + pad, lda / ldw > K."""
    L = _forced(tile)
    try:
        mode, k = ("res16", "f16") if kind == "res16" else ("f16", kind)
        seen = _sweep(dev, mode, k, tile, *F16_TILES[tile])
        print(f"gemm_f16 tile {tile} {kind}: {seen}")
        assert seen.get("scalar", 0) and seen.get("wide", 0) and (kind != "f16" or seen.get("direct", 0))
    finally:
        L.zh_dev_set_gemm_overrides(0, 0, 0)


@pytest.mark.parametrize("kind", ["f32", "f16", "split"])
@pytest.mark.parametrize("tile", sorted(X3_TILES))
def test_gemm_x3_every_tile_every_store_path(dev, tile, kind):
    """zh_gemm_f16x3 with two-plane weights under every tile code of test_gemm_x3_every_tile_variant (32 = the few-row kernel for any M)
    and the dispatcher's own choice (0: the few-row kernel up to 128 rows, ring tiles above), all three output kinds."""
    L = _forced(tile)
    try:
        seen = _sweep(dev, "x3", kind, tile, *X3_TILES[tile])
        print(f"gemm_f16x3 tile {tile} {kind}: {seen}")
        if tile == 32:
            assert set(seen) == {"skinny-vec", "skinny-scalar"}
        else:
            assert seen.get("scalar", 0) and seen.get("wide", 0) and (kind == "f32" or seen.get("direct", 0))
            assert (tile != 0) or (seen.get("skinny-vec", 0) and seen.get("skinny-scalar", 0))
    finally:
        L.zh_dev_set_gemm_overrides(0, 0, 0)


@pytest.mark.parametrize("kind", ["f32", "f16", "split"])
@pytest.mark.parametrize("tile", sorted(X2_TILES))
def test_gemm_x2_every_tile_every_store_path(dev, tile, kind):
    """The one-plane weight form (planeW = 0) under the tile codes of test_gemm_x2_is_bitwise_the_x3_kernel_on_fp16_valued_weights."""
    L = _forced(tile)
    try:
        seen = _sweep(dev, "x2", kind, tile, *X2_TILES[tile])
        print(f"gemm_f16x2 tile {tile} {kind}: {seen}")
        if tile == 32:
            assert set(seen) == {"skinny-vec", "skinny-scalar"}
        else:
            assert seen.get("scalar", 0) and seen.get("wide", 0) and (kind == "f32" or seen.get("direct", 0))
            assert (tile != 0) or (seen.get("skinny-vec", 0) and seen.get("skinny-scalar", 0))
    finally:
        L.zh_dev_set_gemm_overrides(0, 0, 0)


@pytest.mark.parametrize("mode,kind", [("f16", "f32"), ("f16", "f16"), ("x3", "f32"), ("x3", "f16"), ("x3", "split"), ("x2", "split")])
@pytest.mark.parametrize("batch,stride_a0", [(1, False), (3, False), (3, True)])
def test_gemm_batched_padded_strides_and_epilogue_arguments(dev, mode, kind, batch, stride_a0):
    """batch in {1, 3} with padded strideA / strideW / strideC / strideR and with strideA = 0 (the shared operand), K = 128, for: no
    residual, a row-periodic residual with ldr > N, a residual with a row per output row and its own batch stride, bias handed over longer
    than N.  Shapes: 300 rows (ring tiles) and 100 rows (the few-row kernel in the x3 modes) x N = 264 (wide) / 260 (direct for 2-byte
    outputs) / 37 (scalar)."""
    seen = {}
    for M in (300, 100):
        for N, path in ((264, "wide"), (260, "direct" if kind != "f32" else "wide"), (37, "scalar")):
            for residual in (None, "periodic", "full"):
                if residual and kind != "f32" and mode == "f16":
                    p = "direct" if path != "scalar" else path      # fp16 output with an fp32 residual: the direct-store path
                elif residual and kind == "f16" and mode != "f16":
                    p = "direct" if path != "scalar" else path      # x3 fp16 slab: a residual takes the direct-store path
                else:
                    p = path
                lay = _c_layout(kind, N, path)
                ran = gemm_case(dev, mode, kind, M, N, 128, path=p, batch=batch, stride_a0=stride_a0, bias="long", residual=residual,
                                seed=M + N + batch, c_layout=lay)
                seen[ran] = seen.get(ran, 0) + 1
    print(f"batched {mode} {kind} batch {batch} strideA0 {stride_a0}: {seen}")


@pytest.mark.parametrize("mode,kind", [("f16", "f32"), ("res16", "f16"), ("x3", "f32")])
@pytest.mark.parametrize("M", [100, 333])
def test_gemm_inplace_residual(dev, mode, kind, M):
    """residual is out (the residual stream: x += proj(h)), batched with a padded stride, on all store paths the form allows."""
    for N, path in ((264, "wide"), (37, "scalar")) + ((((260, "direct"),)) if kind == "f16" else ()):
        for batch in (1, 3):
            # (fp16 rows of 260 columns are 8-byte multiples: vector-legal, 8-byte residual chunks, but not the 16-byte slab)
            gemm_case(dev, mode, kind, M, N, 64, path=path, batch=batch, residual="inplace", seed=M + N)


@pytest.mark.parametrize("mode,kind", [("f16", "f32"), ("f16", "f16"), ("x3", "f32"), ("x3", "f16"), ("x3", "split"), ("x2", "f32")])
def test_gemm_pos_tables_padded_and_ragged_last_image(dev, mode, kind):
    """The separable row bias with ld_pos > N and a ragged last image (rows clamp, they do not wrap), batch 1: 5 images of 6 x 10 pixels minus
    7 rows; N = 264 (wide) and 260 (2-byte outputs: direct).  A pos table disables the few-row kernel."""
    hh, ww = 6, 10
    M = 5 * hh * ww - 7
    for N in (264, 260):
        path = "wide" if (kind == "f32" or N % 8 == 0) else "direct"
        gemm_case(dev, mode, kind, M, N, 128, path=path, pos=(hh, ww), bias="long", act=2 if (kind == "f16" and mode == "f16") else 0, seed=N)


@pytest.mark.parametrize("mode", ["f16", "x3", "x2"])
@pytest.mark.parametrize("M", [20, 600])
def test_gemm_one_column_ldc_one(dev, mode, M):
    """N = 1, ldc = 1: SelfMask's objectness head (engine_selfmask.py), 20 query rows per image and a many-row form; fp32 out, with bias;
    batch 1 and 3 (strideC = M + 3).  Every row's neighbour IS the next row: an over-wide store lands in the result."""
    for batch in (1, 3):
        ran = gemm_case(dev, mode, "f32", M, 1, 384 if M == 600 else 64, path="scalar", batch=batch, bias="exact", c_layout=(1, 0), seed=M)
        assert ran in ("scalar", "skinny-scalar")


@pytest.mark.parametrize("persist", [8, 40])
@pytest.mark.parametrize("tile,N", [(256, 1024), (192, 960)])
def test_gemm_persistent_walk_inside_guards(dev, tile, N, persist):
    """The persistent-workgroup walk of test_gemm_persistent_tiles_are_bitwise_one_workgroup_per_tile (forced grids of 8 / 40 workgroups, 24 /
    30 tiles, ragged last m-tile, batched) with ldc > N inside guards: fp16 + activation and fp32 + residual epilogues, K = 64 and 768."""
    from zutis_amd import _lib, ops
    L = _forced(tile)
    try:
        _lib.check(L.zh_dev_set_gemm_persist(persist), "zh_dev_set_gemm_persist")
        M = 5 * 256 + 77
        for K, batch in ((64, 1), (768, 2)):
            assert gemm_case(dev, "f16", "f16", M, N, K, path="wide", forced=tile, batch=batch, act=ops.ACT_QUICKGELU, seed=K) == "wide"
            assert gemm_case(dev, "f16", "f32", M, N, K, path="wide", forced=tile, batch=batch, residual="full", seed=K + 1) == "wide"
    finally:
        L.zh_dev_set_gemm_overrides(0, 0, 0)
        L.zh_dev_set_gemm_persist(-1)


def test_gemm_tail_peel_inside_guards(dev):
    """The tail-peel shape of test_gemm_tail_peel_is_bitwise_one_launch (257 m-tiles x 4 n-tiles of 256 x 256: whole rounds + a second call on
    the last m-tile row) with ldc = N + 24: the peeled call starts at row M1 of a PADDED output, and the last tile is ragged."""
    M, N, K = 257 * 256 - 37, 1024, 128
    assert gemm_case(dev, "f16", "f32", M, N, K, path="wide", residual="full", seed=5) == "wide"
    # the dispatcher's word for it: this layout is peeled at the last m-tile row, and not under the forced tile
    kw = dict(out_kind=0, C=1 << 20, ldc=N + 24, residual=1 << 21, ldr=N + 8, res_rows=M)
    assert PC.ask_call(_forced(0), "f16", M, N, K, **kw).peel == 256 * 256
    try:
        assert PC.ask_call(_forced(256), "f16", M, N, K, **kw).peel == 0
    finally:
        _forced(0)
