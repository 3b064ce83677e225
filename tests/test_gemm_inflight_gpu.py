"""-m gpu: the number of launches in flight that the GEMM tile chooser counts (csrc/gemm_dispatch.h, zh_dev_set_gemm_inflight) changes
the tile of a call and never its bits.

Eager calls of zh_gemm_f16x3 at forced `inflight` 1 and 3, and under both forced tiles of each flip that three launches in flight bring to
the headline step, write their outputs into guard bands (tests/_guard.py); the logical outputs are compared as integers, run against run.
The shapes are the smallest that reach both tiles of a flip with a ragged last row tile: they lie below the rows and the K at which the
chooser lets the copies in flight change a tile (the headline's own shapes are 3200 and 14144 rows with K >= 768), so the two tiles of
the flip are reached by force and the runs at inflight 1 and 3 take whatever the chooser gives these small shapes — printed per case.  One run of each case is also held to
the float64 reference, so that equal garbage cannot pass.  The replay test runs three forks of an engine through zutis_amd.plan.run_many,
where the library itself supplies the number, against the eager step."""
import pytest
import torch

from tests import _gemm_inflight as GI
from tests import _gemm_plan_case as PC
from tests._guard import IN_FILL, OUT_FILL, Arena, assert_equal, assert_untouched, assert_within

pytestmark = pytest.mark.gpu

f16, f32 = torch.float16, torch.float32


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


class _Case:
    """One split-pair GEMM at the engine's layout: operands carved once (column slices of wider NaN-filled buffers), a fresh guarded
    output per run.  kind: 'f32' | 'split'; residual: 'inplace' (fp32 out: x += ...) | 'periodic' (a table of res_rows rows)."""

    def __init__(self, dev, M, N, K, kind, residual, bias, res_rows=100, seed=0):
        from zutis_amd import ops
        from zutis_amd.ops import Act
        self.dev, self.M, self.N, self.K, self.kind, self.residual, self.res_rows = dev, M, N, K, kind, residual, res_rows
        self.A32, W32 = _randn((1, M, K), seed * 7 + 1, 0.5), _randn((1, N, K), seed * 7 + 2, 0.2)
        pack = ops.split_weight(W32, allow_x2=False)
        self.W64 = (pack.t[0].double() + pack.t[1].double()) * pack.out_scale
        self.ia = ia = Arena(IN_FILL, dev)
        self.lda, self.ldw = K + 8, K + 16
        va = ia.add("A", f16, M, K, ld=self.lda, planes=2, plane=M * self.lda + 24 + 256 * self.lda)
        vw = ia.add("W", f16, N, K, ld=self.ldw, planes=2, plane=N * self.ldw + 8 + 256 * self.ldw)
        vb = ia.add("bias", f32, 1, N) if bias else None
        self.vr = ia.add("R", f32, res_rows, N, ld=N + 8) if residual == "periodic" else None
        hi = self.A32.to(f16)
        va.put(torch.stack([hi, (self.A32 - hi.float()).to(f16)]))
        vw.put(pack.t)
        self.Aop, self.Wop = va.act(), Act(vw.t, pack.out_scale)
        self.A64 = va.pair()
        self.bias = self.b64 = None
        if bias:
            bv = _randn((N,), seed * 7 + 3, 0.25)
            vb.put(bv)
            self.bias, self.b64 = vb.m2.reshape(-1), bv.double()
        self.rv = _randn((1, M if residual == "inplace" else res_rows, N), seed * 7 + 4, 0.25)
        if self.vr is not None:
            self.vr.put(self.rv)

    def run(self, L, inflight=0, tile=0):
        """One eager call under (forced inflight, forced tile); (logical output as integers [planes, 1, M, N] on the CPU, hi + lo in
        float64, the plan the dispatcher reports for the very arguments of the call)."""
        from zutis_amd import _lib, ops
        M, N, K = self.M, self.N, self.K
        oa = Arena(OUT_FILL, self.dev)
        ldc = N + 24
        split = self.kind == "split"
        vc = oa.add("C", f16 if split else f32, M, N, ld=ldc, planes=2 if split else 1, plane=(M * ldc + 8 + 31) // 8 * 8 if split else None)
        kw = dict(M=M, N=N, K=K, lda=self.lda, ldw=self.ldw, ldc=ldc, bias=self.bias)
        if self.residual == "inplace":
            vc.t[0].copy_(self.rv)
            kw.update(residual=vc.hi, res_rows=M, ldr=ldc)
        elif self.residual == "periodic":
            kw.update(residual=self.vr.hi, res_rows=self.res_rows, ldr=self.vr.ld)
        out = vc.act() if split else vc.hi
        _lib.check(L.zh_dev_set_gemm_overrides(0, tile, 0), "zh_dev_set_gemm_overrides")
        _lib.check(L.zh_dev_set_gemm_inflight(inflight), "zh_dev_set_gemm_inflight")
        try:
            plan = PC.ask_call(L, "x3", M, N, K, out_kind=2 if split else 0, C=ops._hp(out)[0].data_ptr(), ldc=ldc, lda=self.lda, ldw=self.ldw,
                               planeC=ops._hp(out)[1], bias=self.bias.data_ptr() if self.bias is not None else 0,
                               residual=kw["residual"].data_ptr() if "residual" in kw else 0, ldr=kw.get("ldr", 0), res_rows=kw.get("res_rows", 0))
            ops.gemm_x3(self.Aop, self.Wop, out, **kw)
            torch.cuda.synchronize()
        finally:
            L.zh_dev_set_gemm_overrides(0, 0, 0)
            L.zh_dev_set_gemm_inflight(0)
        assert_untouched(oa)
        assert_untouched(self.ia)
        return vc.get().view(torch.int16 if split else torch.int32), vc.pair(), plan

    def check_reference(self, got, what):
        """|err| <= 2e-6 sum_k |a| |w| element-wise (the bound of the direct test of this kernel) against float64 from the logical operands."""
        g = torch.einsum("bmk,nk->bmn", self.A64, self.W64[0])
        absprod = torch.einsum("bmk,nk->bmn", self.A64.abs(), self.W64[0].abs())
        if self.b64 is not None:
            g = g + self.b64
        if self.residual:
            r = self.rv.double()
            g = g + (r if self.residual == "inplace" else r[:, torch.arange(self.M) % self.res_rows])
        assert_within(got, g, 2e-6 * absprod, what)


def _same_bits(dev, M, N, K, kind, residual, bias, tiles, expect_flip):
    from zutis_amd import _lib
    L = _lib.load(raw=True)
    case = _Case(dev, M, N, K, kind, residual, bias, seed=M + K)
    what = f"x3 {kind} {M} x {N} x {K} {residual}"
    base, pair, p1 = case.run(L, inflight=1)
    case.check_reference(pair, what)
    got3, _, p3 = case.run(L, inflight=3)
    print(f"{what}: inflight 1 -> {p1.code} ({p1.tile_m} x {p1.tile_n}), inflight 3 -> {p3.code} ({p3.tile_m} x {p3.tile_n})")
    assert p1.family == p3.family == 0 and p1.path == p3.path == 2, (p1, p3)       # ring tiles, the LDS-staged epilogue
    assert (p1 != p3) == expect_flip, (what, p1, p3)
    assert_equal(got3, base, what + ": inflight 3 against 1")
    for tile, shape in tiles.items():
        got, _, p = case.run(L, tile=tile)
        assert (p.code, p.tile_m, p.tile_n, p.path) == (tile,) + shape + (2,), (what, tile, p)
        assert_equal(got, base, f"{what}: forced tile {tile} against the chooser's at inflight 1")


@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("kind,residual,bias", [("f32", "inplace", True), ("split", None, True)])
def test_two_slot_flip_same_bits(dev, K, kind, residual, bias):
    """192 x 256 against 256 x 256 on two slots (c_proj / out_proj in flight): M = 4100 (68 rows in the last row tile of the one, 4 in
    that of the other), N = 768, K = 64 (the two-slice minimum of the ring) and 192; fp32 with bias and in-place residual, split pair out.
    At 4100 rows and these K the chooser keeps the lone launch's 128 x 128 tile (a 3-slot tile gives way to a two-slot one only from
    K = 1024 on)."""
    _same_bits(dev, 4100, 768, K, kind, residual, bias, {448: (192, 256), 512: (256, 256)}, expect_flip=False)


@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("kind,bias", [("f32", True), ("split", False)])
def test_decoder_flip_same_bits(dev, K, kind, bias):
    """128 x 96 (both ring forms) against 256 x 128 and 192 x 128 (the decoder's N = 768 GEMMs at 3 and 2 in flight): M = 300, N = 768,
    K = 64 and 192, a row-periodic residual of res_rows = 100 (the decoder's query tables).  300 rows are the few-tile regime: the chooser
    keeps its one-launch tile at every number in flight."""
    _same_bits(dev, 300, 768, K, kind, "periodic", bias, {7096: (128, 96), 96: (128, 96), 256: (256, 128), 192: (192, 128)}, expect_flip=False)


def test_replay_in_flight_is_bitwise_the_eager_step(dev):
    """Three forks of the tiny configuration (2 + 2 layers, width 192), replayed round-robin on three streams by zutis_amd.plan.run_many —
    zh_plan_run_multi tells the chooser that three launches meet on the chip — against the eager step of each fork, bit for bit.  At the
    smoke test's batch no GEMM of the tiny model fills the chip, so none flips; 48 images of 128 x 128 (3120 token rows) is the smallest
    batch at which one does (c_fc, 3120 x 768 x 192: 128 x 96 -> 256 x 128), asserted through zh_dev_gemm_plan_inflight."""
    from zutis_amd import _lib, detgen
    from zutis_amd import plan as zplan
    from zutis_amd.engine import ZutisEngine
    L = _lib.load(raw=True)
    cfg = detgen.TINY
    P = {k: torch.from_numpy(v).to(dev) for k, v in detgen.zutis_state_dict(cfg).items()}
    x = torch.from_numpy(detgen.images(48, 128, 128)).to(dev)
    eng = ZutisEngine(P, cfg.patch, cfg.dec_heads, precision="exact")
    engs = [eng, eng.fork(), eng.fork()]
    keys = ("patch_tokens", "mask_proposals")
    plans, outs = [], []
    for e in engs:
        e.forward(x)                                 # eager warm-up: packs weights, sizes the buffer cache
        with zplan.Recorder() as rec:
            out = e.forward(x)
        plans.append(rec.build())
        outs.append([out[k] for k in keys])
        flipped = GI.flips(L, rec.calls, 3)
        assert flipped, "no GEMM of the recorded step changes its tile at three launches in flight"
    print("flips at 3 in flight:", sorted({(c.M, c.N, c.K, p1.code, p3.code) for c, p1, p3 in flipped}))
    torch.cuda.synchronize()
    for ts in outs:
        for t in ts:
            t.fill_(float("nan"))
    streams = [torch.cuda.Stream(device=dev) for _ in engs]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    zplan.run_many(plans, [s.cuda_stream for s in streams])
    zplan.run_many(plans, [s.cuda_stream for s in streams])
    torch.cuda.synchronize()
    replayed = [[t.clone() for t in ts] for ts in outs]
    assert L.zh_dev_set_gemm_inflight(0) == 0        # (not forced: the eager step below runs at 1, the replay above ran at 3)
    for e, got in zip(engs, replayed):
        out = e.forward(x)
        torch.cuda.synchronize()
        for k, g in zip(keys, got):
            assert bool(torch.isfinite(g).all()), k
            assert g.dtype == f32 and out[k].dtype == f32
            assert_equal(g.contiguous().view(torch.int32), out[k].contiguous().view(torch.int32), f"replay in flight against the eager step: {k}")
