"""CPU: the GEMM tile chooser's plans for a given number of launches in flight (csrc/gemm_dispatch.h through the developer entries
zh_dev_gemm_plan_inflight / zh_dev_set_gemm_inflight).  One launch in flight is the golden record of tests/golden/gemm_plans.json; three
in flight flip the shapes that tools/gemm_inflight_ab.py measured faster (profiles/gemm_inflight_ab.json) and no other shape of the
headline step.  Nothing is launched."""
import ctypes
import json
import os

import pytest

from tests import _gemm_inflight as GI
from tests import _gemm_plan_case as PC
from zutis_amd import _lib, build

RING, WIDE = 0, 2


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    L = _lib.load(raw=True)
    yield L
    L.zh_dev_set_gemm_overrides(0, 0, 0)
    L.zh_dev_set_gemm_inflight(0)


def _ask_at(lib, inflight):
    out = (ctypes.c_int * 6)()

    def ask(c):
        return PC.Plan(*out) if lib.zh_dev_gemm_plan_inflight(*c, inflight, out) == 0 else None
    return ask


def _site(mode, M, N, K, epilogue):
    """A GEMM of the step with aligned rows.  epilogue: 'res32' (fp32 + bias + a residual row per output row), 'pair' (split pair out, or
    fp16 for plain fp16 operands, + bias), 'tab' (the same + a row-periodic residual table)."""
    kind = 0 if epilogue == "res32" else (1 if mode == "f16" else 2)
    res = {"res32": "full", "pair": None, "tab": "periodic"}[epilogue]
    return PC._case(mode, M, N, K, 1, kind, bias=0, res=res, lda=K, ldw=K)


def _code(lib, case, inflight):
    p = GI.plan_at(lib, case, inflight)
    assert (p.family, p.path, p.peel) == (RING, WIDE, 0), (case, inflight, p)
    return p.code, p.tile_m, p.tile_n


def test_one_launch_in_flight_is_the_golden_record(lib, golden_dir):
    """Every entry of tests/golden/gemm_plans.json gets the plan it has today when it is asked for through the new query at inflight = 1 —
    also while another number is forced for the launches of the process."""
    gold = json.load(open(os.path.join(golden_dir, "gemm_plans.json")))["groups"]
    bad = []
    for forced_inflight in (0, 3):
        assert lib.zh_dev_set_gemm_inflight(forced_inflight) == 0
        try:
            for g in PC.groups():
                if forced_inflight and (g[1] or g[2]):
                    continue                          # (the forced-tile groups once: a forced tile does not look at the number at all)
                mode, forced, tile_small = g
                assert lib.zh_dev_set_gemm_overrides(0, forced, tile_small) == 0
                try:
                    lines = [PC.line(c, _ask_at(lib, 1)) for c in PC.cases(mode, forced)]
                finally:
                    lib.zh_dev_set_gemm_overrides(0, 0, 0)
                want = gold[PC.group_name(g)]
                if (len(lines), PC.digest(lines)) != (want["cases"], want["sha256"]):
                    bad.append((forced_inflight, PC.group_name(g)))
        finally:
            lib.zh_dev_set_gemm_inflight(0)
    assert not bad, f"plans at one launch in flight differ from the record: {bad}"


@pytest.mark.parametrize("mode", ["x3", "x2"])
def test_three_in_flight_flip_the_measured_shapes_and_no_other(lib, mode):
    """Split pair, the shapes of the headline step (B = 32, 336 px) and what the in-flight table measured for them."""
    small = 7096 if mode == "x3" else 96             # 128 x 96: two-plane weights take it on the circular ring
    # c_proj / out_proj: 192 x 256 (222 tiles, one round) alone, 256 x 256 in flight (504 tiles of three launches: 1.97 rounds, not 2.6)
    for K in (3072, 768):
        c = _site(mode, 14144, 768, K, "res32")
        assert _code(lib, c, 1) == (448, 192, 256) and _code(lib, c, 2) == (448, 192, 256) and _code(lib, c, 3) == (512, 256, 256), K
    # the decoder's N = 768 GEMMs: 128 x 96 (200 tiles, one round) alone, 256 x 128 at three (234 tiles of three launches: one round) and
    # 192 x 128 at two in flight (204 tiles of two)
    for K, epi in ((768, "res32"), (768, "tab"), (2048, "res32")):
        c = _site(mode, 3200, 768, K, epi)
        assert _code(lib, c, 1) == (small, 128, 96) and _code(lib, c, 2) == (192, 192, 128) and _code(lib, c, 3) == (256, 256, 128), (K, epi)
    # QKV, c_fc, the K / V projections, the decoder's N = 2048 / 2304 GEMMs keep their tiles at two and at three in flight
    for M, N, K, epi, want in ((14144, 2304, 768, "pair", (512, 256, 256)), (14144, 3072, 768, "pair", (512, 256, 256)),
                               (56448, 4608, 256, "pair", (512, 256, 256)), (3200, 2048, 768, "pair", (256, 256, 128)),
                               (3200, 2304, 768, "tab", (256, 256, 128))):
        c = _site(mode, M, N, K, epi)
        assert [GI.plan_at(lib, c, i)[:5] for i in (1, 3)] == [(RING,) + want + (WIDE,)] * 2, (M, N, K)
        assert GI.plan_at(lib, c, 2)[:5] == (RING,) + want + (WIDE,), (M, N, K)


@pytest.mark.parametrize("mode", ["x3", "x2"])
def test_config4_encoder_takes_the_two_slot_tile_only_where_it_measured_faster(lib, mode):
    """8200 token rows (8 images of 518 px), 256 x 128 alone.  The round model would take 256 x 256 at two and 192 x 256 at three in flight
    for both N = 768 GEMMs; the clock confirms c_proj (K = 3072) at three (345.4 -> 311.4 us per group) and nothing else (c_proj at two
    205.2 -> 214.6, out_proj at three 103.1 -> 109.3): a 3-slot tile gives way to a two-slot one only with K >= 1024 at three or more."""
    proj, out = _site(mode, 8200, 768, 3072, "res32"), _site(mode, 8200, 768, 768, "res32")
    assert [_code(lib, proj, i) for i in (1, 2, 3, 4)] == [(256, 256, 128)] * 2 + [(448, 192, 256), (512, 256, 256)]
    assert [_code(lib, out, i) for i in (1, 2, 3, 4)] == [(256, 256, 128)] * 4
    # QKV: 192 x 256 alone and at three, 256 x 256 at two (a tie on the clock); c_fc keeps 256 x 256 (the model's 192 x 256 at two would shrink it)
    qkv, fc = _site(mode, 8200, 2304, 768, "pair"), _site(mode, 8200, 3072, 768, "pair")
    assert [_code(lib, qkv, i)[0] for i in (1, 2, 3)] == [448, 512, 448]
    assert [GI.plan_at(lib, fc, i) for i in (2, 3)] == [GI.plan_at(lib, fc, 1)] * 2 and GI.plan_at(lib, fc, 1).code == 512


def test_plain_fp16_counts_three_in_flight_for_the_narrow_outputs_only(lib):
    """`fast`: the flips the table shows winning — N = 768 at three in flight — and the present picks everywhere else."""
    for M, K, epi, lone, three in ((14144, 3072, "res32", (192, 256, 192), (256, 256, 256)), (14144, 768, "res32", (192, 256, 192), (256, 256, 256)),
                                   (3200, 768, "res32", (7096, 128, 96), (128, 128, 128)), (3200, 768, "pair", (7096, 128, 96), (128, 128, 128)),
                                   (3200, 2048, "res32", (7096, 128, 96), (128, 128, 128)),
                                   (8200, 3072, "res32", (128, 128, 128), (192, 256, 192)), (8200, 768, "res32", (128, 128, 128), (192, 256, 192))):
        c = _site("f16", M, 768, K, epi)
        assert [_code(lib, c, i) for i in (1, 2, 3)] == [lone, lone, three], (M, K, epi)
    for M, N in ((14144, 2304), (14144, 3072), (56448, 4608), (3200, 2048), (3200, 2304), (8200, 2304), (8200, 3072)):
        c = _site("f16", M, N, 768 if N != 4608 else 256, "pair")
        lone = GI.plan_at(lib, c, 1)
        assert all(GI.plan_at(lib, c, i) == lone for i in (2, 3, 4, 8)), (M, N)
    r = PC._case("res16", 14144, 768, 3072, 1, 1, bias=0, res="full")               # the fp16 residual stream goes through the same chooser
    assert [GI.plan_at(lib, r, i).code for i in (1, 2, 3)] == [192, 192, 256]


@pytest.mark.parametrize("mode", sorted(PC.MODES))
def test_one_image_keeps_its_tile_at_every_number_in_flight(lib, mode):
    """M = 442 (one image of 336 px) and 1201 (native resolution): the few-tile regime is not counted."""
    res = "full" if mode == "res16" else None
    for M in (442, 1201):
        for N in (768, 2304, 3072):
            for K in (768, 3072):
                c = PC._case(mode, M, N, K, 1, PC._kinds(mode)[-1], bias=0, res=res)
                lone = GI.plan_at(lib, c, 1)
                assert all(GI.plan_at(lib, c, i) == lone for i in range(2, 65)), (mode, M, N, K)


@pytest.mark.parametrize("mode", sorted(PC.MODES))
def test_launches_in_flight_never_shrink_the_tile_and_leave_the_few_tile_regime_alone(lib, mode):
    """Over the case list of the golden record: below 2048 rows, or with at most one 128 x 64 tile per CU, the plan is the lone launch's at
    every number in flight; above, the tile area never decreases and the store path never changes."""
    changed = 0
    for c in PC.cases(mode, 0):
        lone = _ask_at(lib, 1)(c)
        for i in (2, 3, 4, 64):
            p = _ask_at(lib, i)(c)
            assert (p is None) == (lone is None), (c, i)
            if p is None:
                continue
            if c.M < 2048 or -(-c.M // 128) * -(-c.N // 64) * c.batch <= 256:
                assert p == lone, (c, i, lone, p)
            else:
                assert (p.family, p.path) == (lone.family, lone.path) and p.tile_m * p.tile_n >= lone.tile_m * lone.tile_n, (c, i, lone, p)
                changed += p != lone
    assert changed > 0


def test_config5_peels_the_same_row_alone_and_in_flight(lib):
    """The 147712-row GEMMs of config 5 (one-plane weights): the surplus over whole rounds is 4 / 12 / 16 tiles for one launch and
    12 / 36 / 48 for three — one m-tile row of 256 x 256 tiles either way."""
    for N, K in ((1024, 1024), (1024, 4096), (3072, 1024), (4096, 1024)):
        c = PC._case("x2", 147712, N, K, 1, 0 if N == 1024 else 2, bias=0, res="full" if N == 1024 else None, lda=K, ldw=K)
        plans = [GI.plan_at(lib, c, i) for i in (1, 3)]
        assert plans[0] == plans[1] and plans[0].code == 512 and plans[0].peel == 576 * 256, (N, K, plans)


def test_forced_number_steers_the_plain_query_and_bad_numbers_are_argument_errors(lib):
    c = _site("x3", 14144, 768, 3072, "res32")
    ask = PC.library_ask(lib)
    assert ask(c).code == 448
    for n, code in ((3, 512), (1, 448), (2, 448), (0, 448)):
        assert lib.zh_dev_set_gemm_inflight(n) == 0
        assert ask(c).code == code, n
        assert GI.plan_at(lib, c, 3).code == 512 and GI.plan_at(lib, c, 1).code == 448          # the explicit query ignores the forced number
    for bad in (-1, 65):
        assert lib.zh_dev_set_gemm_inflight(bad) != 0 and b"zh_dev_set_gemm_inflight" in lib.zh_last_error()
    assert ask(c).code == 448                                                                   # a refused number changes nothing
    out = (ctypes.c_int * 6)()
    for bad in (0, 65):
        assert lib.zh_dev_gemm_plan_inflight(*c, bad, out) != 0 and b"inflight" in lib.zh_last_error()
    # a forced tile does not look at the number
    assert lib.zh_dev_set_gemm_overrides(0, 448, 0) == 0
    try:
        assert GI.plan_at(lib, c, 3).code == 448
    finally:
        lib.zh_dev_set_gemm_overrides(0, 0, 0)
