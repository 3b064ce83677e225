"""CPU: the GEMM dispatcher's plans (csrc/gemm_dispatch.h through the developer entry zh_dev_gemm_plan) are held to
tests/golden/gemm_plans.json — the record of what the dispatchers launched before they were rewritten onto the plan functions, over the
case list of tests/_gemm_plan_case.py — and to the properties the rewrite was meant to keep.  Nothing is launched."""
import json
import os

import pytest

from tests import _gemm_plan_case as PC
from zutis_amd import _lib, build

RING, SKINNY, WIDE = 0, 1, 2
# tile code -> (tile_m, tile_n): the shapes the developer entry documents (include/zutis_hip.h), stated here independently of the tables
SHAPES = {"f16": {64: (128, 64), 128: (128, 128), 192: (256, 192), 256: (256, 256), 2064: (128, 64), 2128: (128, 128), 3064: (64, 64),
                  7032: (64, 64), 7096: (128, 96), 7128: (128, 128)},
          "x3": {64: (128, 64), 96: (128, 96), 192: (192, 128), 256: (256, 128), 448: (192, 256), 512: (256, 256), 3064: (64, 64),
                 3066: (64, 64), 1288: (128, 128), 6464: (128, 64), 6496: (128, 96), 7096: (128, 96), 7128: (128, 128)},
          "x2": {64: (128, 64), 96: (128, 96), 192: (192, 128), 256: (256, 128), 448: (192, 256), 512: (256, 256), 3064: (64, 64),
                 3066: (64, 64), 1288: (128, 128), 6464: (128, 64), 6496: (128, 96), 5122: (256, 256), 5124: (256, 256), 4484: (192, 256)}}
SHAPES["res16"] = SHAPES["f16"]


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    L = _lib.load(raw=True)
    yield L
    L.zh_dev_set_gemm_overrides(0, 0, 0)


def _ask(lib, case, tile=0, tile_small=0):
    assert lib.zh_dev_set_gemm_overrides(0, tile, tile_small) == 0
    try:
        return PC.library_ask(lib)(case)
    finally:
        lib.zh_dev_set_gemm_overrides(0, 0, 0)


def test_plans_match_the_golden_record(lib, golden_dir):
    gold = json.load(open(os.path.join(golden_dir, "gemm_plans.json")))["groups"]
    groups = PC.groups()
    assert sorted(gold) == sorted(PC.group_name(g) for g in groups)
    bad = []
    for g in groups:
        lines = PC.group_lines(lib, g)
        want = gold[PC.group_name(g)]
        if (len(lines), PC.digest(lines)) != (want["cases"], want["sha256"]):
            bad.append(PC.group_name(g))
    assert not bad, f"plans differ from the record (tools/gemm_plan_table.py --show GROUP prints the lines): {bad}"


@pytest.mark.parametrize("mode", sorted(PC.MODES))
def test_every_table_code_is_reachable_by_force_and_reports_its_row(lib, mode):
    """Wide-path shape of 600 x 768 (ring tiles in every mode; no rule rewrites a forced code there)."""
    assert sorted(SHAPES[mode]) == sorted(PC.CODES[mode])
    res = "full" if mode == "res16" else None
    case = PC._case(mode, 600, 768, 64, 1, PC._kinds(mode)[0], res=res)
    for code, shape in SHAPES[mode].items():
        p = _ask(lib, case, tile=code)
        assert p is not None and (p.family, p.code, p.path, p.peel) == (RING, code, WIDE, 0), (mode, code, p)
        assert (p.tile_m, p.tile_n) == shape, (mode, code, p)


def test_unknown_forced_code_is_the_f16_argument_error(lib):
    case = PC._case("f16", 600, 768, 64, 1, 0)
    assert _ask(lib, case, tile=777) is None
    assert "ZH_GEMM_TILE(_SMALL)=777 is not a tile code (64|128|192|256|2064|2128|3064|7032|7096|7128)" in lib.zh_last_error().decode()
    assert _ask(lib, case, tile_small=777) is None                         # M <= 4096: tile_small applies
    assert _ask(lib, case._replace(M=4097), tile_small=777) is not None    # ... and not above


@pytest.mark.parametrize("mode", ["x3", "x2"])
def test_x3_ignores_a_forced_code_of_another_mode(lib, mode):
    """A code that is not one of the mode's own (zh_gemm_f16's 7032; for one-plane weights the circular-ring 7128) forces no tile and is
    no error: the x3 GEMMs of a process that forces an f16 tile keep running.  It plans as an unforced call does, except for what ANY set
    code switches off in this dispatcher, as before the rewrite: the few-row kernel, the promotion of 128 x 96 to the circular ring
    (7096) and the tail peel."""
    foreign = PC.FOREIGN[mode]
    seen = set()
    for c in PC.cases(mode, 0):
        free, forced = _ask(lib, c), _ask(lib, c, tile=foreign)
        assert (free is None) == (forced is None), c
        if free is None:
            continue
        if free.family == SKINNY or free.peel or free.code == 7096:
            seen.add("skinny" if free.family == SKINNY else ("peel" if free.peel else "7096"))
            assert forced.family == RING and forced.peel == 0 and forced.code != 7096, (c, free, forced)
            if free.code == 7096:
                assert (forced.code, forced.tile_m, forced.tile_n, forced.path) == (96, 128, 96, WIDE), (c, forced)
        else:
            seen.add("same")
            assert forced == free, (c, free, forced)
    assert seen == ({"skinny", "peel", "7096", "same"} if mode == "x3" else {"skinny", "peel", "same"})


@pytest.mark.parametrize("mode", sorted(PC.MODES))
def test_peeled_parts_are_not_peeled_again(lib, mode):
    """The main part of a peeled call runs big tiles on whole rounds of the 256-CU chip (or just under: at most 64 tiles short), the
    tail takes a small tile of its own."""
    n = 0
    for c in PC.cases(mode, 0):
        p = _ask(lib, c)
        if p is None or not p.peel:
            continue
        n += 1
        assert p.family == RING and p.path == WIDE and 0 < p.peel < c.M and p.peel % p.tile_m == 0, (c, p)
        head, tail = (_ask(lib, s) for s in PC.peel_parts(c, p.peel))
        assert head.peel == 0 and tail.peel == 0 and head.path == WIDE and tail.path == WIDE, (c, head, tail)
        # (the main part chooses for itself too: 65472 x 768 leaves 192 x 256 tiles for 256 x 256, three rounds exactly)
        tiles = -(-p.peel // head.tile_m) * -(-c.N // head.tile_n)
        assert head.tile_m * head.tile_n >= p.tile_m * p.tile_n and (tiles % 256 == 0 or tiles % 256 >= 256 - 64), (c, p, head, tiles)
        assert tail.tile_m * tail.tile_n < p.tile_m * p.tile_n, (c, tail)
        assert _ask(lib, c, tile=p.code).peel == 0                         # never under a forced tile
    assert n > 0
