"""zutis_amd/shape_rules.py (no GPU): the module stays pure, its constants are the kernels', and every rule's decisions at the
product's shapes are pinned.  The pinned numbers were computed with the inline expressions the rules replaced (engine_base at
1d4869b); tests/test_launch_trace_gpu.py is the authority on what the engines launch with them — a disagreement between the two is a
finding, not a number to adjust."""
import ast
import os

import pytest

from zutis_amd import shape_rules as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_module_imports_only_math_and_os():
    tree = ast.parse(open(os.path.join(ROOT, "zutis_amd", "shape_rules.py")).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add("." * node.level + (node.module or ""))
    assert names <= {"math", "os"}, names


def test_constants_match_the_kernels():
    """shape_rules' literals == the header's constants (which static_asserts hold the kernels to) == what the library's launch plan reports."""
    from zutis_amd import _lib, build
    from tests._attention_plan_case import ask
    zh = _lib.constants()
    assert SR.QUERY_BLOCK == zh["ZH_ATTN_QUERY_BLOCK"] == 128
    assert (SR.key_tile(False), SR.key_tile(True)) == (zh["ZH_ATTN_KEY_TILE_F16"], zh["ZH_ATTN_KEY_TILE_X3"])
    build.build(verbose=False)
    lib = _lib.load(raw=True)
    for x3 in (False, True):
        assert ask(lib, Tq=1, Tk=1, x3=x3).key_tile == SR.key_tile(x3)
        # the query block as the plan shows it: one block up to QUERY_BLOCK queries, two from the next on
        assert [ask(lib, Tq=SR.QUERY_BLOCK + d, Tk=1, x3=x3).nqb for d in (-1, 0, 1)] == [1, 1, 2]
        # ... and the key tile: a split of 2 fits from key_tile + 1 keys on, in chunks of one tile
        assert ask(lib, Tq=1, Tk=SR.key_tile(x3), x3=x3, ksplit=2) is None
        assert ask(lib, Tq=1, Tk=SR.key_tile(x3) + 1, x3=x3, ksplit=2).kchunk == SR.key_tile(x3)
    assert SR.CUS == 256
    assert SR.key_tiles(5505, True) == 173 and SR.key_tiles(5505, False) == 87 and SR.key_tiles(64, False) == 1


T, F = True, False
SELF_ATTENTION = [      # (T, heads, head_dim): {(B, x3): S}
    ((442, 12, 64), {(1, T): 5, (1, F): 4, (2, T): 5, (2, F): 4, (4, T): 1, (4, F): 1}),                                  # ViT-B/16 @336
    ((1201, 12, 64), {(1, T): 2, (1, F): 2, (2, T): 1, (2, F): 1}),                                                        # @480x640
    ((50, 12, 64), {**{(B, T): 2 for B in range(1, 9)}, **{(B, F): 1 for B in range(1, 9)}, (32, T): 1, (32, F): 1}),      # ViT-B/32 @224
    ((5505, 6, 64), {(1, T): 5, (2, T): 4, (4, T): 2, (8, T): 1, (1, F): 2, (2, F): 1}),                                   # DINO 512x683
    ((577, 16, 64), {(1, T): 3, (1, F): 3, (2, T): 1, (2, F): 1}),                                                         # ViT-L/14 @336
]


@pytest.mark.parametrize("shape,want", SELF_ATTENTION, ids=lambda v: "T%d" % v[0] if isinstance(v, tuple) else None)
def test_self_attention_key_split_pinned(shape, want):
    Tn, heads, dh = shape
    got = {(B, x3): SR.self_attention_key_split(B, Tn, heads, dh, x3, False) for B, x3 in want}
    assert got == want
    assert all(SR.self_attention_key_split(B, Tn, heads, dh, x3, True) == 1 for B, x3 in want)           # causal: always 1


def test_cross_attention_key_split_pinned():
    f = SR.cross_attention_key_split
    for B in (1, 2, 8, 32):                                                   # an integer setting never reads the batch
        for x3 in (T, F):
            assert f(1, B, 8, 100, 4800, x3) == 1
            assert f(8, B, 6, 20, 5504, x3) == 8
        assert f(12, B, 8, 100, 4800, T) == 12 and f(12, B, 8, 100, 4800, F) == 11
        assert f(12, B, 8, 100, 1764, T) == 12 and f(12, B, 8, 100, 1764, F) == 10
    for x3 in (T, F):
        assert f("auto", 1, 8, 100, 4800, x3) == 8 and f("auto", 8, 8, 100, 4800, x3) == 4
        assert f("auto", 8, 8, 100, 1764, x3) == 4 and f("auto", 32, 8, 100, 1764, x3) == 1
        for setting in (8, 12, "auto"):
            assert f(setting, 1, 8, 100, 1023, x3) == 1 and f(setting, 1, 8, 129, 4800, x3) == 1      # M < 1024 or Q > 128
    assert f("auto", 1, 8, 100, 1764, T) == 8 and f("auto", 1, 8, 100, 1764, F) == 7


def test_gemm_k_split_pinned():
    for rows in (1, 100, 442, 884, 1201, 2048, 2049, 3536, 14144):
        assert [SR.gemm_k_split(rows, K) for K in (768, 384, 320)] == [1, 1, 1]
        assert SR.gemm_k_split(rows, 1536) == (2 if rows <= 2048 else 1)
        assert [SR.gemm_k_split(rows, K) for K in (2048, 3072)] == ([4, 4] if rows <= 2048 else [1, 1])


def test_rules_stay_inside_their_bounds():
    """fit_key_split never leaves an empty chunk and is the identity when S already fits; every rule returns >= 1 and every key
    split <= its cap."""
    for kt in range(1, 200):
        for S in range(1, 65):
            s = SR.fit_key_split(S, kt)
            assert 1 <= s <= S and (s - 1) * -(-kt // s) < kt
            fits = (S - 1) * -(-kt // S) < kt
            assert (s == S) == fits
            assert s == max(c for c in range(1, S + 1) if (c - 1) * -(-kt // c) < kt)
    for x3 in (T, F):
        for B in (1, 2, 3, 4, 8, 32):
            for Tn, heads, dh in ((1, 3, 64), (17, 3, 64), (50, 12, 64), (442, 12, 64), (1201, 12, 64), (2048, 6, 64), (5505, 6, 64), (4097, 8, 96)):
                for causal in (T, F):
                    assert 1 <= SR.self_attention_key_split(B, Tn, heads, dh, x3, causal) <= 8
            for M in (64, 1023, 1024, 1764, 4800, 5504):
                for Q in (5, 100, 128, 129):
                    for setting in (1, 2, 8, 12, 64, "auto"):
                        s = SR.cross_attention_key_split(setting, B, 8, Q, M, x3)
                        assert 1 <= s <= (8 if setting == "auto" else setting)
    for rows in (1, 2048, 2049, 10 ** 6):
        for K in (1, 63, 64, 320, 512, 1024, 1536, 2048, 3072, 4096, 8192):
            s = SR.gemm_k_split(rows, K)
            assert 1 <= s <= SR.SPLITK_MAX and K % s == 0 and (s == 1 or (K // s) % 64 == 0 and K // s >= SR.SPLITK_MIN_K)
