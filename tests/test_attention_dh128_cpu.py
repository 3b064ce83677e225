"""CPU: head dim 128 (the ViT-L towers' decoder: 8 heads over width 1024) in the attention launcher's plan (csrc/attention_dispatch.h
through zh_dev_attention_plan) and in zutis_amd/shape_rules.py.  The plan takes dh = 128 with the fp16 kernel and the plain
split-pair loop and never with the pipelined one, which has no dh = 128 kernel; every other value outside {64, 96} stays refused.
Nothing is launched.  (That the two dh = 128 kernels compile without scratch at two waves per SIMD is checked by the build itself,
through the MIN_OCCUPANCY entries the last test names: the `lib` fixture is the proof.)"""
import pytest

from tests import _attention_plan_case as PC
from zutis_amd import _lib, build
from zutis_amd import shape_rules as SR

DH = 128
HEADS, QUERIES = 8, 100                             # the decoder: 8 heads, 100 queries
CROSS_KEYS = (1024, 2304, 6120)                     # 224 x 224, 336 x 336 and 480 x 640 at patch 14, after the x2 upsample


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load(raw=True)


def _error(lib):
    return lib.zh_last_error().decode()


def cases():
    out = []
    for B in PC.BATCHES:
        for x3 in (False, True):
            out.append(PC.Case(B, HEADS, QUERIES, QUERIES, DH, x3, False, SR.self_attention_key_split(B, QUERIES, HEADS, DH, x3, False)))
            for M in CROSS_KEYS:
                for S in sorted({SR.cross_attention_key_split(s, B, HEADS, QUERIES, M, x3) for s in PC.CROSS_SETTINGS}):
                    out.append(PC.Case(B, HEADS, QUERIES, M, DH, x3, False, S))
    out += [PC.Case(2, 3, Tq, Tk, DH, x3, False, 1) for x3 in (False, True) for Tq in PC.EDGE_TQ for Tk in PC.EDGE_TK]
    out += [PC.Case(n, 1, 5, 40, DH, x3, False, 1) for n in PC.GRID_EDGES for x3 in (False, True)]
    out += [PC.Case(n // 4, 1, 5, 200, DH, True, False, 4) for n in PC.GRID_EDGES if n % 4 == 0]
    return out


def model(c):
    """_attention_plan_case.model's arithmetic for a dh = 128 case: the same lines without the pipelined-loop one."""
    kt, S = (32 if c.x3 else 64), max(1, c.ksplit)
    nqb = -(-c.Tq // 128)
    items = c.batch * c.heads * nqb * S
    grid = -(-items // 8) * 8
    variant = PC.X3 if c.x3 else PC.F16
    if S == 1:
        return PC.Plan(variant, kt, nqb, items, grid, 0, 1, 0, 0, 0)
    rows = S * c.batch * c.heads * c.Tq
    return PC.Plan(variant, kt, nqb, items, grid, 0, S, -(-(-(-c.Tk // kt)) // S) * kt, rows * (c.dh + 2) * 4,
                   -(-(c.batch * c.Tq * c.heads * c.dh // 4) // 256))


def test_plan_takes_head_dim_128_and_never_pipelines_it(lib):
    cs = cases()
    assert len(set(cs)) > 120 and any(c.ksplit > 1 for c in cs)
    seen, split = set(), 0
    for c in cs:
        p = PC.ask(lib, c)
        assert p is not None, (c, _error(lib))
        assert p.variant in (PC.F16, PC.X3) and p.variant != PC.X3_PIPE and p.pipe == 0, (c, p)
        assert p == model(c), (c, p)
        assert not SR.pipelined_loop(p.items, DH, c.x3)
        seen.add(p.variant)
        if c.ksplit > 1:
            split += 1
            rows = c.ksplit * c.batch * c.heads * c.Tq
            assert p.workspace_bytes == rows * (128 + 2) * 4 == lib.zh_attention_splitk_workspace_size(c.batch, c.heads, c.Tq, DH, c.ksplit)
            assert PC.ask(lib, c, workspace_bytes=p.workspace_bytes - 1) is None and "workspace too small" in _error(lib)
    assert seen == {PC.F16, PC.X3} and split > 20


def test_decoder_cross_attention_splits_as_the_settings_say(lib):
    """The drop-in's setting of 12 splits the keys at every M >= 1024 (M = 1024 is the threshold), batch or no batch: 12 ways, or the
    largest split below that leaves no chunk empty (16 fp16 tiles at M = 1024: 8 chunks of 2)."""
    for x3 in (False, True):
        for M in CROSS_KEYS:
            t = -(-M // (32 if x3 else 64))
            want = max(s for s in range(1, 13) if (s - 1) * -(-t // s) < t)       # M = 1024: 8 of 16 fp16 tiles, 11 of 32 split-pair ones
            assert want == SR.fit_key_split(12, t) and want == {(1024, False): 8, (1024, True): 11}.get((M, x3), 12)
            for B in PC.BATCHES:
                S = SR.cross_attention_key_split(12, B, HEADS, QUERIES, M, x3)
                assert S == want
                p = PC.ask(lib, PC.Case(B, HEADS, QUERIES, M, DH, x3, False, S))
                assert p.ksplit == S and p.items == B * HEADS * S and (S - 1) * p.kchunk < M <= S * p.kchunk
            assert SR.cross_attention_key_split(12, 1, HEADS, QUERIES, M - 1 if M == 1024 else M, x3) == (1 if M == 1024 else want)


def test_pipelined_loop_rule_by_head_dim(lib):
    for n, want in PC.GRID_EDGES.items():
        assert SR.pipelined_loop(n, 128, True) is False and SR.pipelined_loop(n, 128, False) is False
        p = PC.ask(lib, PC.Case(n, 1, 5, 40, 128, True, False, 1))
        assert (p.items, p.variant, p.pipe) == (n, PC.X3, 0)
        assert SR.pipelined_loop(n, 64, True) is want and SR.pipelined_loop(n, 96, True) is True       # unchanged: what GRID_EDGES says
        assert bool(PC.ask(lib, PC.Case(n, 1, 5, 40, 64, True, False, 1)).pipe) is want
        assert PC.ask(lib, PC.Case(n, 1, 5, 40, 96, True, False, 1)).pipe == 1
    assert set(SR.PIPELINED_HEAD_DIMS) == {64, 96} < set(SR.HEAD_DIMS)


def test_long_sequence_model_counts_two_workgroups_per_cu_at_128():
    """The round model's workgroups per CU: 2 at dh = 128 as at dh = 96 (pipelined or not), so the model — which reads the head dim
    nowhere else — gives the two the same split for the same grid, and 96 items on 256 CUs are split at both."""
    f = SR.long_sequence_key_split
    for x3 in (False, True):
        for items, ktiles in ((96, 300), (264, 173), (600, 64), (1056, 173), (2048, 90)):
            assert f(items, ktiles, 128, x3, 10 ** 6) == f(items, ktiles, 96, x3, 10 ** 6)
    assert f(96, 300, 128, True, 10 ** 6) > 1


def test_other_head_dims_stay_refused(lib):
    for dh in (80, 112, 160, 256):
        for x3 in (False, True):
            assert PC.ask(lib, Tq=4, Tk=4, dh=dh, x3=x3) is None and f"head_dim {dh}" in _error(lib)


def test_shape_rules_head_dims_are_the_plans(lib):
    accepted = tuple(dh for dh in range(8, 264, 8) if PC.ask(lib, Tq=4, Tk=4, dh=dh) is not None)
    assert accepted == tuple(sorted(SR.HEAD_DIMS)) == (64, 96, 128)
    assert accepted == tuple(dh for dh in range(8, 264, 8) if PC.ask(lib, Tq=4, Tk=4, dh=dh, x3=True) is not None)


def test_engine_refusal_reads_the_tuple():
    """ZutisEngine refuses a decoder head dim outside shape_rules.HEAD_DIMS at construction (before anything touches a GPU), naming the dims."""
    import torch
    from zutis_amd._lib import ZutisHipError
    from zutis_amd.engine import ZutisEngine
    D = 640                                            # 8 decoder heads -> head dim 80
    P = {"encoder.class_embedding": torch.zeros(D), "encoder.transformer.resblocks.0.ln_1.weight": torch.zeros(D),
         "decoder.layers.0.norm1.weight": torch.zeros(D), "query_embed": torch.zeros(5, D), "encoder.proj": torch.zeros(D, 64),
         "encoder.positional_embedding": torch.zeros(17, D)}
    with pytest.raises(ZutisHipError, match=r"head_dim 80 unsupported by zh_attention_f16 \(64, 96, 128\)"):
        ZutisEngine(P, 16, 8)
    assert ", ".join(map(str, SR.HEAD_DIMS)) == "64, 96, 128"


def test_build_guards_the_two_dh128_kernels():
    occ = build.MIN_OCCUPANCY["attention.hip"]
    assert occ["attn_f16_kernelILi128ELi4ELi0ELi0EE"] == 2 and occ["attn_f16_kernelILi128ELi4ELi1ELi0EE"] == 2      # fp16, split pair (plain loop)
    assert not any("ILi128E" in k and k.endswith("ELi1ELi1EE") for k in occ)                                        # no pipelined dh = 128 kernel
    assert "attention.hip" in build.NO_SCRATCH and len(occ) == 8
