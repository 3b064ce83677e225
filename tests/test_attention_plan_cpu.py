"""CPU: the attention launcher's plan (csrc/attention_dispatch.h through the developer entry zh_dev_attention_plan) is held to the
arithmetic stated in tests/_attention_plan_case.py over the product's shapes and the tile / grid edges, and the pure Python copies of
its rules that zutis_amd/shape_rules.py keeps are held to the plan.  Nothing is launched.
(That every (head_dim, variant) of the plan has a kernel is a static_assert beside the launcher's table, and that
build.py's MIN_OCCUPANCY names all six kernels is checked by the build itself: the `lib` fixture proves both.)"""
import pytest

from tests import _attention_plan_case as PC
from zutis_amd import _lib, build
from zutis_amd import shape_rules as SR


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load(raw=True)


def _error(lib):
    return lib.zh_last_error().decode()


def test_plan_matches_the_model_over_the_sweep(lib):
    cases = PC.sweep()
    assert len(set(cases)) > 300
    seen = set()
    for c in cases:
        p = PC.ask(lib, c)
        assert p == PC.model(c), (c, p, _error(lib))
        seen.add((c.dh, p.variant))
        if c.x3:                                     # the shape_rules copy of the pipelined-loop rule, asked of the workgroups themselves
            assert SR.pipelined_loop(p.items, c.dh, True) == bool(p.pipe), (c, p)
        else:
            assert not SR.pipelined_loop(p.items, c.dh, False) and not p.pipe
    assert seen == {(dh, v) for dh in (64, 96) for v in (PC.F16, PC.X3, PC.X3_PIPE) if (dh, v) != (96, PC.X3)}     # dh = 96 split pairs: always pipelined


def test_pipelined_loop_flips_at_the_round_edges(lib):
    for n, want in PC.GRID_EDGES.items():
        for c in (PC.Case(n, 1, 5, 40, 64, True, False, 1), PC.Case(1, n, 128, 40, 64, True, False, 1)):
            p = PC.ask(lib, c)
            assert (p.items, p.grid, bool(p.pipe)) == (n, -(-n // 8) * 8, want), (c, p)
            assert p.variant == (PC.X3_PIPE if want else PC.X3)
        assert PC.ask(lib, PC.Case(n, 1, 5, 40, 96, True, False, 1)).variant == PC.X3_PIPE
        assert PC.ask(lib, PC.Case(n, 1, 5, 40, 64, False, False, 1)).variant == PC.F16
        assert SR.pipelined_loop(n, 64, True) == want and SR.pipelined_loop(n, 96, True) and not SR.pipelined_loop(n, 64, False)


@pytest.mark.parametrize("x3", [False, True], ids=["f16", "x3"])
def test_key_split_is_accepted_exactly_when_fit_key_split_keeps_it(lib, x3):
    kt = 32 if x3 else 64
    for Tk in range(1, 401):
        ktiles = -(-Tk // kt)
        assert ktiles == SR.key_tiles(Tk, x3)
        for S in range(1, 65):
            p = PC.ask(lib, Tq=3, Tk=Tk, x3=x3, ksplit=S)
            fits = SR.fit_key_split(S, ktiles) == S
            assert (p is not None) == fits, (Tk, S, p)
            if p is None:
                assert "leaves an empty key chunk" in _error(lib)
            elif S > 1:
                assert p.ksplit == S and p.kchunk % kt == 0 and (S - 1) * p.kchunk < Tk <= S * p.kchunk, (Tk, S, p)
            else:
                assert (p.ksplit, p.kchunk, p.workspace_bytes, p.combine_grid) == (1, 0, 0, 0)


def test_workspace_size_has_one_definition(lib):
    n = 0
    for c in PC.sweep():
        if c.ksplit > 1:
            n += 1
            want = PC.model(c).workspace_bytes
            assert lib.zh_attention_splitk_workspace_size(c.batch, c.heads, c.Tq, c.dh, c.ksplit) == want == PC.ask(lib, c).workspace_bytes, c
            assert PC.ask(lib, c, workspace_bytes=want - 1) is None and "workspace too small" in _error(lib)
    assert n > 50


def test_split_entry_refuses_a_short_workspace_before_any_launch(lib):
    """Made-up pointers: a launch would fault; the argument check returns first."""
    c = PC.Case(2, 8, 100, 1764, 96, True, False, 12)
    need = PC.model(c).workspace_bytes
    a = PC.arguments(lib, c, workspace_bytes=need - 1)
    launch_args = a[:17] + (0.125,) + a[18:] + (None,)           # scale in place of the causal flag, the stream last
    assert lib.zh_attention_f16_splitk(*launch_args) == _lib.constants()["ZH_ERR_ARG"]
    assert "workspace too small" in _error(lib) and f"({need - 1} < {need})" in _error(lib)


def test_bad_splits_are_argument_errors(lib):
    assert PC.ask(lib, Tq=100, Tk=64 * 64, ksplit=64) is not None
    assert PC.ask(lib, Tq=100, Tk=64 * 65, ksplit=65) is None and "ksplit 65 not in 1..64" in _error(lib)
    assert PC.ask(lib, Tq=100, Tk=100, causal=True, ksplit=1) is not None
    assert PC.ask(lib, Tq=100, Tk=100, causal=True, ksplit=2) is None and "not for the causal form" in _error(lib)
    assert PC.ask(lib, Tq=4, Tk=4, dh=80) is None and "head_dim 80" in _error(lib)
