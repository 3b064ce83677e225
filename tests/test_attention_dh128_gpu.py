"""-m gpu: zh_attention_f16, zh_attention_causal_f16 and zh_attention_f16_splitk at head_dim 128 (the ViT-L towers' decoder: 8 heads over
width 1024), fp16 and split-pair "x3" operands, against float64.

The kernels are the dh = 128 instantiations of attn_f16_kernel: four 32-row d tiles of O^T, eight k-steps of Q K^T, 16 chunks of 16 bytes
per K / V row (two / four full load passes of a workgroup per 32- / 64-key tile), V rows 160 halves apart in LDS; the split-pair operands
always run the plain loop (there is no pipelined dh = 128 kernel).  Everything goes through the project's own harness,
test_layout_guard_attention_gpu.py::attn_case — operands and outputs in guard-banded arenas at the engine's layouts, float64
softmax(Q K^T scale) V as the reference, its tolerances (4e-3 for a plain fp16 O, 2e-5 for a split-pair O), its two assert_untouched — over
the shapes that file runs at dh = 64 and 96, and over the eight structured-softmax families of tests/_attention_case.py with the
structural asserts of test_attention_softmax_gpu.py.

Largest |O - float64| observed on an MI355X (a record, not a threshold), head_dim 128:
  group / family          fp16 (tol 4e-3)   x3 (tol 2e-5)
  cross layout, 1 x 1        4.7e-04          6.1e-06     (a plain fp16 O from the x3 kernel, tol 4e-3: 9.8e-04)
  cross layout, 3 x 3        8.4e-04          1.0e-05     (a plain fp16 O from the x3 kernel: 1.9e-03)
  packed + causal, 1 x 1     8.7e-04          5.8e-06
  packed + causal, 3 x 3     1.1e-03          8.2e-06
  key split, exact arena     3.1e-04          5.2e-06
  staircase                  6.3e-04          3.0e-07
  row_schedule               5.8e-04          3.3e-07
  peak_tail                  9.8e-04          7.6e-06
  one_hot                    2.6e-09          4.8e-07
  uniform                    1.2e-04          6.7e-08
  common_offset              2.5e-04          5.1e-07
  causal                     1.0e-03          3.0e-06
  key_split                  9.5e-04          6.4e-07
The families sit where head_dim 64 / 96 do (test_attention_softmax_gpu.py's table).  The random-operand groups (randn * 2.5 under x3)
carry the fp32 rounding of a 128-term score of size ~70 and reach half of the x3 tolerance; it is not widened.
"""
from unittest import mock

import pytest

from tests import _attention_case as ac
from tests import test_layout_guard_attention_gpu as lg
from tests.test_layout_guard_attention_gpu import attn_case

pytestmark = pytest.mark.gpu

DH = 128
variants = pytest.mark.parametrize("x3", [False, True])


class _Record:
    """Runs a block with attn_case's assert_close wrapped: the same assertion, its returned max |err| kept per tolerance (the record in
    the docstring above)."""

    def __init__(self, what):
        self.what, self.worst = what, {}

    def __enter__(self):
        inner = lg.assert_close

        def close(got, ref, atol, rtol=0.0, what=""):
            err = inner(got, ref, atol, rtol, what)
            self.worst[atol] = max(self.worst.get(atol, 0.0), err)
            return err
        self._patch = mock.patch.object(lg, "assert_close", close)
        self._patch.start()
        return self

    def __exit__(self, *exc):
        self._patch.stop()
        if exc[0] is None:
            print(f"{self.what}: max |O - float64| " + ", ".join(f"{e:.1e} (tol {t:g})" for t, e in sorted(self.worst.items())))
        return False


@variants
@pytest.mark.parametrize("heads,B", [(1, 1), (3, 3)])
def test_attention_cross_layout_every_edge(dev, x3, heads, B):
    """Cross-attention layout: Tq in {1, 31, 32, 33, 127, 128, 129} x Tk in {1, kt - 1, kt, kt + 1, 2 kt + 5}; the three ragged corners with a
    non-default scale and, for x3, a plain fp16 O."""
    kt, n = lg._kt(x3), 0
    with _Record(f"cross layout x3={x3} heads={heads} B={B}"):
        for Tq in lg.TQ:
            for Tk in (1, kt - 1, kt, kt + 1, 2 * kt + 5):
                attn_case(dev, x3=x3, dh=DH, heads=heads, B=B, Tq=Tq, Tk=Tk, layout="slice", seed=Tq * 7 + Tk)
                n += 1
        for Tq, Tk in ((33, kt + 1), (129, 2 * kt + 5), (1, 1)):
            attn_case(dev, x3=x3, dh=DH, heads=heads, B=B, Tq=Tq, Tk=Tk, layout="slice", scale=0.07, seed=Tq)
            if x3:
                attn_case(dev, x3=True, dh=DH, heads=heads, B=B, Tq=Tq, Tk=Tk, layout="slice", split_o=False, seed=Tq + 1)
            n += 1 + int(x3)
    assert n == 35 + (6 if x3 else 3)


@variants
@pytest.mark.parametrize("heads,B", [(1, 1), (3, 3)])
def test_attention_packed_qkv_and_causal(dev, x3, heads, B):
    """Packed QKV over the query-block and key-tile edges, and the causal entry (which takes any supported head dim) at T in {1, 33, 77}."""
    kt = lg._kt(x3)
    with _Record(f"packed x3={x3} heads={heads} B={B}"):
        for T in sorted({1, 31, 32, 33, kt - 1, kt, kt + 1, 127, 128, 129, 2 * kt + 5}):
            attn_case(dev, x3=x3, dh=DH, heads=heads, B=B, Tq=T, Tk=T, layout="packed", seed=T)
        for T in (1, 33, 77):
            attn_case(dev, x3=x3, dh=DH, heads=heads, B=B, Tq=T, Tk=T, layout="packed", causal=True, seed=T + 100)
            attn_case(dev, x3=x3, dh=DH, heads=heads, B=B, Tq=T, Tk=T, layout="slice", causal=True, scale=0.07, seed=T + 200)


@variants
def test_attention_key_split_workspace_exact(dev, x3):
    """ksplit in {2, 3} with ragged last chunks, the workspace exactly zh_attention_splitk_workspace_size bytes between guards (130 floats per
    partial row at dh = 128); the two splits that leave an empty chunk are refused and write nothing."""
    kt = lg._kt(x3)
    with _Record(f"key split x3={x3}"):
        for ksplit in (2, 3):
            for Tk in (2 * kt + 5, 5 * kt + 5):
                for Tq, heads, B in ((1, 1, 1), (33, 3, 3), (129, 3, 1)):
                    attn_case(dev, x3=x3, dh=DH, heads=heads, B=B, Tq=Tq, Tk=Tk, layout="slice", ksplit=ksplit, seed=Tk + Tq)
            attn_case(dev, x3=x3, dh=DH, heads=3, B=3, Tq=2 * kt + 5, Tk=2 * kt + 5, layout="packed", ksplit=ksplit, scale=0.07, seed=9)
    attn_case(dev, x3=x3, dh=DH, heads=1, B=1, Tq=33, Tk=2 * kt + 5, layout="slice", ksplit=4, expect_error=True)
    attn_case(dev, x3=x3, dh=DH, heads=1, B=1, Tq=33, Tk=3 * kt + 5, layout="slice", ksplit=3, expect_error=True)


# ------------------------------------------------------------------------------------------ the structured-softmax families
def _run(dev, family, x3):
    cs = ac.cases(family, x3, DH)
    assert cs and {c.layout for c in cs} == {"packed", "slice"}
    assert any(c.heads == 3 and c.B == 2 for c in cs) and all(c.dh == DH for c in cs)
    with _Record(f"{family} x3={x3} ({len(cs)} cases)"):
        for case in cs:
            attn_case(dev, **case.kwargs())
    return cs


@variants
def test_staircase_rising_and_falling(dev, x3):
    assert len(_run(dev, "staircase", x3)) == 2 * len(ac.STEPS)


@variants
def test_row_dependent_schedule_in_one_wave(dev, x3):
    assert {c.Tq for c in _run(dev, "row_schedule", x3)} >= {33, 129}


@variants
def test_peak_over_heavy_tail(dev, x3):
    cs = _run(dev, "peak_tail", x3)
    assert {c.desc["depth"] for c in cs} == set(ac.TAIL_DEPTHS) and {c.Tk for c in cs} == {4 * ac.tile_height(x3) + 5, 1029}


@variants
def test_one_hot(dev, x3):
    assert any(c.causal for c in _run(dev, "one_hot", x3))


@variants
def test_uniform_mean(dev, x3):
    kt = ac.tile_height(x3)
    assert {c.Tk for c in _run(dev, "uniform", x3)} == {1, kt - 1, kt + 1, 1029}


@variants
def test_common_offset(dev, x3):
    for case in _run(dev, "common_offset", x3):
        assert float((ac.reference(case) - ac.reference(case.desc["base"])).abs().max()) < 1e-9


@variants
def test_causal_beyond_one_query_block(dev, x3):
    assert {c.Tq for c in _run(dev, "causal", x3)} == set(ac.CAUSAL_T)


@variants
def test_key_split_unequal_chunks(dev, x3):
    cs = _run(dev, "key_split", x3)
    assert {c.ksplit for c in cs if not c.expect_error} == {2, 4} and sum(c.expect_error for c in cs) == 1
