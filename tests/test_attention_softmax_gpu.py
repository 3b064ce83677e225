"""-m gpu: the softmax inside zh_attention_f16, zh_attention_causal_f16 and zh_attention_f16_splitk on scores built to a pattern
(tests/_attention_case.py), fp16 and split-pair "x3" operands, head_dim 64 and 96, against float64.

Random Q and K never move the kernels' lazy running max after the first key tile, leave no mass in subnormal probabilities, mask one
query block only and split keys into chunks of equal maxima.  These cases do, through the guard-banded arenas of
test_layout_guard_attention_gpu.py::attn_case (its `inputs=` argument): the same assert_close against float64 at the project's tolerances
(4e-3 for a plain fp16 O, 2e-5 for a split-pair O), the same two assert_untouched.  Every case has 3 heads x 2 images, each (image, head)
with a pattern of its own; both the packed and the slice layout occur in every family.

Constants read from attention.hip: L = ZH_ATTN_LAZY_LOG2 = 8 log2 units, key-tile height kt = 64 (fp16 kernels) / 32 (x3).

Families (scores in log2 units, the unit of the running max):
  staircase      Tk = 6 kt + 5, tile t at t * step +- 0.01, step in {0.5, 0.99, 1.01, 2} L, rising (the reference point moves at every
                 second / every tile: accumulators and row sum are rescaled by alpha = 2^-step) and falling (max in tile 0, later P down
                 to 2^-96); centred on 0, so x3 stays within +-48.
  row_schedule   a_i in {+1, 0, -1} by (i + head) % 3 against a rising staircase, Tq = 33, 129 and 6 kt + 5: rising, flat and falling rows
                 in neighbouring lanes of one wave — alpha != 1 and alpha == 1 through the same __any branch.
  peak_tail      one key at 0, all others at -15.3 / -17.3 / -12.0, Tk in {4 kt + 5, 1029}; V of the tail opposite in sign to the peak's,
                 or random; peak at key 0, the last key of tile 0, the first key of the ragged last tile, the very last key.  At -15.3 and
                 -17.3 the tail's P are fp16 subnormals (x3: subnormal hi and lo) carrying up to 2.5 % of the row.
  one_hot        one key 40 log2 units above the rest at the same four places, and — causal, T in {33, 64} — the diagonal key of every row:
                 O is that key's V row.
  uniform        Q = 0, Tk in {1, kt - 1, kt + 1, 1029}: O is the mean of V — a constant, V[j] = j / Tk (depends on the exact key count),
                 randn.
  common_offset  every score of a row shifted by +-64 (fp16 and x3) or +-1000 (fp16); the reference equals the unshifted case's.
  causal         T in {64, 65, 128, 129, 200}: a second query block, its key-tile limit and the diagonal test of waves with q0 >= 128;
                 uniform heads (row i = mean of V[0..i]: a mask off by one key shows at every row) and a random head; one non-default scale.
  key_split      ksplit 2 (Tk = 8 kt + 5) and 4 (12 kt + 5), the dominant key in the first chunk / in the last chunk / a chunk 150 log2
                 units below the rest (w_s = 0 exactly) / all chunks equal and uniform; the workspace in attn_case's exact-size arena.
                 ksplit 4 at 8 kt + 5 (9 tiles) would leave its fourth chunk empty: the library refuses it, and that is what is checked.

tests/test_attention_softmax_cpu.py shows that the cases have these structures, that float32 evaluation of the reference costs less than
a quarter of the tolerance, and that a restatement of the tile loop fails them when it flushes subnormal P, forgets alpha on the row sum
or masks one key late.

Largest |O - float64| observed on an MI355X (a record, not a threshold), head_dim 64 / 96:
  family             fp16 (tol 4e-3)         x3 (tol 2e-5)
  staircase        6.9e-04 / 6.1e-04     2.0e-07 / 3.7e-07
  row_schedule     6.3e-04 / 6.7e-04     2.0e-07 / 2.9e-07
  peak_tail        1.0e-03 / 1.0e-03     7.6e-06 / 9.8e-06     (x3: the tail at -15.3, Tk = 1029, opposite-sign V)
  one_hot          2.0e-09 / 1.7e-09     4.8e-07 / 4.8e-07
  uniform          1.2e-04 / 1.2e-04     6.7e-08 / 7.2e-08
  common_offset    2.0e-04 / 2.0e-04     6.5e-07 / 6.5e-07
  causal           9.8e-04 / 9.8e-04     1.4e-06 / 2.0e-06
  key_split        9.3e-04 / 9.6e-04     6.4e-07 / 9.3e-07
The fp16 figures are the rounding of a plain fp16 O (2^-11 |o|) nearly throughout.  The x3 peak_tail figure is the split pair's absolute
quantum: a probability below 2^-14 is held to a multiple of 2^-24, 2^-15.3 = 415.87 quanta is stored as 416, and 1028 equal keys add the
0.13 quanta coherently (7.7e-6 for |v| = 1, as the CPU restatement gives too); it stays inside 2e-5, so no derived bound is used.
"""
import pytest

from tests import _attention_case as ac
from tests.test_layout_guard_attention_gpu import attn_case

pytestmark = pytest.mark.gpu

variants = pytest.mark.parametrize("x3", [False, True])
head_dims = pytest.mark.parametrize("dh", [64, 96])


def _run(dev, family, x3, dh):
    cs = ac.cases(family, x3, dh)
    assert cs and {c.layout for c in cs} == {"packed", "slice"}
    assert any(c.heads == 3 and c.B == 2 for c in cs)
    for case in cs:
        attn_case(dev, **case.kwargs())
    print(f"{family} x3={x3} dh={dh}: {len(cs)} cases")
    return cs


@variants
@head_dims
def test_staircase_rising_and_falling(dev, x3, dh):
    """The reference point moves at every tile (1.01 L, 2 L), every second tile (0.99 L), rarely (0.5 L) or never (falling)."""
    assert len(_run(dev, "staircase", x3, dh)) == 2 * len(ac.STEPS)


@variants
@head_dims
def test_row_dependent_schedule_in_one_wave(dev, x3, dh):
    """Rising, flat and falling rows in neighbouring lanes: the rescale must reach exactly the lanes whose reference moved."""
    assert {c.Tq for c in _run(dev, "row_schedule", x3, dh)} >= {33, 129}


@variants
@head_dims
def test_peak_over_heavy_tail(dev, x3, dh):
    """Subnormal probabilities that carry mass: a kernel that flushes them is off by up to 5e-2 (fp16) / 2.5e-2 (x3) here."""
    cs = _run(dev, "peak_tail", x3, dh)
    assert {c.desc["depth"] for c in cs} == set(ac.TAIL_DEPTHS) and {c.Tk for c in cs} == {4 * ac.tile_height(x3) + 5, 1029}


@variants
@head_dims
def test_one_hot(dev, x3, dh):
    """O is one V row, wherever the key sits — the diagonal key of a causal row included."""
    assert any(c.causal for c in _run(dev, "one_hot", x3, dh))


@variants
@head_dims
def test_uniform_mean(dev, x3, dh):
    kt = ac.tile_height(x3)
    assert {c.Tk for c in _run(dev, "uniform", x3, dh)} == {1, kt - 1, kt + 1, 1029}


@variants
@head_dims
def test_common_offset(dev, x3, dh):
    """attn_case's reference is that of the shifted operands; in float64 it is the unshifted case's to 1e-9, so the kernel is held to the
    unshifted result."""
    for case in _run(dev, "common_offset", x3, dh):
        assert float((ac.reference(case) - ac.reference(case.desc["base"])).abs().max()) < 1e-9


@variants
@head_dims
def test_causal_beyond_one_query_block(dev, x3, dh):
    assert {c.Tq for c in _run(dev, "causal", x3, dh)} == set(ac.CAUSAL_T)


@variants
@head_dims
def test_key_split_unequal_chunks(dev, x3, dh):
    cs = _run(dev, "key_split", x3, dh)
    assert {c.ksplit for c in cs if not c.expect_error} == {2, 4} and sum(c.expect_error for c in cs) == 1
