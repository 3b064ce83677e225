"""No GPU: tests/_guard.py can fail.  Torch stand-ins for a kernel write through the arena's views; every seeded overrun must be
reported at the right (view, plane, batch, row, col), a correct stand-in must pass, and a stand-in that reads one element of 0xFF
padding must produce a NaN that the value check reports."""
import pytest
import torch

from tests._guard import (IN_FILL, LEAD_GUARD, OUT_FILL, Arena, GuardViolation, assert_close, assert_equal, assert_untouched, assert_within)

f16, f32 = torch.float16, torch.float32


def _out_arena():
    """Two outputs: a batched fp32 matrix with row and batch padding behind a 4-byte-offset base, and a split pair with a padded plane."""
    ar = Arena(OUT_FILL)
    c = ar.add("C", f32, 5, 7, ld=12, batch=3, bstride=5 * 12 + 20, misalign=4)
    s = ar.add("S", f16, 6, 8, ld=16, batch=2, bstride=6 * 16 + 8, planes=2, plane=2 * (6 * 16 + 8) + 24)
    return ar, c, s


def _correct_standin(c, s):
    c.t.copy_(torch.arange(3 * 5 * 7, dtype=f32).reshape(1, 3, 5, 7))
    s.t.copy_(torch.ones((2, 2, 6, 8)))


def test_layout_and_alignment():
    ar, c, s = _out_arena()
    assert c.t.data_ptr() % 256 == 4 and s.t.data_ptr() % 256 == 0
    assert c.off >= LEAD_GUARD and s.off - (c.off + ((3 - 1) * 80 + 4 * 12 + 7) * 4) >= LEAD_GUARD + 256 * 12 * 4
    assert c.t.stride() == (0, 80, 12, 1) and s.t.stride() == (232, 104, 16, 1) and s.act().plane == 232
    assert bool((ar.bytes == OUT_FILL).all())
    assert int(ar.allowed_mask().ne(0).sum()) == 3 * 5 * 7 * 4 + 2 * 2 * 6 * 8 * 2


def test_correct_standin_passes_and_values_round_trip():
    ar, c, s = _out_arena()
    _correct_standin(c, s)
    assert_untouched(ar)
    assert_equal(c.get(), torch.arange(105, dtype=f32).reshape(1, 3, 5, 7))
    assert float(s.pair().min()) == 2.0 and s.pair().shape == (2, 6, 8)
    with pytest.raises(GuardViolation):                 # only C declared: the (legal) write to S is then a violation
        assert_untouched(ar, [c])


def _raw(view):
    """The view's whole element range as a flat tensor (what a kernel's pointer arithmetic sees)."""
    return view.arena.bytes[view.off:view.end].view(view.dtype)


@pytest.mark.parametrize("name,elem,where", [
    ("one element past N in a row", lambda c, s: 1 * 80 + 2 * 12 + 7, ("C", 0, 1, 2, 7)),
    ("one row past M (last batch item)", lambda c, s: 2 * 80 + 5 * 12 + 3, ("C", 0, 2, 5, 3)),
    ("inter-batch padding", lambda c, s: 0 * 80 + 5 * 12 + 1, ("C", 0, 0, 5, 1)),
])
def test_overruns_of_a_batched_matrix_are_located(name, elem, where):
    ar, c, s = _out_arena()
    _correct_standin(c, s)
    _raw(c)[elem(c, s)] = 1.0
    with pytest.raises(GuardViolation) as e:
        assert_untouched(ar)
    assert e.value.where == where, (name, e.value.where)
    assert f"view '{where[0]}'" in str(e.value) and f"row {where[3]} col {where[4]}" in str(e.value)


def test_write_between_split_planes_is_located():
    ar, c, s = _out_arena()
    _correct_standin(c, s)
    _raw(s)[1 * 104 + 5 * 16 + 8 + 10] = 3.0            # behind the hi plane's last row, before the lo plane starts at 232
    with pytest.raises(GuardViolation) as e:
        assert_untouched(ar)
    assert e.value.where == ("S", 0, 1, 6, 2)
    ar, c, s = _out_arena()
    _correct_standin(c, s)
    _raw(s)[232 + 3 * 16 + 8] = 3.0                      # lo plane, one element past N
    with pytest.raises(GuardViolation) as e:
        assert_untouched(ar)
    assert e.value.where == ("S", 1, 0, 3, 8)


def test_write_into_the_leading_guard_is_located():
    ar, c, s = _out_arena()
    ar.bytes[s.off - 2] = 0
    with pytest.raises(GuardViolation) as e:
        assert_untouched(ar)
    assert e.value.where[0] == "S" and e.value.where[3] < 0


def test_restoring_the_sentinel_elsewhere_does_not_hide_a_write():
    """A stand-in that writes past N and then puts the sentinel back into ANOTHER padding byte: still one byte that is not 0xA5."""
    ar, c, s = _out_arena()
    _correct_standin(c, s)
    _raw(c)[2 * 12 + 9] = 5.0
    ar.bytes[c.off + (3 * 12 + 9) * 4] = OUT_FILL
    with pytest.raises(GuardViolation) as e:
        assert_untouched(ar)
    assert e.value.where == ("C", 0, 0, 2, 9)
    # ... and a write of the sentinel VALUE into padding is, by construction, invisible: the checks rest on values that differ from it
    ar, c, s = _out_arena()
    _correct_standin(c, s)
    ar.bytes[c.off + (2 * 12 + 9) * 4] = OUT_FILL
    assert_untouched(ar)


def test_workspace_is_exactly_its_size():
    ar = Arena(OUT_FILL)
    ws = ar.workspace("ws", 1000)
    ws.t.fill_(7)
    assert_untouched(ar)
    ar.bytes[ws.off + 1000] = 7
    with pytest.raises(GuardViolation) as e:
        assert_untouched(ar)
    assert e.value.where == ("ws", 0, 0, 1, 0)


@pytest.mark.parametrize("dtype", [f16, f32])
def test_reading_input_padding_gives_a_nan_the_value_check_reports(dtype):
    ia = Arena(IN_FILL)
    a = ia.add("A", dtype, 4, 6, ld=8)
    x = torch.arange(24, dtype=f32).reshape(4, 6)
    a.put(x)
    good = a.m2.float().sum(1)
    assert_close(good, x.double().sum(1), 1e-6, what="row sums")
    bad = _raw(a)[:4 * 8].view(4, 8)[:, :7].float().sum(1)         # reads column 6: one element of 0xFF padding per row
    with pytest.raises(AssertionError, match="non-finite"):
        assert_close(bad, x.double().sum(1), 1e-6, what="row sums")
    assert int(ia.bytes[a.off + 6 * a.isz]) == 0xFF
    # the integer faces of the same fill
    assert int(ia.bytes[:8].view(torch.int64)[0]) == -1 and int(ia.bytes[0]) == 255


def test_value_checks_report_the_index():
    with pytest.raises(AssertionError, match=r"at \(1, 2\)"):
        assert_close(torch.tensor([[0., 0., 0.], [0., 0., 1.]]), torch.zeros(2, 3), 1e-3, what="x")
    with pytest.raises(AssertionError, match=r"first at \(0, 1\)"):
        assert_equal(torch.tensor([[1, 2]]), torch.tensor([[1, 3]]), "labels")
    assert_equal(torch.tensor([float("nan")]), torch.tensor([float("nan")]))
    with pytest.raises(AssertionError, match=r"> 1 at \(2,\)"):
        assert_within(torch.tensor([1.0, 2.0, 3.5]), torch.tensor([1.0, 2.0, 3.0]), torch.tensor([0.1, 0.1, 0.4]), "y")
    with pytest.raises(AssertionError, match="non-finite"):
        assert_within(torch.tensor([float("nan")]), torch.tensor([0.0]), torch.tensor([1.0]), "y")
    assert assert_within(torch.tensor([1.05]), torch.tensor([1.0]), torch.tensor([0.1])) == pytest.approx(0.5, rel=1e-5)


def test_pointer_in_front_of_a_view_and_row_offset():
    """View.origin(): the buffer pointer a row kernel is handed when its mapping starts `offset` rows into the buffer lies in the view's
    own leading guard; rows the mapping skips are guard bytes and a write to one is located."""
    ar = Arena(OUT_FILL)
    D, T = 8, 5
    v = ar.add("stacked", f32, T, D, batch=3, bstride=2 * T * D, lead=T * D * 4, tail_rows=4)       # rows [T, 2T) of every block of 2T
    buf = v.origin(T * D)
    assert buf.data_ptr() == v.t.data_ptr() - T * D * 4
    for g in range(3):
        buf[(g * 2 * T + T) * D:(g * 2 * T + 2 * T) * D] = 1.0
    assert_untouched(ar)
    assert float(v.get().min()) == 1.0
    buf[(1 * 2 * T + 2) * D + 3] = 1.0                   # row 2 of block 1: a skipped row (between group 0's rows and group 1's)
    with pytest.raises(GuardViolation) as e:
        assert_untouched(ar)
    assert e.value.where == ("stacked", 0, 0, T + 2, 3)
