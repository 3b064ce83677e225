"""The cases of tests/_rle_guard_case.py have the structure tests/test_rle_guard_gpu.py relies on: transition counts, which staging /
list / item / layout branch each shape takes, the group-count edges, capacities with a string on either side, the 17-run list."""
import numpy as np
import pytest

from tests import _rle_guard_case as R


@pytest.mark.parametrize("first", (0, 1))
@pytest.mark.parametrize("H,W,n", [(1, 1, 0), (3, 5, 0), (3, 5, 1), (3, 5, 14), (24, 24, 254), (24, 24, 512), (96, 96, 8192), (96, 96, 8193)])
def test_builder_gives_exactly_n_transitions(H, W, n, first):
    m = R.mask_with_transitions(H, W, n, first)
    t = R.transitions(m)
    assert m.shape == (H, W) and len(t) == n and R.lead_of(m) == first
    assert t.tolist() == list(range(1, n + 1))
    runs = R.runs_of(t, first, H * W)
    assert sum(runs) == H * W and len(runs) == n + 1 + first
    assert R.string_of_runs(runs) == R.string_of_mask(m)


def test_references_agree_with_the_host_encoder():
    for (H, W) in ((1, 1), (5, 7), (37, 65)):
        for name, m in R.mask_set(H, W, 3).items():
            runs = R.runs_of(R.transitions(m), R.lead_of(m), H * W)
            assert R.string_of_runs(runs) == R.string_of_mask(m), (H, W, name)
            x0, y0, x1, y1, area = R.box_area(m)
            assert area == int((m != 0).sum())
            if area:
                assert (m[y0:y1 + 1, x0:x1 + 1] != 0).sum() == area and (m[y0] != 0).any() and (m[:, x1] != 0).any()
    m = R.mask_first_pixel_set(9, 11, 1)
    assert R.lead_of(m) == 1 and R.runs_of(R.transitions(m), 1, 99)[0] == 0


def test_mask_set_holds_the_masks_it_names():
    H, W = 37, 144
    m = R.mask_set(H, W, 5)
    assert not m["empty"].any() and m["full"].all()
    assert R.transitions(m["pixel0"]).tolist() == [1] and R.transitions(m["last_pixel"]).tolist() == [H * W - 1]
    assert R.transitions(m["last_row"]).tolist() == sorted([c * H + H - 1 for c in range(W)] + [c * H for c in range(1, W)])
    assert len(R.transitions(m["row_stripes"])) == (H - 1) * W and len(R.transitions(m["col_stripes"])) == W - 1   # H odd: no wrap transition
    assert len(R.transitions(R.mask_set(16, 33, 5)["row_stripes"])) == 16 * 33 - 1
    assert set(np.unique(m["bytes"]).tolist()) == {0, 0x02, 0x80, 0xFF}
    assert 0 < len(R.transitions(m["noise"])) < R.RLE_LDS_RUNS
    # a 16-row chunk of row stripes has 16 transitions in every column: the fifth plane of the fused kernel's counter
    # (rows 16 .. 31 of H = 33; rows 0 .. 15 of H = 16, where row 0 differs from the last row of the column to the left)
    f = R.flat(R.mask_set(33, 33, 5)["row_stripes"]).reshape(33, 33)          # [column][row]
    assert int((f[1, 16:32] != f[1, 15:31]).sum()) == 16
    f = R.flat(R.mask_set(16, 33, 5)["row_stripes"]).reshape(33, 16)
    assert int((f[1, 1:16] != f[1, 0:15]).sum() + (f[1, 0] != f[0, 15])) == 16


def test_panel_shapes_reach_both_staging_paths_and_every_row_segment_count():
    stag = {W: R.panel_staging(W) for W in R.PANEL_W}
    assert stag == {1: "scalar", 63: "scalar", 64: "vector", 65: "scalar", 72: "scalar", 80: "vector", 144: "vector"}
    assert R.panel_staging(80, misalign=4) == "scalar"
    assert 80 % R.RUNS_PANEL == 16 and 144 % R.RUNS_PANEL == 16                # a 16-column last panel on the vector path
    assert 72 % 16 != 0 and 65 % R.RUNS_PANEL == 1                             # W % 16 != 0; a one-column last panel
    assert min(R.PANEL_H) < R.RUNS_SEG and R.RUNS_SEG in R.PANEL_H and R.RUNS_SEG + 1 in R.PANEL_H and R.RUNS_SEG - 1 in R.PANEL_H


def test_fused_shapes_have_the_items_per_thread_they_claim():
    for H, W in R.FUSED_MULTI:
        items, threads = R.fused_items_threads(H, W)
        assert items > threads, (H, W, items, threads)
    assert R.fused_items_threads(1040, 1) == (65, 64) and R.fused_items_threads(520, 33) == (66, 64)
    assert R.fused_items_threads(640, 480) == (600, 512) and R.fused_items_threads(640, 427) == (560, 448)
    for H, W in R.FUSED_SINGLE + ((61, 83), (48, 64), (37, 200), (120, 1024)):
        items, threads = R.fused_items_threads(H, W)
        assert items <= threads, (H, W, items, threads)
    for W in R.FUSED_W:
        for H in R.FUSED_WIDE_H.get(W, R.FUSED_H):
            items, threads = R.fused_items_threads(H, W)
            assert items <= 3 * threads and W <= 1024
    assert {R.fused_packing(H, W) for W in R.FUSED_W for H in R.FUSED_H} == {"vector", "bytes"}
    assert R.fused_packing(640, 480) == "vector" and R.fused_packing(640, 480, misalign=4) == "bytes" and R.fused_packing(33, 33) == "bytes"


def test_both_layout_branches():
    a, b = R.frle_layout(8, 8, 8192), R.frle_layout(640, 480, 64)
    assert a["branch"] == "string" and a["string"] == 40976 and a["dead"] == (1 + 2) * 8 + 1 * 64 * 2
    assert b["branch"] == "bits" and b["string"] == 336 and b["dead"] == (4800 + 2) * 8 + 40 * 512 * 2
    assert a["total"] == 40976 + 64 * 4 + 8192 * 4 and b["total"] == b["dead"] + 512 * 4 + 64 * 4
    for H, W in R.FUSED_MULTI + R.FUSED_SINGLE:
        assert R.frle_layout(H, W, 8192)["total"] <= 150 * 1024


def test_list_lengths_either_side_of_the_lds_copy():
    assert R.list_source(8192) == "lds" and R.list_source(8193) == "global" and 8193 < 96 * 96
    # nc = nt + 1 + lead on both sides of the 256-value chunks
    for nc in R.NC_EDGES:
        for lead in (0, 1):
            nt = nc - 1 - lead
            if nt < 0:
                continue
            m = R.mask_with_transitions(24, 24, nt, lead)
            assert len(R.runs_of(R.transitions(m), R.lead_of(m), 576)) == nc
    assert {nc % R.RLE_CHUNK for nc in R.NC_EDGES} >= {255, 0, 1}


def test_value_edge_case_holds_every_edge():
    runs = R.value_edge_runs()
    pos, lead, HW = R.list_from_runs(runs)
    assert lead == 1 and HW < R.FIVE_CHAR_PIXELS and R.runs_of(pos, lead, HW) == runs
    vals = R.stored_values(runs)
    assert set(R.VALUE_EDGES) <= set(vals[3:])
    want = {15: 1, 16: 2, -16: 1, -17: 2, 511: 2, 512: 3, -512: 2, -513: 3, 16383: 3, 16384: 4, -16384: 3, -16385: 4,
            524287: 4, 524288: 5, -524288: 4, -524289: 5}
    assert set(want) == set(R.VALUE_EDGES)
    for x, n in want.items():
        assert R.groups(x) == n and len(R.string_of_runs([x])) == n, x
    assert len(R.string_of_runs(runs)) == sum(R.groups(v) for v in vals)


def test_capacity_arithmetic_and_cases_have_a_string_on_either_side():
    nts = [3, 0, 700, 12, 5]
    assert R.place(nts, 8192) == [(0, 0, 0), (3, 1, 31), (3, 2, 47), (703, 3, 3563), (715, 4, 3639)]
    assert R.place(nts, 10) == [(0, 0, 0), (3, 1, 31), (3, 2, 47), (13, 3, 113), (23, 4, 179)]
    caps = R.packed_capacities(nts, 8192)
    assert caps == {"exact": 720, "minus1": 719, "inside": 709, "one": 1}
    for name, cap in caps.items():
        wr = [R.packed_written(off, nt, 8192, cap) for nt, (off, _, _) in zip(nts, R.place(nts, 8192))]
        fits = [R.list_fits(off, nt, 8192, cap) for nt, (off, _, _) in zip(nts, R.place(nts, 8192))]
        assert sum(wr) == min(cap, 720) and any(fits) == (name != "one")
        assert all(fits) == (name == "exact")
    # strings: out_capacity at the last needed byte and one below
    lists = [(np.arange(1, nt + 1), 0) for nt in nts]
    last = R.place(nts, 8192)[-1][2] + 5 * (nts[-1] + 1)
    for cap, n_bad in ((last, 0), (last - 1, 1)):
        lens, written = R.expected_strings(lists, 8192, 1000, 720, cap)
        assert sum(n < 0 for n in lens) == n_bad and len(written) == 5 - n_bad and lens[0] > 0


def test_the_17_run_list_is_97_characters_against_96_and_85():
    runs = R.big_runs(17)
    pos, lead, HW = R.list_from_runs(runs)
    nt, nc = len(pos), len(pos) + 1 + lead
    assert (HW, nt, nc, lead) == (150994970, 16, 17, 0) and HW >= R.FIVE_CHAR_PIXELS
    s = R.string_of_runs(runs)
    assert len(s) == 97 and 5 * nt + 16 == 96 and 5 * nc == 85
    assert not R.string_fits(0, nt, lead, len(s), HW, 85) and not R.string_fits(0, nt, lead, len(s), HW, 1 << 20)
    # the five runs A, A, 1, 1, A fit their slot
    runs = R.big_runs(5)
    pos, lead, HW = R.list_from_runs(runs)
    s = R.string_of_runs(runs)
    # (values A, A, 1, 1 - A, A - 1: the fifth is a delta against the third run, six characters like the fourth)
    assert (HW, len(pos), len(pos) + 1 + lead, len(s)) == (3 * R.BIG_A + 2, 4, 5, 25) and 5 * 4 + 16 == 36
    assert [R.groups(v) for v in R.stored_values(runs)] == [6, 6, 1, 6, 6]
    assert R.string_fits(0, 4, 0, 25, HW, 25) and not R.string_fits(0, 4, 0, 25, HW, 24)


@pytest.mark.parametrize("case", ("nc", "lds", "edges"))
def test_out_capacity_cases_have_a_string_on_either_side(case):
    """`out` at the last needed byte: every string fits; one below: exactly the last one does not."""
    if case == "edges":
        lists, HW = R.value_edge_case()
        max_runs = 64
    else:
        H, W, masks, orders, max_runs = R.nc_edge_case() if case == "nc" else R.lds_edge_case()
        lists, HW = R.kept_lists(masks, orders), H * W
    nts = [len(p) for p, _ in lists]
    assert max(nts) <= max_runs
    total, last = R.packed_total(nts, max_runs), R.last_needed(lists, max_runs)
    exact, _ = R.expected_strings(lists, max_runs, HW, total, last)
    below, written = R.expected_strings(lists, max_runs, HW, total, last - 1)
    assert min(exact) > 0 and below == exact[:-1] + [-1] and len(written) == len(lists) - 1
    if case == "nc":
        assert {nt + 1 + lead for (p, lead), nt in zip(lists, nts)} == set(R.NC_EDGES)


def test_over_max_runs_case_refuses_masks_in_the_middle():
    H, W, masks, orders, max_runs = R.over_max_runs_case()
    lists = R.kept_lists(masks, orders)
    nts = [len(p) for p, _ in lists]
    lens, _ = R.expected_strings(lists, max_runs, H * W, R.packed_total(nts, max_runs), R.last_needed(lists, max_runs))
    assert [n < 0 for n in lens] == [False, True, False, True, False, False, False, True, False]
    assert [x[0] for x in R.place(nts, max_runs)] == [0, 5, 305, 605, 905, 905, 922, 939, 1239]      # placed by min(nt, max_runs)


def test_big_cases_between_their_neighbours():
    lists, HW = R.big_case(17)
    assert [x[2] for x in R.place([len(p) for p, _ in lists], 64)] == [0, 26, 122]
    assert R.expected_strings(lists, 64, HW, 64, 26 + 85)[0] == [8, -1, -1] and R.expected_strings(lists, 64, HW, 64, 1024)[0] == [8, -1, 8]
    lists, HW = R.big_case(5)
    assert [R.expected_strings(lists, 64, HW, 64, cap)[0] for cap in (1024, 26 + 25, 26 + 24)] == [[8, 25, 8], [8, 25, -1], [8, -1, -1]]
