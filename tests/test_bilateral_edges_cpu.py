"""The cases of tests/_bilateral_case.py reach what tests/test_bilateral_edges_gpu.py relies on — checked on the float64 oracle alone
(oracle/bilateral_ref.py), never on the kernel: lattice-boundary colour cells, degenerate lattices, more vertices than the fixed
grid covers, spatial cells past the splat table, and a PCG residual that is nowhere near the stop threshold when the stop test runs
(so that equal iteration counts can be demanded of a differently rounded loop)."""
import numpy as np
import pytest
import torch

from oracle import bilateral_ref as B
from tests import _bilateral_case as K

SOLVES = [(n, k) for n in K.NAMES for k in (K.KINDS if n in K.ORDERED_SPLAT else ("u8",))]


@pytest.mark.parametrize("name", K.NAMES)
def test_coordinates_stay_below_the_reference_hash_base(name):
    """The reference hashes a vertex as sum c_d 255^d: coordinates of 255 or more alias (out of scope: the dense lattice does not)."""
    k = K.CASES[name]
    ref = K.oracle(name)
    assert ref.grid.coords.min() >= 0 and ref.grid.coords.max() < 255
    # and every coordinate lies inside the dense lattice as bg_dims sizes it
    assert (ref.grid.coords.max(0) < np.array(K.dims(*k.target.shape, k.sigmas))).all()


@pytest.mark.parametrize("name,kind", SOLVES)
def test_restated_loop_counts_what_solve_reports_and_stops_far_from_the_threshold(name, kind):
    ref = K.oracle(name, kind)
    k = K.CASES[name]
    t = K.target_of(name, kind).reshape(-1).astype(np.float64)
    its, ratios, bn = K.pcg_trace(ref.grid, t, ref.n, ref.m)
    soft, its_solve, _, _ = B.solve(ref.grid, t, np.full(t.size, K.CONFIDENCE))
    assert its == its_solve == ref.its and np.array_equal(soft.reshape(k.target.shape), ref.soft)
    assert bn > 0
    assert all(r >= 1.5 for r in ratios[:its]), ratios
    if its < K.CG_MAXITER:
        assert ratios[its] <= 0.67, ratios


@pytest.mark.parametrize("name", K.BATCH)
def test_batch_images_stop_far_from_the_threshold(name):
    ref = K.batch_oracle(name)
    rgb, target = K.batch_item(name)
    assert rgb.shape == K.BATCH_HW + (3,) and ref.grid.coords.max() < 255
    if name == "empty":
        assert not target.any() and ref.bnorm == 0 and ref.its == 0 and not ref.soft.any()
        return
    assert all(r >= 1.5 for r in ref.ratios[:ref.its]), ref.ratios
    if ref.its < K.CG_MAXITER:
        assert ref.ratios[ref.its] <= 0.67, ref.ratios
    if name == "cube_corners":
        uc = ref.grid.ucoords
        assert {0, 15} <= set(uc[:, 2]) and {0, 31} <= set(uc[:, 3]) and {0, 31} <= set(uc[:, 4])
    # different vertex counts share the launches
    assert len({K.batch_oracle(n).V for n in K.BATCH if n != "empty"}) == 4


def test_degenerate_lattices():
    one = K.oracle("one_pixel")
    assert one.V == 1 and (one.grid.nbr < 0).all() and one.its == 0
    for name, d in (("row", (3, 1)), ("column", (1, 3))):
        k, ref = K.CASES[name], K.oracle(name)
        assert K.dims(*k.target.shape, k.sigmas)[:2] == d
        assert ref.V == 40 and (ref.grid.nbr < 0).all()                    # every pixel a vertex of its own, none adjacent
        assert 0 < k.target.sum() < k.target.size
    k, ref = K.CASES["one_spatial_column"], K.oracle("one_spatial_column")
    assert K.dims(17, 16, k.sigmas)[:2] == (1, 2) and 256 < ref.V <= 272    # just past one block of 256 vertices
    k, ref = K.CASES["solid"], K.oracle("solid")
    assert ref.V == 9 and len({tuple(c) for c in ref.grid.ucoords[:, 2:]}) == 1 and K.largest_cell(ref) == 256
    ref = K.oracle("grey")
    assert (ref.grid.coords[:, 3:] == 16).all() and len(set(ref.grid.ucoords[:, 2])) == 16    # chroma degenerate, every luma cell


def test_corner_cases_occupy_every_boundary_colour_cell():
    for name in ("cube_corners", "corner_ramps"):
        k, ref = K.CASES[name], K.oracle(name)
        D = K.dims(*k.target.shape, k.sigmas)
        assert D[2:] == (16, 32, 32)
        uc, nbr = ref.grid.ucoords, ref.grid.nbr
        for d in (2, 3, 4):
            lo, hi = uc[:, d] == 0, uc[:, d] == D[d] - 1
            assert lo.any() and hi.any(), (name, d)
            assert (nbr[lo, d, 0] < 0).all() and (nbr[hi, d, 1] < 0).all()
            if name == "corner_ramps":                                         # a neighbour on the inner side only
                assert (nbr[lo, d, 1] >= 0).any() and (nbr[hi, d, 0] >= 0).any(), d
    assert K.oracle("corner_ramps").its >= 3
    # aliasing into the next row of the dense id — what an off-by-one bound in the neighbour test would read — finds an OCCUPIED cell:
    # for a vertex at coordinate dims[d] - 1, id + stride_d is the cell (0, c_{d+1} + 1) of the same other coordinates.  (Not so in
    # cube_corners: a band's colour exists in no other spatial column.)
    for name in ("corner_ramps", "many_vertices"):
        k, ref = K.CASES[name], K.oracle(name)
        D = np.array(K.dims(*k.target.shape, k.sigmas), np.int64)
        stride = np.concatenate([[1], np.cumprod(D)[:-1]])
        ids = ref.grid.ucoords.astype(np.int64) @ stride
        occupied = set(ids.tolist())
        hits = sum(int(i + stride[d]) in occupied for d in range(5) for i in ids[ref.grid.ucoords[:, d] == D[d] - 1])
        assert hits > 0, name


def test_many_vertices_pass_the_fixed_grid():
    k, ref = K.CASES["many_vertices"], K.oracle("many_vertices")
    assert ref.V > K.VGRID_VERTICES == 49152
    D = K.dims(*k.target.shape, k.sigmas)
    assert -(-int(np.prod(D)) // 64) > 1024                                   # bitmap words: more than one scan block


def test_sigma_cases_reach_the_splat_fallback_and_the_fractional_window():
    assert K.dims(96, 128, (8, 4, 4))[2:] == (64, 64, 64)
    for name in ("large_smooth", "coarse_smooth"):
        assert K.largest_cell(K.oracle(name)) > K.SPLAT_TAB, name
    assert K.largest_cell(K.oracle("coarse_smooth")) == 576                   # whole 24 x 24 cells: both splats take the loop
    for name in K.NAMES:
        if K.CASES[name].sigmas == K.DEFAULT:
            assert K.largest_cell(K.oracle(name)) <= 256
    ss = K.CASES["fractional_smooth"].sigmas[0]
    assert ss != int(ss)
    for kind in ("nonbinary", "f64"):
        for name in K.ORDERED_SPLAT:
            t = K.target_of(name, kind)
            assert len(np.unique(t)) > 2 and t.dtype == (np.uint8 if kind == "nonbinary" else np.float64)


def test_lattice_dimensions_hold_the_largest_colour_without_the_clamp():
    """bg_cells_kernel clamps (l, u, v) to the lattice bg_dims sized.  Y is a sum of products with positive weights, rounded monotonically,
    so white has the largest luma, and U / V peak at blue / red: at most 255 (255 or the double below it, depending on how the sum is
    contracted), and 255.5, 255.5 exactly.  The sizes are int(255 / sl) + 1 and int(255.5 / sc) + 1 and IEEE division is monotone, so no
    sigma makes the clamp change a cell; the 255 / k candidates (where 255 / sigma rounds next to an integer) are run through the
    oracle's own binning here, and the 2^24-colour sweeps of the GPU test assert the same on every colour."""
    ext = np.array([[[255, 255, 255], [0, 0, 255], [255, 0, 0]]], np.uint8)
    yuv = np.tensordot(ext, B.RGB_TO_YUV, ([2], [1])) + B.YUV_OFFSET.reshape(1, 1, -1)
    assert np.nextafter(255.0, 0) <= yuv[0, 0, 0] <= 255.0 and yuv[0, 1, 1] == 255.5 and yuv[0, 2, 2] == 255.5
    sig = [255.0 / k for k in range(1, 65)] + [255.5 / k for k in range(1, 65)] + [16, 8, 4, 24, 20, 12, 12.5, 7.3, 5.1, 64, 32]
    for s in sig:
        c = B.grid_coords(ext, 16, s, s).reshape(3, 5)
        _, _, nl, nu, nv = K.dims(1, 3, (16, s, s))
        assert c[0, 2] <= nl - 1 and c[1, 3] <= nu - 1 and c[2, 4] <= nv - 1, s


def test_refusal_sizes():
    """65 x 65 at sigmas (16, 0.5, 0.5) has 2^31 cells or more; 64 x 64 has 511 * 2^22, just below (4 * 4 * 511 * 512 * 512)."""
    assert int(np.prod(K.dims(65, 65, (16, 0.5, 0.5)), dtype=np.int64)) >= 2 ** 31
    assert int(np.prod(K.dims(64, 64, (16, 0.5, 0.5)), dtype=np.int64)) == 511 * 2 ** 22 < 2 ** 31


def test_caller_buffers_are_validated_before_anything_is_launched():
    from zutis_amd import _lib, ops
    ok = torch.zeros(12, dtype=torch.float64)
    assert ops._caller_buffer(ok, torch.float64, (2, 2, 3), "out").shape == (2, 2, 3)
    assert ops._caller_buffer(ok, torch.float64, (2, 2, 3), "out").data_ptr() == ok.data_ptr()
    for bad in (torch.zeros(11, dtype=torch.float64), torch.zeros(12, dtype=torch.float32), torch.zeros(24, dtype=torch.float64)[::2]):
        with pytest.raises(_lib.ZutisHipError):
            ops._caller_buffer(bad, torch.float64, (2, 2, 3), "out")
