"""-m gpu: the bilateral solver (zutis_amd/csrc/bilateral.hip) at lattice, size and workspace edges against the float64 NumPy/SciPy
oracle (oracle/bilateral_ref.py), and its glue kernels (lattice coordinates, threshold, de-normalise) against theirs.

The cases are tests/_bilateral_case.py's; tests/test_bilateral_edges_cpu.py asserts on the oracle alone that they reach what is claimed
for them (boundary colour cells, Nx = 1 / Ny = 1 / V = 1, V > 49 152, spatial cells past the 320-entry splat table, a residual at
least 1.5x above the stop threshold before the stop and at most 0.67x at it — which is why EQUAL iteration counts are demanded here).

Every solve runs with its workspace (exactly B * zh_bilateral_workspace_size bytes), soft output, stats and debug outputs inside one
0xA5-filled arena and its picture and target inside a 0xFF-filled one (tests/_guard.py); the workspace is pre-filled with 0xFF, 0xA5
and 0x00 in turn and the three runs must agree bit for bit — a word read before it is written shows there, a fresh torch.empty is
nearly always zeros.

Bounds.  stats: exact.  soft: 1e-9 * max(1, max |ref|), the bound of test_bilateral_gpu.py; `> 0.5` equal wherever |ref - 0.5| > 1e-9.
n / m at the default sigmas: 1e-13 / 1e-11 (test_solver_vs_reference_golden).  At other sigmas no bound existed; measured on one MI355X
against the oracle, max |err| over each case (V, largest m of the case):
    (8, 4, 4)          noise 0 / 0 (12 285, 2)     smooth 0 / 0 (867, 43)
    (24, 20, 12)       noise 0 / 0 (10 340, 4)     smooth 0 / 0 (95, 446)
    (12.5, 7.3, 5.1)   noise 0 / 0 (12 232, 2)     smooth 0 / 0 (435, 105), also with the non-binary u8 and the float64 target
    (24, 64, 32)                                   smooth 0 / 0 (47, 576)
Every n and every m is the oracle's double (so are they at the default sigmas, 1x1 to 240x256): the counts are integers, sqrt and the
division are IEEE, the blur is summed in the oracle's order and nothing is contracted.  8x the largest measured error, 0, is 0: the
bound at other sigmas is equality, which is what the design claims for the grid quantities and is below the 1e-9 of the soft output.
The soft output's own largest error in this file was 4.4e-14 for binary targets (3.2e-12 at a target of up to 255, bound 2.6e-7).
"""
import numpy as np
import pytest
import torch

from oracle import bilateral_ref as B
from tests import _bilateral_case as K
from tests._guard import IN_FILL, OUT_FILL, Arena, assert_equal, assert_untouched

pytestmark = pytest.mark.gpu

SOLVES = [(n, k) for n in K.NAMES for k in (K.KINDS if n in K.ORDERED_SPLAT else ("u8",))]
FILLS = (0xFF, 0xA5, 0x00)
N_BOUND_DEFAULT, M_BOUND_DEFAULT = 1e-13, 1e-11
N_BOUND_OTHER, M_BOUND_OTHER = 0.0, 0.0                  # measured 0 (module docstring): bit-identical to the oracle
SOFT_REL = 1e-9

_runs = {}


def _solve_guarded(dev, rgb, target, sigmas, fill):
    """One call of ops.bilateral_solve on [B,H,W,3] / [B,H,W] arrays with everything between guards.  Returns CPU arrays
    {out [B,H,W], stats [B,2], n, m [B,H*W]} after both arenas passed assert_untouched."""
    from zutis_amd import ops
    Bn, H, W, _ = rgb.shape
    a_in, a_out = Arena(IN_FILL, dev), Arena(OUT_FILL, dev)
    v_rgb = a_in.add("rgb", torch.uint8, Bn * H, W * 3, tail_rows=1)
    v_t = a_in.add("target", torch.from_numpy(target).dtype, Bn * H, W, tail_rows=1)
    need = Bn * ops.bilateral_workspace_size(H, W, *sigmas)
    v_ws = a_out.workspace("workspace", need)
    v_out = a_out.add("out", torch.float64, Bn * H, W, tail_rows=1)
    v_st = a_out.add("stats", torch.int32, Bn, 2, tail_rows=1)
    v_n = a_out.add("n", torch.float64, Bn, H * W, tail_rows=1)
    v_m = a_out.add("m", torch.float64, Bn, H * W, tail_rows=1)
    v_rgb.put(torch.from_numpy(rgb))
    v_t.put(torch.from_numpy(target))
    v_ws.m2.fill_(fill)
    r = v_rgb.m2.view(Bn, H, W, 3)
    t = v_t.m2.view(Bn, H, W)
    before = (r.clone(), t.clone())
    ops.bilateral_solve(r, t, *sigmas, confidence=K.CONFIDENCE, lam=K.LAM, a_diag_min=K.A_DIAG_MIN, cg_tol=K.CG_TOL, cg_maxiter=K.CG_MAXITER,
                        debug=(v_n.m2, v_m.m2), workspace=v_ws.m2.view(-1), out=v_out.m2, stats=v_st.m2)
    torch.cuda.synchronize()
    assert_untouched(a_out)
    assert_untouched(a_in)
    assert torch.equal(before[0], r) and torch.equal(before[1], t)
    return {"out": v_out.m2.view(Bn, H, W).cpu().numpy(), "stats": v_st.m2.cpu().numpy(), "n": v_n.m2.cpu().numpy(), "m": v_m.m2.cpu().numpy()}


def _run(dev, name, kind, fill):
    key = (name, kind, fill)
    if key not in _runs:
        k = K.CASES[name]
        _runs[key] = _solve_guarded(dev, k.rgb[None], K.target_of(name, kind)[None], k.sigmas, fill)
    return _runs[key]


def _check_against(got, i, ref, default_sigmas, what):
    """Image i of a guarded run against its oracle result: stats exact, soft and mask, n and m."""
    V, its = (int(v) for v in got["stats"][i])
    assert (V, its) == (ref.V, ref.its), (what, V, its, ref.V, ref.its)
    soft = got["out"][i]
    assert np.isfinite(soft).all(), what
    err = float(np.abs(soft - ref.soft).max())
    bound = SOFT_REL * max(1.0, float(np.abs(ref.soft).max()))
    en, em = float(np.abs(got["n"][i, :V] - ref.n).max()), float(np.abs(got["m"][i, :V] - ref.m).max())
    print(f"{what}: V {V}, {its} it, soft err {err:.3e} (bound {bound:.1e}), n err {en:.3e}, m err {em:.3e}, max m {float(ref.m.max()):.4g}")
    assert err <= bound, (what, err, bound)
    clear = np.abs(ref.soft - 0.5) > 1e-9
    assert np.array_equal((soft > 0.5)[clear], (ref.soft > 0.5)[clear]), what
    nb, mb = (N_BOUND_DEFAULT, M_BOUND_DEFAULT) if default_sigmas else (N_BOUND_OTHER, M_BOUND_OTHER)
    assert en <= nb and em <= mb, (what, en, nb, em, mb)
    # the debug rows past V are not written
    assert (got["n"][i, V:].view(np.uint8) == OUT_FILL).all() and (got["m"][i, V:].view(np.uint8) == OUT_FILL).all(), what


@pytest.mark.parametrize("name,kind", SOLVES)
def test_solve_vs_oracle_between_guards(dev, name, kind):
    """stats exact, soft within the project's bound, the > 0.5 mask, n and m; nothing outside the logical outputs or the exactly sized
    workspace is written, picture and target are left alone (asserted inside the guarded run)."""
    _check_against(_run(dev, name, kind, FILLS[0]), 0, K.oracle(name, kind), K.CASES[name].sigmas == K.DEFAULT, f"{name}/{kind}")


@pytest.mark.parametrize("name,kind", SOLVES)
def test_dirty_workspace_is_never_read_before_it_is_written(dev, name, kind):
    """0xFF (NaN / -1), 0xA5 and 0x00 in every byte of the workspace before the call: bitwise equal out, stats, n and m."""
    first = _run(dev, name, kind, FILLS[0])
    for fill in FILLS[1:]:
        other = _run(dev, name, kind, fill)
        for key in ("out", "stats", "n", "m"):
            a, b = first[key], other[key]
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, kind, key, hex(fill))


def test_batch_between_guards_equals_single_solves_in_both_orders(dev):
    """One batched call over pictures of very different lattices (and an empty target), per-image workspace slices between guards: every
    image bitwise equal to its own single solve and within the bounds of the oracle; in two orders, so that a slice overrun into the
    next image's slice would show in a different neighbour."""
    singles = {}
    for name in K.BATCH:
        rgb, target = K.batch_item(name)
        singles[name] = _solve_guarded(dev, rgb[None], target[None], K.DEFAULT, 0xFF)
        _check_against(singles[name], 0, K.batch_oracle(name), True, f"batch item {name}")
    assert int(singles["empty"]["stats"][0, 1]) == 0 and not singles["empty"]["out"].view(np.uint8).any()   # exactly +0.0, 0 iterations
    for order in (list(K.BATCH), [K.BATCH[i] for i in (3, 0, 4, 2, 1)]):
        rgb = np.stack([K.batch_item(n)[0] for n in order])
        target = np.stack([K.batch_item(n)[1] for n in order])
        for fill in (0xFF, 0x00):
            got = _solve_guarded(dev, rgb, target, K.DEFAULT, fill)
            for i, name in enumerate(order):
                V = int(singles[name]["stats"][0, 0])
                assert np.array_equal(got["stats"][i], singles[name]["stats"][0]), (order, name)
                assert np.array_equal(got["out"][i].view(np.uint8), singles[name]["out"][0].view(np.uint8)), (order, name)
                for key in ("n", "m"):
                    assert np.array_equal(got[key][i, :V].view(np.uint8), singles[name][key][0, :V].view(np.uint8)), (order, name, key)
                    assert (got[key][i, V:].view(np.uint8) == OUT_FILL).all(), (order, name, key)


def _raw_solve(lib, rgb, target, H, W, sigmas, out, stats, ws, ws_bytes):
    from zutis_amd import ops
    return lib.zh_bilateral_solve_batch(rgb.data_ptr(), target.data_ptr(), None, 1, H, W, float(sigmas[0]), float(sigmas[1]), float(sigmas[2]),
                                        K.CONFIDENCE, K.LAM, K.A_DIAG_MIN, K.CG_TOL, K.CG_MAXITER, out.data_ptr(), stats.data_ptr(), None, None,
                                        ws.data_ptr(), ws_bytes, ops._stream())


def test_refusals_launch_nothing(dev):
    """Host-side checks: a workspace one byte short is ZH_ERR_WORKSPACE (-3), a lattice of 2^31 cells or more is refused by name; in both
    cases not a byte of output or workspace changes."""
    from zutis_amd import _lib, ops
    lib = _lib.load(raw=True)
    H, W = 33, 47
    need = ops.bilateral_workspace_size(H, W, *K.DEFAULT)
    a = Arena(OUT_FILL, dev)
    v_ws = a.workspace("workspace", need - 1)
    v_out = a.add("out", torch.float64, H, W, tail_rows=1)
    v_st = a.add("stats", torch.int32, 1, 2, tail_rows=1)
    rgb = torch.full((H, W, 3), 128, dtype=torch.uint8, device=dev)
    target = torch.ones((H, W), dtype=torch.uint8, device=dev)
    rc = _raw_solve(lib, rgb, target, H, W, K.DEFAULT, v_out.m2, v_st.m2, v_ws.m2, need - 1)
    assert rc == -3 and "workspace too small" in lib.zh_last_error().decode()
    with pytest.raises(_lib.ZutisHipError, match="workspace"):
        ops.bilateral_solve(rgb, target, workspace=v_ws.m2.view(-1), out=v_out.m2, stats=v_st.m2)
    with pytest.raises(_lib.ZutisHipError):                                       # a caller's output of the wrong size
        ops.bilateral_solve(rgb, target, out=v_out.m2.view(-1)[:-1])
    # sigmas (16, 0.5, 0.5): 65 x 65 is 5 * 5 * 511 * 512 * 512 >= 2^31 cells and refused whatever the workspace; 64 x 64 is
    # 511 * 2^22 cells, the largest such lattice below 2^31: it passes that check and is stopped by the workspace check alone
    sg = (16, 0.5, 0.5)
    rgb = torch.zeros((65, 65, 3), dtype=torch.uint8, device=dev)
    target = torch.ones((65, 65), dtype=torch.uint8, device=dev)
    rc = _raw_solve(lib, rgb, target, 65, 65, sg, v_out.m2, v_st.m2, v_ws.m2, need - 1)
    assert rc == -1 and "lattice too large" in lib.zh_last_error().decode()
    rc = _raw_solve(lib, rgb, target, 64, 64, sg, v_out.m2, v_st.m2, v_ws.m2, need - 1)
    assert rc == -3 and "workspace too small" in lib.zh_last_error().decode()
    torch.cuda.synchronize()
    assert_untouched(a, views=[])


# ---------------------------------------------------------------------------------------------------------------- glue kernels
_all_colours = {}


def _colours():
    if "rgb" not in _all_colours:
        r, g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
        _all_colours["rgb"] = np.stack([r, g, b], -1).reshape(4096, 4096, 3)
    return _all_colours["rgb"]


@pytest.mark.parametrize("sigmas", [(8, 4, 4), (24, 20, 12), (12.5, 7.3, 5.1)])
def test_lattice_coordinates_of_all_colours_at_other_sigmas(dev, sigmas):
    """All 2^24 colours as a 4096 x 4096 picture (so x / ss and y / ss run over 4096 positions, fractional ss included): exact.  And on
    the oracle: no colour reaches past the lattice bg_dims sizes, so bg_cells_kernel's clamp changes no cell at these sigmas."""
    from zutis_amd import ops
    rgb = _colours()
    got = ops.bgrid_coords(torch.from_numpy(rgb).to(dev), *sigmas).cpu().numpy()
    ref = B.grid_coords(rgb, *sigmas)
    assert np.array_equal(got, ref)
    nx, ny, nl, nu, nv = K.dims(4096, 4096, sigmas)
    mx = ref.max(0)
    assert ref.min() >= 0 and mx[0] == nx - 1 and mx[1] == ny - 1 and mx[2] <= nl - 1 and mx[3] <= nu - 1 and mx[4] <= nv - 1, (mx, nl, nu)


@pytest.mark.parametrize("thr", [0.5, -0.25, 0.0])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_threshold_f64_at_the_threshold_and_specials(dev, n, thr):
    from zutis_amd import ops
    special = np.array([thr, np.nextafter(thr, np.inf), np.nextafter(thr, -np.inf), 0.0, -0.0, np.inf, -np.inf, np.nan,
                        5e-324, -5e-324, 1.0, 0.5], np.float64)
    x = np.random.default_rng(0).normal(thr, 1.0, n)
    idx = np.arange(n)
    sel = idx % 3 != 2 if n > 1 else idx == 0                                      # two specials, one random value, ...; first and last are specials
    x[sel] = special[(idx[sel] * 7 + (n % 5)) % len(special)]
    x[-1] = np.nextafter(thr, np.inf)
    if n > 1:
        x[0] = thr
    with np.errstate(invalid="ignore"):
        ref = (x > thr).astype(np.uint8)                                           # NaN > thr is False: 0
    a = Arena(OUT_FILL, dev)
    v = a.add("mask", torch.uint8, 1, n, tail_rows=1)
    ops.threshold_f64_u8(torch.from_numpy(x).to(dev), thr, out=v.m2)
    torch.cuda.synchronize()
    assert_untouched(a)
    assert_equal(v.m2, torch.from_numpy(ref)[None], f"threshold n={n} thr={thr}")
    assert ref[-1] == 1 and (n == 1 or ref[0] == 0)


def _denorm_pre(x, mean, std):
    """The fp32 value the truncation sees, (x * std + mean) * 255, per channel (x [3, n])."""
    y = x.astype(np.float32) * np.asarray(std, np.float32)[:, None] + np.asarray(mean, np.float32)[:, None]
    return y * np.float32(255)


def _run_denorm(dev, x, mean, std):
    from zutis_amd import ops
    _, H, W = x.shape
    a = Arena(OUT_FILL, dev)
    v = a.add("rgb", torch.uint8, H, W * 3, tail_rows=1)
    ops.denormalize_u8(torch.from_numpy(x).to(dev), mean, std, out=v.m2)
    torch.cuda.synchronize()
    assert_untouched(a)
    assert_equal(v.m2.view(H, W, 3), torch.from_numpy(B.denormalize_to_u8(x, mean, std)), f"denormalize {H}x{W}")


@pytest.mark.parametrize("mean,std", [((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), ((0.5, 0.25, 0.4), (0.5, 0.3, 0.2))])
def test_denormalize_at_every_byte_edge(dev, mean, std):
    """Truncation decides at the integers.  For every channel and byte value b: 129 fp32 inputs around ((b / 255) - mean) / std, a
    quarter of an ulp of the sum x * std + mean apart (finer than fp32 resolves either the product or the sum, so the window holds the
    last input whose (x * std + mean) * 255 is below b and the first at or above it: the deciding inputs).  Asserted on the inputs
    themselves: for every b in 1 .. 255 both sides are present, and some inputs land on b exactly."""
    W = 129
    x = np.empty((3, 256, W), np.float32)
    for c in range(3):
        y = np.arange(256) / 255.0
        ulp = np.spacing(np.maximum(np.maximum(y, mean[c]), 1 / 255.0).astype(np.float32)).astype(np.float64)
        x[c] = ((y - mean[c]) / std[c])[:, None] + (np.arange(W) - W // 2)[None, :] * (ulp / std[c] / 4)[:, None]
    pre = _denorm_pre(x.reshape(3, -1), mean, std).reshape(3, 256, W)
    b = np.arange(256, dtype=np.float32)[None, :, None]
    assert (pre < b)[:, 1:].any(-1).all() and (pre >= b)[:, 1:].any(-1).all()
    assert (np.diff(pre, axis=-1) >= 0).all()
    hits = (pre == b).any(-1)
    print(f"denormalize edges: {int(hits.sum())} of {hits.size} (channel, byte) pairs have an input landing exactly on the byte")
    assert hits.sum() >= hits.size // 4
    _run_denorm(dev, x, mean, std)


@pytest.mark.parametrize("hw", [(1, 1), (5, 51), (257, 1)])
def test_denormalize_far_values_and_infinities(dev, hw):
    """Far below 0 and far above 1, +-inf (clipped to 0 / 255), at H*W = 1, 255 and 257 with a non-default mean / std."""
    # NaN is left out: NumPy's float -> uint8 cast of NaN is undefined.  The kernel gives 0 (fmaxf(NaN, 0) = 0).
    H, W = hw
    mean, std = (0.5, 0.25, 0.4), (0.5, 0.3, 0.2)
    special = np.array([-np.inf, np.inf, -1e30, 1e30, -3.0, 7.0, 0.0, 1.0, -1e-30, 3.4e38, -3.4e38], np.float32)
    x = np.random.default_rng(0).normal(0, 1.5, (3, H * W)).astype(np.float32)
    i = np.arange(H * W)
    for c in range(3):
        sel = (i + c) % 2 == 0
        x[c, sel] = special[(i[sel] // 2 + 3 * c) % len(special)]
    out = B.denormalize_to_u8(x.reshape(3, H, W), mean, std)
    assert H * W == 1 or (out.min() == 0 and out.max() == 255)
    _run_denorm(dev, x.reshape(3, H, W), mean, std)
