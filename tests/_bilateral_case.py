"""Edge cases of the bilateral solver and their float64 oracle results (oracle/bilateral_ref.py), shared by
tests/test_bilateral_edges_cpu.py (the conditions the cases must meet, on the oracle alone) and tests/test_bilateral_edges_gpu.py.

Every input is np.random.default_rng(0) or plain arithmetic.  oracle(name, kind) runs once per process and is cached; callers do not
modify what it returns.  Plain helper module (no fixtures, no pytest hooks)."""
import collections
import functools

import numpy as np

from oracle import bilateral_ref as B

DEFAULT = (16, 16, 8)                       # (sigma_spatial, sigma_luma, sigma_chroma) of the reference's bilateral_solver_output
CONFIDENCE, LAM, A_DIAG_MIN, CG_TOL, CG_MAXITER = 0.999, 256.0, 1e-5, 1e-5, 25
SPLAT_TAB = 320                             # bg_splat_final_kernel's table of repeated adds: larger counts take its loop
VGRID_VERTICES = 192 * 256                  # vertices the fixed grid of the vertex kernels covers without striding

Case = collections.namedtuple("Case", "name rgb target sigmas")
Ref = collections.namedtuple("Ref", "V its soft n m ratios grid bnorm")


def noise(h, w):
    return np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth(h, w):
    yy, xx = np.mgrid[:h, :w]
    return ((yy + xx)[..., None] * np.array([1.0, 0.6, 0.3])).astype(np.uint8)


def disk(h, w):
    """Centred in the image, radius min(H, W) / 3."""
    yy, xx = np.mgrid[:h, :w]
    return (((yy - h / 2.0) ** 2 + (xx - w / 2.0) ** 2) < (min(h, w) / 3.0) ** 2).astype(np.uint8)


CORNERS = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.int64)   # black ... white: the RGB cube's corners


def cube_corners(h, w):
    """Eight bands of w / 8 columns, one corner of the RGB cube each."""
    return np.broadcast_to(CORNERS[(np.arange(w) * 8) // w][None], (h, w, 3)).astype(np.uint8)


def corner_ramps(h, w):
    """Every corner of the cube, moved towards the cube's centre by 0, 12, 24 and 36 in all three channels and in each single channel
    (104 colours), every colour in every 16 x 16 spatial cell: colour cells on the lattice boundary that do have a neighbour, on the
    inner side only.  The diagonal steps alone give such neighbours on the luma axis only (black, white: the other corners change two
    lattice coordinates per step), and a picture of one colour per spatial cell couples nothing (the oracle then stops after at most
    one iteration whatever the target); the single-channel steps reach the chroma boundaries, the per-pixel mixing couples the cells."""
    cols = []
    for c in CORNERS:
        for mask in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            for s in (0, 12, 24, 36):
                d = s * np.array(mask)
                cols.append(np.where(c == 0, c + d, c - d))
    cols = np.unique(np.array(cols), axis=0)
    yy, xx = np.mgrid[:h, :w]
    return cols[((yy % 16) * 16 + (xx % 16)) % len(cols)].astype(np.uint8)


def half_plane(h, w):
    """y > x - w / 4: cuts every row band and every column band of corner_ramps."""
    yy, xx = np.mgrid[:h, :w]
    return (yy * w > (xx - w // 4) * h).astype(np.uint8)


def second_half(h, w):
    t = np.zeros((h, w), np.uint8)
    t.reshape(-1)[(h * w) // 2:] = 1
    return t


def _cases():
    c = []

    def add(name, rgb, target=None, sigmas=DEFAULT):
        h, w = rgb.shape[:2]
        c.append(Case(name, np.ascontiguousarray(rgb), disk(h, w) if target is None else target, sigmas))
    add("one_pixel", np.array([[[10, 20, 30]]], np.uint8), np.ones((1, 1), np.uint8))
    add("row", noise(1, 40), second_half(1, 40))
    add("column", noise(40, 1), second_half(40, 1))
    add("one_spatial_column", noise(17, 16))
    add("solid", np.full((33, 47, 3), 128, np.uint8))
    add("grey", np.repeat(noise(64, 80)[..., :1], 3, axis=2))
    add("cube_corners", cube_corners(48, 64))
    add("corner_ramps", corner_ramps(64, 64), half_plane(64, 64))
    add("many_vertices", noise(240, 256))
    for tag, sg in (("small", (8, 4, 4)), ("large", (24, 20, 12)), ("fractional", (12.5, 7.3, 5.1))):
        add(f"{tag}_noise", noise(96, 128), sigmas=sg)
        add(f"{tag}_smooth", smooth(96, 128), sigmas=sg)
    add("coarse_smooth", smooth(96, 128), sigmas=(24, 64, 32))
    return collections.OrderedDict((k.name, k) for k in c)


CASES = _cases()
NAMES = list(CASES)
# cases that are also solved with a non-binary u8 target and with a float64 target (the ordered splat)
ORDERED_SPLAT = ("many_vertices", "fractional_smooth")
KINDS = ("u8", "nonbinary", "f64")
# one batched call: every picture resampled to 64 x 80 by plain index arithmetic
BATCH_HW = (64, 80)
BATCH = ("cube_corners", "grey", "solid", "many_vertices", "empty")


def target_of(name, kind):
    """kind 'u8': the case's own binary target; 'nonbinary': u8 values 0 .. 255; 'f64': float64 values in [0, 0.7)."""
    k = CASES[name]
    h, w = k.target.shape
    if kind == "u8":
        return k.target
    r = np.random.default_rng(0)
    if kind == "nonbinary":
        return (k.target * r.integers(1, 256, (h, w))).astype(np.uint8)
    assert kind == "f64"
    return k.target * (0.1 + 0.6 * r.random((h, w)))


def dims(h, w, sigmas):
    """(Nx, Ny, Nl, Nu, Nv) as bg_dims (bilateral.hip) sizes the dense lattice."""
    ss, sl, sc = (float(s) for s in sigmas)
    nu = int(255.5 / sc) + 1
    return int((w - 1) / ss) + 1, int((h - 1) / ss) + 1, int(255.0 / sl) + 1, nu, nu


def pcg_trace(grid, target, n, m, lam=LAM, a_diag_min=A_DIAG_MIN, rtol=CG_TOL, maxiter=CG_MAXITER, confidence=CONFIDENCE):
    """The loop of oracle.bilateral_ref.solve / pcg restated with a record of ||r|| / atol at the top of every iteration, the quantity
    the stop test compares with 1.  Returns (iterations, [ratio at iteration 0, 1, ...], ||b||)."""
    conf = np.full(grid.npixels, confidence)
    w_splat = grid.splat(conf)
    b = grid.splat(target * conf)
    bn = float(np.linalg.norm(b))
    if bn == 0:
        return 0, [], bn

    def matvec(y):
        return lam * (m * y - n * grid.blur(n * y)) + w_splat * y
    minv = 1.0 / np.maximum(lam * (m - n * 10.0 * n) + w_splat, a_diag_min)
    x = b / w_splat
    r = b - matvec(x)
    atol = rtol * bn
    ratios, p, rho_prev = [], None, None
    for it in range(maxiter):
        ratios.append(float(np.linalg.norm(r)) / atol)
        if np.linalg.norm(r) < atol:
            return it, ratios, bn
        z = minv * r
        rho = np.dot(r, z)
        p = z.copy() if it == 0 else z + (rho / rho_prev) * p
        q = matvec(p)
        alpha = rho / np.dot(p, q)
        x += alpha * p
        r -= alpha * q
        rho_prev = rho
    return maxiter, ratios, bn


def _solve(rgb, target, sigmas):
    grid = B.Grid(rgb, *sigmas)
    t = target.reshape(-1).astype(np.float64)
    soft, its, n, m = B.solve(grid, t, np.full(t.size, CONFIDENCE), LAM, A_DIAG_MIN, CG_TOL, CG_MAXITER)
    its2, ratios, bn = pcg_trace(grid, t, n, m)
    assert its2 == its, (its2, its)
    return Ref(grid.nvertices, int(its), soft.reshape(target.shape), n, m, ratios, grid, bn)


@functools.lru_cache(maxsize=None)
def oracle(name, kind="u8"):
    k = CASES[name]
    return _solve(k.rgb, target_of(name, kind), k.sigmas)


def resample(a, hw):
    """Nearest-neighbour by index arithmetic (rows i * h // H): any picture or target at the batch test's size."""
    h, w = a.shape[:2]
    return np.ascontiguousarray(a[(np.arange(hw[0]) * h) // hw[0]][:, (np.arange(hw[1]) * w) // hw[1]])


@functools.lru_cache(maxsize=None)
def batch_item(name):
    """(rgb, target) of one image of the batched call; 'empty' is the noise picture with an all-zero target."""
    src = CASES["many_vertices" if name == "empty" else name]
    rgb = resample(src.rgb, BATCH_HW)
    target = np.zeros(BATCH_HW, np.uint8) if name == "empty" else disk(*BATCH_HW)
    return rgb, target


@functools.lru_cache(maxsize=None)
def batch_oracle(name):
    rgb, target = batch_item(name)
    return _solve(rgb, target, DEFAULT)


def largest_cell(ref):
    return int(np.bincount(ref.grid.pix2v).max())
