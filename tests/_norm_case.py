"""LayerNorm-family inputs by construction, their float64 references, the tolerances and float32 restatements of the kernels of
zutis_amd/csrc/norm.hip (tests/test_norm_structured_gpu.py runs the cases through the kernels, tests/test_norm_structured_cpu.py checks
the cases themselves: that they have the structure they claim, that a float32 restatement of each kernel stays under half of the tolerance,
and that wrong restatements do not).

Every other test of these kernels feeds randn * s + c with |c| <= 1: mean / std is about 0.3 and all chunks of an image have the same
mean.  The cases here are rows with a common offset (mean / std up to 1e4), rows with a few outlier channels, constant / zero / tiny /
large rows, rows on the fp16 grid, and images whose 4096-float chunks differ in mean by 70 — the data on which a one-pass variance, a
mean taken after a rounding, a masked tail lane that leaks, an unweighted combine of the chunk partials or a lost between-chunk term of
the variance show.  Plain helper module: no fixtures, no pytest hooks, no GPU and no library.

Tolerances (derived, not tuned; nothing here comes from what a kernel returned)
------------------------------------------------------------------------------
A row output keeps the project's flat tolerance for that output (test_layout_guard_norm_gpu.py: 2e-5 + 1e-5 |ref| for fp32 outputs and split
pairs, 4e-3 + 2e-3 |ref| for plain fp16, 6e-3 + 2e-3 |ref| for the *_plus fp16 output, 4e-5 for the chained LayerNorm) plus a
conditioning term

    12 * 2^-24 * cond_row * |gamma_i|,      cond_row = mean|x| / sqrt(var + eps)   (float64, from the operands as the kernel reads them).

Derivation.  y_i = (x_i - mean) * rstd * gamma_i + beta_i.  x_i - mean is exact or one rounding of a small number; what a badly conditioned
row adds is the error of `mean` itself, which shifts every element by delta_mean / sqrt(var + eps) * gamma_i.  An element passes through at
most 12 fp32 roundings on its way into the mean: 2 inside its float4 ((a + b) + (c + d)), up to 3 across the lane's float4s (LN_MAXV = 4:
s += ...), 6 levels of the wave's shuffle tree, 1 division by D.  Every partial sum of k elements is at most k * max|x| in size and is
divided by D in the end, so each rounding moves the mean by at most 2^-24 * mean|x| (to first order, for rows whose elements share a sign
or whose |x| is level — the offset and constant rows this term exists for; on the other rows cond_row < 2 and the term is below 1.5e-6).
Hence |delta_mean| / sigma_eff <= 12 * 2^-24 * cond_row.  The same shift enters the variance as delta_mean^2: second order.  For a
constant row c the float64 result is exactly beta, cond_row = |c| / sqrt(eps), and the term bounds the noise (c - mean_fp32) * rsqrt(eps).

Chained LayerNorm z = LN(y; gamma2, beta2, eps2) of zh_sum_layernorm_f32: the term above built from y, plus the first stage's own
tolerance carried through the second normalisation: tol1_i / sqrt(var(y) + eps2) * |gamma2_i|.

zh_global_ln_l2 keeps 2e-6 + 1e-5 |ref| (fp32, pair) and 1e-3 + 1e-5 |ref| (plain fp16) plus 12 * 2^-24 * cond_image / sqrt(C): the image mean is
built by the same kind of tree (per 4096-float chunk in fp32, the chunks in fp64, one rounding to fp32), its error shifts every channel
of a pixel by delta / sigma, and the L2 normalisation divides by a norm of about sqrt(C).

Restatements
------------
ln_rows_f32 / gln_f32 / l2_rows_f32 do in NumPy float32 what the comments of norm.hip say the kernels do, in the kernels' order of
operations (the float4 pair sums, the lane's float4s, the shuffle tree; per-chunk (n, mean, M2) in fp32, weighted fp64 combine, float(mean),
fp32 apply).  They are not bit-exact twins: the compiler contracts a * a + b into an fma.  `wrong=` selects a deliberately broken variant.
"""
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

f16, f32, f64 = torch.float16, torch.float32, torch.float64
U = 2.0 ** -24                                   # fp32 unit roundoff
N_ROUNDINGS = 12                                 # 2 (float4) + 3 (lane's float4s) + 6 (shuffle levels) + 1 (division)
LN_MAXV, GLN_CHUNK = 4, 4096                     # norm.hip: float4 per lane; floats per partial block
ROW_DIMS = (8, 192, 516, 1024)
OFFSETS = ((1e2, 1.0), (1e3, 1.0), (1e4, 1.0), (3e4, 30.0), (1.0, 1e-3))
CONSTANTS = (0.0, 1.0, 3.3, 1000.1, -0.007)
OUTLIERS = (300.0, -180.0)
ROW_FAMILIES = ("offset", "outlier", "constant", "tiny", "large", "mixed")
IMAGE_SHAPES = ((2, 37, 516), (1, 257, 1024), (3, 1, 8))
IMAGE_FAMILIES = ("step", "offset", "per_image", "constant")
IMAGE_CONSTANTS = (0.0, 0.75, 3.0)               # short mantissas: every partial sum is exact, the float64 result (0) is the kernel's
IMAGE_EPS = ((1e-5, 1e-7), (1e-5, 1.0))          # the engine's setting; the variance-observable one (rstd does not cancel)
L2_FAMILIES = ("dominant", "scaled", "zero")
# the project's flat tolerances (atol, rtol) per output
TOL_F32, TOL_F16, TOL_F16_PLUS, TOL_CHAIN = (2e-5, 1e-5), (4e-3, 2e-3), (6e-3, 2e-3), (4e-5, 0.0)
TOL_SUM_F32 = (2e-5, 0.0)                        # zh_sum_layernorm_f32's first LayerNorm (test_sum_layernorm)
TOL_IMG_F32, TOL_IMG_F16 = (2e-6, 1e-5), (1e-3, 1e-5)
TOL_L2_F32, TOL_L2_F16 = (1e-6, 1e-5), (1e-3, 1e-5)


def randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def dim_for(D, in_f16):
    """The fp16-input form needs D % 8 == 0: 520 stands in for 516."""
    return 520 if in_f16 and D == 516 else D


def as_seen(x, in_f16):
    """x as the kernel reads it, in float32: itself, or rounded to fp16."""
    return x.to(f16).float() if in_f16 else x.to(f32)


@dataclass
class RowCase:
    family: str
    name: str
    D: int
    x: torch.Tensor                              # [rows, D] float32, as the kernel sees it (on the fp16 grid when in_f16)
    in_f16: bool = False
    eps: float = 1e-5
    desc: dict = field(default_factory=dict)

    @property
    def rows(self):
        return self.x.shape[0]


def affine(D, seed=0):
    """gamma, beta as the layout tests draw them: 1 + 0.1 randn, 0.1 randn."""
    return randn((D,), 32 + seed) * 0.1 + 1, randn((D,), 33 + seed) * 0.1


def _outlier_row(D, seed, first, last):
    """randn with OUTLIERS[0] at column `first` of the first float4 of lane 0 and / or OUTLIERS[1] at column D - 4 + `last` of the last
    valid float4 (None: left out)."""
    r = randn((D,), seed)
    if first is not None:
        r[first] = OUTLIERS[0]
    if last is not None:
        r[D - 4 + last] = OUTLIERS[1]
    return r


def row_cases(family, D, in_f16=False):
    """The cases of one row family at width D (dim_for() applied), rows in {5, 6, 7}."""
    D = dim_for(D, in_f16)
    mk = lambda name, x, **desc: RowCase(family, f"{family}/{name} D={D}" + (" f16-in" if in_f16 else ""), D, as_seen(x, in_f16), in_f16, 1e-5, desc)
    if family == "offset":
        out = []
        for i, (c, sigma) in enumerate(OFFSETS):
            sign = torch.tensor([1.0, -1.0, 1.0, -1.0, 1.0, -1.0])[:, None]
            z = randn((6, D), 100 + i + D).double()
            z = (z - z.mean(-1, keepdim=True)) / z.std(-1, unbiased=False, keepdim=True)     # sample std 1: |c| / sigma holds at D = 8 too
            # ... but not std = sigma and mean = c EXACTLY: E[x^2] = c^2 + sigma^2 would then be an fp32 number and a one-pass variance exact
            jitter = 0.0137 * sigma * torch.arange(1, 7, dtype=f64)[:, None]
            out.append(mk(f"c={c:g} sigma={sigma:g}", (z * (0.97 * sigma) + sign.double() * c + jitter).float(), c=c, sigma=sigma))
        return out
    if family == "outlier":
        rows = [_outlier_row(D, 200 + D, 0, 3), _outlier_row(D, 201 + D, 3, 0), _outlier_row(D, 202 + D, 1, None),
                _outlier_row(D, 203 + D, None, 2), _outlier_row(D, 204 + D, 2, 1)]
        rows[4] = -rows[4]                       # -300 in front, +180 at the end
        return [mk("first and last float4", torch.stack(rows), first=(0, 3, 1, None, 2), last=(3, 0, None, 2, 1))]
    if family == "constant":
        return [mk("one c per row", torch.tensor(CONSTANTS)[:, None].expand(len(CONSTANTS), D).clone(), c=CONSTANTS)]
    if family == "tiny":
        return [mk("randn * 1e-30", randn((5, D), 300 + D, 1e-30))]
    if family == "large":
        return [mk("randn * 1e4", randn((7, D), 301 + D, 1e4).clamp(-6e4, 6e4))]
    if family == "mixed":
        rows = [randn((D,), 400 + D) + 1e3, randn((D,), 401 + D) - 1e4, _outlier_row(D, 402 + D, 0, 3), torch.full((D,), 1000.1),
                randn((D,), 403 + D, 1e-30), randn((D,), 404 + D, 1e4), torch.zeros(D)]
        return [mk("one row of each", torch.stack(rows))]
    if family == "fp16_grid":
        assert in_f16, "fp16_grid exists for the fp16-input form only"
        big = randn((2, D), 502 + D)
        big[0, 1], big[0, D - 2], big[1, 2], big[1, D - 3] = 3e4, -3e4, -3e4, 3e4
        x = torch.cat([randn((2, D), 500 + D) + 1000, randn((2, D), 501 + D, 1e-4), big])
        return [mk("spacing 0.5, subnormals, +-3e4", x)]
    raise ValueError(family)


def all_row_cases(D, in_f16=False):
    fams = ROW_FAMILIES + (("fp16_grid",) if in_f16 else ())
    return [c for fam in fams for c in row_cases(fam, D, in_f16)]


def benign_rows(D, rows=6, seed=7):
    """What every earlier test feeds: randn * 3 + 1."""
    return randn((rows, D), seed + D) * 3 + 1


# ------------------------------------------------------------------------------------------------------------ references and tolerances
def ln64(x, g, b, eps):
    """float64 LayerNorm of the rows as given (test_layout_guard_norm_gpu._ln64)."""
    return F.layer_norm(x.double(), (x.shape[-1],), None if g is None else g.double(), None if b is None else b.double(), eps)


def cond_row(x, eps):
    """mean|x| / sqrt(var + eps) per row, float64: [rows, 1]."""
    xd = x.double()
    return xd.abs().mean(-1, keepdim=True) / (xd.var(-1, unbiased=False, keepdim=True) + eps).sqrt()


def cond_term(x, g, eps):
    """12 * 2^-24 * cond_row * |gamma_i|: [rows, D]."""
    gam = torch.ones(x.shape[-1], dtype=f64) if g is None else g.double().abs()
    return N_ROUNDINGS * U * cond_row(x, eps) * gam


def row_bound(x, g, eps, ref, flat):
    """Per-element bound of a row output: flat = (atol, rtol) of that output, plus the conditioning term of the normalised row x."""
    return flat[0] + flat[1] * ref.double().abs() + cond_term(x, g, eps)


def chain_bound(y, g2, eps2, tol1):
    """Bound of the chained LayerNorm z = LN(y; gamma2, beta2, eps2): its flat 4e-5, the conditioning term of y, and the first stage's bound
    tol1 [rows, D] carried through: tol1_i / sqrt(var(y) + eps2) * |gamma2_i|."""
    sig = (y.double().var(-1, unbiased=False, keepdim=True) + eps2).sqrt()
    return TOL_CHAIN[0] + cond_term(y, g2, eps2) + tol1 / sig * g2.double().abs()


# ------------------------------------------------------------------------------------------------------------ float32 restatements
def _tree64(v):
    """wave_sum: the xor-shuffle tree over the last axis (64 lanes), float32; every lane ends with the same value."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    return v[..., 0]


def _lanes(x, D, h8):
    """[rows, D] float32 -> ([rows, LN_MAXV, 64, 4], mask): a lane's float4 registers v[0..3] in the kernel's order.  fp32 form: column
    4 (lane + 64 j) + k in v[j]; fp16 form (h8): the 8-column chunk j of a lane in v[2j], v[2j + 1]."""
    rows = x.shape[0]
    pad = np.zeros((rows, 256 * LN_MAXV), np.float32)
    pad[:, :D] = x
    m = np.zeros((rows, 256 * LN_MAXV), bool)
    m[:, :D] = True
    if h8:
        sh = lambda a: a.reshape(rows, 2, 64, 2, 4).transpose(0, 1, 3, 2, 4).reshape(rows, 4, 64, 4)
    else:
        sh = lambda a: a.reshape(rows, 4, 64, 4)
    return sh(pad), sh(m)


def _lane_sum(v, m):
    """sum over a lane's float4s, s += (a + b) + (c + d) in register order, then the wave tree: [rows]."""
    v = np.where(m, v, np.float32(0))
    p = (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])        # [rows, 4, 64]
    s = np.zeros_like(p[:, 0])
    for j in range(LN_MAXV):
        s = s + p[:, j]
    return _tree64(s)


def ln_rows_f32(x, g, b, eps, h8=False, wrong=None):
    """ln_normalize (either row layout) + affine in float32: two-pass mean, centred biased variance, rsqrt(var + eps).  wrong in
    {None, "one_pass", "mean_fp16", "drop_last_float4"}: E[x^2] - mean^2; the mean taken from the fp16-rounded row; the last float4 of the
    row left out of both sums.  Returns float32 [rows, D]."""
    x = np.ascontiguousarray(x.numpy() if isinstance(x, torch.Tensor) else x, np.float32)
    rows, D = x.shape
    v, m = _lanes(x, D, h8)
    ms = m.copy()
    if wrong == "drop_last_float4":
        last = np.zeros((rows, 256 * LN_MAXV), bool)
        last[:, D - 4:D] = True
        ms &= ~_lanes(last.astype(np.float32), 256 * LN_MAXV, h8)[0].astype(bool)
    fD = np.float32(D)
    if wrong == "mean_fp16":
        mean = _lane_sum(_lanes(x.astype(np.float16).astype(np.float32), D, h8)[0], ms) / fD
    else:
        mean = _lane_sum(v, ms) / fD
    mean = mean.astype(np.float32)
    if wrong == "one_pass":
        var = _lane_sum(v * v, ms) / fD - mean * mean
        var = np.maximum(var, np.float32(0))
    else:
        d = v - mean[:, None, None, None]
        var = _lane_sum(d * d, ms) / fD
    rstd = (np.float32(1) / np.sqrt((var + np.float32(eps)).astype(np.float32))).astype(np.float32)
    y = (x - mean[:, None]) * rstd[:, None]
    if g is not None:
        y = y * g.numpy().astype(np.float32) + b.numpy().astype(np.float32)
    return torch.from_numpy(y.astype(np.float32))


# ------------------------------------------------------------------------------------------------------------ images: zh_global_ln_l2
@dataclass
class ImageCase:
    family: str
    name: str
    x: torch.Tensor                              # [B, M, C] float32
    desc: dict = field(default_factory=dict)

    @property
    def shape(self):
        return tuple(self.x.shape)


def n_chunks(M, C):
    return -(-(M * C) // GLN_CHUNK)


def image_cases(family, B, M, C):
    mk = lambda name, x, **desc: ImageCase(family, f"{family}/{name} B={B} M={M} C={C}", x.to(f32).contiguous(), desc)
    n = M * C
    if family == "step":
        x = randn((B, n), 600 + C)
        third = n // 3
        x[:, :third] += 50
        x[:, third:] -= 20
        x[:, n - 4:] = 900
        return [mk("+50 / -20 / 900", x.view(B, M, C), third=third)]
    if family == "offset":
        return [mk("randn + 1e3", randn((B, M, C), 601 + C) + 1e3)]
    if family == "per_image":
        off, sc = (50.0, -3.0, 0.0), (1.0, 0.01, 100.0)
        x = torch.stack([randn((M, C), 602 + C + b) * sc[b % 3] + off[b % 3] for b in range(B)])
        return [mk("+50/1, -3/0.01, 0/100", x, offsets=off[:B], scales=sc[:B])]
    if family == "constant":
        return [mk(f"c={c:g}", torch.full((B, M, C), c), c=c) for c in IMAGE_CONSTANTS]
    raise ValueError(family)


def all_image_cases(B, M, C):
    return [c for fam in IMAGE_FAMILIES for c in image_cases(fam, B, M, C)]


def benign_image(B, M, C, seed=52):
    return randn((B, M, C), seed) * 2 + 0.3


def gln64(x, eps, l2_eps):
    xd = x.double()
    v = F.layer_norm(xd, xd.shape[1:], eps=eps)
    return v / (v.norm(dim=-1, keepdim=True) + l2_eps)


def cond_image(x, eps):
    """mean|x| / sqrt(var + eps) over each image, float64: [B, 1, 1]."""
    xd = x.double().flatten(1)
    return (xd.abs().mean(1) / (xd.var(1, unbiased=False) + eps).sqrt())[:, None, None]


def image_bound(x, eps, ref, flat):
    return flat[0] + flat[1] * ref.double().abs() + N_ROUNDINGS * U * cond_image(x, eps) / np.sqrt(x.shape[-1])


def chunk_partials_f32(img):
    """gln_partial_kernel on one flat image: (n, mean, M2) per 4096-float chunk, float32 [nchunks, 3].  A thread's float4s j = 0..3 at
    element (t + 256 j) * 4, four waves, (red0 + red1) + (red2 + red3)."""
    n = img.shape[0]
    out = []
    for base in range(0, n, GLN_CHUNK):
        cnt = min(GLN_CHUNK, n - base)
        pad = np.zeros(GLN_CHUNK, np.float32)
        pad[:cnt] = img[base:base + cnt]
        m = (np.arange(GLN_CHUNK) < cnt).reshape(4, 4, 64, 4)        # [j, wave, lane, k]
        v = pad.reshape(4, 4, 64, 4)

        def block_sum(a):
            a = np.where(m, a, np.float32(0))
            p = (a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])      # [j, wave, lane]
            s = np.zeros_like(p[0])
            for j in range(4):
                s = s + p[j]
            red = _tree64(s)                                         # [wave]
            return (red[0] + red[1]) + (red[2] + red[3])
        mean = np.float32(block_sum(v) / np.float32(cnt))
        d = v - mean
        out.append((np.float32(cnt), mean, np.float32(block_sum(d * d))))
    return np.array(out, np.float32)


def gln_f32(x, eps, l2_eps, wrong=None):
    """zh_global_ln_l2 in float32 / float64 as norm.hip states it: chunk partials in fp32, Chan's combine in fp64 weighted by the chunk
    counts, float(mean), rstd = float(1 / sqrt(m2 / n + eps)), then per pixel v = (x - mean) * rstd, y = v * (1 / (sqrt(sum v^2) + l2_eps)).
    wrong in {None, "unweighted", "no_between", "cap64"}: the plain average of the chunk means; the n * d * d term of the variance dropped;
    only the first 64 chunks combined.  Returns float32 [B, M, C]."""
    xn = np.ascontiguousarray(x.numpy(), np.float32)
    B, M, C = xn.shape
    out = np.empty_like(xn)
    for b in range(B):
        part = chunk_partials_f32(xn[b].reshape(-1))
        if wrong == "cap64":
            part = part[:64]
        cnt, mu, m2c = part[:, 0].astype(np.float64), part[:, 1].astype(np.float64), part[:, 2].astype(np.float64)
        sn = cnt.sum()
        mean = mu.mean() if wrong == "unweighted" else (cnt * mu).sum() / sn
        d = mu - mean
        m2 = m2c.sum() if wrong == "no_between" else (m2c + cnt * d * d).sum()
        fmean, rstd = np.float32(mean), np.float32(1.0 / np.sqrt(m2 / sn + np.float64(np.float32(eps))))
        v = ((xn[b] - fmean) * rstd).astype(np.float32)
        lanes, mask = _lanes(v, C, False)
        q = _lane_sum(lanes * lanes, mask)
        inv = (np.float32(1) / (np.sqrt(q).astype(np.float32) + np.float32(l2_eps))).astype(np.float32)
        out[b] = v * inv[:, None]
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------------------ zh_l2norm_rows
def l2_cases(family, D):
    mk = lambda name, x, **desc: RowCase(family, f"l2 {family}/{name} D={D}", D, x.to(f32), False, 0.0, desc)
    if family == "dominant":
        x = randn((5, D), 700 + D, 1e-2)
        cols = [0, D - 1, D // 2, 3, D - 4]
        for r, c in enumerate(cols):
            x[r, c] = 1e3 if r % 2 == 0 else -1e3
        return [mk("one element 1e3", x, cols=cols)]
    if family == "scaled":
        return [mk(f"randn * {s:g}", randn((6, D), 701 + D + i, s), scale=s) for i, s in enumerate((1e-3, 1.0, 1e3))]
    if family == "zero":
        x = randn((7, D), 710 + D)
        x[2] = 0
        x[6] = 0                                 # one zero row inside a full workgroup, one in the ragged one
        return [mk("zero rows 2 and 6", x, zero_rows=(2, 6))]
    raise ValueError(family)


def all_l2_cases(D):
    return [c for fam in L2_FAMILIES for c in l2_cases(fam, D)]


def l2_64(x, eps):
    """x / (||x|| + eps) in float64; a zero row with eps = 0 is NaN, as x / x.norm() is in torch."""
    xd = x.double()
    return xd / (xd.norm(dim=-1, keepdim=True) + eps)


def l2_rows_f32(x, eps):
    xn = np.ascontiguousarray(x.numpy(), np.float32)
    lanes, mask = _lanes(xn, xn.shape[1], False)
    q = _lane_sum(lanes * lanes, mask)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (np.float32(1) / (np.sqrt(q).astype(np.float32) + np.float32(eps))).astype(np.float32)
        return torch.from_numpy((xn * inv[:, None]).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------ zh_sum_layernorm_f32
def cancelling_parts(row, n_parts, seed):
    """n_parts fp32 planes whose plane-order sum is (close to) `row` [rows, D]: parts[0] = +big, parts[1] = -big + row, the rest small.  The
    sum the kernel normalises is whatever fp32 makes of them — plane_sum() — not `row` itself."""
    if n_parts == 1:
        return row.to(f32)[None].clone()
    big = randn(row.shape, seed, 1e3)
    parts = [big, (-big + row.to(f32))] + [randn(row.shape, seed + s, 1e-3) for s in range(2, n_parts)]
    return torch.stack(parts)


def plane_sum(parts, bias=None, residual=None):
    """The kernel's order, float32: ((parts[0] + parts[1] + ...) + bias) + residual."""
    x = parts[0].clone()
    for s in range(1, parts.shape[0]):
        x = x + parts[s]
    if bias is not None:
        x = x + bias
    if residual is not None:
        x = x + residual
    return x


def sum_cases(D):
    """The rows zh_sum_layernorm_f32 is given as a sum."""
    return row_cases("mixed", D) + row_cases("offset", D)[1:4] + row_cases("outlier", D) + row_cases("constant", D)


def sum_operands(case, n_parts, ci):
    """(parts, bias, residual) of sum case number ci: the cancelling planes, a small bias and residual (randn * 1e-2)."""
    return cancelling_parts(case.x, n_parts, 80 + case.D + ci), randn((case.D,), 81, 1e-2), randn((case.rows, case.D), 82, 1e-2)


def chain_affine(D):
    """gamma1 ~ 0.01 and beta1 ~ 50 + noise make y = LN(x) a badly conditioned input of the chained LayerNorm (mean / std about 50);
    gamma2, beta2 as the layout test draws them."""
    return randn((D,), 83) * 0.002 + 0.01, randn((D,), 84) + 50, randn((D,), 85) * 0.2 + 1, randn((D,), 86) * 0.1
