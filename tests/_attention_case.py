"""Attention inputs by construction: (q32, k32, v32) float32 tensors whose scaled scores follow a chosen pattern, for the softmax tests
(tests/test_attention_softmax_gpu.py runs them through the kernels, tests/test_attention_softmax_cpu.py checks the cases themselves).

The structure sits in ONE feature of each head: q[i, 0] = a_i and k[j, 0] = b_j / c with c = scale * log2(e), so the scaled score of
(query i, key j) is a_i * b_j in LOG2 UNITS — the unit of the kernels' running max (attention.hip keeps m_run in log2 units and compares
it with ZH_ATTN_LAZY_LOG2).  Feature 1 carries an optional common offset of a row (q[i, 1] = offset, k[j, 1] = 1 / c: the very same k
value for every key, so the shift is exactly common whatever the rounding).  Every other feature is 0.01 * randn (about 1e-4 log2 units of
score noise; fp16 cases) or zero (x3 cases: see below).  All tensors are returned AS THE KERNEL SEES THEM: rounded to fp16, or to the split pair hi + lo (x3) — so the
float64 softmax(Q K^T scale) V of tests/test_layout_guard_attention_gpu.py::attn_case is the reference of exactly these operands, and the
helper only chooses inputs.

Constants: the key-tile heights are the header's (ZH_ATTN_KEY_TILE_F16 / _X3 of include/zutis_hip.h, which static_asserts hold the kernels to);
the lazy-max threshold L = ZH_ATTN_LAZY_LOG2 is private to zutis_amd/csrc/attention.hip and read from it by regex (kernel_constants()).  The
cases follow them if they change.

Split-pair (x3) cases keep |scaled score| <= 64 log2 units for every key that carries weight: the raw fp32 score is then below 512
(c >= 0.147 at head_dim 96), its ulp 2^-15, i.e. at most 2^-16 * c * ln 2 = 1.9e-6 of relative error in a probability, and the float32
rounding of scale * log2(e) (2^-24 relative, times 64) adds 2.6e-6 * ln 2 at most — together under a quarter of the 2e-5 tolerance.  That
counts ONE rounding per score, so the x3 cases leave the other features zero: sixty-odd noise terms added to a score of 400 round at its
ulp each time, whatever their size (measured here: 2e-5 of error in O from the noise alone).  For the same reason the random causal heads
use randn * 1.5 operands under x3, not the * 2.5 of the layout tests (a sum of 64 or 96 products of that size carries 6e-6 by itself).  The
one exception is the key-split chunk placed 150 log2 units below the rest (at -90, the rest at +60): its weight is exactly 0.
test_attention_softmax_cpu.py::test_float32_reference_within_quarter_tolerance holds every case to this.
"""
import math
import pathlib
import re
from dataclasses import dataclass, field

import torch

from zutis_amd import _lib

f16, f32, f64 = torch.float16, torch.float32, torch.float64
LOG2E = 1.4426950408889634
FAMILIES = ("staircase", "row_schedule", "peak_tail", "one_hot", "uniform", "common_offset", "causal", "key_split")
STEPS = (0.5, 0.99, 1.01, 2.0)                  # staircase steps in units of L
TAIL_DEPTHS = (-15.3, -17.3, -12.0)             # log2 units below the peak
JITTER = 0.01
_SRC = pathlib.Path(__file__).resolve().parents[1] / "zutis_amd" / "csrc" / "attention.hip"


def kernel_constants():
    """(L, kt_fp16, kt_x3): L from attention.hip, the tile heights from the header."""
    lazy = re.search(r"#define\s+ZH_ATTN_LAZY_LOG2\s+([0-9]+(?:\.[0-9]*)?)f?\b", _SRC.read_text())
    assert lazy, "attention.hip no longer defines ZH_ATTN_LAZY_LOG2"
    zh = _lib.constants()
    return float(lazy.group(1)), zh["ZH_ATTN_KEY_TILE_F16"], zh["ZH_ATTN_KEY_TILE_X3"]


LAZY, KT_F16, KT_X3 = kernel_constants()


def tile_height(x3):
    return KT_X3 if x3 else KT_F16


def as_seen(x, x3):
    """x rounded to what the kernel reads: fp16, or the split pair hi + lo (exact in float32: 22 bits)."""
    x = x.to(f32)
    hi = x.to(f16)
    if not x3:
        return hi.float()
    return hi.float() + (x - hi.float()).to(f16).float()


@dataclass
class Case:
    family: str
    name: str
    x3: bool
    dh: int
    heads: int
    B: int
    Tq: int
    Tk: int
    q: torch.Tensor                              # [B, Tq, heads * dh] float32, as the kernel sees it
    k: torch.Tensor
    v: torch.Tensor
    layout: str = "slice"
    causal: bool = False
    scale: float = None
    ksplit: int = 1
    expect_error: bool = False
    desc: dict = field(default_factory=dict)     # the target structure

    @property
    def tol(self):
        return 2e-5 if self.x3 else 4e-3         # the project's own (attn_case)

    @property
    def sc(self):
        return 1.0 / math.sqrt(self.dh) if self.scale is None else self.scale

    def kwargs(self):
        """The keyword arguments of attn_case."""
        return dict(x3=self.x3, dh=self.dh, heads=self.heads, B=self.B, Tq=self.Tq, Tk=self.Tk, layout=self.layout, causal=self.causal,
                    ksplit=self.ksplit, scale=self.scale, expect_error=self.expect_error, inputs=(self.q, self.k, self.v))

    def per_head(self, t):
        return t.view(self.B, -1, self.heads, self.dh).transpose(1, 2)       # [B, heads, T, dh]

    def __repr__(self):
        return f"{self.family}/{self.name} x3={self.x3} dh={self.dh} heads={self.heads} B={self.B} Tq={self.Tq} Tk={self.Tk} {self.layout}"


def scores_log2(case):
    """float64 [B, heads, Tq, Tk]: the scaled scores of the operands as seen, in log2 units (no mask)."""
    qh, kh = case.per_head(case.q.double()), case.per_head(case.k.double())
    return qh @ kh.transpose(-1, -2) * (case.sc * LOG2E)


def _mask(case, s):
    if case.causal:
        s = s + torch.full((case.Tq, case.Tk), float("-inf"), dtype=s.dtype).triu_(1)
    return s


def reference(case):
    """float64 softmax(Q K^T scale) V of the operands as seen: [B, Tq, heads * dh] — what attn_case computes."""
    qh, kh, vh = (case.per_head(t.double()) for t in (case.q, case.k, case.v))
    s = _mask(case, qh @ kh.transpose(-1, -2) * case.sc)
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(case.B, case.Tq, -1)


def reference_f32(case):
    """The same softmax with every per-element step in float32 — the raw score, the kernel's scale constant float32(scale) *
    1.4426950408889634f, the subtraction of the row max, exp2 — which is what the inputs themselves cost.  The two reductions (row sum and
    P V) add those float32 probabilities in float64: the order of a float32 sum is the kernel's business, not the inputs' (a peak of 1
    followed by a thousand addends of 2^-15 loses 1e-5 in a sequential float32 sum and nothing in the kernels' tile-wise one)."""
    c = torch.tensor(case.sc, dtype=f32) * torch.tensor(LOG2E, dtype=f32)
    qh, kh, vh = (case.per_head(t.to(f32)) for t in (case.q, case.k, case.v))
    s = _mask(case, qh @ kh.transpose(-1, -2))
    m = s.max(-1, keepdim=True).values * c
    p = torch.exp2(s * c - m).double()
    return ((p @ vh.double()) / p.sum(-1, keepdim=True)).transpose(1, 2).reshape(case.B, case.Tq, -1)


def lazy_schedule(tile_max, L=LAZY):
    """The tiles at which a running reference point that only moves past L moves: tile_max[t] in log2 units -> (moves, margins); margin
    = distance of the decision from the threshold (inf for the first tile)."""
    m, moves, margins = -math.inf, [], []
    for x in tile_max:
        x = float(x)
        moves.append(x > m + L)
        margins.append(abs(x - (m + L)) if math.isfinite(m) else math.inf)
        if moves[-1]:
            m = x
    return moves, margins


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, s=1.0):
    return torch.randn(shape, generator=_gen(seed)) * s


def _jitter(shape, seed):
    return (torch.rand(shape, generator=_gen(seed)) * 2 - 1) * JITTER


def _assemble(family, name, *, x3, dh, heads, B, Tq, Tk, a, b, v, offset=None, seed=0, scale=None, **kw):
    """a [B, heads, Tq], b [B, heads, Tk] (broadcastable): scaled score (i, j) = a_i * b_j (+ offset [B, heads]) log2 units."""
    sc = 1.0 / math.sqrt(dh) if scale is None else scale
    c = sc * LOG2E
    noise = 0.0 if x3 else 0.01
    q = _randn((B, heads, Tq, dh), seed + 11, noise)
    k = _randn((B, heads, Tk, dh), seed + 12, noise)
    q[..., 0] = torch.as_tensor(a, dtype=f64).expand(B, heads, Tq).to(f32)
    k[..., 0] = (torch.as_tensor(b, dtype=f64).expand(B, heads, Tk) / c).to(f32)
    q[..., 1], k[..., 1] = 0.0, 0.0
    if offset is not None:
        q[..., 1] = torch.as_tensor(offset, dtype=f32).expand(B, heads)[..., None]
        k[..., 1] = 1.0 / c
    return _finish(family, name, x3=x3, dh=dh, heads=heads, B=B, Tq=Tq, Tk=Tk, qh=q, kh=k, vh=v, scale=scale, **kw)


def _finish(family, name, *, x3, dh, heads, B, Tq, Tk, qh, kh, vh, **kw):
    """qh / kh / vh: [B, heads, T, dh] -> the [B, T, heads * dh] tensors as seen."""
    flat = lambda t, T: as_seen(t.to(f32).transpose(1, 2).reshape(B, T, heads * dh).contiguous(), x3)
    return Case(family, name, x3, dh, heads, B, Tq, Tk, flat(qh, Tq), flat(kh, Tk), flat(vh, Tk), **kw)


def _slots(B, heads):
    return [(bi, h) for bi in range(B) for h in range(heads)]


def _placements(Tk, kt):
    """Key 0, the last key of tile 0, the first key of the ragged last tile, the very last key."""
    return [0, min(kt, Tk) - 1, (Tk - 1) // kt * kt, Tk - 1]


# ---------------------------------------------------------------------------------------------------------------- staircase
def stair_levels(ntiles, step_l, rising):
    """Tile t at t * step (rising) or (ntiles - 1 - t) * step (falling), centred on 0 so that 2 L steps stay within +-6 L."""
    lv = (torch.arange(ntiles, dtype=f64) - (ntiles - 1) / 2) * (step_l * LAZY)
    return lv if rising else lv.flip(0)


def _stair_b(Tk, kt, step_l, rising, seed):
    ntiles = (Tk + kt - 1) // kt
    lv = stair_levels(ntiles, step_l, rising)
    return lv[torch.arange(Tk) // kt] + _jitter((Tk,), seed).double(), lv


def staircase(x3, dh):
    """Tk = 6 kt + 5; head 0 carries (step, direction), head 1 the opposite direction, head 2 another step; image 1 the heads rotated."""
    kt = tile_height(x3)
    Tk, heads, B = 6 * kt + 5, 3, 2
    out = []
    for si, step in enumerate(STEPS):
        for rising in (True, False):
            other = STEPS[(si + 2) % len(STEPS)]
            pats = [(step, rising), (step, not rising), (other, rising)]
            b = torch.zeros(B, heads, Tk, dtype=f64)
            spec = {}
            for n, (bi, h) in enumerate(_slots(B, heads)):
                st, up = pats[(h + bi) % 3]
                b[bi, h], lv = _stair_b(Tk, kt, st, up, 100 * si + n)
                spec[(bi, h)] = dict(step=st, rising=up, levels=lv)
            layout = "slice" if rising else "packed"
            Tq = 33 if layout == "slice" else Tk
            out.append(_assemble("staircase", f"step{step}L-{'rising' if rising else 'falling'}", x3=x3, dh=dh, heads=heads, B=B, Tq=Tq, Tk=Tk,
                                 a=1.0, b=b, v=_randn((B, heads, Tk, dh), 7 + si), seed=si, layout=layout, desc=dict(kt=kt, heads=spec)))
    return out


# ---------------------------------------------------------------------------------------------------------------- row schedule
def row_schedule(x3, dh):
    """a_i in {+1, 0, -1} by (i + head) % 3 against a rising staircase: neighbouring lanes of one wave rise, stay flat and fall."""
    kt = tile_height(x3)
    Tk, heads, B = 6 * kt + 5, 3, 2
    out = []
    for Tq, layout in ((33, "slice"), (129, "slice"), (Tk, "packed")):
        b = torch.zeros(B, heads, Tk, dtype=f64)
        a = torch.zeros(B, heads, Tq, dtype=f64)
        spec = {}
        for n, (bi, h) in enumerate(_slots(B, heads)):
            step = (1.01, 2.0, 0.99)[(h + bi) % 3]
            b[bi, h], lv = _stair_b(Tk, kt, step, True, 300 + n)
            a[bi, h] = torch.tensor([1.0, 0.0, -1.0], dtype=f64)[(torch.arange(Tq) + h) % 3]
            spec[(bi, h)] = dict(step=step, levels=lv)
        out.append(_assemble("row_schedule", f"Tq{Tq}-{layout}", x3=x3, dh=dh, heads=heads, B=B, Tq=Tq, Tk=Tk, a=a, b=b,
                             v=_randn((B, heads, Tk, dh), 17 + Tq), seed=Tq, layout=layout, desc=dict(kt=kt, heads=spec)))
    return out


# ---------------------------------------------------------------------------------------------------------------- peak over a tail
def peak_tail(x3, dh):
    """One key at 0, all others `depth` log2 units below; V of the tail opposite in sign to the peak's ("opposite") or random.  The peak's
    place differs per (image, head): the four placements of _placements()."""
    kt = tile_height(x3)
    heads, B, out = 3, 2, []
    for depth in TAIL_DEPTHS:
        for Tk in (4 * kt + 5, 1029):
            for vmode in ("opposite", "random"):
                layout = "packed" if (Tk < 1029 and vmode == "random") else "slice"
                Tq = Tk if layout == "packed" else 33
                b = torch.full((B, heads, Tk), depth, dtype=f64)
                w = 0.5 + 0.5 * torch.arange(dh, dtype=f32) / dh          # 0.5 .. 1: every column sees the tail
                v = -w.expand(B, heads, Tk, dh).clone() if vmode == "opposite" else _randn((B, heads, Tk, dh), 23 + Tk)
                spec = {}
                for n, (bi, h) in enumerate(_slots(B, heads)):
                    p = _placements(Tk, kt)[n % 4]
                    b[bi, h, p] = 0.0
                    if vmode == "opposite":
                        v[bi, h, p] = w
                    spec[(bi, h)] = dict(peak=p)
                mass = (Tk - 1) * 2.0 ** depth
                out.append(_assemble("peak_tail", f"depth{depth}-Tk{Tk}-{vmode}", x3=x3, dh=dh, heads=heads, B=B, Tq=Tq, Tk=Tk, a=1.0, b=b, v=v,
                                     seed=Tk, layout=layout,
                                     desc=dict(kt=kt, depth=depth, vmode=vmode, heads=spec, tail_mass=mass / (1.0 + mass))))
    return out


# ---------------------------------------------------------------------------------------------------------------- one-hot
ONE_HOT_GAP = 40.5                               # the target; >= 40 after jitter and operand rounding (checked on the CPU)


def one_hot(x3, dh):
    """One key 40 log2 units above the rest: O is that key's V row.  The four placements, and — causal — the diagonal key of every row
    (identity features: q_i = A e_(i), k_j = A e_(j), T <= head_dim)."""
    kt = tile_height(x3)
    heads, B, out = 3, 2, []
    for Tk, layout in ((4 * kt + 5, "slice"), (4 * kt + 5, "packed"), (1029, "slice")):
        Tq = Tk if layout == "packed" else 33
        b = (-ONE_HOT_GAP / 2 + _jitter((B, heads, Tk), 31 + Tk)).double()
        spec = {}
        for n, (bi, h) in enumerate(_slots(B, heads)):
            p = _placements(Tk, kt)[(n + 1) % 4]
            b[bi, h, p] = ONE_HOT_GAP / 2 + JITTER
            spec[(bi, h)] = dict(hot=p)
        out.append(_assemble("one_hot", f"Tk{Tk}-{layout}", x3=x3, dh=dh, heads=heads, B=B, Tq=Tq, Tk=Tk, a=1.0, b=b,
                             v=_randn((B, heads, Tk, dh), 37 + Tk), seed=Tk, layout=layout, desc=dict(kt=kt, heads=spec)))
    for T, layout in ((33, "packed"), (64, "slice")):
        assert T <= dh
        A = math.sqrt(ONE_HOT_GAP / (LOG2E / math.sqrt(dh)))
        qh = torch.zeros(B, heads, T, dh)
        qh[..., torch.arange(T), torch.arange(T)] = A
        out.append(_finish("one_hot", f"diagonal-causal-T{T}-{layout}", x3=x3, dh=dh, heads=heads, B=B, Tq=T, Tk=T, qh=qh, kh=qh.clone(),
                           vh=_randn((B, heads, T, dh), 41 + T), layout=layout, causal=True, desc=dict(kt=kt, diagonal=True)))
    return out


# ---------------------------------------------------------------------------------------------------------------- uniform
def _uniform_v(B, heads, Tk, dh, seed):
    """head 0: the constant 0.75; head 1: V[j] = j / Tk (a mean that depends on the exact key count); head 2: randn."""
    v = _randn((B, heads, Tk, dh), seed)
    v[:, 0] = 0.75
    v[:, 1] = (torch.arange(Tk, dtype=f32) / Tk)[:, None]
    return v


def uniform(x3, dh):
    """Q = 0: O is the mean of V over the valid keys (K is randn and must not matter)."""
    kt = tile_height(x3)
    heads, B, out = 3, 2, []
    for Tk, layout in ((1, "slice"), (kt - 1, "slice"), (kt + 1, "slice"), (kt + 1, "packed"), (1029, "slice")):
        Tq = Tk if layout == "packed" else 33
        out.append(_finish("uniform", f"Tk{Tk}-{layout}", x3=x3, dh=dh, heads=heads, B=B, Tq=Tq, Tk=Tk, qh=torch.zeros(B, heads, Tq, dh),
                           kh=_randn((B, heads, Tk, dh), 43 + Tk), vh=_uniform_v(B, heads, Tk, dh, 47 + Tk), layout=layout, desc=dict(kt=kt)))
    return out


# ---------------------------------------------------------------------------------------------------------------- common offset
def common_offset(x3, dh):
    """Every score of a row shifted by one constant: head 0 by +C, head 1 by -C, head 2 unshifted; C = 64 (fp16 and x3) and 1000 (fp16).
    The unshifted scores lie in [-8, 0] where the shift is +C and in [0, 8] where it is -C (|score| <= C throughout).  desc["base"] is
    the same case without the shift: its reference is the shifted case's."""
    kt = tile_height(x3)
    Tk, heads, B, out = 2 * kt + 5, 3, 2, []
    for C in (64.0, 1000.0):
        if x3 and C > 64.0:
            continue
        for layout in ("slice", "packed"):
            Tq = Tk if layout == "packed" else 33
            u = torch.rand((B, heads, Tk), generator=_gen(53)).double() * 8.0
            sign = torch.tensor([1.0, -1.0, 1.0], dtype=f64)[None, :, None]
            b = -sign * u
            off = torch.tensor([C, -C, 0.0]).expand(B, heads)
            common = dict(x3=x3, dh=dh, heads=heads, B=B, Tq=Tq, Tk=Tk, a=1.0, b=b, v=_randn((B, heads, Tk, dh), 59), seed=int(C), layout=layout)
            base = _assemble("common_offset", f"C{C:g}-{layout}-base", offset=torch.zeros(B, heads), **common)
            out.append(_assemble("common_offset", f"C{C:g}-{layout}", offset=off, desc=dict(kt=kt, C=C, base=base), **common))
    return out


# ---------------------------------------------------------------------------------------------------------------- causal
CAUSAL_T = (64, 65, 128, 129, 200)


def causal(x3, dh):
    """Causal attention past one query block.  Heads 0 and 2 are uniform (Q = 0: row i is the mean of V[0..i]), head 1 is random; each T
    in the packed and the slice layout, T = 129 in the slice layout also with a non-default scale."""
    kt = tile_height(x3)
    heads, B, out = 3, 2, []
    for T in CAUSAL_T:
        for layout, scale in (("packed", None), ("slice", None)) + ((("slice", 0.07),) if T == 129 else ()):
            qh = _randn((B, heads, T, dh), 61 + T, 1.5 if x3 else 1.0)
            qh[:, 0], qh[:, 2] = 0.0, 0.0
            out.append(_finish("causal", f"T{T}-{layout}" + ("" if scale is None else f"-scale{scale}"), x3=x3, dh=dh, heads=heads, B=B, Tq=T, Tk=T,
                               qh=qh, kh=_randn((B, heads, T, dh), 67 + T, 1.5 if x3 else 1.0), vh=_randn((B, heads, T, dh), 71 + T), layout=layout,
                               causal=True, scale=scale, desc=dict(kt=kt, uniform_heads=(0, 2))))
    return out


# ---------------------------------------------------------------------------------------------------------------- key split
KSPLIT_HIGH, KSPLIT_LOW, KSPLIT_REST = 60.0, -90.0, -20.0


def key_split(x3, dh):
    """Unequal key chunks for attn_combine_kernel's w_s = 2^(m_s - m).  Head 0: a dominant key (0 against -20) in the FIRST chunk; head 1:
    in the LAST chunk (its very last key); head 2: one whole chunk at -90 against +60 elsewhere — 150 log2 units down, w_s = 0 exactly
    (the chunk is the first one in image 0 and the last one in image 1).  Plus all chunks equal and uniform (Q = 0): the exact mean.
    ksplit = 2 at Tk = 8 kt + 5 (chunks of 5 and 4 tiles); ksplit = 4 needs 13 tiles (12 kt + 5: 4 + 4 + 4 + 1) — at 8 kt + 5 its
    fourth chunk would be empty, which the library refuses: that case is kept as the refusal it is."""
    kt = tile_height(x3)
    heads, B, out = 3, 2, []
    for ksplit, Tk in ((2, 8 * kt + 5), (4, 12 * kt + 5)):
        ntiles = (Tk + kt - 1) // kt
        kchunk = (ntiles + ksplit - 1) // ksplit * kt
        assert (ksplit - 1) * kchunk < Tk
        b = (KSPLIT_REST + _jitter((B, heads, Tk), 73 + ksplit)).double()
        b[:, 0, 3] = 0.0
        b[:, 1, Tk - 1] = 0.0
        b[:, 2] += KSPLIT_HIGH - KSPLIT_REST
        b[0, 2, :kchunk] += KSPLIT_LOW - KSPLIT_HIGH
        b[1, 2, (ksplit - 1) * kchunk:] += KSPLIT_LOW - KSPLIT_HIGH
        for layout in ("slice", "packed"):
            Tq = Tk if layout == "packed" else 33
            out.append(_assemble("key_split", f"unequal-ksplit{ksplit}-{layout}", x3=x3, dh=dh, heads=heads, B=B, Tq=Tq, Tk=Tk, a=1.0, b=b,
                                 v=_randn((B, heads, Tk, dh), 79 + ksplit), seed=ksplit, layout=layout, ksplit=ksplit,
                                 desc=dict(kt=kt, kchunk=kchunk)))
        out.append(_finish("key_split", f"uniform-ksplit{ksplit}", x3=x3, dh=dh, heads=heads, B=B, Tq=33, Tk=Tk, qh=torch.zeros(B, heads, 33, dh),
                           kh=_randn((B, heads, Tk, dh), 83), vh=_uniform_v(B, heads, Tk, dh, 89), ksplit=ksplit, desc=dict(kt=kt, kchunk=kchunk)))
    Tk = 8 * kt + 5
    out.append(_finish("key_split", "ksplit4-empty-chunk-refused", x3=x3, dh=dh, heads=1, B=1, Tq=33, Tk=Tk, qh=torch.zeros(1, 1, 33, dh),
                       kh=_randn((1, 1, Tk, dh), 97), vh=_randn((1, 1, Tk, dh), 101), ksplit=4, expect_error=True, desc=dict(kt=kt)))
    return out


_BUILDERS = dict(staircase=staircase, row_schedule=row_schedule, peak_tail=peak_tail, one_hot=one_hot, uniform=uniform,
                 common_offset=common_offset, causal=causal, key_split=key_split)
_CACHE = {}


def cases(family, x3, dh):
    """The cases of one family for one kernel variant (built once per process; treat them as read-only)."""
    key = (family, bool(x3), int(dh))
    if key not in _CACHE:
        _CACHE[key] = _BUILDERS[family](bool(x3), int(dh))
    return _CACHE[key]
