"""Guard-band arenas for kernel tests: operands and outputs at the engine's layouts (padded leading dimensions, batch strides, split-pair
plane offsets, offset base pointers) carved out of one uint8 buffer whose every other byte is a sentinel.

  * an OUTPUT arena is filled with 0xA5; assert_untouched() proves that a call wrote the logical [batch, M, N] elements of its outputs
    (both planes of a split pair) and not one byte of row padding, of the space between batch items or planes, or of the guards;
  * an INPUT arena is filled with 0xFF — a NaN as fp16 / fp32, -1 as int64, 255 as u8 — so that an element read from outside the logical
    input and allowed to reach a result shows in assert_close() as a NaN or a wrong integer;
  * every view has >= 4 KiB of guard in front and, behind it, `tail_rows` x the leading dimension (the largest tile that can touch it:
    256 rows for GEMM operands and outputs, one key tile for attention, one row group for the row kernels): an overrun of one tile,
    read or write, stays inside the allocation and is reported instead of damaging something else;
  * a workspace is a uint8 view of exactly the bytes its *_workspace_size function returned, guarded the same way.

Plain helper module (no fixtures, no pytest hooks); works on the CPU too, which is how tests/test_guard_cpu.py proves it can fail.
"""
import torch

OUT_FILL, IN_FILL = 0xA5, 0xFF
LEAD_GUARD = 4096
_ORIGIN_ALIGN = 4096
_SAME_SIZE_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _isz(dtype) -> int:
    return torch.empty((), dtype=dtype).element_size()


class View:
    """`planes` x `batch` x [M, N] elements of `dtype` inside an arena: element (p, b, m, n) lies p * plane + b * bstride + m * ld + n
    elements behind the view's base.  .t is the strided tensor [planes, batch, M, N] (what zutis_amd.ops.Act wraps), .hi = .t[0]."""

    def __init__(self, arena, name, dtype, batch, M, N, ld, bstride, planes, plane, off, end):
        self.arena, self.name, self.dtype = arena, name, dtype
        self.batch, self.M, self.N, self.ld, self.bstride, self.planes, self.plane = batch, M, N, ld, bstride, planes, plane
        self.off, self.end = off, end                 # byte offset of the base from the arena's origin; end of the trailing guard
        self.isz = _isz(dtype)

    def _strided(self, buf, dtype):
        span = (self.planes - 1) * self.plane + (self.batch - 1) * self.bstride + (self.M - 1) * self.ld + self.N
        flat = buf[self.off:self.off + span * self.isz].view(dtype)
        return flat.as_strided((self.planes, self.batch, self.M, self.N), (self.plane, self.bstride, self.ld, 1))

    @property
    def t(self):
        return self._strided(self.arena.bytes, self.dtype)

    @property
    def hi(self):
        return self.t[0]

    @property
    def m2(self):
        """[M, N] of plane 0, batch item 0."""
        return self.t[0, 0]

    def act(self, out_scale=1.0):
        from zutis_amd.ops import Act
        return Act(self.t, out_scale)

    def origin(self, back=0, out_scale=1.0):
        """For kernels that take a buffer pointer plus a row offset: a flat tensor of this dtype whose element 0 lies `back` elements in
        front of the view's base (inside its leading guard: carve the view with lead >= back * itemsize); a split pair comes back as an
        ops.Act over that pointer with the view's plane offset."""
        start = self.off - back * self.isz
        assert start >= 0 and back >= 0
        flat = self.arena.bytes[start:self.end].view(self.dtype)
        if self.planes == 1:
            return flat
        from zutis_amd.ops import Act
        a = Act.__new__(Act)
        a.t, a.hi, a.plane, a.out_scale, a.x2 = flat, flat, self.plane, float(out_scale), False
        return a

    def put(self, x):
        """Write the logical elements: x is [planes, batch, M, N] or any shape with as many elements."""
        self.t.copy_(x.reshape(self.planes, self.batch, self.M, self.N).to(self.dtype))
        return self

    def get(self):
        """The logical elements as a contiguous CPU tensor [planes, batch, M, N]."""
        return self.t.detach().cpu().contiguous()

    def pair(self):
        """hi + lo in float64 (split pair), or the plane itself: [batch, M, N] on the CPU."""
        g = self.get().double()
        return g[0] + g[1] if self.planes == 2 else g[0]

    def locate(self, byte_off):
        """(plane, batch, row, col) of arena byte `byte_off` in this view's addressing (row >= M / col >= N: padding or guard)."""
        rel = (byte_off - self.off) // self.isz
        if rel < 0:
            return (0, 0, rel // self.ld if self.ld else rel, rel % self.ld if self.ld else 0)
        p = 0
        if self.planes == 2 and rel >= self.plane:
            p, rel = 1, rel - self.plane
        b = 0
        if self.batch > 1 and self.bstride:
            b = min(rel // self.bstride, self.batch - 1)
            rel -= b * self.bstride
        return (p, b, rel // self.ld, rel % self.ld)


class Arena:
    """fill = OUT_FILL (outputs, workspaces) or IN_FILL (inputs).  add() / workspace() carve views; the buffer exists from the first
    .bytes access on, so carve everything first."""

    def __init__(self, fill, device="cpu"):
        self.fill, self.device = fill, torch.device(device)
        self.views, self._size, self._buf, self._origin = [], 0, None, 0

    def add(self, name, dtype, M, N, *, ld=None, batch=1, bstride=None, planes=1, plane=None, align=256, misalign=0, tail_rows=256, lead=0):
        """ld / bstride / plane in elements (defaults: dense).  The base pointer is `align`-byte aligned plus `misalign` bytes; `lead`: extra
        bytes of leading guard (a kernel that is handed a pointer in FRONT of the view and a row offset: View.origin())."""
        assert self._buf is None, "carve every view before the buffer is used"
        isz = _isz(dtype)
        ld = N if ld is None else ld
        bstride = M * ld if bstride is None else bstride
        inner = (batch - 1) * bstride + (M - 1) * ld + N
        plane = (inner if plane is None else plane) if planes == 2 else 0
        assert ld >= N and (batch == 1 or bstride >= (M - 1) * ld + N) and (planes == 1 or plane >= inner)
        assert misalign % isz == 0 and _ORIGIN_ALIGN % align == 0
        off = self._size + LEAD_GUARD + lead
        off = (off + align - 1) // align * align + misalign
        span = ((planes - 1) * plane + inner) * isz
        end = off + span + max(LEAD_GUARD, tail_rows * ld * isz)
        end = (end + 15) // 16 * 16
        v = View(self, name, dtype, batch, M, N, ld, bstride, planes, plane, off, end)
        self.views.append(v)
        self._size = end
        return v

    def workspace(self, name, nbytes, align=256):
        """A workspace of exactly `nbytes` bytes (what the *_workspace_size function returned): a uint8 view [1, 1, 1, nbytes]."""
        return self.add(name, torch.uint8, 1, max(int(nbytes), 1), align=align, tail_rows=0)

    @property
    def bytes(self):
        if self._buf is None:
            raw = torch.full((self._size + _ORIGIN_ALIGN,), self.fill, dtype=torch.uint8, device=self.device)
            self._origin = (-raw.data_ptr()) % _ORIGIN_ALIGN          # view offsets count from a 4 KiB-aligned address
            self._raw, self._buf = raw, raw[self._origin:self._origin + self._size]
        return self._buf

    def allowed_mask(self, views=None):
        """uint8 [size]: non-zero at every byte of a logical element of `views` (default: all of the arena's)."""
        mask = torch.zeros((self._size,), dtype=torch.uint8, device=self.device)
        for v in (self.views if views is None else views):
            assert v.arena is self
            v._strided(mask, _SAME_SIZE_INT[v.isz]).fill_(-1 if v.isz > 1 else 255)
        return mask

    def describe(self, byte_off):
        """'view, plane, batch, row, col' of the view whose region (leading guard .. end of trailing guard) holds the byte."""
        prev_end = 0
        for v in self.views:
            if prev_end <= byte_off < v.end:
                p, b, r, c = v.locate(byte_off)
                return v.name, p, b, r, c
            prev_end = v.end
        raise AssertionError(f"byte {byte_off} outside the arena")


class GuardViolation(AssertionError):
    """.where = (view name, plane, batch, row, col) of the first byte written outside the logical outputs."""

    def __init__(self, msg, where, byte_off):
        super().__init__(msg)
        self.where, self.byte_off = where, byte_off


def assert_untouched(arena, views=None):
    """Every byte of `arena` outside the logical elements of `views` (default: all its views) still holds the fill value.  Exact."""
    buf = arena.bytes
    bad = (buf != arena.fill) & (arena.allowed_mask(views) == 0)
    n = int(bad.sum())
    if n:
        off = int(torch.nonzero(bad)[0, 0])
        name, p, b, r, c = arena.describe(off)
        v = next(x for x in arena.views if x.name == name)
        raise GuardViolation(f"{n} byte(s) outside the logical output were written; first at arena byte {off} (value 0x{int(buf[off]):02x}): "
                             f"view '{name}' plane {p} batch {b} row {r} col {c}  (logical: {v.planes} x {v.batch} x [{v.M}, {v.N}], ld {v.ld}, "
                             f"batch stride {v.bstride}, plane {v.plane})", (name, p, b, r, c), off)


def assert_close(got, ref, atol, rtol=0.0, what=""):
    """|got - ref| <= atol + rtol * |ref| element-wise in float64, and every element finite: a NaN (an 0xFF pad element that reached the
    result) is reported with its index, not swallowed by a comparison that is false for NaN."""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    nonfinite = ~torch.isfinite(got)
    if bool(nonfinite.any()):
        idx = tuple(int(i) for i in torch.nonzero(nonfinite)[0])
        raise AssertionError(f"{what}: {int(nonfinite.sum())} non-finite result element(s), first at {idx}: padding reached the result")
    excess = (got - ref).abs() - (atol + rtol * ref.abs())
    if bool((excess > 0).any()):
        idx = tuple(int(i) for i in torch.nonzero(excess == excess.max())[0])
        raise AssertionError(f"{what}: max |err| {float((got - ref).abs().max()):.3e} exceeds atol {atol:.3e} + rtol {rtol:.1e} |ref| at {idx} "
                             f"(got {float(got[idx])!r}, want {float(ref[idx])!r})")
    return float((got - ref).abs().max()) if got.numel() else 0.0


def assert_within(got, ref, bound, what=""):
    """|got - ref| <= bound element-wise (bound: a tensor of per-element error bounds) in float64, every element finite."""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    bound = torch.as_tensor(bound).detach().cpu().double().expand_as(ref)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    nonfinite = ~torch.isfinite(got)
    if bool(nonfinite.any()):
        idx = tuple(int(i) for i in torch.nonzero(nonfinite)[0])
        raise AssertionError(f"{what}: {int(nonfinite.sum())} non-finite result element(s), first at {idx}: padding reached the result")
    ratio = (got - ref).abs() / bound
    if bool((ratio > 1.0).any()):
        idx = tuple(int(i) for i in torch.nonzero(ratio == ratio.max())[0])
        raise AssertionError(f"{what}: |err| / bound = {float(ratio.max()):.3f} > 1 at {idx} (got {float(got[idx])!r}, want {float(ref[idx])!r}, "
                             f"bound {float(bound[idx]):.3e})")
    return float(ratio.max()) if got.numel() else 0.0


def assert_equal(got, ref, what=""):
    """Exact equality (integer, u8 and bit-exact float outputs), with the first differing index."""
    got, ref = torch.as_tensor(got).detach().cpu(), torch.as_tensor(ref).detach().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    ne = got != ref
    if got.is_floating_point():
        ne = ne & ~(torch.isnan(got) & torch.isnan(ref))
    if bool(ne.any()):
        idx = tuple(int(i) for i in torch.nonzero(ne)[0])
        raise AssertionError(f"{what}: {int(ne.sum())} element(s) differ, first at {idx}: got {got[idx].item()!r}, want {ref[idx].item()!r}")
