"""The image the device JPEG decoder makes, defined in NumPy: what zh_jpeg_decode (csrc/jpeg.hip over csrc/jpeg_codec.h) and
zh_jpeg_decode_host produce byte for byte, and what `Image.open(p).convert("RGB")` gives for the files it serves (Pillow on
libjpeg-turbo: integer arithmetic throughout, restated here from the public algorithms).

  served          SOF0 (baseline sequential Huffman), 8-bit samples, 8-bit quantisation tables, ONE interleaved scan over all components
                  with Ss, Se, Ah, Al = 0, 63, 0, 0; one component at sampling (1, 1), or three with luma (1, 1), (2, 1) or (2, 2), both
                  chroma (1, 1) on the same tables, a JFIF APP0 or component ids 1, 2, 3, no Adobe APP14; no DNL; every table defined;
                  the scan followed by EOI.  parse() returns None for everything else — progressive, arithmetic, 12-bit, CMYK / YCCK,
                  RGB-coded, multi-scan, other samplings, files that are no JPEG, anything it is unsure of — and the host decodes those.
  entropy         T.81 Huffman decoding, FF 00 unstuffed; the scan is cut at its RSTn markers into segments that decode independently
                  (the DC predictors start at 0 in each); coefficients de-zigzagged to natural order.
  inverse DCT     "islow": 13-bit constants, columns first descaled by 11 bits, rows by 18, + 128, clamped to 0 .. 255.
  cropping        a component's plane is cut to ceil(W h / hmax) x ceil(H v / vmax) samples BEFORE it is upsampled.
  upsampling      the "fancy" triangle filter, h2v1 and h2v2; a component whose cropped width is <= 2 is replicated instead.
  colour          YCbCr -> RGB in 16-bit fixed point, F(x) = int(x * 65536 + 0.5); a grey file gives Y three times.

pack() lays the descriptor arrays of one launch out (scan bytes, segment rows sorted by length, image rows, table sets deduplicated
across the batch, output offsets); table_set_bytes() is the ONE form of the canonical Huffman tables that decode_np, the host entry and
the kernel read.  chunk_rows() cuts the segments of a launch into the chunk rows of zh_jpeg_decode_split (decoder "device-split": a
scan without restart markers split among lanes; include/zutis_hip.h has the method), chunk_rows_np() is their definition byte by byte.
The second half of the module defines the ENCODER the same way: encode_np(), the baseline JPEG file zh_jpeg_encode's scans are framed
into, byte for byte Pillow's (its rules stand in front of it).  No torch at import.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import List, Optional, Sequence

import numpy as np

from . import _lib

_K = _lib.constants()
IMAGE_WORDS, SEGMENT_WORDS = _K["ZH_JPEG_IMAGE_WORDS"], _K["ZH_JPEG_SEGMENT_WORDS"]
TABLE_BYTES, TABLE_SET_BYTES = _K["ZH_JPEG_HUFF_TABLE_BYTES"], _K["ZH_JPEG_TABLE_SET_BYTES"]
MAX_TABLE_SETS, MAX_SEGMENTS = _K["ZH_JPEG_MAX_TABLE_SETS"], _K["ZH_JPEG_MAX_SEGMENTS"]
STATUS = {k[len("ZH_JPEG_STATUS_"):].lower(): v for k, v in _K.items() if k.startswith("ZH_JPEG_STATUS_")}
CHUNK_WORDS, CHUNK_BYTES, CHUNK_BYTES_MIN = _K["ZH_JPEG_CHUNK_WORDS"], _K["ZH_JPEG_CHUNK_BYTES"], _K["ZH_JPEG_CHUNK_BYTES_MIN"]
SPLIT_LANES, SPLIT_PASSES, MAX_CHUNKS = _K["ZH_JPEG_SPLIT_LANES"], _K["ZH_JPEG_SPLIT_PASSES"], _K["ZH_JPEG_MAX_CHUNKS"]
MAX_SEGMENT_BYTES = 2 ** 28                       # split decoding counts a segment's unstuffed BITS in int32
DECODERS = ("host", "device", "device-split")
ALIGN = 16                                        # byte alignment of an image inside the output (descriptors hold offset / 16)
_LOOK, _MAXCODE, _VALOFF, _VALS = 0, 512, 584, 656      # byte offsets inside one Huffman table: u16 [256], i32 [18], i32 [18], u8 [256]

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class DamagedScan(ValueError):
    """decode_np met entropy-coded data no decoder can follow; .status holds the codec's status bit."""

    def __init__(self, status: int, what: str):
        super().__init__(what)
        self.status = status


@dataclasses.dataclass(frozen=True)
class JpegPlan:
    """What parse() read from one file.  segments int64 [n, 3]: (first byte, end byte, first MCU) of every entropy segment, offsets
    into the file; quant int [2, 64] (luma, chroma) in natural order; huff: the four canonical tables (luma DC, luma AC, chroma DC,
    chroma AC) as (counts [16], values); a grey file's chroma entries are empty."""
    width: int
    height: int
    ncomp: int
    hs: int
    vs: int
    quant: np.ndarray
    huff: tuple
    restart_interval: int
    segments: np.ndarray

    @property
    def mcux(self):
        return -(-self.width // (8 * self.hs))

    @property
    def mcuy(self):
        return -(-self.height // (8 * self.vs))

    @property
    def n_mcus(self):
        return self.mcux * self.mcuy

    @property
    def blocks_per_mcu(self):
        return self.hs * self.vs + (2 if self.ncomp == 3 else 0)

    @property
    def n_blocks(self):
        return self.n_mcus * self.blocks_per_mcu


# ------------------------------------------------------------------------------------------------- tables
def huffman_table_bytes(counts, values) -> Optional[np.ndarray]:
    """u8 [TABLE_BYTES] of one canonical table (T.81 Annex C): look u16 [256] = (length << 8 | value) of the code that is a prefix of the
    8 bits, 0 when it is longer; maxcode i32 [18] (index = length, -1: no code of that length); valoff i32 [18] = index of the length's
    first value minus its first code; vals u8 [256].  None when the counts describe no prefix code.  No counts: all zero (no code).
    Cached: files written without optimised tables all carry the same four; the array is shared and read-only."""
    return _huffman_table(tuple(int(c) for c in counts), tuple(int(v) for v in values))


@functools.lru_cache(maxsize=4096)
def _huffman_table(counts: tuple, values: tuple) -> Optional[np.ndarray]:
    out = np.zeros(TABLE_BYTES, np.uint8)
    if len(counts) != 16 or sum(counts) != len(values) or len(values) > 256:
        return None
    look, maxcode, valoff = out[_LOOK:_MAXCODE].view("<u2"), out[_MAXCODE:_VALOFF].view("<i4"), out[_VALOFF:_VALS].view("<i4")
    maxcode[:] = -1
    code = k = 0
    for length in range(1, 17):
        n = counts[length - 1]
        if code + n > (1 << length):
            return None
        valoff[length] = k - code
        for j in range(n):
            if length <= 8:
                first = (code + j) << (8 - length)
                look[first:first + (1 << (8 - length))] = (length << 8) | values[k + j]
        k += n
        code += n
        if n:
            maxcode[length] = code - 1
        code <<= 1
    out[_VALS:_VALS + len(values)] = values
    out.setflags(write=False)
    return out


def table_set_bytes(plan: JpegPlan) -> bytes:
    """The file's table set as the codec reads it: four Huffman tables (luma DC, luma AC, chroma DC, chroma AC), then the two
    quantisation tables u16 [2, 64] in natural order."""
    parts = [huffman_table_bytes(c, v) for c, v in plan.huff]
    return b"".join(p.tobytes() for p in parts) + np.asarray(plan.quant, "<u2").tobytes()


# ------------------------------------------------------------------------------------------------- the file's markers
def _u16(d, at):
    return (d[at] << 8) | d[at + 1]


def parse(data) -> Optional[JpegPlan]:
    """The plan of one file's bytes, or None when the device does not serve it (module docstring)."""
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        return None
    quant, huff = {}, {}
    frame = None
    jfif = False
    ri = 0
    at = 2
    while True:
        if at + 4 > n or d[at] != 0xFF:
            return None
        while at < n and d[at] == 0xFF:                       # fill bytes in front of a marker
            at += 1
        if at >= n:
            return None
        m = d[at]
        at += 1
        if m in (0x00, 0x01, 0xD8, 0xD9) or 0xD0 <= m <= 0xD7:
            return None
        if at + 2 > n:
            return None
        L = _u16(d, at)
        if L < 2 or at + L > n:
            return None
        body = d[at + 2:at + L]
        if m == 0xE0:
            jfif = jfif or body[:5] == b"JFIF\x00"
        elif m == 0xEE:
            if body[:5] == b"Adobe":
                return None
        elif m == 0xDB:
            p = 0
            while p < len(body):
                pq, tq = body[p] >> 4, body[p] & 15
                if pq != 0 or tq > 3 or p + 65 > len(body):
                    return None
                q = np.zeros(64, np.int64)
                q[ZIGZAG] = np.frombuffer(body[p + 1:p + 65], np.uint8)
                quant[tq] = q
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(body):
                if p + 17 > len(body):
                    return None
                tc, th = body[p] >> 4, body[p] & 15
                counts = list(body[p + 1:p + 17])
                nv = sum(counts)
                if tc > 1 or th > 3 or nv > 256 or p + 17 + nv > len(body):
                    return None
                values = list(body[p + 17:p + 17 + nv])
                if huffman_table_bytes(counts, values) is None or (tc == 0 and any(v > 11 for v in values)):
                    return None
                huff[(tc, th)] = (counts, values)
                p += 17 + nv
        elif m == 0xC0:
            if frame is not None or len(body) < 6:
                return None
            nc = body[5]
            if body[0] != 8 or len(body) != 6 + 3 * nc or nc not in (1, 3):
                return None
            frame = (_u16(body, 1), _u16(body, 3), [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nc)])
        elif 0xC1 <= m <= 0xCF or m in (0xDC, 0xDE, 0xDF):     # other frame types, arithmetic conditioning, DNL, hierarchical
            return None
        elif m == 0xDD:
            if L != 4:
                return None
            ri = _u16(body, 0)
        elif m == 0xDA:
            break
        at += L
    # ---- the frame and the scan header
    if frame is None:
        return None
    H, W, comps = frame
    if H < 1 or W < 1:
        return None
    nc = len(comps)
    if len(body) != 4 + 2 * nc or body[0] != nc or tuple(body[1 + 2 * nc:]) != (0, 63, 0):
        return None
    sel = []
    for i, (cid, _, _, _) in enumerate(comps):
        if body[1 + 2 * i] != cid:
            return None
        sel.append((body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15))
    if nc == 1:
        if (comps[0][1], comps[0][2]) != (1, 1):
            return None
    else:
        if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            return None
        if not jfif and [c[0] for c in comps] != [1, 2, 3]:
            return None
        if comps[1][3] != comps[2][3] or sel[1] != sel[2]:      # both chroma on the same tables: a table set has two classes
            return None
    classes = [0] if nc == 1 else [0, 1]
    for cls in classes:
        tq, (td, ta) = comps[cls][3], sel[cls]
        if tq not in quant or (0, td) not in huff or (1, ta) not in huff:
            return None
    q2 = np.zeros((2, 64), np.int64)
    tables = []
    for cls in (0, 1):
        if cls in classes:
            q2[cls] = quant[comps[cls][3]]
            tables += [huff[(0, sel[cls][0])], huff[(1, sel[cls][1])]]
        else:
            tables += [([0] * 16, []), ([0] * 16, [])]
    hs, vs = comps[0][1], comps[0][2]
    n_mcus = -(-W // (8 * hs)) * -(-H // (8 * vs))
    # ---- the entropy segments: a vectorised search for FF xx with xx neither 00 (a stuffed byte) nor FF (fill)
    start = at + L
    a = np.frombuffer(d, np.uint8, n - start, start)
    ff = np.flatnonzero(a[:-1] == 0xFF) if a.size > 1 else np.zeros(0, np.int64)
    marks = ff[(a[ff + 1] != 0) & (a[ff + 1] != 0xFF)]
    codes = a[marks + 1]
    rst = (codes >= 0xD0) & (codes <= 0xD7)
    stop = np.flatnonzero(~rst)
    if stop.size == 0 or codes[stop[0]] != 0xD9:              # the scan is followed by EOI (no second scan, no DNL, no cut file)
        return None
    k = int(stop[0])
    if not np.array_equal(codes[:k], 0xD0 + (np.arange(k) & 7)) or (k and not ri):
        return None
    lo = np.concatenate(([0], marks[:k] + 2))
    hi = marks[:k + 1].copy()
    for i in range(k + 1):                                    # fill bytes in front of a marker are not data
        while hi[i] > lo[i] and a[hi[i] - 1] == 0xFF:
            hi[i] -= 1
    segs = np.stack([lo + start, hi + start, np.arange(k + 1) * (ri if ri else 0)], axis=1).astype(np.int64)
    return JpegPlan(W, H, nc, hs, vs, q2, tuple((tuple(c), tuple(v)) for c, v in tables), ri, segs)


# ------------------------------------------------------------------------------------------------- entropy decoding
class _Bits:
    """The bits of one segment, FF 00 unstuffed; reading past the end or meeting a marker is DamagedScan."""

    def __init__(self, seg: bytes):
        a = np.frombuffer(seg, np.uint8)
        ff = np.flatnonzero(a == 0xFF)
        if ff.size and (ff[-1] == a.size - 1 or (a[ff + 1] != 0).any()):       # every FF of a segment is followed by its stuffed 00
            raise DamagedScan(STATUS["marker"], "a marker inside an entropy segment")
        seg = seg.replace(b"\xff\x00", b"\xff")
        self.total = 8 * len(seg)
        self.value = int.from_bytes(seg + b"\x00\x00\x00\x00", "big")
        self.pos = 0

    def peek16(self):
        return (self.value >> (self.total + 32 - self.pos - 16)) & 0xFFFF

    def take(self, nbits):
        v = (self.value >> (self.total + 32 - self.pos - nbits)) & ((1 << nbits) - 1) if nbits else 0
        self.pos += nbits
        if self.pos > self.total:
            raise DamagedScan(STATUS["truncated"], "the entropy segment ends inside a symbol")
        return v


def _symbol(bits: _Bits, table):
    look, maxcode, valoff, vals = table
    peek = bits.peek16()
    e = look[peek >> 8]
    if e:
        bits.take(e >> 8)
        return e & 255
    for length in range(9, 17):
        code = peek >> (16 - length)
        if code <= maxcode[length]:
            bits.take(length)
            return vals[(code + valoff[length]) & 255]
    raise DamagedScan(STATUS["code"], "an undefined Huffman code")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _tables_of(set_bytes: bytes):
    out = []
    for t in range(4):
        b = np.frombuffer(set_bytes, np.uint8, TABLE_BYTES, t * TABLE_BYTES)
        out.append((b[_LOOK:_MAXCODE].view("<u2").tolist(), b[_MAXCODE:_VALOFF].view("<i4").tolist(), b[_VALOFF:_VALS].view("<i4").tolist(),
                    b[_VALS:].tolist()))
    return out


def decode_coefficients(plan: JpegPlan, data) -> np.ndarray:
    """int16 [n_blocks, 64]: the quantised coefficients of every block in natural order, blocks in scan order (MCU by MCU, inside an MCU
    the luma blocks row by row, then Cb, Cr)."""
    d = bytes(data)
    tables = _tables_of(table_set_bytes(plan))
    bpm, lum = plan.blocks_per_mcu, plan.hs * plan.vs
    coef = np.zeros((plan.n_blocks, 64), np.int64)
    zz = ZIGZAG.tolist()
    done = 0
    for lo, hi, first in plan.segments.tolist():
        if first < 0 or first >= plan.n_mcus or (plan.restart_interval == 0 and first != 0):
            raise DamagedScan(STATUS["segment"], "an entropy segment outside the image")
        count = min(plan.restart_interval, plan.n_mcus - first) if plan.restart_interval else plan.n_mcus
        bits = _Bits(d[lo:hi])
        pred = [0, 0, 0]
        for mcu in range(first, first + count):
            for b in range(bpm):
                comp = 0 if b < lum else b - lum + 1
                cls = 1 if comp else 0
                row = coef[mcu * bpm + b]
                s = _symbol(bits, tables[2 * cls])
                if s > 11:
                    raise DamagedScan(STATUS["bits"], "a DC category above 11")
                pred[comp] += _extend(bits.take(s), s)
                row[0] = pred[comp]
                k = 1
                while k < 64:
                    rs = _symbol(bits, tables[2 * cls + 1])
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        k += 16
                        if k > 64:
                            raise DamagedScan(STATUS["index"], "a zero run past coefficient 63")
                        continue
                    if s > 10:
                        raise DamagedScan(STATUS["bits"], "an AC category above 10")
                    k += r
                    if k > 63:
                        raise DamagedScan(STATUS["index"], "a coefficient index past 63")
                    row[zz[k]] = _extend(bits.take(s), s)
                    k += 1
        done += count
    if done != plan.n_mcus:
        raise DamagedScan(STATUS["incomplete"], "the entropy segments do not cover the image's MCUs")
    return coef.astype(np.int16)


# ------------------------------------------------------------------------------------------------- pixels
def _idct_pass(x, shift):
    """One pass of the islow inverse DCT over axis -2 of int64 [..., 8, n] -> the same shape, descaled by `shift` bits with rounding."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (x[..., k, :] for k in range(8))
    z1 = (i2 + i6) * 4433
    t2 = z1 - i6 * 15137
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], axis=-2)
    return (out + (1 << (shift - 1))) >> shift


def idct_blocks(coef: np.ndarray, q: np.ndarray) -> np.ndarray:
    """u8 [n, 8, 8] samples of int [n, 64] quantised coefficients under the quantisation table q [64] (both in natural order)."""
    x = (coef.astype(np.int64) * q.astype(np.int64)).reshape(-1, 8, 8)
    w = _idct_pass(x, 11)                                     # columns: index [n, v, x] -> [n, y, x]
    r = _idct_pass(w.transpose(0, 2, 1), 18).transpose(0, 2, 1)      # rows
    return np.clip(r + 128, 0, 255).astype(np.uint8)


def _h2v1(s):
    ch, cw = s.shape
    s = s.astype(np.int64)
    out = np.empty((ch, 2 * cw), np.int64)
    left, right = np.concatenate((s[:, :1], s[:, :-1]), 1), np.concatenate((s[:, 1:], s[:, -1:]), 1)
    out[:, 0::2] = (3 * s + left + 1) >> 2
    out[:, 1::2] = (3 * s + right + 2) >> 2
    out[:, 0], out[:, -1] = s[:, 0], s[:, -1]
    return out


def _h2v2(s):
    ch, cw = s.shape
    s = s.astype(np.int64)
    above, below = np.concatenate((s[:1], s[:-1]), 0), np.concatenate((s[1:], s[-1:]), 0)
    out = np.empty((2 * ch, 2 * cw), np.int64)
    for v, nb in ((0, above), (1, below)):
        cs = 3 * s + nb
        left, right = np.concatenate((cs[:, :1], cs[:, :-1]), 1), np.concatenate((cs[:, 1:], cs[:, -1:]), 1)
        even, odd = (3 * cs + left + 8) >> 4, (3 * cs + right + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * cs[:, 0] + 8) >> 4, (4 * cs[:, -1] + 7) >> 4
        out[v::2, 0::2], out[v::2, 1::2] = even, odd
    return out


def _upsample(s, hs, vs, W, H):
    """The cropped chroma plane s at the image's size."""
    if (hs, vs) == (1, 1):
        return s.astype(np.int64)
    if s.shape[1] <= 2:
        up = np.repeat(np.repeat(s, vs, 0), hs, 1).astype(np.int64)
    else:
        up = _h2v1(s) if vs == 1 else _h2v2(s)
    return up[:H, :W]


def _fix(x):
    return int(x * 65536 + 0.5)


def pixels_of(plan: JpegPlan, coef: np.ndarray) -> np.ndarray:
    """u8 [H, W, 3] from the coefficients of decode_coefficients."""
    W, H, hs, vs = plan.width, plan.height, plan.hs, plan.vs
    bpm, lum = plan.blocks_per_mcu, hs * vs
    per_mcu = coef.reshape(plan.mcuy, plan.mcux, bpm, 64)

    def plane(first, h, v, q):
        px = idct_blocks(per_mcu[:, :, first:first + h * v].reshape(-1, 64), q).reshape(plan.mcuy, plan.mcux, v, h, 8, 8)
        return px.transpose(0, 2, 4, 1, 3, 5).reshape(plan.mcuy * v * 8, plan.mcux * h * 8)

    y = plane(0, hs, vs, plan.quant[0])[:H, :W].astype(np.int64)
    if plan.ncomp == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    cw, ch = -(-W // hs), -(-H // vs)
    cb = _upsample(plane(lum, 1, 1, plan.quant[1])[:ch, :cw], hs, vs, W, H) - 128
    cr = _upsample(plane(lum + 1, 1, 1, plan.quant[1])[:ch, :cw], hs, vs, W, H) - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], 2), 0, 255).astype(np.uint8)


def decode_np(data, plan: Optional[JpegPlan] = None) -> np.ndarray:
    """u8 [H, W, 3]: the definition.  ValueError for a file parse() does not serve, DamagedScan for a scan no decoder can follow."""
    plan = parse(data) if plan is None else plan
    if plan is None:
        raise ValueError("jpeg_device.decode_np: not a file the device decoder serves")
    return pixels_of(plan, decode_coefficients(plan, data))


# ------------------------------------------------------------------------------------------------- one launch
@dataclasses.dataclass
class Packed:
    """The flat arrays of one launch (include/zutis_hip.h, zh_jpeg_decode): scan u8 [scan_bytes]; segments int32 [S, 4] = (image, first
    byte, end byte, first MCU), longest first; images int32 [B, 12]; tables u8 [n_sets, TABLE_SET_BYTES]; out_off int64 [B] (bytes,
    multiples of 16) and out_bytes; n_blocks: 8 x 8 blocks of the whole batch (the workspace's size)."""
    scan: np.ndarray
    segments: np.ndarray
    images: np.ndarray
    tables: np.ndarray
    out_off: np.ndarray
    out_bytes: int
    n_blocks: int
    shapes: List[tuple]
    max_image_blocks: int = 1        # the largest image's blocks and pixels: the widths of the pixel stage's grids
    max_image_pixels: int = 1
    kept: Optional[List[int]] = None      # positions, in pack()'s argument lists, of the images these arrays describe (all, unless skip_overflow)
    chunks: Optional[np.ndarray] = None   # pack(chunk_bytes=...): int32 [C, 4], the chunk rows of zh_jpeg_decode_split (chunk_rows)
    chunk_bytes: Optional[int] = None


def pack(plans: Sequence[JpegPlan], datas: Sequence, out_off: Optional[Sequence[int]] = None, out_bytes: Optional[int] = None,
         skip_overflow: bool = False, chunk_bytes: Optional[int] = None) -> Packed:
    """The descriptor arrays of one launch over `plans` (of the files `datas`).  out_off: where each image's [H, W, 3] bytes go (default:
    back to back, aligned to 16).  More than MAX_TABLE_SETS distinct table sets is a ValueError — or, with skip_overflow, the images
    that would bring a set past the limit are left out (Packed.kept lists the others: the caller leaves the rest to the host); more
    than MAX_SEGMENTS segments is a ValueError.  chunk_bytes: also the chunk rows of zh_jpeg_decode_split (Packed.chunks); an image
    with a segment of MAX_SEGMENT_BYTES or more is then treated as one that brings a table set too many."""
    sets, set_index, kept = {}, [], []
    for i, p in enumerate(plans):
        if chunk_bytes is not None and len(p.segments) and int((p.segments[:, 1] - p.segments[:, 0]).max()) >= MAX_SEGMENT_BYTES:
            if not skip_overflow:
                raise ValueError(f"jpeg_device.pack: an entropy segment of {MAX_SEGMENT_BYTES} bytes or more cannot be split into chunks")
            continue
        key = table_set_bytes(p)
        if key not in sets and len(sets) == MAX_TABLE_SETS:
            if not skip_overflow:
                raise ValueError(f"jpeg_device.pack: more than {MAX_TABLE_SETS} distinct table sets in one launch")
            continue
        set_index.append(sets.setdefault(key, len(sets)))
        kept.append(i)
    if out_off is not None:
        out_off = [out_off[i] for i in kept]
    plans, datas = [plans[i] for i in kept], [datas[i] for i in kept]
    B = len(plans)
    if out_off is None:
        sizes = [-(-3 * p.width * p.height // ALIGN) * ALIGN for p in plans]
        out_off = np.concatenate(([0], np.cumsum(sizes)))[:-1] if B else np.zeros(0)
        out_bytes = int(sum(sizes))
    out_off = np.asarray(out_off, np.int64).reshape(B)
    if (out_off % ALIGN).any():
        raise ValueError("jpeg_device.pack: output offsets are multiples of 16")
    images = np.zeros((B, IMAGE_WORDS), np.int32)
    chunks, rows, at, blocks = [], [], 0, 0
    for b, (p, d) in enumerate(zip(plans, datas)):
        d = np.frombuffer(bytes(d) if not isinstance(d, np.ndarray) else d, np.uint8)
        images[b] = (p.width, p.height, p.ncomp, p.hs, p.vs, p.mcux, p.mcuy, set_index[b], blocks, out_off[b] // ALIGN, p.restart_interval, 0)
        blocks += p.n_blocks
        for lo, hi, first in p.segments.tolist():
            chunks.append(d[lo:hi])
            rows.append((b, at, at + hi - lo, first))
            at += hi - lo
    if len(rows) > MAX_SEGMENTS or at >= 2 ** 31 or blocks >= 2 ** 24:
        raise ValueError(f"jpeg_device.pack: {len(rows)} segments / {at} scan bytes / {blocks} blocks exceed one launch")
    segments = np.asarray(rows, np.int32).reshape(-1, SEGMENT_WORDS)
    order = np.argsort(-(segments[:, 2] - segments[:, 1]), kind="stable")       # a wave's lanes finish together
    scan = np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)
    tables = np.frombuffer(b"".join(sets), np.uint8).reshape(len(sets), TABLE_SET_BYTES).copy() if sets else np.zeros((0, TABLE_SET_BYTES), np.uint8)
    packed = Packed(np.ascontiguousarray(scan), np.ascontiguousarray(segments[order]), images, tables, out_off, int(out_bytes), blocks,
                    [(p.height, p.width) for p in plans], max([p.n_blocks for p in plans], default=1), max([p.width * p.height for p in plans], default=1), kept)
    if chunk_bytes is not None:
        packed.chunks, packed.chunk_bytes = chunk_rows(packed, chunk_bytes), int(chunk_bytes)
    return packed


def _check_chunk_bytes(chunk_bytes) -> int:
    cb = int(chunk_bytes)
    if cb != chunk_bytes or cb < CHUNK_BYTES_MIN or cb > 4096 or cb % 16:
        raise ValueError(f"jpeg_device: chunk_bytes {chunk_bytes!r} is not a multiple of 16 in {CHUNK_BYTES_MIN} .. 4096")
    return cb


def chunk_rows(packed: Packed, chunk_bytes: int = CHUNK_BYTES) -> np.ndarray:
    """int32 [C, CHUNK_WORDS] = (segment row, first byte, unstuffed bits of the segment in front of it, 1 for a segment's first chunk):
    every segment [lo, hi) of packed.segments cut every chunk_bytes bytes, segment after segment in the order of the rows; a cut that
    falls on the 00 of an FF 00 pair moves behind it; a segment without bytes has one chunk.  The stuffed bytes are those of an FF 00
    pair that lies inside one segment.  Vectorised: one search of the stuffed bytes against the cuts."""
    cb = _check_chunk_bytes(chunk_bytes)
    seg = packed.segments.astype(np.int64).reshape(-1, SEGMENT_WORDS)
    lo, hi = seg[:, 1], seg[:, 2]
    n = np.maximum(1, -(-(hi - lo) // cb))
    total = int(n.sum())
    if total > MAX_CHUNKS:
        raise ValueError(f"jpeg_device.chunk_rows: {total} chunks exceed one launch ({MAX_CHUNKS})")
    row = np.repeat(np.arange(len(seg)), n)
    j = np.arange(total) - np.repeat(np.cumsum(n) - n, n)
    start = lo[row] + cb * j
    scan = packed.scan
    ff = np.flatnonzero(scan[:-1] == 0xFF) if scan.size > 1 else np.zeros(0, np.int64)
    zeros = ff[scan[ff + 1] == 0] + 1
    stuffed = np.zeros(scan.size + 1, bool)
    stuffed[zeros] = True
    stuffed[lo] = False                                     # an FF that ends a segment in front of a 00 that begins the next is no pair
    zeros = zeros[stuffed[zeros]]
    start = start + stuffed[start]
    ubits = 8 * ((start - lo[row]) - (np.searchsorted(zeros, start) - np.searchsorted(zeros, lo[row])))
    return np.ascontiguousarray(np.stack([row, start, ubits, j == 0], axis=1).astype(np.int32))


def chunk_rows_np(packed: Packed, chunk_bytes: int = CHUNK_BYTES) -> np.ndarray:
    """chunk_rows, defined byte by byte (plain loops; the tests compare the two)."""
    cb = _check_chunk_bytes(chunk_bytes)
    scan, rows = packed.scan.tolist(), []
    for r, (_, lo, hi, _) in enumerate(packed.segments.tolist()):
        stuffed = [q > lo and scan[q] == 0 and scan[q - 1] == 0xFF for q in range(lo, hi)]
        for j in range(max(1, -(-(hi - lo) // cb))):
            start = lo + cb * j
            if start < hi and stuffed[start - lo]:
                start += 1
            rows.append((r, start, 8 * (start - lo - sum(stuffed[:start - lo])), int(j == 0)))
    return np.asarray(rows, np.int32).reshape(-1, CHUNK_WORDS)


def sequences(packed: Packed) -> int:
    """The sequences (workgroups of SPLIT_LANES chunk rows) of a launch: as many passes always reach every true state."""
    return max(1, -(-len(packed.chunks) // SPLIT_LANES))


def unpack(packed: Packed, out: np.ndarray) -> List[np.ndarray]:
    """The images u8 [H, W, 3] of a launch's flat output."""
    return [out[o:o + 3 * h * w].reshape(h, w, 3) for o, (h, w) in zip(packed.out_off.tolist(), packed.shapes)]


def decode_host(packed: Packed):
    """zh_jpeg_decode_host over a launch's arrays: (images, status int32 [B]).  The CPU twin of zh_jpeg_decode: same codec, same
    arithmetic, no GPU."""
    import ctypes as C
    lib = _lib.load(raw=True)
    B = len(packed.shapes)
    out = np.zeros(max(packed.out_bytes, 1), np.uint8)
    status = np.zeros(max(B, 1), np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = lib.zh_jpeg_decode_host(ptr(packed.scan), packed.scan.size, ptr(packed.segments), len(packed.segments), ptr(packed.images), B,
                                 ptr(packed.tables), len(packed.tables), packed.n_blocks, ptr(out), packed.out_bytes, ptr(status))
    _lib.check(rc, "zh_jpeg_decode_host")
    return unpack(packed, out), status[:B]


def decode_split_host(packed: Packed, chunk_bytes: Optional[int] = None, passes: int = SPLIT_PASSES):
    """zh_jpeg_decode_split_host over a launch's arrays: (images, status int32 [B]).  The CPU twin of zh_jpeg_decode_split.  The chunk
    rows are packed.chunks (pack(chunk_bytes=...)) when chunk_bytes is None or theirs, chunk_rows(packed, chunk_bytes) otherwise."""
    import ctypes as C
    lib = _lib.load(raw=True)
    if packed.chunks is not None and chunk_bytes in (None, packed.chunk_bytes):
        chunks, cb = packed.chunks, packed.chunk_bytes
    else:
        cb = CHUNK_BYTES if chunk_bytes is None else chunk_bytes
        chunks = chunk_rows(packed, cb)
    B = len(packed.shapes)
    out = np.zeros(max(packed.out_bytes, 1), np.uint8)
    status = np.zeros(max(B, 1), np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = lib.zh_jpeg_decode_split_host(ptr(packed.scan), packed.scan.size, ptr(packed.segments), len(packed.segments), ptr(chunks), len(chunks), int(cb),
                                       int(passes), ptr(packed.images), B, ptr(packed.tables), len(packed.tables), packed.n_blocks, ptr(out),
                                       packed.out_bytes, ptr(status))
    _lib.check(rc, "zh_jpeg_decode_split_host")
    return unpack(packed, out), status[:B]


def check_decoder(name: str, decoder) -> str:
    if decoder not in DECODERS:
        raise ValueError(f"{name}: decoder {decoder!r} is not \"host\", \"device\" or \"device-split\"")
    return decoder


# ---- the encoder: the baseline JPEG zh_jpeg_encode (csrc/jpeg_enc.hip over csrc/jpeg_codec.h) and zh_jpeg_encode_host write, defined in
# NumPy.  encode_np(a, q, s, r) is byte for byte what Pillow (libjpeg-turbo) writes for Image.fromarray(a).save(f, "JPEG", quality=q,
# subsampling=0 | 2, restart_marker_blocks=r); restated from the public algorithms like the decoder above.
#   quantisation    the Annex K tables scaled by libjpeg's rule (quant_tables)
#   colour          RGB -> YCbCr in 16-bit fixed point, F(x) = int(x * 65536 + 0.5); the chroma rounding constant is 32767, not 32768
#   edges           luma (and 4:4:4 chroma) edge-replicated to the MCU grid; 4:2:0 chroma: the full-resolution plane replicated to even
#                   rows and 16-multiple columns, downsampled, and the last DOWNSAMPLED row replicated down to the 8-multiple
#   h2v2            (a + b + c + d + bias) >> 2, bias 1 on even output columns and 2 on odd ones
#   forward DCT     samples - 128, "islow": 13-bit constants, rows first (scaled up by 2 bits), then columns: 8 x the coefficient
#   quantise        sign(c) * ((|c| + (8 q >> 1)) // (8 q))
#   dummy blocks    a luma block of an MCU outside the component's ceil(H / 8) x ceil(W / 8) real blocks is not transformed: AC = 0, DC =
#                   that of the block before it in its block row of the MCU (right edge) or of the last block of the MCU's previous block
#                   row (a dummy row)
#   entropy         DC category + extra bits (prediction 0 at every restart), AC run / size with ZRL only in front of a nonzero
#                   coefficient, EOB unless coefficient 63 is nonzero; codes from the most significant bit; the last byte of an interval
#                   padded with 1-bits; FF stuffed as FF 00; RSTn (n mod 8) behind every interval but the last
#   header          SOI, APP0 (JFIF 1.01, units 0, density 1 x 1), DQT x 2, SOF0, DHT x 4, DRI (always), SOS
ENC_INTERVAL_MCUS, ENC_BLOCK_BYTES, ENC_SLOT_EXTRA = _K["ZH_JPEG_ENC_INTERVAL_MCUS"], _K["ZH_JPEG_ENC_BLOCK_BYTES"], _K["ZH_JPEG_ENC_SLOT_EXTRA"]
ENCODERS = ("host", "device")
SUBSAMPLINGS = {"4:4:4": 0, "4:2:0": 2}                # name -> Pillow's (and zh_jpeg_encode's) code
OVERLAY_FORMATS = ("png", "jpeg")

_ANNEX_K_QUANT = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66] + [99] * 38])
# Annex K.3: (codes of each length 1 .. 16, values) of luma DC, luma AC, chroma DC, chroma AC
ANNEX_K_HUFF = (
    ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), bytes(range(12))),
    ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
        "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
        "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")),
    ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), bytes(range(12))),
    ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119), bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43444546474849"
        "4a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
        "c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")),
)


def check_encode_args(name: str, quality, subsampling, interval_mcus=ENC_INTERVAL_MCUS) -> int:
    """Pillow's code of `subsampling` after the checks every encoder entry shares: ValueError naming the argument."""
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError(f"{name}: jpeg_quality {quality!r} is not an integer in 1 .. 100")
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"{name}: jpeg_subsampling {subsampling!r} is not one of {sorted(SUBSAMPLINGS)}")
    if isinstance(interval_mcus, bool) or not isinstance(interval_mcus, (int, np.integer)) or not 1 <= interval_mcus <= 65535:
        raise ValueError(f"{name}: interval_mcus {interval_mcus!r} is not an integer in 1 .. 65535")
    return SUBSAMPLINGS[subsampling]


def check_encoder(name: str, jpeg_encoder) -> str:
    if jpeg_encoder not in ENCODERS:
        raise ValueError(f"{name}: jpeg_encoder {jpeg_encoder!r} is not \"host\" or \"device\"")
    return jpeg_encoder


def check_overlay_format(name: str, overlay_format) -> str:
    if overlay_format not in OVERLAY_FORMATS:
        raise ValueError(f"{name}: overlay_format {overlay_format!r} is not \"png\" or \"jpeg\"")
    return overlay_format


def quant_tables(quality: int) -> np.ndarray:
    """int [2, 64] (luma, chroma) in natural order: Annex K scaled by s = 5000 // q below 50, 200 - 2 q from there; (t s + 50) // 100 in 1 .. 255."""
    check_encode_args("jpeg_device.quant_tables", quality, "4:4:4")
    s = 5000 // int(quality) if quality < 50 else 200 - 2 * int(quality)
    return np.clip((_ANNEX_K_QUANT * s + 50) // 100, 1, 255)


@functools.lru_cache(maxsize=None)
def _encode_tables():
    """(code, length) int64 [256] by symbol of the four Annex K tables: the canonical codes of T.81 Annex C."""
    out = []
    for counts, values in ANNEX_K_HUFF:
        code, length, c, k = np.zeros(256, np.int64), np.zeros(256, np.int64), 0, 0
        for n, count in enumerate(counts, 1):
            for _ in range(count):
                code[values[k]], length[values[k]] = c, n
                c, k = c + 1, k + 1
            c <<= 1
        out.append((code, length))
    return tuple(out)


def _geometry(H: int, W: int, sub: int):
    hs = 2 if sub == 2 else 1
    return hs, -(-W // (8 * hs)), -(-H // (8 * hs))              # luma blocks per MCU side, MCUs per row, MCU rows


def header_bytes(H: int, W: int, quality: int = 90, subsampling: str = "4:2:0", interval_mcus: int = ENC_INTERVAL_MCUS) -> bytes:
    """Everything in front of the scan: SOI, APP0, DQT (luma), DQT (chroma), SOF0, DHT x 4, DRI, SOS."""
    sub = check_encode_args("jpeg_device.header_bytes", quality, subsampling, interval_mcus)
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"jpeg_device.header_bytes: a JPEG of {H} x {W} pixels")
    seg = lambda marker, body: bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body  # noqa: E731
    q = quant_tables(quality)
    out = [b"\xff\xd8", seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    out += [seg(0xDB, bytes([i]) + bytes(int(v) for v in q[i][ZIGZAG])) for i in range(2)]
    out.append(seg(0xC0, bytes([8]) + int(H).to_bytes(2, "big") + int(W).to_bytes(2, "big") + bytes([3, 1, 0x22 if sub == 2 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])))
    out += [seg(0xC4, bytes([cls]) + bytes(counts) + values) for cls, (counts, values) in zip((0x00, 0x10, 0x01, 0x11), ANNEX_K_HUFF)]
    out.append(seg(0xDD, int(interval_mcus).to_bytes(2, "big")))
    out.append(seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


def _fdct_pass(d, first: bool):
    """One pass of the islow forward DCT over the last axis of int64 [..., 8]."""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    shift = 11 if first else 15
    desc = lambda x, n: (x + (1 << (n - 1))) >> n  # noqa: E731
    out = np.empty_like(d)
    out[..., 0] = (t10 + t11) << 2 if first else desc(t10 + t11, 2)
    out[..., 4] = (t10 - t11) << 2 if first else desc(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[..., 2] = desc(z1 + t13 * 6270, shift)
    out[..., 6] = desc(z1 - t12 * 15137, shift)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[..., 7], out[..., 5], out[..., 3], out[..., 1] = desc(t4 + z1 + z3, shift), desc(t5 + z2 + z4, shift), desc(t6 + z2 + z3, shift), desc(t7 + z1 + z4, shift)
    return out


def _plane_blocks(plane: np.ndarray, q: np.ndarray) -> np.ndarray:
    """The quantised coefficients int64 [rows / 8, cols / 8, 64] in zig-zag order of a sample plane whose sides are multiples of 8."""
    R, Cc = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.astype(np.int64).reshape(R, 8, Cc, 8).transpose(0, 2, 1, 3) - 128
    c = _fdct_pass(_fdct_pass(d, True).swapaxes(-1, -2), False).swapaxes(-1, -2).reshape(R, Cc, 64)
    q8 = 8 * q.astype(np.int64)
    return (np.sign(c) * ((np.abs(c) + (q8 >> 1)) // q8))[..., ZIGZAG]


def encode_coefficients(image_u8: np.ndarray, quality: int = 90, subsampling: str = "4:2:0") -> np.ndarray:
    """The quantised coefficients of the image's JPEG: int16 [MCUs * blocks per MCU, 64], blocks in scan order, each in zig-zag order."""
    sub = check_encode_args("jpeg_device.encode_coefficients", quality, subsampling)
    a = np.asarray(image_u8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or not (1 <= a.shape[0] <= 65535 and 1 <= a.shape[1] <= 65535):
        raise ValueError(f"jpeg_device: a u8 image [H, W, 3] with 1 <= H, W <= 65535 expected, got {a.dtype} {a.shape}")
    H, W = a.shape[:2]
    hs, mcux, mcuy = _geometry(H, W, sub)
    q = quant_tables(quality)
    r, g, b = (a[..., i].astype(np.int64) for i in range(3))
    y = (_fix(0.299) * r + _fix(0.587) * g + _fix(0.114) * b + 32768) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(0.5) * r - _fix(0.41869) * g - _fix(0.08131) * b + (128 << 16) + 32767) >> 16
    edge = lambda p, rows, cols: np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")  # noqa: E731
    yb = _plane_blocks(edge(y, mcuy * 8 * hs, mcux * 8 * hs), q[0]).reshape(mcuy, hs, mcux, hs, 64).transpose(0, 2, 1, 3, 4).copy()
    rows, cols = -(-H // 8), -(-W // 8)
    for by in range(hs):                                           # the dummy blocks, in the order libjpeg fills an MCU
        for bx in range(hs):
            dummy = ((np.arange(mcuy) * hs + by >= rows)[:, None] | (np.arange(mcux) * hs + bx >= cols)[None, :])
            if by == 0 and bx == 0:
                continue
            row_real = (np.arange(mcuy) * hs + by < rows)[:, None] & np.ones((1, mcux), bool)
            src = np.where(row_real, yb[:, :, by, bx - 1, 0], yb[:, :, by - 1, hs - 1, 0])
            yb[:, :, by, bx, 1:] = np.where(dummy[..., None], 0, yb[:, :, by, bx, 1:])
            yb[:, :, by, bx, 0] = np.where(dummy, src, yb[:, :, by, bx, 0])
    chroma = []
    for p in (cb, cr):
        if sub == 2:
            f = edge(p, H + (H & 1), mcux * 16)
            bias = np.where(np.arange(mcux * 8) % 2 == 0, 1, 2)
            p = (f[0::2, 0::2] + f[0::2, 1::2] + f[1::2, 0::2] + f[1::2, 1::2] + bias) >> 2
        chroma.append(_plane_blocks(edge(p, mcuy * 8, mcux * 8), q[1]))
    out = np.concatenate([yb.reshape(mcuy, mcux, hs * hs, 64), chroma[0][:, :, None], chroma[1][:, :, None]], 2)
    return out.reshape(-1, 64).astype(np.int16)


def scan_of_blocks(blocks: np.ndarray, subsampling: str = "4:2:0", interval_mcus: int = ENC_INTERVAL_MCUS) -> bytes:
    """The entropy-coded bytes of int16 [n, 64] zig-zag blocks in scan order (n a multiple of the blocks per MCU: 3 or 6): what
    scan_np makes of encode_coefficients(); category and bound edges are tested through here.  DC in -2047 .. 2047 apart from its
    predecessor's, AC in -1023 .. 1023."""
    sub = check_encode_args("jpeg_device.scan_of_blocks", 90, subsampling, interval_mcus)
    c = np.asarray(blocks).astype(np.int64).reshape(-1, 64)
    bpm = 6 if sub == 2 else 3
    n = c.shape[0]
    if n == 0 or n % bpm:
        raise ValueError(f"jpeg_device.scan_of_blocks: {n} blocks are not whole MCUs of {bpm}")
    idx = np.arange(n)
    interval, j = (idx // bpm) // int(interval_mcus), idx % bpm
    comp = np.where(j < bpm - 2, 0, j - (bpm - 3))
    diff = c[:, 0].copy()
    for k in range(3):                                             # the DC differences per component, 0 predicted at every restart
        sel = np.flatnonzero(comp == k)
        prev = np.concatenate([[0], c[sel[:-1], 0]])
        prev[np.concatenate([[True], interval[sel[1:]] != interval[sel[:-1]]])] = 0
        diff[sel] = c[sel, 0] - prev
    size = lambda v: np.where(v == 0, 0, np.floor(np.log2(np.maximum(np.abs(v), 1))).astype(np.int64) + 1)  # noqa: E731
    extra = lambda v, s: np.where(v < 0, v + (1 << s) - 1, v)  # noqa: E731
    if np.abs(diff).max() > 2047 or np.abs(c[:, 1:]).max(initial=0) > 1023:
        raise ValueError("jpeg_device.scan_of_blocks: a coefficient outside the baseline categories")
    tables = _encode_tables()
    chroma = comp != 0
    # tokens [n, 65, 4]: slot 0 the DC symbol, slot k the AC coefficient k (up to three ZRLs in front of its symbol), slot 64 the EOB
    val, bits = np.zeros((n, 65, 4), np.int64), np.zeros((n, 65, 4), np.int64)
    s = size(diff)
    code, length = (np.where(chroma, tables[2][i][s], tables[0][i][s]) for i in range(2))
    val[:, 0, 3], bits[:, 0, 3] = (code << s) | extra(diff, s), length + s
    ac = c[:, 1:]
    nz = ac != 0
    k = np.arange(1, 64)[None, :]
    last = np.maximum.accumulate(np.where(nz, k, 0), axis=1)
    run = k - np.concatenate([np.zeros((n, 1), np.int64), last[:, :-1]], 1) - 1
    s = size(ac)
    sym = np.where(nz, ((run & 15) << 4) | s, 0)
    ch = chroma[:, None]
    code, length = (np.where(ch, tables[3][i][sym], tables[1][i][sym]) for i in range(2))
    val[:, 1:64, 3], bits[:, 1:64, 3] = np.where(nz, (code << s) | extra(ac, s), 0), np.where(nz, length + s, 0)
    zrl_code, zrl_len = (np.where(ch, tables[3][i][0xF0], tables[1][i][0xF0]) for i in range(2))
    for z in range(3):
        need = nz & ((run >> 4) > z)
        val[:, 1:64, 2 - z], bits[:, 1:64, 2 - z] = np.where(need, zrl_code, 0), np.where(need, zrl_len, 0)
    eob = c[:, 63] == 0
    val[:, 64, 3] = np.where(eob, np.where(chroma, tables[3][0][0], tables[1][0][0]), 0)
    bits[:, 64, 3] = np.where(eob, np.where(chroma, tables[3][1][0], tables[1][1][0]), 0)
    # every interval's bits from the most significant, its last byte filled with ones
    per_block = bits.reshape(n, -1).sum(1)
    n_int = int(interval[-1]) + 1
    int_bits = np.bincount(interval, weights=per_block, minlength=n_int).astype(np.int64)
    int_at = np.cumsum((int_bits + 7) // 8 * 8) - (int_bits + 7) // 8 * 8
    val, bits = val.reshape(-1), bits.reshape(-1)
    within = np.cumsum(bits) - bits
    tok_int = np.repeat(interval, 65 * 4)
    first = np.searchsorted(tok_int, np.arange(n_int))
    off = within - within[first][tok_int] + int_at[tok_int]
    stream = np.ones(int(int_at[-1] + (int_bits[-1] + 7) // 8 * 8), np.uint8)
    for b in range(int(bits.max())):
        sel = bits > b
        stream[off[sel] + b] = (val[sel] >> (bits[sel] - 1 - b)) & 1
    data = np.packbits(stream).tobytes()
    out = []
    for i in range(n_int):
        lo = int(int_at[i]) // 8
        out.append(data[lo:lo + int(int_bits[i] + 7) // 8].replace(b"\xff", b"\xff\x00"))
        if i + 1 < n_int:
            out.append(bytes([0xFF, 0xD0 + i % 8]))
    return b"".join(out)


def scan_np(image_u8: np.ndarray, quality: int = 90, subsampling: str = "4:2:0", interval_mcus: int = ENC_INTERVAL_MCUS) -> bytes:
    """The entropy-coded bytes between the SOS header and EOI, RSTn markers included: what zh_jpeg_encode writes byte for byte (at
    interval_mcus = ENC_INTERVAL_MCUS)."""
    check_encode_args("jpeg_device.scan_np", quality, subsampling, interval_mcus)
    return scan_of_blocks(encode_coefficients(image_u8, quality, subsampling), subsampling, interval_mcus)


def encode_np(image_u8: np.ndarray, quality: int = 90, subsampling: str = "4:2:0", interval_mcus: int = ENC_INTERVAL_MCUS) -> bytes:
    """The complete file: header_bytes, scan_np, FF D9 — byte for byte Pillow's for the same settings (see above)."""
    a = np.asarray(image_u8)
    scan = scan_np(a, quality, subsampling, interval_mcus)
    return header_bytes(a.shape[0], a.shape[1], quality, subsampling, interval_mcus) + scan + b"\xff\xd9"


def scan_slot(H: int, W: int) -> int:
    """The bytes a picture's scan has in the stage's copy back: the raw picture's and ENC_SLOT_EXTRA.  A scan that does not fit (the JPEG
    would be larger than the pixels: noise at quality 100) is encoded on the host from the raw picture instead."""
    return int(H) * int(W) * 3 + ENC_SLOT_EXTRA


def scan_bound(H: int, W: int, subsampling: str = "4:2:0", interval_mcus: int = ENC_INTERVAL_MCUS) -> int:
    """The exact worst case of the scan's length.  A block costs at most 11 + 11 bits of DC (the longest DC code, chroma category 11,
    and its extra bits) and 63 x (16 + 10) bits of AC (every coefficient nonzero: no ZRL and no EOB, which would stand for coefficients
    at less than 26 bits each): 1660 bits, ENC_BLOCK_BYTES = 208 bytes rounded up.  An interval of m MCUs of bpm blocks is ceil(1660 m
    bpm / 8) bytes before stuffing, every one of which may be FF and double; a 2-byte marker stands between two intervals.  Nothing
    real comes close: a luma DC code has at most 9 bits (2 bits a luma block less), the chroma code of run 0 / size 10 has 12 bits, not
    16 (its 16-bit codes all carry a run, which stands for coefficients at no bits at all: 63 x 4 = 252 bits a chroma block less), and
    bytes that are all FF would be runs of 1-bits no sequence of codes spells.  scan_of_blocks() of blocks whose DC alternates between
    -1024 and 1023 inside every component and whose AC are all +-1023 comes to 9 + 11 + 63 x 26 = 1658 bits a luma block and 11 + 11 +
    63 x 22 = 1408 a chroma block, less at most 2 bits for the first DC of each component in an interval (1023 against a prediction of 0
    is category 10): its bytes before stuffing are at least ceil((m (1658 lum + 2 x 1408) - 6) / 8) an interval of m MCUs, against the
    bound's ceil(1660 m bpm / 8)."""
    sub = check_encode_args("jpeg_device.scan_bound", 90, subsampling, interval_mcus)
    hs, mcux, mcuy = _geometry(H, W, sub)
    mcus, bpm = mcux * mcuy, hs * hs + 2
    full, rest = divmod(mcus, int(interval_mcus))
    worst = lambda m: 2 * ((1660 * m * bpm + 7) // 8)  # noqa: E731
    return full * worst(int(interval_mcus)) + (worst(rest) if rest else 0) + 2 * (full + (1 if rest else 0) - 1)


def pack_pictures(images: Sequence[np.ndarray], slot_bytes: Optional[int] = None):
    """The arrays of one zh_jpeg_encode launch over u8 [h, w, 3] images of any sizes: (pixels u8 [sum 3 h w], img_off int64 [B], hw int32
    [B, 2], out_off int64 [B], slot_bytes, max_mcus at 4:4:4 — no smaller at 4:2:0).  slot_bytes: None -> the largest scan_slot."""
    arrays = [np.ascontiguousarray(a) for a in images]
    for a in arrays:
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"jpeg_device: a u8 image [H, W, 3] expected, got {a.dtype} {a.shape}")
    if slot_bytes is None:
        slot_bytes = max((scan_slot(*a.shape[:2]) for a in arrays), default=0)
    sizes = np.asarray([a.size for a in arrays], np.int64)
    pixels = np.concatenate([a.reshape(-1) for a in arrays]) if arrays else np.zeros(0, np.uint8)
    hw = np.asarray([a.shape[:2] for a in arrays], np.int32).reshape(-1, 2)
    max_mcus = max((-(-a.shape[0] // 8) * -(-a.shape[1] // 8) for a in arrays), default=1)
    return pixels, np.cumsum(sizes) - sizes, hw, np.arange(len(arrays), dtype=np.int64) * int(slot_bytes), int(slot_bytes), int(max_mcus)


def scan_host(images: Sequence[np.ndarray], quality: int = 90, subsampling: str = "4:2:0", slot_bytes: Optional[int] = None, fill: int = 0xA5):
    """zh_jpeg_encode_host over one launch of images: (out u8 [B, slot_bytes] — `fill` where nothing was written —, lengths int32 [B]).
    The CPU twin of zh_jpeg_encode: same codec functions, same checks."""
    import ctypes
    sub = check_encode_args("jpeg_device.scan_host", quality, subsampling)
    pixels, img_off, hw, out_off, slot, max_mcus = pack_pictures(images, slot_bytes)
    B = len(hw)
    out, lengths = np.full(B * slot, fill, np.uint8), np.zeros(B, np.int32)
    quant = np.ascontiguousarray(quant_tables(quality), np.uint16)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = _lib.load().zh_jpeg_encode_host(ptr(pixels), pixels.size, ptr(img_off), ptr(hw), B, sub, max_mcus, ptr(quant), ptr(out_off), ptr(out), out.size,
                                         slot, ptr(lengths))
    _lib.check(rc, "zh_jpeg_encode_host")
    return out.reshape(B, slot), lengths


def quant_tensor(quality: int, device):
    """quant_tables(quality) as zh_jpeg_encode reads them: int16 [2, 64] on the device (values 1 .. 255)."""
    import torch
    return torch.from_numpy(quant_tables(quality).astype(np.int16)).to(device)


def encode_device(images, quality: int = 90, subsampling: str = "4:2:0") -> List[bytes]:
    """The JPEG files of a u8 [B, H, W, 3] tensor on the GPU, encoded there (ops.jpeg_encode): encode_np of every image, byte for byte.
    One launch sequence and one copy back of scan_slot bytes a picture; a scan that does not fit its slot (larger than the pixels) is
    encoded by encode_np from the pixels instead."""
    import torch
    from . import ops
    sub = check_encode_args("jpeg_device.encode_device", quality, subsampling)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or not images.is_cuda:
        raise ValueError(f"jpeg_device.encode_device: a u8 [B, H, W, 3] tensor on the GPU expected, got {images.dtype} {tuple(images.shape)} on {images.device}")
    B, H, W, _ = images.shape
    if B == 0:
        return []
    images, slot, dev = images.contiguous(), scan_slot(H, W), images.device
    hs, mcux, mcuy = _geometry(H, W, sub)
    off = torch.arange(B, dtype=torch.int64, device=dev)
    out, lengths = torch.empty(B * slot, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    ops.jpeg_encode(images, off * (H * W * 3), torch.tensor([[H, W]] * B, dtype=torch.int32, device=dev), sub, quant_tensor(quality, dev), out, off * slot,
                    slot, lengths, mcux * mcuy)
    scans, n = out.cpu().numpy().reshape(B, slot), lengths.cpu().numpy()
    if (n <= 0).any():
        raise RuntimeError(f"jpeg_device.encode_device: zh_jpeg_encode refused an image of {H} x {W} pixels")
    head = header_bytes(H, W, quality, subsampling)
    return [head + scans[b, :n[b]].tobytes() + b"\xff\xd9" if n[b] <= slot else encode_np(images[b].cpu().numpy(), quality, subsampling) for b in range(B)]


@functools.lru_cache(maxsize=None)
def pillow_writes_restart_blocks() -> bool:
    """Whether the installed Pillow knows save(..., restart_marker_blocks=): it then writes the DRI segment encode_np defines."""
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.new("RGB", (8, 8)).save(buf, "JPEG", restart_marker_blocks=1)
    return b"\xff\xdd\x00\x04\x00\x01" in buf.getvalue()


def require_host_encoder(name: str):
    """jpeg_encoder="host" is Pillow with restart_marker_blocks: a clear error, before any work, where the installed one lacks it."""
    if not pillow_writes_restart_blocks():
        raise RuntimeError(f"{name}: jpeg_encoder=\"host\" needs a Pillow whose JPEG writer takes restart_marker_blocks (the files carry a restart "
                           f"marker every {ENC_INTERVAL_MCUS} MCUs); use jpeg_encoder=\"device\" or a newer Pillow")


def write_scan(path: str, scan, H: int, W: int, quality: int, subsampling: str):
    """What a writer thread does with a finished scan: the header in front, FF D9 behind, the file."""
    data = header_bytes(H, W, quality, subsampling) + bytes(scan) + b"\xff\xd9"
    with open(path, "wb") as f:
        f.write(data)
