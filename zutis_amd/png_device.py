"""The PNG the device encoder writes, defined in NumPy: the zlib stream zh_png_deflate (csrc/png.hip) produces byte for byte, and the
framing the writer threads put around it.

A PNG is a signature, IHDR, (PLTE,) IDAT = a zlib stream of the filtered rows, IEND.  The stream is fixed here so that a kernel can make
it in parallel and be compared exactly:

  filtered bytes  every row of the u8 [H, W] / [H, W, 3] image as filter type 2 (Up): its filter byte 2, then byte minus the byte above
                  mod 256 (the first row against zeros); n = H * (W * c + 1) bytes, row-major.  Up turns the vertically coherent regions
                  of label maps into zeros, also for "rg16", whose R, G, 0 period defeats distance-1 runs on the raw bytes.
  segments        consecutive SEGMENT_BYTES of the filtered bytes, whatever the row length (the last one shorter): one workgroup each.
  a segment       one deflate block BFINAL = 0, BTYPE = 01 (the fixed code of RFC 1951 3.2.6): its tokens, end-of-block; then an empty
                  stored block (000, zero bits to the byte, 00 00 FF FF): every segment ends on a byte and refers to nothing before it.
  tokens          greedy over the maximal runs of equal bytes, clipped to the segment: a run of length L is its first byte as a literal,
                  then the other L - 1 bytes as matches of distance 1 and length min(258, what is left) while 3 or more are left, then
                  literals.  In closed form (run_tokens): the byte at offset k >= 1 of its run, j = k - 1, q = j // 258, m = j % 258,
                  tail = L - 1 - 258 q, is a literal when tail < 3, starts a match of length min(258, tail) when m == 0, and is covered
                  by a match otherwise.
  stream          78 01, the segments, 03 00 (a final empty fixed block), Adler-32 of the filtered bytes, big-endian.

Huffman codes are packed from their most significant bit, extra bits from their least significant one, bytes are filled from bit 0.
No torch at import.
"""
from __future__ import annotations

import struct
import zlib
from typing import Optional

import numpy as np

from . import _lib

SEGMENT_BYTES = _lib.constants()["ZH_PNG_SEGMENT_BYTES"]
ENCODERS = ("host", "device")
MODES = {"L": (1, 0), "P": (1, 3), "RGB": (3, 2)}       # mode -> (channels, PNG colour type)

# RFC 1951 3.2.5: length symbols 257 .. 285, their extra bits and base lengths
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]


def _reverse(code: np.ndarray, nbits: np.ndarray) -> np.ndarray:
    out = np.zeros_like(code)
    for b in range(9):
        out |= np.where(nbits > b, ((code >> b) & 1) << np.maximum(nbits - 1 - b, 0), 0)
    return out


def _length_table():
    """(value, bits) of the match token of every length 3 .. 258 at distance 1, as it enters the stream from bit 0: the length symbol's
    fixed code reversed, its extra bits, the 5-bit distance code 0."""
    val, nb = np.zeros(259, np.int64), np.zeros(259, np.int64)
    for length in range(3, 259):
        s = 28 if length == 258 else max(i for i in range(28) if _LEN_BASE[i] <= length)
        sym = 257 + s
        code, n = (sym - 256, 7) if sym < 280 else (0xC0 + sym - 280, 8)
        rev = int(_reverse(np.asarray([code]), np.asarray([n]))[0])
        val[length] = rev | ((length - _LEN_BASE[s]) << n)
        nb[length] = n + _LEN_EXTRA[s] + 5
    return val, nb


_LEN_VAL, _LEN_BITS = _length_table()
_LIT = np.arange(256)
_LIT_BITS = np.where(_LIT < 144, 8, 9).astype(np.int64)
_LIT_VAL = _reverse(np.where(_LIT < 144, 0x30 + _LIT, 0x190 + _LIT - 144).astype(np.int64), _LIT_BITS)


def filtered(image_u8: np.ndarray) -> np.ndarray:
    """The filtered bytes of a u8 [H, W] or [H, W, 3] image: u8 [H * (W * c + 1)]."""
    a = np.asarray(image_u8)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"png_device: a u8 image [H, W] or [H, W, 3] with H, W >= 1 expected, got {a.dtype} {a.shape}")
    rows = a.reshape(a.shape[0], -1)
    up = np.zeros_like(rows)
    up[1:] = rows[:-1]
    out = np.empty((rows.shape[0], rows.shape[1] + 1), np.uint8)
    out[:, 0] = 2
    out[:, 1:] = rows - up                     # u8 arithmetic: mod 256
    return out.reshape(-1)


def run_tokens(data: np.ndarray):
    """(values, bits) int64 of the tokens of one segment's bytes, in stream order — the closed form of the module's docstring."""
    d = np.asarray(data, np.uint8).reshape(-1)
    n = d.size
    idx = np.arange(n)
    head = np.ones(n, bool)
    head[1:] = d[1:] != d[:-1]
    heads = np.flatnonzero(head)
    run = np.cumsum(head) - 1
    k = idx - heads[run]
    L = np.append(heads[1:], n)[run] - heads[run]
    j = k - 1
    q, m = j // 258, j % 258
    tail = L - 1 - 258 * q
    literal = (k == 0) | (tail < 3)
    match = (k >= 1) & (tail >= 3) & (m == 0)
    mlen = np.clip(np.minimum(258, tail), 3, 258)
    val = np.where(literal, _LIT_VAL[d], _LEN_VAL[mlen])
    bits = np.where(literal, _LIT_BITS[d], _LEN_BITS[mlen])
    keep = literal | match
    return val[keep], bits[keep]


def _pack(val: np.ndarray, bits: np.ndarray) -> bytes:
    off = np.cumsum(bits) - bits
    total = int(bits.sum())
    stream = np.zeros((total + 7) // 8 * 8, np.uint8)
    for b in range(int(bits.max()) if bits.size else 0):
        sel = bits > b
        stream[off[sel] + b] = (val[sel] >> b) & 1
    return np.packbits(stream, bitorder="little").tobytes()


def deflate_filtered(data: np.ndarray) -> bytes:
    """The stream of already filtered bytes u8 [n] (what deflate_np makes of filtered(image); token edges are tested through here)."""
    d = np.ascontiguousarray(np.asarray(data, np.uint8).reshape(-1))
    out = [b"\x78\x01"]
    for at in range(0, d.size, SEGMENT_BYTES):
        val, bits = run_tokens(d[at:at + SEGMENT_BYTES])
        # 0, 1, 0: BFINAL = 0, BTYPE = 01 from its low bit; 7 zero bits: end-of-block; 3 zero bits: the stored block's header
        out.append(_pack(np.concatenate(([2], val, [0])), np.concatenate(([3], bits, [10]))) + b"\x00\x00\xff\xff")
    out.append(b"\x03\x00" + struct.pack(">I", zlib.adler32(d.tobytes())))
    return b"".join(out)


def deflate_np(image_u8: np.ndarray) -> bytes:
    """The zlib stream of the image's PNG: the definition zh_png_deflate equals byte for byte."""
    return deflate_filtered(filtered(image_u8))


def segment_bound(n: int) -> int:
    """Bytes of a segment of n filtered bytes at the most: 3 header bits, 9 bits a byte (no run, every byte >= 144), 7 bits end-of-block,
    3 bits of stored header, rounded up to the byte, and the stored block's four length bytes."""
    return (9 * int(n) + 13 + 7) // 8 + 4


def stream_bound(H: int, W: int, c: int) -> int:
    """The exact worst case of the stream's length for an H x W image of c channels: n = H * (W * c + 1) filtered bytes make n //
    SEGMENT_BYTES full segments and, when n % SEGMENT_BYTES is not 0, a last one; a token never costs more than the 9-bit literals of the
    bytes it stands for (a match of 3 .. 258 bytes is at most 18 bits), so a segment of s bytes holds at most 3 + 9 s + 7 + 3 bits,
    padded to the byte, plus 00 00 FF FF: segment_bound(s).  Around the segments: 78 01 in front, 03 00 and the four Adler-32 bytes
    behind.  Reached by an image whose every segment has no two equal neighbours and no byte below 144."""
    n = int(H) * (int(W) * int(c) + 1)
    full, rest = divmod(n, SEGMENT_BYTES)
    return 2 + full * segment_bound(SEGMENT_BYTES) + (segment_bound(rest) if rest else 0) + 6


def segments(H: int, W: int, c: int) -> int:
    """Segments (= workgroups of the first launch) of an H x W image of c channels."""
    return -(-(int(H) * (int(W) * int(c) + 1)) // SEGMENT_BYTES)


def _chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(body, zlib.crc32(kind)))


def frame(stream, H: int, W: int, mode: str, palette_bytes: Optional[bytes] = None) -> bytes:
    """The PNG file around a stream: signature, IHDR (8 bits, colour type of mode "L" / "P" / "RGB", no interlace), PLTE for "P"
    (palette_bytes: r, g, b per entry, at most 256 entries), one IDAT, IEND; chunk CRCs from zlib.crc32."""
    if mode not in MODES:
        raise ValueError(f"png_device.frame: mode {mode!r} is not one of {sorted(MODES)}")
    if (mode == "P") != (palette_bytes is not None):
        raise ValueError("png_device.frame: a palette goes with mode \"P\", and only with it")
    if H < 1 or W < 1:
        raise ValueError(f"png_device.frame: a PNG of {H} x {W} pixels")
    out = [b"\x89PNG\r\n\x1a\n", _chunk(b"IHDR", struct.pack(">IIBBBBB", int(W), int(H), 8, MODES[mode][1], 0, 0, 0))]
    if mode == "P":
        palette_bytes = bytes(palette_bytes)
        if not palette_bytes or len(palette_bytes) % 3 or len(palette_bytes) > 768:
            raise ValueError(f"png_device.frame: a palette of {len(palette_bytes)} bytes is not 1 .. 256 (r, g, b) entries")
        out.append(_chunk(b"PLTE", palette_bytes))
    out += [_chunk(b"IDAT", bytes(stream)), _chunk(b"IEND", b"")]
    return b"".join(out)


def encode_np(image: np.ndarray, mode: str, palette_bytes: Optional[bytes] = None) -> bytes:
    """frame() of deflate_np(): the file the device path writes for the image."""
    a = np.asarray(image)
    if mode in MODES and (a.ndim - 1 if a.ndim == 2 else a.shape[-1]) != MODES[mode][0]:
        raise ValueError(f"png_device.encode_np: an image of shape {a.shape} is not mode {mode}")
    return frame(deflate_np(a), a.shape[0], a.shape[1], mode, palette_bytes)


def check_encoder(name: str, png_encoder) -> str:
    if png_encoder not in ENCODERS:
        raise ValueError(f"{name}: png_encoder {png_encoder!r} is not \"host\" or \"device\"")
    return png_encoder


def write_stream(path: str, stream, H: int, W: int, mode: str, palette_bytes: Optional[bytes]):
    """What a writer thread does with a finished stream: frame it (the IDAT CRC is the work) and write the file."""
    data = frame(stream, H, W, mode, palette_bytes)
    with open(path, "wb") as f:
        f.write(data)
