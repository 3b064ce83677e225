"""COCO run-length encoding and mask boxes without pycocotools / torchvision.

The reference calls pycocotools.mask.encode(np.asfortranarray(m)) (networks/zutis.py:290,448) and
torchvision.ops.masks_to_boxes (zutis.py:294,452).  Neither package is in this image, so their published
algorithms are restated here (pycocotools 2.0 maskApi.c: rleEncode + rleToString; torchvision.ops.boxes.masks_to_boxes).
The RLE byte string is pinned by hand-derived vectors of the published format (tests/golden/rle_vectors.json, worked out in
tests/test_rle.py: multi-character values, negative deltas, the sign-guard group) plus decode(encode(m)) == m; pycocotools
itself is not available to compare with.  When pycocotools IS importable, networks.zutis uses it instead.
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np


def _counts(mask: np.ndarray) -> np.ndarray:
    """Run lengths of the column-major flattened mask, starting with the run of zeros (may be 0)."""
    flat = np.asarray(mask, dtype=np.uint8).reshape(-1, order="F")
    if flat.size == 0:
        return np.zeros((0,), np.int64)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    bounds = np.concatenate(([0], change, [flat.size]))
    runs = np.diff(bounds)
    if flat[0] != 0:
        runs = np.concatenate(([0], runs))
    return runs.astype(np.int64)


def _to_string(cnts: np.ndarray) -> bytes:
    out = bytearray()
    for i, c in enumerate(cnts.tolist()):
        x = int(c)
        if i > 2:
            x -= int(cnts[i - 2])
        more = True
        while more:
            ch = x & 0x1F
            x >>= 5
            more = (x != -1) if (ch & 0x10) else (x != 0)
            if more:
                ch |= 0x20
            out.append(ch + 48)
    return bytes(out)


def _from_string(s: bytes) -> List[int]:
    cnts: List[int] = []
    p = 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return cnts


def encode_py(mask: np.ndarray) -> Dict:
    """Pure NumPy/Python form (kept as the readable restatement and as the checker of the C helper)."""
    assert mask.ndim == 2
    h, w = mask.shape
    return {"size": [int(h), int(w)], "counts": _to_string(_counts(mask))}


def _host_capacity(n_values: int, chars_per_value: int = 8) -> int:
    """Bytes of the buffer handed to the host entry points (csrc/rle_host.hip) for a string of n_values run values.  The bound is
    derived once, in csrc/rle_codec.h ("the character bound"): a value below 2^34 in magnitude takes at most 7 characters, so 8 per
    value plus 16 holds every mask of fewer than 2^31 pixels; the entry points check the capacity for every value all the same and
    return -1.  encode() asks for 4 per PIXEL instead: a value is at most the longer of runs k and k - 2 in magnitude, each run is
    charged for at most two values, and a run of L >= 1 pixels needs no more than 2 L characters for a value up to L."""
    return chars_per_value * n_values + 16


def encode(mask: np.ndarray) -> Dict:
    """mask [H,W] {0,1}/bool -> {"size": [H, W], "counts": bytes} (pycocotools.mask.encode for one mask).
    Uses the C helper zh_rle_encode_host from libzutis_hip.so (host code, no GPU needed)."""
    import ctypes as C
    from . import _lib
    assert mask.ndim == 2
    h, w = mask.shape
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    cap = min(_host_capacity(m.size + 2, 4), 6 * (h * w + 2))
    buf = C.create_string_buffer(cap)
    n = _lib.load().zh_rle_encode_host(m.ctypes.data, h, w, C.addressof(buf), cap)
    if n < 0:
        raise RuntimeError("zh_rle_encode_host: buffer too small")
    return {"size": [int(h), int(w)], "counts": buf.raw[:n]}


def decode(rle: Dict) -> np.ndarray:
    h, w = rle["size"]
    cnts = _from_string(rle["counts"] if isinstance(rle["counts"], (bytes, bytearray)) else rle["counts"].encode("ascii"))
    flat = np.zeros(h * w, np.uint8)
    pos, val = 0, 0
    for c in cnts:
        if val:
            flat[pos:pos + c] = 1
        pos += c
        val ^= 1
    return flat.reshape((h, w), order="F")


def decode_np(rle: Dict) -> np.ndarray:
    """decode() in NumPy, for the read-back check of the pseudo-label writers (pseudo_masks.save_rle_json), where the per-character Python
    loop of decode() was the longest step of the tail.  The run lengths are counts_np's (the one NumPy string parser: a string that ends
    inside a value, or holds a value of more than 12 characters, is its ValueError); only the repeat into pixels happens here.  decode()
    stays as the readable restatement it is checked against (tests/test_pseudo_files_cpu.py)."""
    h, w = rle["size"]
    s = rle["counts"]
    cnts = counts_np(s if isinstance(s, (bytes, bytearray, str)) else bytes(s))
    flat = np.zeros(h * w, np.uint8)
    runs = np.repeat((np.arange(cnts.size) & 1).astype(np.uint8), cnts)[:h * w]
    flat[:runs.size] = runs
    return flat.reshape((h, w), order="F")


def mask_to_box(mask: np.ndarray) -> List[float]:
    """torchvision.ops.masks_to_boxes for one mask: [xmin, ymin, xmax, ymax] of the non-zero pixels (float32 values)."""
    rows = np.flatnonzero(mask.any(axis=1))
    cols = np.flatnonzero(mask.any(axis=0))
    return [float(cols[0]), float(rows[0]), float(cols[-1]), float(rows[-1])]


def rle_from_transitions(positions: np.ndarray, first_value: int, h: int, w: int) -> Dict:
    """COCO RLE dict from the column-major transition positions produced by zh_mask_runs (device):
    counts = diff([0, positions..., h*w]) with a leading empty zero-run when pixel 0 is set."""
    import ctypes as C
    from . import _lib
    edges = np.concatenate(([0], positions.astype(np.int64), [h * w]))
    counts = np.diff(edges)
    if first_value:
        counts = np.concatenate(([0], counts))
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    cap = _host_capacity(counts.size)
    buf = C.create_string_buffer(cap)
    n = _lib.load().zh_rle_counts_to_string_host(counts.ctypes.data, counts.size, C.addressof(buf), cap)
    assert n >= 0
    return {"size": [int(h), int(w)], "counts": buf.raw[:n]}


def rles_from_transitions(positions: np.ndarray, nruns: np.ndarray, h: int, w: int, packed_max_runs: int = 0):
    """The COCO RLE dicts of all n masks from zh_mask_runs' host copies in ONE C call (zh_rle_from_transitions_host): positions int32
    [n, keep], nruns int32 [n, 2] = (transitions, value of pixel 0).  Entry i is None when mask i has more transitions than `keep`
    (the caller re-encodes it from the mask itself).  packed_max_runs > 0: positions is zh_mask_runs_kept's packed list (1-D: mask i's
    min(transitions, packed_max_runs) entries follow mask i - 1's)."""
    import ctypes as C
    from . import _lib
    pos = positions if (positions.dtype == np.int32 and positions.flags.c_contiguous) else np.ascontiguousarray(positions, dtype=np.int32)
    nr = nruns if (nruns.dtype == np.int32 and nruns.flags.c_contiguous) else np.ascontiguousarray(nruns, dtype=np.int32)
    n = nr.shape[0]
    keep = int(packed_max_runs) if packed_max_runs else pos.shape[1]
    nt = nr[:, 0].tolist()
    cap = _host_capacity(sum(min(t, keep) for t in nt) + 3 * n)
    buf = C.create_string_buffer(cap)
    off = np.empty(n + 1, dtype=np.int64)
    total = _lib.load(raw=True).zh_rle_from_transitions_host(pos.ctypes.data, keep, 1 if packed_max_runs else 0, nr.ctypes.data, n, h * w,
                                                             C.addressof(buf), cap, off.ctypes.data)
    assert total >= 0
    raw = buf.raw
    size = [int(h), int(w)]
    o = off.tolist()
    return [({"size": size, "counts": raw[o[i]:o[i + 1]]} if nt[i] <= keep else None) for i in range(n)]


def counts_np(counts) -> np.ndarray:
    """The uncompressed run lengths (int64, the run of zeros first) behind any of the three forms a COCO RLE's "counts" takes: the
    compressed string as bytes or as str (what json writes and reads back), or the list of an uncompressed RLE.  The string parser, in
    NumPy: the characters of a value are its 5-bit groups (bit 0x20 = more follow, bit 0x10 of the last = sign), values from the fourth on
    are deltas against the value two places back, i.e. running sums over the odd and over the even places.  COCO mask AP
    (zutis_amd/coco_eval.py) works on the runs themselves; decode_np repeats them into pixels."""
    if not isinstance(counts, (bytes, bytearray, str)):
        return np.asarray(counts, dtype=np.int64).reshape(-1)
    c = np.frombuffer(counts.encode("ascii") if isinstance(counts, str) else bytes(counts), np.uint8).astype(np.int64) - 48
    if not c.size:
        return np.zeros((0,), np.int64)
    ends = np.flatnonzero((c & 0x20) == 0)
    if not ends.size or ends[-1] != c.size - 1:
        raise ValueError("RLE string ends inside a value")
    starts = np.concatenate(([0], ends[:-1] + 1))
    nchar = ends - starts + 1
    if nchar.max() > 12:
        raise ValueError("RLE string holds a value of more than 12 characters")
    part = (c & 0x1F) << (5 * (np.arange(c.size) - np.repeat(starts, nchar)))
    cnts = np.add.reduceat(part, starts)
    cnts = np.where((c[ends] & 0x10) != 0, cnts | np.left_shift(np.int64(-1), 5 * nchar), cnts)
    cnts[1::2] = np.cumsum(cnts[1::2])
    cnts[2::2] = np.cumsum(cnts[2::2])
    return cnts


def _polygon_boundary(xy, h: int, w: int) -> np.ndarray:
    """rleFrPoly (pycocotools maskApi.c) up to its sort: the column-major positions x * h + y at which one polygon's boundary crosses a
    pixel column.  xy = [x0, y0, x1, y1, ...] in pixels.  C's (int) truncates toward zero: int() here."""
    scale = 5.0
    k = len(xy) // 2
    x = [int(scale * float(xy[2 * j]) + .5) for j in range(k)]
    y = [int(scale * float(xy[2 * j + 1]) + .5) for j in range(k)]
    x.append(x[0])
    y.append(y[0])
    u, v = [], []                                   # every integer step along every edge, at 5 x the resolution
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = (ye - ys) / dx if dx else 0.0       # (dx == dy == 0: C divides 0 by 0 and multiplies the NaN by t = 0 only — one point)
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(int(ys + s * t + .5))
        else:
            s = (xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + .5))
    out = []
    for j in range(1, len(u)):                      # where the walk changes column: keep the crossings of pixel-column centres
        if u[j] == u[j - 1]:
            continue
        xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
        xd = (xd + .5) / scale - .5
        if np.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
        yd = (yd + .5) / scale - .5
        yd = 0.0 if yd < 0 else (float(h) if yd > h else yd)
        out.append(int(xd) * h + int(np.ceil(yd)))
    return np.asarray(out, dtype=np.int64)


def _polygon_counts(xy, h: int, w: int) -> np.ndarray:
    """rleFrPoly's tail: sort the crossings, take differences, and merge what a zero-length run separates."""
    a = np.sort(np.concatenate((_polygon_boundary(xy, h, w), [h * w])))
    a = np.diff(np.concatenate(([0], a))).tolist()
    b, j = [a[0]], 1
    while j < len(a):
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < len(a):
                b[-1] += a[j]
                j += 1
    return np.asarray(b, dtype=np.int64)


def _dense(cnts, h: int, w: int) -> np.ndarray:
    return np.repeat((np.arange(len(cnts)) & 1).astype(np.uint8), cnts)[:h * w].reshape((h, w), order="F")


def from_polygons(polys, h: int, w: int) -> Dict:
    """COCO RLE dict of the union of polygons [[x0, y0, x1, y1, ...], ...] on an h x w image: pycocotools' annToRLE for a polygon
    annotation (mask.frPyObjects + mask.merge), its rleFrPoly procedure restated — scale by 5, walk each edge in integer steps, keep
    the crossings of pixel-column centres, downsample, take differences.  One flat list of numbers is one polygon."""
    if len(polys) and not isinstance(polys[0], (list, tuple, np.ndarray)):
        polys = [polys]
    if len(polys) == 1:
        cnts = _polygon_counts(polys[0], h, w)
    else:
        m = np.zeros((h, w), np.uint8)
        for p in polys:
            m |= _dense(_polygon_counts(p, h, w), h, w)
        cnts = _counts(m) if m.size else np.zeros((0,), np.int64)
    return {"size": [int(h), int(w)], "counts": _to_string(cnts)}
