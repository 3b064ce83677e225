"""The corpus of the JPEG decoder tests, written by Pillow at test time from seeds, and the damaged scans.

Sizes (H x W), the smallest at which each rule can go wrong: single-sample planes (1 x 1), a partial MCU on one axis (8 x 9), narrow
chroma at cropped width 1 (17 x 1, 9 x 2), cropped width 2 (9 x 3) and the first width above it (9 x 5), one row / two rows (1 x 17,
2 x 9), an exact MCU fit (16 x 16), partial MCUs on both axes over several MCU rows with vertical context (37 x 53, 33 x 64, 64 x 48).
Each size in 8 settings x 2 content kinds.  Plain helper module: no fixtures, no pytest hooks."""
import dataclasses
import io

import numpy as np
from PIL import Image

from zutis_amd import jpeg_device as J

SIZES = [(1, 1), (8, 9), (17, 1), (1, 17), (9, 2), (9, 3), (9, 5), (2, 9), (16, 16), (37, 53), (33, 64), (64, 48)]
SETTINGS = {
    "q90-420": dict(quality=90, subsampling=2),
    "q90-444": dict(quality=90, subsampling=0),
    "q90-422": dict(quality=90, subsampling=1),
    "q75-opt": dict(quality=75, optimize=True),
    "q100-420": dict(quality=100, subsampling=2),
    "q30": dict(quality=30),
    "q90-rst": dict(quality=90, restart_marker_blocks=3),
    "q85-grey": dict(quality=85, grey=True),
}
KINDS = ("noise", "smooth")
_FILES = {}


def pixels(h: int, w: int, kind: str, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng([h, w, KINDS.index(kind), seed])
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([96 + 80 * np.sin(xx / 7.0 + 1), 128 + 90 * np.cos(yy / 5.0), 100 + 2.0 * xx + 1.5 * yy], 2)
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(a: np.ndarray, **kw) -> bytes:
    kw = dict(kw)
    im = Image.fromarray(a)
    if kw.pop("grey", False):
        im = im.convert("L")
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def file_bytes(h: int, w: int, setting: str, kind: str) -> bytes:
    """One file of the corpus (cached: built once a process)."""
    key = (h, w, setting, kind)
    if key not in _FILES:
        _FILES[key] = encode(pixels(h, w, kind), **SETTINGS[setting])
    return _FILES[key]


def variants(h: int, w: int):
    """[(name, file bytes)] of the 16 variants of a size."""
    return [(f"{h}x{w}-{s}-{k}", file_bytes(h, w, s, k)) for s in SETTINGS for k in KINDS]


def corpus():
    return [v for h, w in SIZES for v in variants(h, w)]


def pillow(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


# ---- damaged scans: a good file's plan over other scan bytes.  Each is (plan, data): parse() of a good file, its one segment (or its
# restart interval) replaced; the bytes in front of the scan are the file's own.
DAMAGED = ("cut", "ff00", "marker", "zeros", "dri")


def damaged(kind: str, h: int = 33, w: int = 64):
    data = file_bytes(h, w, "q90-rst" if kind == "dri" else "q90-420", "smooth")
    plan = J.parse(data)
    lo, hi = int(plan.segments[0, 0]), int(plan.segments[-1, 1])
    scan = data[lo:hi]
    if kind == "dri":            # the file has a marker every 3 MCUs; the header now says 2: segments hold more data than asked for and cover too few MCUs
        segs = plan.segments.copy()
        segs[:, 2] = np.arange(len(segs)) * 2
        return dataclasses.replace(plan, restart_interval=2, segments=segs), data
    new = {"cut": scan[:len(scan) // 3], "ff00": b"\xff\x00" * (len(scan) // 2), "marker": scan[:len(scan) // 2] + b"\xff\xc4" + scan[len(scan) // 2:],
           "zeros": bytes(len(scan))}[kind]
    out = data[:lo] + new + b"\xff\xd9"
    return dataclasses.replace(plan, segments=np.asarray([[lo, lo + len(new), 0]], np.int64)), out
