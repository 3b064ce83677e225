"""The pictures of the JPEG encoder tests and their reference scans (jpeg_device.scan_np), computed once a process and shared.

Sizes: those of tests/_jpeg_case.py (single samples, partial MCUs on either axis, dummy blocks at the right and the bottom edge, an exact
fit, several MCU rows), and two with more than 8 restart intervals, which wrap RST7 to RST0: 100 x 150 at 4:4:4 (247 MCUs, 16 intervals)
and 200 x 200 at 4:2:0 (169 MCUs, 11 intervals).  Both content kinds of _jpeg_case.pixels, qualities 1, 50, 90, 100, both subsamplings.
Constructed pictures: flat black and white (every block EOB, every DC difference 0), a saturated checkerboard (DC category 11, AC
category 10 at quality 100), one cosine pattern per block that leaves a lone coefficient behind 16 or more zeros (ZRL) and one that
leaves coefficient 63 (three ZRLs, no EOB).  Plain helper module: no fixtures, no pytest hooks."""
import functools
import io

import numpy as np
from PIL import Image

from tests import _jpeg_case as C
from zutis_amd import jpeg_device as J

QUALITIES = (1, 50, 90, 100)
SUBSAMPLINGS = ("4:4:4", "4:2:0")
WRAP = {"4:4:4": (100, 150), "4:2:0": (200, 200)}
OVERFLOW = dict(h=64, w=64, quality=100, subsampling="4:4:4")      # noise: its scan is longer than its pixels and scan_slot's extra


def pillow_has_restart_blocks() -> bool:
    """Whether the installed Pillow knows restart_marker_blocks (it then writes a DRI segment)."""
    buf = io.BytesIO()
    Image.new("RGB", (8, 8)).save(buf, "JPEG", restart_marker_blocks=1)
    return b"\xff\xdd\x00\x04\x00\x01" in buf.getvalue()


def pillow_file(a: np.ndarray, quality: int, subsampling: str, interval_mcus: int = J.ENC_INTERVAL_MCUS) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=quality, subsampling=J.SUBSAMPLINGS[subsampling], restart_marker_blocks=interval_mcus)
    return buf.getvalue()


def cosine(u: int, v: int, amplitude: float = 100.0, h: int = 8, w: int = 8) -> np.ndarray:
    """Grey u8 [h, w, 3]: 128 + amplitude cos((2 x + 1) u pi / 16) cos((2 y + 1) v pi / 16) in every 8 x 8 block: DCT basis (row v, column u)."""
    y, x = np.mgrid[0:h, 0:w] % 8
    g = np.clip(np.rint(128 + amplitude * np.cos((2 * x + 1) * u * np.pi / 16) * np.cos((2 * y + 1) * v * np.pi / 16)), 0, 255).astype(np.uint8)
    return np.repeat(g[..., None], 3, 2)


def checkerboard(h: int = 32, w: int = 48) -> np.ndarray:
    """Left half: 8 x 8 blocks alternately 0 and 255 (DC differences of 2040: category 11); right half: 4 x 4 tiles (AC category 10)."""
    y, x = np.mgrid[0:h, 0:w]
    g = np.where(x < w // 2, ((y // 8 + x // 8) % 2) * 255, ((y // 4 + x // 4) % 2) * 255).astype(np.uint8)
    return np.repeat(g[..., None], 3, 2)


@functools.lru_cache(maxsize=None)
def constructed():
    """{name: (image, quality)}; every one is encoded at both subsamplings."""
    out = {"black": (np.zeros((24, 40, 3), np.uint8), 90), "white": (np.full((24, 40, 3), 255, np.uint8), 90), "checker": (checkerboard(), 100),
           "zrl": (cosine(1, 7, h=16, w=24), 50), "coef63": (cosine(7, 7, h=16, w=24), 50), "ff": (C.pixels(33, 64, "noise", seed=3), 100)}
    for a, _ in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cases(quality: int, subsampling: str):
    """[(name, image, scan_np(image))] of one (quality, subsampling): what one zh_jpeg_encode call can take.  Shared, never written."""
    out = []
    for h, w in C.SIZES + [WRAP[subsampling]]:
        for kind in C.KINDS:
            out.append((f"{h}x{w}-{kind}", C.pixels(h, w, kind)))
    out += [(name, a) for name, (a, q) in constructed().items() if q == quality]
    for _, a in out:
        a.setflags(write=False)
    return [(name, a, J.scan_np(a, quality, subsampling)) for name, a in out]


def named(quality: int, subsampling: str, name: str):
    """(image, scan) of the case `name`."""
    (hit,) = [c for c in cases(quality, subsampling) if c[0] == name]
    return hit[1], hit[2]


@functools.lru_cache(maxsize=None)
def overflow():
    """(image, scan): 64 x 64 noise at quality 100, 4:4:4 — longer than scan_slot."""
    a = C.pixels(OVERFLOW["h"], OVERFLOW["w"], "noise", seed=1)
    a.setflags(write=False)
    return a, J.scan_np(a, OVERFLOW["quality"], OVERFLOW["subsampling"])
