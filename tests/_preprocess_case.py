"""Shared by tests/test_preprocess_cpu.py and tests/test_preprocess_gpu.py: the seeded images of the device pre-processing tests.

Every image is generated from a seed and written with Pillow into the test's tmp_path; nothing is downloaded and nothing reads
the reference.  SHAPES are the (h, w) -> n_px cases Pillow's resampler was restated on (down- and up-scaling, identity passes,
extreme aspect ratios, the 55.5 -> 56 crop offset of 640 x 427 at 224)."""
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "zutis_amd", "dropin")

SHAPES = [(375, 500, 336), (500, 375, 336), (333, 500, 224), (1200, 1600, 336), (200, 300, 336), (336, 336, 336),
          (337, 1000, 336), (64, 48, 224), (2000, 1500, 336), (480, 640, 224), (17, 900, 224), (336, 500, 336),
          (427, 640, 224), (640, 427, 224)]


def dropin():
    """The drop-in's module (imported the way a user of the reference's layout imports it)."""
    if DROPIN not in sys.path:
        sys.path.insert(0, DROPIN)
    from utils import extract_image_embeddings
    return extract_image_embeddings


def pixels(h: int, w: int, seed: int, channels: int = 3) -> np.ndarray:
    """Random bytes with saturated and black rows, so that both clamps of the resampler are exercised."""
    a = np.random.default_rng(seed).integers(0, 256, (h, w, channels), dtype=np.uint8)
    a[::7] = 255
    a[3::11] = 0
    return a


def write_rgb(tmp_path, name: str, h: int, w: int, seed: int) -> str:
    p = str(tmp_path / name)
    Image.fromarray(pixels(h, w, seed)).save(p, compress_level=1)
    return p


def write_modes(tmp_path):
    """A grayscale, a palette and an RGBA PNG (what convert("RGB") has to turn into three bytes per pixel)."""
    out = []
    g = pixels(61, 83, 101, 1)[..., 0]
    p = str(tmp_path / "gray.png"); Image.fromarray(g, "L").save(p); out.append(p)
    pal = Image.fromarray(pixels(70, 45, 102)).convert("P", palette=Image.ADAPTIVE, colors=64)
    p = str(tmp_path / "palette.png"); pal.save(p); out.append(p)
    p = str(tmp_path / "rgba.png"); Image.fromarray(pixels(52, 97, 103, 4), "RGBA").save(p); out.append(p)
    return out
