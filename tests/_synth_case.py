"""Shared by tests/test_synth_cpu.py and tests/test_synth_gpu.py: seeded images and pseudo-masks of the training-sample tests.

Every image is generated from a seed and written with Pillow (PNG or JPEG) into the test's tmp_path, every mask as the RLE JSON the
pseudo-label writers produce; nothing is downloaded.  Recipes are written out by hand (sub()) where a test needs one particular
geometry, and drawn with draw_recipe where it needs many."""
import importlib.util
import json
import os
import random

import numpy as np
from PIL import Image

from zutis_amd import rle, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORE = 255


def photo(h: int, w: int, seed: int) -> np.ndarray:
    """A smooth coloured field plus noise, with a saturated and a black band: both clamps and non-trivial hues."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = [127 + 120 * np.sin(x / (7 + 3 * c + seed % 5) + c) * np.cos(y / (11 + 2 * c) + seed) for c in range(3)]
    a = np.clip(np.stack(chans, -1) + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)
    a[h // 3] = 255
    a[:, w // 4] = 0
    return a


def blob(h: int, w: int, seed: int, kind: str = "ellipse") -> np.ndarray:
    """u8 {0, 1} [h, w]: "ellipse" somewhere inside, "border" touching the top-left border, "full" everything, "empty" nothing."""
    if kind == "empty":
        return np.zeros((h, w), np.uint8)
    if kind == "full":
        return np.ones((h, w), np.uint8)
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "border":
        return ((x < w * 0.45) & (y < h * 0.6)).astype(np.uint8)
    cy, cx = h * rng.uniform(0.35, 0.65), w * rng.uniform(0.35, 0.65)
    ry, rx = h * rng.uniform(0.15, 0.3), w * rng.uniform(0.15, 0.3)
    return ((((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2) < 1.0).astype(np.uint8)


def write_pair(tmp_path, name: str, h: int, w: int, seed: int, kind: str = "ellipse", jpeg: bool = False):
    """(image path, mask path) of one seeded file pair."""
    p_image = str(tmp_path / (name + (".jpg" if jpeg else ".png")))
    if jpeg:
        Image.fromarray(photo(h, w, seed)).save(p_image, quality=90)
    else:
        Image.fromarray(photo(h, w, seed)).save(p_image, compress_level=1)
    p_mask = str(tmp_path / (name + ".json"))
    r = rle.encode_py(blob(h, w, seed, kind))
    with open(p_mask, "w") as f:
        json.dump({"size": r["size"], "counts": r["counts"].decode("ascii")}, f)
    return p_image, p_mask


def sub(size_wh, scale: float, *, corner=0, u_crop=(0.5, 0.5), flip=False, jitter=False, order=(0, 1, 2, 3), factors=(1.0, 1.0, 1.0),
        hue=0, grey=False, blur=False, sigma=1.0, u_paste=(0.5, 0.5), label=1, p_image="", p_mask="") -> synth.SubRecipe:
    w, h = size_wh
    return synth.SubRecipe(p_image, p_mask, label, (w, h), (int(w * scale), int(h * scale)), corner, u_crop[0], u_crop[1], flip, jitter,
                           tuple(order), factors[0], factors[1], factors[2], hue, grey, blur, sigma, u_paste[0], u_paste[1])


class Dataset:
    """The fields of an IndexDataset that __getitem__ reads (datasets/index_dataset.py:39-89)."""

    def __init__(self, pairs, labels, crop_size=64, scale_range=(0.1, 1.0), max_n_masks=10, random_duplicate=False, device=None):
        self.p_images = [p for p, _ in pairs]
        self.p_pseudo_masks = [m for _, m in pairs]
        self.p_image_to_label_id = dict(zip(self.p_images, labels))
        self.category_to_p_images = {}
        for p, l in zip(self.p_images, labels):
            self.category_to_p_images.setdefault(f"category{l}", []).append(p)
        self.ignore_index, self.max_n_masks, self.scale_range, self.crop_size = IGNORE, max_n_masks, scale_range, crop_size
        self.random_duplicate, self.device = random_duplicate, device
        self.mean, self.std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


SHAPES_HW = [(120, 160), (160, 120), (90, 90), (200, 70), (64, 300), (150, 210), (333, 250), (48, 64)]


def corpus(tmp_path, n: int = 8, jpeg_every: int = 2):
    """n file pairs of mixed, non-square shapes (every jpeg_every-th a JPEG) and their label ids 1 .. 5."""
    pairs = [write_pair(tmp_path, f"img{i}", *SHAPES_HW[i % len(SHAPES_HW)], seed=100 + i, kind=("border" if i % 5 == 3 else "ellipse"),
                        jpeg=(i % jpeg_every == 1)) for i in range(n)]
    return pairs, [1 + i % 5 for i in range(n)]


def drawn_recipes(fields, n: int, seed: int):
    rng = random.Random(seed)
    return [synth.draw_recipe(rng, fields) for _ in range(n)]


def packed_items(packed):
    """The meaningful bytes of a Packed on the host: its head, then every sub-image's image and mask (the alignment gaps between them are
    never read and hold whatever the staging buffer held)."""
    buf = packed.staging.cpu().numpy()
    N = packed.n_sub
    desc = buf[:N * 128].view(np.int32).reshape(N, 32)
    pix = buf[packed.head:]
    out = [buf[:packed.head].copy()]
    for d in desc:
        w, h = int(d[1]), int(d[2])
        out.append(pix[d[0] * 16:d[0] * 16 + 3 * w * h].copy())
        out.append(pix[d[5] * 16:d[5] * 16 + w * h].copy())
    return out


def reference_copy_paste():
    """The reference's own copy_paste module, loaded BY FILE PATH (its package __init__ imports cv2), or None when no reference checkout
    lies next to this repository (or where ZUTIS_REFERENCE_DIR points)."""
    base = os.environ.get("ZUTIS_REFERENCE_DIR") or os.path.join(os.path.dirname(ROOT), "reference")
    path = os.path.join(base, "datasets", "augmentations", "copy_paste.py")
    if not os.path.exists(path):
        return None
    spec = importlib.util.spec_from_file_location("zutis_reference_copy_paste", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod
