"""Training samples on the device: IndexDataset.__getitem__ (datasets/index_dataset.py:301-385) from files, as a recipe + kernels.

The reference builds one 384 x 384 sample on the host from 1 - 10 files: random_scale / random_crop / random_hflip
(datasets/augmentations/geometric_transforms.py), ColorJitter + RandomGrayscale + a 39-tap cv2.GaussianBlur
(datasets/base_dataset.py:62-78), to_tensor + normalize, then copy_paste (datasets/augmentations/copy_paste.py).  Here:

  SampleRecipe / SubRecipe   every random draw of one sample, separated from the pixel work: plain picklable data
  draw_recipe                draws a recipe with the reference's distributions (NOT its RNG streams) from one random.Random
  *_np                       NumPy restatements of every stage — the CPU tests pin them against Pillow / torch / the reference's own
                             copy_paste, the GPU tests compare the kernels against them; sample_np chains them into one sample
  pack_arrays / synthesize   a batch of recipes + decoded bytes -> the collate_fn batch on the device (csrc/synth.hip)
  TrainBatchLoader           recipes drawn on the main thread from one seeded generator, files decoded by threads one batch ahead
                             into pinned staging, one host-to-device copy per batch
  dataset_train_batches      the adapter for an IndexDataset-shaped object

Contract: the same distributions, and the same pixels for the same recipe — bit for bit, except the blur (fp32 sums of the ideal
Gaussian: within one level of its float64 evaluation; cv2's own 8-bit path is not available to compare with).
"""
from __future__ import annotations

import collections
import dataclasses
import functools
import json
import math
import random
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from . import preprocess, rle

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # IndexDataset.mean / .std (datasets/index_dataset.py:43)
MAX_SUB = 64                    # sub-images per sample the compose kernel serves (csrc/synth.hip SY_MAX_SUB)
BLUR_RMAX = 48                  # blur radius the kernel serves (SY_BLUR_RMAX)
DESC_INTS, WORK_INTS, SAMPLE_INTS = 32, 12, 4
F_JITTER, F_GREY, F_BLUR, F_PADDED = 1, 2, 4, 8
OPS = ("brightness", "contrast", "saturation", "hue")           # ColorJitter's fn_idx 0 .. 3
# random_crop's corner chain (geometric_transforms.py:33-40) draws random() AGAIN in every elif, so the corners are not 1/4 each:
# P(0) = 1/4, P(1) = 3/4 * 1/4, P(2) = (3/4)^2 * 1/4 and the else branch takes the rest, (3/4)^3.
CORNER_P = (0.25, 0.75 * 0.25, 0.75 * 0.75 * 0.25, 0.75 ** 3)
# corner -> (pad on the left, pad on the top): [pad_w, pad_h, 0, 0], [pad_w, 0, 0, pad_h], [0, pad_h, pad_w, 0], [0, 0, pad_w, pad_h]
CORNER_LEFT_TOP = ((True, True), (True, False), (False, True), (False, False))


# ------------------------------------------------------------------------------------------------------------------ the recipe
@dataclasses.dataclass
class SubRecipe:
    """One sub-image of a sample: its files and every draw the reference makes for it."""
    p_image: str
    p_mask: str
    label_id: int
    size: Tuple[int, int]               # (w, h) of the file
    scaled: Tuple[int, int]             # (int(w * s), int(h * s)): random_scale
    corner: int                         # which corner takes the padding (CORNER_LEFT_TOP)
    u_crop_top: float                   # unit-interval draws, resolved as floor(u * (range + 1)) once the range is known
    u_crop_left: float
    flip: bool
    jitter: bool                        # RandomApply([ColorJitter], p=0.8)
    order: Tuple[int, int, int, int]    # permutation of OPS
    brightness: float
    contrast: float
    saturation: float
    hue_shift: int                      # the uint8 that adjust_hue adds to the H plane: np.uint8(hue_factor * 255)
    grey: bool
    blur: bool
    sigma: float
    u_paste_top: float
    u_paste_left: float


@dataclasses.dataclass
class SampleRecipe:
    subs: List[SubRecipe]
    crop_size: int
    ignore_index: int

    @property
    def category_ids(self) -> List[int]:
        return [s.label_id for s in self.subs]


@dataclasses.dataclass
class DatasetFields:
    """What IndexDataset.__getitem__ reads from `self`."""
    p_images: List[str]
    p_pseudo_masks: List[str]
    p_image_to_label_id: Dict[str, int]
    category_to_p_images: Dict[str, List[str]]
    ignore_index: int
    max_n_masks: int = 10
    scale_range: Optional[Tuple[float, float]] = (0.1, 1.0)
    crop_size: Optional[int] = 384
    random_duplicate: bool = False
    mean: Tuple[float, float, float] = MEAN
    std: Tuple[float, float, float] = STD

    @classmethod
    def from_dataset(cls, ds) -> "DatasetFields":
        return cls(list(ds.p_images), list(ds.p_pseudo_masks), dict(ds.p_image_to_label_id), dict(ds.category_to_p_images),
                   int(ds.ignore_index), int(ds.max_n_masks), ds.scale_range, ds.crop_size, bool(ds.random_duplicate),
                   tuple(getattr(ds, "mean", MEAN)), tuple(getattr(ds, "std", STD)))

    def check(self):
        """The device path restates the reference's DEFAULT pipeline: both geometric arguments set."""
        if self.crop_size is None:
            raise NotImplementedError("zutis_amd.synth: crop_size=None (samples of the files' own sizes) is not served by the device path")
        if self.scale_range is None:
            raise NotImplementedError("zutis_amd.synth: scale_range=None (no random_scale) is not served by the device path")
        if not 1 < int(self.ignore_index) <= 255:
            raise ValueError(f"zutis_amd.synth: ignore_index {self.ignore_index} outside (1, 255]: the mask travels as a byte")
        if len(self.p_images) != len(self.p_pseudo_masks) or not self.p_images:
            raise ValueError("zutis_amd.synth: one pseudo-mask path per image, at least one image")
        if not 1 <= int(self.max_n_masks) <= MAX_SUB:
            raise ValueError(f"zutis_amd.synth: max_n_masks {self.max_n_masks} outside [1, {MAX_SUB}]")


def image_size(path: str) -> Tuple[int, int]:
    with Image.open(path) as im:                # header only
        return im.size


def resolve(u: float, span: int) -> int:
    """randint(0, span) from a unit-interval draw: floor(u * (span + 1)) in float64 — the rule of the kernels and of the host chain."""
    return int(math.floor(float(u) * float(span + 1)))


def blur_ksize(crop_size: int) -> int:
    """datasets/base_dataset.py:77: int((0.1 * min(w, h) // 2 * 2) + 1) — 39 at 384."""
    return int((0.1 * crop_size // 2 * 2) + 1)


def hue_shift(hue_factor: float) -> int:
    """torchvision adjust_hue on a PIL image: np_h += np.uint8(hue_factor * 255) — the C cast truncates towards zero, then wraps."""
    return int(hue_factor * 255) & 0xFF


def draw_recipe(rng: random.Random, fields: DatasetFields, size_of: Callable[[str], Tuple[int, int]] = image_size) -> SampleRecipe:
    """One sample's draws with the distributions of IndexDataset.__getitem__ and the transforms it calls (the reference's RNG STREAMS —
    Python random, torch and NumPy interleaved — are not reproduced).  size_of(path) -> (w, h): the scaled size needs the file's own."""
    fields.check()
    n_masks = rng.randint(1, fields.max_n_masks)                            # index_dataset.py:309
    category = None
    if fields.random_duplicate and rng.random() > 0.5:                      # :315-317
        category = rng.choice(list(fields.category_to_p_images.keys()))
        assert category != "background", ValueError(category)
    mask_of = None
    subs = []
    for _ in range(n_masks):
        if category is not None:                                            # :322-326
            pool = fields.category_to_p_images[category]
            p_image = pool[rng.randint(0, len(pool) - 1)]
            if mask_of is None:
                mask_of = dict(zip(fields.p_images, fields.p_pseudo_masks))
            p_mask = mask_of[p_image]
        else:                                                               # :328-331
            i = rng.randint(0, len(fields.p_images) - 1)
            p_image, p_mask = fields.p_images[i], fields.p_pseudo_masks[i]
        w, h = size_of(p_image)
        s = rng.uniform(*fields.scale_range)                                # random_scale
        nw, nh = int(w * s), int(h * s)
        if nw < 1 or nh < 1:
            raise ValueError(f"{p_image}: {w} x {h} scaled by {s} has an empty side (Pillow refuses it in the reference too)")
        # random_crop's chain AS WRITTEN: every condition draws again (see CORNER_P)
        if rng.random() < 0.25:
            corner = 0
        elif 0.25 <= rng.random() < 0.5:
            corner = 1
        elif 0.5 <= rng.random() < 0.75:
            corner = 2
        else:
            corner = 3
        u_top, u_left = rng.random(), rng.random()
        flip = rng.random() > 0.5                                           # random_hflip(p=0.5): flips when random() > p
        jitter = rng.random() <= 0.8                                        # RandomApply: skipped when p < rand
        order = list(range(4))
        rng.shuffle(order)                                                  # ColorJitter.get_params: randperm(4), then the four factors
        b, c, sat = rng.uniform(0.2, 1.8), rng.uniform(0.2, 1.8), rng.uniform(0.2, 1.8)
        hue = rng.uniform(-0.2, 0.2)
        grey = rng.random() < 0.2                                           # RandomGrayscale(0.2)
        blur = rng.random() < 0.5                                           # gaussian_blur.py:19-21
        sigma = (2.0 - 0.1) * rng.random() + 0.1
        subs.append(SubRecipe(p_image, p_mask, int(fields.p_image_to_label_id[p_image]), (w, h), (nw, nh), corner, u_top, u_left, flip,
                              jitter, tuple(order), b, c, sat, hue_shift(hue), grey, blur, sigma, rng.random(), rng.random()))
    return SampleRecipe(subs, int(fields.crop_size), int(fields.ignore_index))


# ------------------------------------------------------------------------------------------------- host restatements of the stages
def nearest_index(in_size: int, out_size: int) -> np.ndarray:
    """ATen nearest: src = min(floor(dst * scale), in - 1), scale = float32(in) / float32(out), the product in fp32."""
    scale = np.float32(in_size) / np.float32(out_size)
    return np.minimum(np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64), in_size - 1)


def resize_nearest_np(mask: np.ndarray, nw: int, nh: int) -> np.ndarray:
    return mask[nearest_index(mask.shape[0], nh)[:, None], nearest_index(mask.shape[1], nw)[None, :]]


def fill_colour(scaled_u8: np.ndarray) -> np.ndarray:
    """np.array(image).mean(axis=(0, 1)).astype(np.uint8) as an integer channel sum and an integer division (csrc/synth.hip has the
    argument why the truncated float64 mean is that byte)."""
    return (scaled_u8.reshape(-1, 3).astype(np.int64).sum(0) // (scaled_u8.shape[0] * scaled_u8.shape[1])).astype(np.uint8)


def crop_window(sub: SubRecipe, C: int):
    """(pad_left, pad_top, crop_left, crop_top) of random_crop for the recipe's scaled size."""
    nw, nh = sub.scaled
    pad_w, pad_h = max(C - nw, 0), max(C - nh, 0)
    on_left, on_top = CORNER_LEFT_TOP[sub.corner]
    top, left = resolve(sub.u_crop_top, nh + pad_h - C), resolve(sub.u_crop_left, nw + pad_w - C)
    return (pad_w if on_left else 0), (pad_h if on_top else 0), left, top


def geometry_np(image_u8: np.ndarray, mask_u8: np.ndarray, sub: SubRecipe, C: int, ignore_index: int, resize=None):
    """random_scale + random_crop + random_hflip of one sub-image: (u8 [C, C, 3], u8 [C, C]).  resize(a, nw, nh): Pillow's BILINEAR
    (default: preprocess.pil_resize_reference, its NumPy restatement)."""
    nw, nh = sub.scaled
    if resize is None:
        resize = lambda a, w_, h_: preprocess.pil_resize_reference(a, w_, h_, "bilinear")       # noqa: E731
    scaled = resize(image_u8, nw, nh)
    smask = resize_nearest_np(mask_u8, nw, nh)
    pad_left, pad_top, left, top = crop_window(sub, C)
    pw, ph = nw + max(C - nw, 0), nh + max(C - nh, 0)
    canvas = np.empty((ph, pw, 3), np.uint8)
    canvas[...] = fill_colour(scaled)
    cmask = np.full((ph, pw), ignore_index, np.uint8)
    canvas[pad_top:pad_top + nh, pad_left:pad_left + nw] = scaled
    cmask[pad_top:pad_top + nh, pad_left:pad_left + nw] = smask
    img, m = canvas[top:top + C, left:left + C], cmask[top:top + C, left:left + C]
    if sub.flip:
        img, m = img[:, ::-1], m[:, ::-1]
    return np.ascontiguousarray(img), np.ascontiguousarray(m)


def blend_u8(a, b, f: float) -> np.ndarray:
    """Image.blend(a, b, f) (Pillow Blend.c): a + f * (b - a) in fp32, truncated for 0 <= f <= 1, otherwise clipped to [0, 255] first."""
    f = np.float32(f)
    a, b = np.asarray(a, np.int32), np.asarray(b, np.int32)
    v = a.astype(np.float32) + f * (b - a).astype(np.float32)
    if not 0.0 <= f <= 1.0:
        v = np.clip(v, 0, 255)
    return v.astype(np.int32).astype(np.uint8)


def grey_u8(rgb: np.ndarray) -> np.ndarray:
    """Image.convert("L")."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)


def contrast_mean(rgb: np.ndarray) -> int:
    """ImageEnhance.Contrast: int(ImageStat.Stat(image.convert("L")).mean[0] + 0.5), in integers."""
    g = grey_u8(rgb)
    return int((2 * int(g.astype(np.int64).sum()) + g.size) // (2 * g.size))


def rgb_to_hsv_u8(rgb: np.ndarray) -> np.ndarray:
    """Image.convert("HSV") (Pillow Convert.c rgb2hsv_row), its float / double steps one by one."""
    f32, f64 = np.float32, np.float64
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    cr = (maxc - minc).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = cr / maxc.astype(f32)
        rc, gc, bc = ((maxc - c).astype(f32) / cr for c in (r, g, b))
        h = np.where(r == maxc, bc - gc, np.where(g == maxc, (2.0 + rc.astype(f64) - bc.astype(f64)).astype(f32),
                                                  (4.0 + gc.astype(f64) - rc.astype(f64)).astype(f32)))
        h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
        flat = maxc == minc
        uh = np.clip((np.where(flat, 0, h).astype(f64) * 255.0).astype(np.int64), 0, 255)
        us = np.clip((np.where(flat, 0, s).astype(f64) * 255.0).astype(np.int64), 0, 255)
    return np.stack([uh, us, maxc], -1).astype(np.uint8)


def hsv_to_rgb_u8(hsv: np.ndarray) -> np.ndarray:
    """Image.convert("RGB") of an HSV image (Pillow Convert.c hsv2rgb): p, q, t rounded half away from zero in double; fs * f is an fp32
    product, the other two factors are formed in double."""
    f32, f64 = np.float32, np.float64
    h, s, v = (hsv[..., i] for i in range(3))
    hf = h.astype(f32).astype(f64) * 6.0 / 255.0
    i = np.floor(hf)
    f = (hf - i.astype(f32).astype(f64)).astype(f32)
    fs = (s.astype(f32).astype(f64) / 255.0).astype(f32)
    vf = v.astype(f64)

    def rnd(x):
        return np.clip(np.floor(x + 0.5), 0, 255).astype(np.uint8)

    p = rnd(vf * (1.0 - fs.astype(f64)))
    q = rnd(vf * (1.0 - (fs * f).astype(f64)))
    t = rnd(vf * (1.0 - fs.astype(f64) * (1.0 - f.astype(f64))))
    i = i.astype(np.int64) % 6
    r, g, b = np.choose(i, [v, q, p, p, t, v]), np.choose(i, [t, v, v, q, p, p]), np.choose(i, [p, p, t, v, v, q])
    grey = s == 0
    return np.stack([np.where(grey, v, r), np.where(grey, v, g), np.where(grey, v, b)], -1).astype(np.uint8)


def adjust_hue_u8(rgb: np.ndarray, shift: int) -> np.ndarray:
    hsv = rgb_to_hsv_u8(rgb)
    hsv[..., 0] += np.uint8(shift)                  # wraps mod 256
    return hsv_to_rgb_u8(hsv)


def photometric_np(rgb: np.ndarray, sub: SubRecipe) -> np.ndarray:
    """ColorJitter (when applied) in the recipe's order, then RandomGrayscale, on a u8 [.., .., 3] image."""
    img = np.ascontiguousarray(rgb)
    if sub.jitter:
        for op in sub.order:
            if op == 0:
                img = blend_u8(0, img, sub.brightness)
            elif op == 1:
                img = blend_u8(contrast_mean(img), img, sub.contrast)
            elif op == 2:
                img = blend_u8(grey_u8(img)[..., None], img, sub.saturation)
            else:
                img = adjust_hue_u8(img, sub.hue_shift)
    if sub.grey:
        img = np.repeat(grey_u8(img)[..., None], 3, axis=-1)
    return img


def gaussian_weights(ksize: int, sigma: float) -> np.ndarray:
    """exp(-x^2 / 2 sigma^2) normalised to sum 1, float64."""
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2
    w = np.exp(-(x * x) / (2.0 * float(sigma) ** 2))
    return w / w.sum()


def gaussian_blur_f64(rgb: np.ndarray, ksize: int, sigma: float) -> np.ndarray:
    """The separable Gaussian with BORDER_REFLECT_101 in float64, unrounded: [H, W, 3]."""
    w, r = gaussian_weights(ksize, sigma), ksize // 2
    a = np.pad(rgb.astype(np.float64), ((r, r), (r, r), (0, 0)), mode="reflect")
    H, W = rgb.shape[:2]
    hp = sum(w[t] * a[:, t:t + W] for t in range(ksize))
    return sum(w[t] * hp[t:t + H] for t in range(ksize))


def gaussian_blur_np(rgb: np.ndarray, ksize: int, sigma: float) -> np.ndarray:
    return np.clip(np.rint(gaussian_blur_f64(rgb, ksize, sigma)), 0, 255).astype(np.uint8)


def object_box(mask_u8: np.ndarray, label: int, ignore_index: int):
    """mask_to_bbox of copy_paste's object test 0 < semantic < ignore_index: (ymin, ymax, xmin, xmax), maxima as the reference uses them
    (EXCLUSIVE slice ends: the object's last row and column are never pasted), None for an empty object."""
    obj = (mask_u8 == 1) & (0 < label < ignore_index)
    ys, xs = np.nonzero(obj)
    if ys.size == 0:
        return None
    return int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())


def paste_offsets(masks: Sequence[np.ndarray], recipe: SampleRecipe) -> List[Optional[Tuple[int, int]]]:
    """(offset_top, offset_left) of every sub-image j >= 1 that pastes, None for an empty object (entry 0 is None)."""
    C, out = recipe.crop_size, [None]
    for m, s in zip(masks[1:], recipe.subs[1:]):
        box = object_box(m, s.label_id, recipe.ignore_index)
        out.append(None if box is None else (resolve(s.u_paste_top, C - (box[1] - box[0])), resolve(s.u_paste_left, C - (box[3] - box[2]))))
    return out


def compose_np(images: Sequence[np.ndarray], masks: Sequence[np.ndarray], recipe: SampleRecipe):
    """copy_paste stated per OUTPUT pixel: the winner is the last sub-image j >= 1 whose shifted object region covers the pixel, else 0.
    images [n][C, C, K] (any dtype), masks u8 [n][C, C] -> (image [C, C, K], semantic int64 [C, C], one-hot bool [n, C, C])."""
    C, ign, n = recipe.crop_size, recipe.ignore_index, len(images)
    win = np.zeros((C, C), np.int64)
    src_y, src_x = np.meshgrid(np.arange(C), np.arange(C), indexing="ij")
    src_y, src_x = src_y.copy(), src_x.copy()
    offs = paste_offsets(masks, recipe)
    for j in range(1, n):
        if offs[j] is None:
            continue
        ymin, ymax, xmin, xmax = object_box(masks[j], recipe.subs[j].label_id, ign)
        top, left = offs[j]
        region = masks[j][ymin:ymax, xmin:xmax] == 1
        ys, xs = np.nonzero(region)
        win[top + ys, left + xs] = j
        src_y[top + ys, left + xs] = ymin + ys
        src_x[top + ys, left + xs] = xmin + xs
    stack_i, stack_m = np.stack(images), np.stack(masks)
    image = stack_i[win, src_y, src_x]
    m = stack_m[win, src_y, src_x].astype(np.int64)
    labels = np.asarray([s.label_id for s in recipe.subs], np.int64)
    semantic = np.where(m == 1, labels[win], m)
    inst = np.where(m == 1, win + 1, m)
    return image, semantic, np.stack([inst == k + 1 for k in range(n)])


def normalise_np(rgb_u8: np.ndarray, lut: np.ndarray) -> np.ndarray:
    """to_tensor + normalize through preprocess.normalise_table: u8 [H, W, 3] -> f32 [3, H, W]."""
    return np.stack([lut[c][rgb_u8[..., c]] for c in range(3)])


def load_files(sub: SubRecipe):
    """(u8 [h, w, 3], u8 [h, w]) of a sub-image's files: index_dataset.py:333-334."""
    image = np.asarray(Image.open(sub.p_image).convert("RGB"))
    with open(sub.p_mask) as f:
        mask = rle.decode_np(json.load(f))
    if mask.shape != image.shape[:2]:
        raise ValueError(f"{sub.p_mask}: mask {mask.shape} for an image of {image.shape[:2]}")
    return image, mask


def sample_np(recipe: SampleRecipe, arrays=None, mean=MEAN, std=STD, resize=None, blur: bool = True, stages: bool = False):
    """The whole host chain of one sample — the CPU oracle of the device path, and the stand-in of tools/synth_bench.py.  arrays:
    [(image u8, mask u8)] per sub-image (default: read from the recipe's files).  blur=False skips the blur stage whatever the recipe says.
    -> {"image" f32 [3, C, C], "semantic_mask" int64, "instance_mask" bool [n, C, C], "category_ids"}; stages=True adds "u8": the
    sub-images after the blur stage and "masks"."""
    C = recipe.crop_size
    lut = preprocess.normalise_table(mean, std)
    imgs, masks = [], []
    for k, sub in enumerate(recipe.subs):
        image, mask = load_files(sub) if arrays is None else arrays[k]
        img, m = geometry_np(image, mask, sub, C, recipe.ignore_index, resize)
        img = photometric_np(img, sub)
        if blur and sub.blur:
            img = gaussian_blur_np(img, blur_ksize(C), sub.sigma)
        imgs.append(img)
        masks.append(m)
    u8, semantic, onehot = compose_np(imgs, masks, recipe)
    out = {"image": normalise_np(u8, lut), "semantic_mask": semantic, "instance_mask": onehot, "category_ids": recipe.category_ids}
    if stages:
        out["u8"], out["masks"] = imgs, masks
    return out


# ------------------------------------------------------------------------------------------------------------ the device path
Packed = collections.namedtuple("Packed", "staging head n_sub n_samples crop_size ignore_index ksize kmax fill_wh n_host")
Packed.__doc__ = """A batch laid out for the kernels.  staging: u8 tensor = [head | pixel bytes] (host, pinned when the loader pins, or
device); head: its size in bytes — descriptor rows int32 [N, 32], sample rows int32 [B, 4], the work rows' initial values int32 [N, 12],
the blur weights f32 [N, ksize], padded to 16 bytes; then every sub-image's [h, w, 3] image and [h, w] mask at 16-byte-aligned offsets
(relative to the end of the head).  kmax: the largest tap count; fill_wh: the largest scaled extent among the padded sub-images;
n_host: sub-images scaled on the host (outside the kernel's tap envelope)."""


def _bits32(x: float) -> int:
    return int(np.float32(x).view(np.int32))


def _layout(recipes: Sequence[SampleRecipe]):
    """The head (as an int32 array) and, per sub-image, (image offset, mask offset, w, h, host_scaled) of a batch of recipes."""
    subs = [s for r in recipes for s in r.subs]
    N, B = len(subs), len(recipes)
    if B == 0:
        raise ValueError("zutis_amd.synth: empty batch")
    C, ign = recipes[0].crop_size, recipes[0].ignore_index
    if any(r.crop_size != C or r.ignore_index != ign for r in recipes):
        raise ValueError("zutis_amd.synth: one crop_size and ignore_index per batch")
    if not 1 < ign <= 255:
        raise ValueError(f"zutis_amd.synth: ignore_index {ign} outside (1, 255]")
    if any(not 1 <= len(r.subs) <= MAX_SUB for r in recipes):
        raise ValueError(f"zutis_amd.synth: a sample has 1 .. {MAX_SUB} sub-images")
    ks = blur_ksize(C)
    if ks // 2 > BLUR_RMAX or ks // 2 >= C:
        raise NotImplementedError(f"zutis_amd.synth: crop_size {C} gives a {ks}-tap blur, the kernel serves {2 * BLUR_RMAX + 1}")
    desc = np.zeros((N, DESC_INTS), np.int32)
    work = np.zeros((N, WORK_INTS), np.int32)
    work[:, 8:] = (C, -1, C, -1)
    weights = np.zeros((N, ks), np.float32)
    samples = np.zeros((B, SAMPLE_INTS), np.int32)
    items, off, kmax, fill_w, fill_h, first = [], 0, 3, 0, 0, 0
    for b, r in enumerate(recipes):
        samples[b] = (first, len(r.subs), first, 0)
        first += len(r.subs)
    for n, s in enumerate(subs):
        (w, h), (nw, nh) = s.size, s.scaled
        host = not preprocess._taps_ok(w, h, nw, nh, "bilinear")
        if host:                                    # scaled by Pillow in the decode worker, packed as an identity image
            w, h = nw, nh
        kmax = max(kmax, preprocess.ksize(w, nw, "bilinear"), preprocess.ksize(h, nh, "bilinear"))
        img_off = off
        off += -(-3 * w * h // 16) * 16
        mask_off = off
        off += -(-w * h // 16) * 16
        pad_left, pad_top, left, top = crop_window(s, C)
        padded = nw < C or nh < C
        if padded:
            fill_w, fill_h = max(fill_w, nw), max(fill_h, nh)
        flags = (F_JITTER if s.jitter else 0) | (F_GREY if s.grey else 0) | (F_BLUR if s.blur else 0) | (F_PADDED if padded else 0)
        order = sum(int(op) << (2 * k) for k, op in enumerate(s.order))
        d = desc[n]
        d[:20] = (img_off // 16, w, h, nw, nh, mask_off // 16, pad_left, pad_top, left, top, int(s.flip), s.label_id, flags, order,
                  s.hue_shift & 0xFF, _bits32(s.brightness), _bits32(s.contrast), _bits32(s.saturation),
                  _bits32(np.float32(h) / np.float32(nh)), _bits32(np.float32(w) / np.float32(nw)))
        d[20:24] = np.asarray([s.u_paste_top, s.u_paste_left], np.float64).view(np.int32)
        weights[n] = gaussian_weights(ks, s.sigma)
        items.append((img_off, mask_off, w, h, host))
    head = np.concatenate([desc.reshape(-1), samples.reshape(-1), work.reshape(-1), weights.view(np.int32).reshape(-1)])
    head = np.concatenate([head, np.zeros(-head.size % 4, np.int32)])
    return head, items, off, (N, B, C, ign, ks, kmax, (fill_w, fill_h))


def _place(dst_img: np.ndarray, dst_mask: np.ndarray, image: np.ndarray, mask: np.ndarray, sub: SubRecipe, host: bool):
    """Copy one sub-image's decoded arrays into its staging slices (scaled here first when the kernel does not serve its taps)."""
    if mask.shape != image.shape[:2] or (image.shape[1], image.shape[0]) != tuple(sub.size):
        raise ValueError(f"{sub.p_image}: image {image.shape[:2]} / mask {mask.shape} for a recipe size (w, h) = {sub.size}")
    if host:
        nw, nh = sub.scaled
        image = np.asarray(Image.fromarray(image).resize((nw, nh), Image.BILINEAR))
        mask = resize_nearest_np(mask, nw, nh)
    np.copyto(dst_img, image)
    np.copyto(dst_mask, mask)


def _views(pix: np.ndarray, item):
    img_off, mask_off, w, h, _ = item
    return pix[img_off:img_off + 3 * w * h].reshape(h, w, 3), pix[mask_off:mask_off + w * h].reshape(h, w)


def pack_arrays(recipes: Sequence[SampleRecipe], arrays: Sequence[Sequence]) -> Packed:
    """Packed for recipes whose sub-images are given as arrays: arrays[b][k] = (image u8 [h, w, 3], mask u8 [h, w])."""
    head, items, nbytes, (N, B, C, ign, ks, kmax, fill) = _layout(recipes)
    staging = torch.zeros(head.size * 4 + nbytes, dtype=torch.uint8)
    buf = staging.numpy()
    buf[:head.size * 4] = head.view(np.uint8)
    pix = buf[head.size * 4:]
    flat = [(a, s) for r, arr in zip(recipes, arrays) for a, s in zip(arr, r.subs)]
    for item, ((image, mask), sub) in zip(items, flat):
        _place(*_views(pix, item), np.asarray(image, np.uint8), np.asarray(mask, np.uint8), sub, item[4])
    return Packed(staging, head.size * 4, N, B, C, ign, ks, kmax, fill, sum(i[4] for i in items))


_LUTS: Dict = {}


def _lut(mean, std, dev) -> torch.Tensor:
    key = (tuple(float(m) for m in mean), tuple(float(s) for s in std), str(dev))
    if key not in _LUTS:
        _LUTS[key] = torch.from_numpy(preprocess.normalise_table(mean, std)).to(dev)
    return _LUTS[key]


def device_views(packed: Packed, staged: torch.Tensor):
    """(desc [N, 32], samples [B, 4], work [N, 12] (a fresh copy the kernels write), weights [N, ks], pixel bytes) of a staging tensor."""
    N, B, ks = packed.n_sub, packed.n_samples, packed.ksize
    ints = staged[:packed.head].view(torch.int32)
    a, b, c = N * DESC_INTS, N * DESC_INTS + B * SAMPLE_INTS, N * DESC_INTS + B * SAMPLE_INTS + N * WORK_INTS
    return (ints[:a].view(N, DESC_INTS), ints[a:b].view(B, SAMPLE_INTS), ints[b:c].view(N, WORK_INTS).clone(),
            ints[c:c + N * ks].view(torch.float32).view(N, ks), staged[packed.head:])


def synthesize(decoded: Packed, recipes: Sequence[SampleRecipe], mean=MEAN, std=STD, device=None, blur: bool = True, stages: bool = False) -> dict:
    """The collate_fn batch of `recipes` (datasets/index_dataset.py:279-296) on the device, from `decoded` (pack_arrays or
    TrainBatchLoader): {"image" f32 [B, 3, C, C], "semantic_mask" int64 [B, C, C], "instance_mask": [bool [n_i, C, C]],
    "category_ids": [[int]]}.  Six launches per batch (csrc/synth.hip); there is no host fallback.  blur=False skips the blur stage for
    every sub-image (then the result is bit-identical to sample_np(..., blur=False)); stages=True adds "u8": the u8 [N, C, C, 4]
    (R, G, B, mask) sub-images after the blur stage."""
    from . import ops
    if len(recipes) != decoded.n_samples or sum(len(r.subs) for r in recipes) != decoded.n_sub:
        raise ValueError("synthesize: `decoded` was not packed for these recipes")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        staged = decoded.staging if decoded.staging.is_cuda else decoded.staging.to(dev, non_blocking=True)
        desc, samples, work, weights, pix = device_views(decoded, staged)
        N, B, C = decoded.n_sub, decoded.n_samples, decoded.crop_size
        if not blur:
            desc = desc.clone()
            desc[:, 12] &= ~F_BLUR
        rgbm = ops.synth_geometry(pix, desc, C, decoded.ignore_index, decoded.kmax, decoded.fill_wh, work)
        ops.synth_photometric(rgbm, desc, work)
        any_blur = blur and any(s.blur for r in recipes for s in r.subs)
        blurred = ops.synth_blur(rgbm, desc, weights) if any_blur else rgbm
        image, semantic, onehot = ops.synth_compose(rgbm, blurred, desc, samples, work, _lut(mean, std, dev), decoded.ignore_index)
    counts = [len(r.subs) for r in recipes]
    out = {"image": image, "semantic_mask": semantic, "instance_mask": list(torch.split(onehot, counts, 0)),
           "category_ids": [r.category_ids for r in recipes]}
    if stages:
        flags = desc[:, 12].bitwise_and(F_BLUR).bool().view(N, 1, 1, 1)
        out["u8"] = torch.where(flags, blurred.view(N, C, C, 4), rgbm.view(N, C, C, 4)) if any_blur else rgbm.view(N, C, C, 4)
    return out


# ------------------------------------------------------------------------------------------------------------------ the loader
class TrainBatch(collections.namedtuple("TrainBatch", "recipes packed")):
    __slots__ = ()
    staging = property(lambda self: self.packed.staging)        # what preprocess.device_batches copies to the device


class TrainBatchLoader:
    """Batches of training samples from files.  Recipes are drawn on the MAIN thread from one random.Random(seed), so the batches do not
    depend on n_workers; min(n_workers, 16) threads open and decode the images (Pillow releases the GIL) and RLE-decode the masks of the
    NEXT batch straight into one of two reused (pinned) staging buffers while the caller works on the current one — the loop and the
    buffers of every loader (preprocess.prefetch, preprocess.DoubleBuffer).  Iterating yields TrainBatch(recipes, packed) for
    synthesize(); batches() yields synthesize()'s dicts, one host-to-device
    copy each.  The caller must be done with a batch's staging (its copy complete) before it advances the loader.  `n_batches`: the
    length of one pass (default: ceil(len(p_images) / batch_size), the reference's DataLoader length)."""

    def __init__(self, dataset_fields: DatasetFields, batch_size: int, n_workers: int = 16, seed: int = 0, n_batches: Optional[int] = None, pin=None):
        dataset_fields.check()
        if batch_size < 1:
            raise ValueError("TrainBatchLoader: batch_size must be positive")
        self.fields, self.batch_size, self.seed = dataset_fields, int(batch_size), seed
        self.n_threads = max(1, min(int(n_workers), preprocess.MAX_THREADS))
        self.n_batches = -(-len(dataset_fields.p_images) // self.batch_size) if n_batches is None else int(n_batches)
        self.pin = torch.cuda.is_available() if pin is None else bool(pin)
        self._staging = preprocess.DoubleBuffer(self.pin)
        self._sizes: Dict[str, Tuple[int, int]] = {}

    def __len__(self):
        return self.n_batches

    def _size_of(self, path: str):
        if path not in self._sizes:
            self._sizes[path] = image_size(path)
        return self._sizes[path]

    @staticmethod
    def _decode(sub: SubRecipe, dst_img, dst_mask, host):
        _place(dst_img, dst_mask, *load_files(sub), sub, host)

    def _start(self, rng: random.Random, pool: ThreadPoolExecutor, slot: int, k: int):
        recipes = [draw_recipe(rng, self.fields, self._size_of) for _ in range(self.batch_size)]
        head, items, nbytes, (N, B, C, ign, ks, kmax, fill) = _layout(recipes)
        staging = self._staging.take(slot, head.size * 4 + nbytes)
        buf = staging.numpy()
        buf[:head.size * 4] = head.view(np.uint8)
        pix = buf[head.size * 4:]
        subs = [s for r in recipes for s in r.subs]
        futures = [pool.submit(self._decode, s, *_views(pix, item), item[4]) for s, item in zip(subs, items)]
        packed = Packed(staging, head.size * 4, N, B, C, ign, ks, kmax, fill, sum(i[4] for i in items))
        return TrainBatch(recipes, packed), futures

    def __iter__(self):
        return preprocess.prefetch(range(self.n_batches), functools.partial(self._start, random.Random(self.seed)), self.n_threads)

    def batches(self, device=None):
        """synthesize() of every batch: the dicts IndexDataset.collate_fn returns, on the device (`device` is the current one while the
        generator is open)."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)

        def transform(batch, staged):
            return None, synthesize(batch.packed._replace(staging=staged), batch.recipes, self.fields.mean, self.fields.std, dev)

        with preprocess.device_batches(self, dev, transform) as steps:
            for _, _, out in steps:
                yield out


def dataset_train_batches(self, batch_size: int, n_workers: int = 16, seed: int = 0, n_batches: Optional[int] = None, device=None):
    """The training batches of an IndexDataset-shaped object over the device path: what
    `DataLoader(dataset, batch_size, shuffle=True, num_workers=n_workers, collate_fn=dataset.collate_fn)` yields, with the samples built by
    csrc/synth.hip.  Bind it next to dataset_generate_pseudo_masks — `IndexDataset.train_batches = zutis_amd.synth.dataset_train_batches`
    — or call it with the dataset as `self`.  Reads p_images, p_pseudo_masks, p_image_to_label_id, category_to_p_images, ignore_index,
    max_n_masks, scale_range, crop_size, random_duplicate (and mean / std when present) from `self`, and `self.device` when `device` is
    not given.  crop_size=None and scale_range=None raise NotImplementedError.  A batch goes into HipCriterion unchanged."""
    fields = DatasetFields.from_dataset(self)
    fields.check()
    dev = device if device is not None else getattr(self, "device", None)
    return TrainBatchLoader(fields, batch_size, n_workers, seed, n_batches).batches(dev)
