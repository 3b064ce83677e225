"""Host side of the device pre-processing of embedding extraction (csrc/preprocess.hip, ops.resize_crop_normalize) and of pseudo-label
generation from files (ops.resize_normalize).

The reference feeds CLIP through SimpleDataset's transform (utils/extract_image_embeddings.py:97-103: Resize BICUBIC, CenterCrop,
ToTensor, Normalize) under a 16-worker DataLoader (:64-65).  Here the workers are THREADS that only open and decode (Pillow
releases the GIL while it decodes); the resize, crop and normalisation run in one kernel per batch on the decoded bytes, which
is also what crosses PCIe (3 bytes per source pixel instead of 12 per output pixel).

  pil_resize_reference  NumPy restatement of Pillow's 8-bit resampler (bicubic, bilinear) — the CPU oracle of the tests, not a product path
  normalise_table       the 3 x 256 fp32 table the kernel looks normalised values up in
  BatchLoader           paths -> batches of (packed bytes + descriptor rows) in reused staging buffers, decoded one batch ahead
  ShapeBucketLoader     the same staging for MaskDataset's transform (datasets/index_dataset.py:405-411): batches of ONE resized shape,
                        gathered from a bounded window of paths ahead, so that the batched SelfMask + solver run batched

  EvalBatchLoader       ShapeBucketLoader for evaluation: every image travels with its ground-truth PNG (one staging buffer, one copy)
  PredictBatchLoader    EvalBatchLoader's batches without the ground truth: images of one file size, for predictions at that size

Threads, not processes: no child ever holds the device open, nothing is pickled, a worker's exception is raised by the caller.
"""
from __future__ import annotations

import collections
import math
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, List, Sequence

import numpy as np
import torch
from PIL import Image

PRECISION_BITS = 32 - 8 - 2     # Pillow's fixed-point coefficients: src/libImaging/Resample.c
KMAX = 152                      # taps per output pixel the kernel serves (include/zutis_hip.h ZH_RCN_KMAX)
MAX_WORKERS = 16
ALIGN = 16                      # byte alignment of an image inside the packed buffer (descriptors hold offset / 16)
DESC_INTS = 8                   # offset / 16, w, h, nw, nh, left, top, 0


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


# Pillow's filters (src/libImaging/Resample.c: BICUBIC, BILINEAR): name -> (function, support, PIL.Image constant)
FILTERS = {"bicubic": (_bicubic, 2.0, Image.BICUBIC), "bilinear": (_bilinear, 1.0, Image.BILINEAR)}


def ksize(in_size: int, out_size: int, filter: str = "bicubic") -> int:
    """Taps per output pixel of Pillow's resampler for in_size -> out_size (its coefficient row length)."""
    return int(math.ceil(FILTERS[filter][1] * max(in_size / out_size, 1.0))) * 2 + 1


def pil_coefficients(in_size: int, out_size: int, filter: str = "bicubic"):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for `filter`: (K int64 [out, ksize], bounds int64 [out, 2] =
    (first source index, tap count)).  IEEE double, the weights summed in tap order, rounding half away from zero."""
    fn, filter_support, _ = FILTERS[filter]
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = filter_support * filterscale
    ks = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ks), np.int64)
    bounds = np.zeros((out_size, 2), np.int64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v /= ww
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return kk, bounds


def _pass(a: np.ndarray, out_size: int, filter: str) -> np.ndarray:
    """a u8 [L, in, C] -> u8 [L, out, C]: one resampling pass along axis 1."""
    kk, bounds = pil_coefficients(a.shape[1], out_size, filter)
    out = np.empty((a.shape[0], out_size, a.shape[2]), np.uint8)
    ai = a.astype(np.int64)
    for xx in range(out_size):
        xmin, n = bounds[xx]
        s = (1 << (PRECISION_BITS - 1)) + np.tensordot(ai[:, xmin:xmin + n, :], kk[xx, :n], ([1], [0]))
        out[:, xx, :] = np.clip(s >> PRECISION_BITS, 0, 255)
    return out


def pil_resize_reference(a_u8: np.ndarray, nw: int, nh: int, filter: str = "bicubic") -> np.ndarray:
    """Image.fromarray(a_u8).resize((nw, nh), Image.BICUBIC | Image.BILINEAR) for a u8 [h, w, C] array, byte for byte: horizontal pass to a u8
    intermediate, then vertical; a pass whose size does not change is skipped, as Pillow skips it."""
    a = np.ascontiguousarray(a_u8)
    if a.dtype != np.uint8 or a.ndim != 3:
        raise ValueError("pil_resize_reference: u8 [h, w, C] expected")
    h, w, _ = a.shape
    if nw != w:
        a = _pass(a, nw, filter)
    if nh != h:
        a = _pass(a.transpose(1, 0, 2), nh, filter).transpose(1, 0, 2)
    return np.ascontiguousarray(a)


def normalise_table(mean, std) -> np.ndarray:
    """fp32 [3, 256]: table[c][v] = (float32(v) / 255.0 - mean[c]) / std[c] in NumPy's fp32, the very expression the host
    pre-processing applies to a cropped image — gathering the table over the bytes gives its result bit for bit."""
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    a = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)          # [256, 3] as an H x W x 3 image row would be
    a = np.asarray(a, np.float32) / 255.0
    return np.ascontiguousarray(((a - mean) / std).T)


def _taps_ok(w: int, h: int, nw: int, nh: int, filter: str = "bicubic") -> bool:
    return ksize(w, nw, filter) <= KMAX and ksize(h, nh, filter) <= KMAX and 3 * w * h < 2 ** 31


def device_supported(w: int, h: int, n_px: int) -> bool:
    """Whether the kernel resizes a w x h source itself when its shorter side becomes n_px (Resize's convention): both axes within
    KMAX taps per output pixel (a shorter side up to ~37 x n_px: 8400 pixels at 224) and the packed image addressable.
    Anything else the loader resizes on the host."""
    nw, nh = (n_px, int(n_px * h / w)) if w <= h else (int(n_px * w / h), n_px)
    return nw > 0 and nh > 0 and _taps_ok(w, h, nw, nh)


Batch = collections.namedtuple("Batch", "paths staging packed desc kmax n_host")
Batch.__doc__ = """One decoded batch.  staging: u8 tensor [32 * B + pixel bytes] (pinned when the loader pins), descriptor rows first —
one host-to-device copy moves both; packed / desc: its two views (u8 [bytes], int32 [B, 8]), offsets relative to `packed`; kmax: the
batch's largest tap count; n_host: images that were resized on the host (outside device_supported).  Valid until the loader is advanced."""


def split_staging(staging: torch.Tensor, B: int):
    """(packed, desc) views of a staging tensor (host or device) laid out as BatchLoader lays it out."""
    return staging[B * DESC_INTS * 4:], staging[:B * DESC_INTS * 4].view(torch.int32).view(B, DESC_INTS)


class BatchLoader:
    """Iterate over `paths` in batches of `batch_size`: a pool of min(n_workers, 16) threads reads the headers, then decodes every
    image (`Image.open(p).convert("RGB")`) straight into its slice of one of two reused staging buffers; the next batch decodes while
    the caller works on the current one.  `box(w, h, n_px)` gives ((nw, nh), (left, top)) of the resize and crop.  An image the kernel
    does not serve (device_supported) is resized and cropped by Pillow in its worker and packed as an n_px x n_px image whose two
    passes are the identity.  The order of a batch is the order of its paths; a worker's exception (a missing or unreadable file) is
    raised by the iteration step that needs the batch, at the latest.
    The caller must be done reading a batch (its host-to-device copy complete) before it advances the loader."""

    def __init__(self, paths: Sequence[str], n_px: int, batch_size: int, n_workers: int, box: Callable, pin=None):
        if batch_size < 1 or n_px < 1:
            raise ValueError("BatchLoader: batch_size and n_px must be positive")
        self.paths, self.n_px, self.batch_size, self.box = list(paths), int(n_px), int(batch_size), box
        self.n_threads = max(1, min(int(n_workers), MAX_WORKERS))
        self.pin = torch.cuda.is_available() if pin is None else bool(pin)
        self.filter = "bicubic"
        self._buffers: List[torch.Tensor] = [torch.empty(0, dtype=torch.uint8), torch.empty(0, dtype=torch.uint8)]

    def __len__(self):
        return (len(self.paths) + self.batch_size - 1) // self.batch_size

    def _staging(self, slot: int, nbytes: int) -> torch.Tensor:
        """The slot's staging buffer, grown (from the calling thread) when the batch needs more."""
        if self._buffers[slot].numel() < nbytes:
            self._buffers[slot] = torch.empty(nbytes + nbytes // 4, dtype=torch.uint8, pin_memory=self.pin)
        return self._buffers[slot][:nbytes]

    @staticmethod
    def _size(path: str):
        with Image.open(path) as im:            # header only
            return im.size

    def _decode(self, path: str, dst: np.ndarray, size, host_box, out_wh):
        im = Image.open(path).convert("RGB")
        if im.size != size:
            raise ValueError(f"{path}: decoded size {im.size} differs from its header's {size}")
        if host_box is not None:
            (nw, nh), (left, top) = host_box
            im = im.resize((nw, nh), FILTERS[self.filter][2]).crop((left, top, left + out_wh[0], top + out_wh[1]))
        np.copyto(dst, np.asarray(im))

    def _pack(self, pool: ThreadPoolExecutor, slot: int, chunk, sizes, boxes, out_wh, extra: int = 0):
        """Lay `chunk` (files of `sizes` = (w, h), resized and cropped as `boxes` = ((nw, nh), (left, top)) say, to out_wh = (w, h) of the
        kernel's output) out in staging buffer `slot` and start its decodes: (staging, packed, desc, kmax, images resized on the host,
        futures).  extra: bytes the staging buffer holds behind the packed images (packed stops in front of them)."""
        B, (ow, oh) = len(chunk), out_wh
        rows = np.zeros((B, DESC_INTS), np.int32)
        host_boxes, shapes, kmax, off = [], [], ksize(1, 1, self.filter), 0
        for i, ((w, h), bx) in enumerate(zip(sizes, boxes)):
            (nw, nh), (left, top) = bx
            if _taps_ok(w, h, nw, nh, self.filter):
                host_boxes.append(None)
            else:
                host_boxes.append(bx)
                w, h, nw, nh = ow, oh, ow, oh
                left = top = 0
            kmax = max(kmax, ksize(w, nw, self.filter), ksize(h, nh, self.filter))
            rows[i] = (off // ALIGN, w, h, nw, nh, left, top, 0)
            shapes.append((off, h, w))
            off += -(-3 * w * h // ALIGN) * ALIGN
        head = B * DESC_INTS * 4
        staging = self._staging(slot, head + off + extra)
        packed, desc = split_staging(staging[:head + off], B)
        desc.numpy()[...] = rows
        pix = packed.numpy()
        futures = [pool.submit(self._decode, p, pix[o:o + 3 * w * h].reshape(h, w, 3), size, hb, out_wh)
                   for p, (o, h, w), size, hb in zip(chunk, shapes, sizes, host_boxes)]
        return staging, packed, desc, kmax, sum(hb is not None for hb in host_boxes), futures

    def _submit(self, pool: ThreadPoolExecutor, k: int):
        """Fix batch k's layout from the headers and start its decodes: (Batch, futures)."""
        chunk = self.paths[k * self.batch_size:(k + 1) * self.batch_size]
        sizes = list(pool.map(self._size, chunk))
        n = self.n_px
        staging, packed, desc, kmax, n_host, futures = self._pack(pool, k % 2, chunk, sizes, [self.box(w, h, n) for w, h in sizes], (n, n))
        return Batch(chunk, staging, packed, desc, kmax, n_host), futures

    def __iter__(self):
        n_batches = len(self)
        if n_batches == 0:
            return
        with ThreadPoolExecutor(max_workers=self.n_threads, thread_name_prefix="zutis-decode") as pool:
            pending = self._submit(pool, 0)
            try:
                for k in range(n_batches):
                    batch, futures = pending
                    pending = None
                    for f in futures:
                        f.result()              # raises what the worker raised
                    if k + 1 < n_batches:
                        pending = self._submit(pool, k + 1)
                    yield batch
            finally:
                if pending is not None:
                    for f in pending[1]:
                        f.cancel()


def mask_dataset_size(w: int, h: int, image_size):
    """(nw, nh) of MaskDataset's `TF.resize(image, size=image_size, interpolation=BILINEAR)` (datasets/index_dataset.py:408-409) for a
    w x h file: the shorter side becomes image_size, the other int(image_size * long / short); an image whose shorter side already is
    image_size, and image_size None, stay as they are."""
    if image_size is None:
        return w, h
    s = int(image_size)
    if (w <= h and w == s) or (h <= w and h == s):
        return w, h
    return (s, int(s * h / w)) if w < h else (int(s * w / h), s)


def longer_edge_size(w: int, h: int, max_size):
    """(nw, nh) of ImageNetSDataset's `resize(image, size=max_size, edge="longer", interpolation="bilinear")` (datasets/imagenet_s.py:71-76)
    for a w x h file: an image whose longer edge exceeds max_size gets that edge capped and the other one int(float(a) / b * max_size)
    (geometric_transforms.compute_size: the quotient first, truncated); any other image, and max_size None, stay as they are."""
    if max_size is None or max(w, h) <= int(max_size):
        return w, h
    s = int(max_size)
    if w > h:
        return s, int(float(h) / w * s)
    return int(float(w) / h * s), s


def _buckets(shapes, batch_size: int, window: int):
    open_buckets = {}                                # shape -> indices, in order of each bucket's oldest image (dicts keep insertion order)
    for i, key in enumerate(shapes):
        for k in [k for k, idx in open_buckets.items() if idx[0] <= i - window]:
            yield open_buckets.pop(k)
        idx = open_buckets.setdefault(key, [])
        idx.append(i)
        if len(idx) == batch_size:
            yield open_buckets.pop(key)
    yield from open_buckets.values()


def bucket_batches(shapes: Sequence, batch_size: int, window: int) -> List[List[int]]:
    """The grouping of ShapeBucketLoader as a pure function of the images' shape keys in path order: image i joins the open bucket of
    its shape; a bucket is emitted when it holds batch_size images (full buckets first), when its oldest image lies `window` paths
    behind the one being read (the window closes on it), or at the end of the list, oldest bucket first.  Lists of indices into
    `shapes`; every index exactly once; one shape and at most batch_size images per list."""
    if batch_size < 1 or window < 1:
        raise ValueError("bucket_batches: batch_size and window must be positive")
    return list(_buckets(shapes, batch_size, window))


ShapeBatch = collections.namedtuple("ShapeBatch", "paths indices sizes_hw out_hw staging packed desc kmax n_host")
ShapeBatch.__doc__ = """One decoded batch of ONE resized shape.  paths / indices: its files and their positions in the loader's path list;
sizes_hw: the files' own (H, W); out_hw: the (out_h, out_w) every image of the batch resizes to; the rest as in Batch."""


class ShapeBucketLoader(BatchLoader):
    """BatchLoader's threads and staging for MaskDataset's transform (datasets/index_dataset.py:388-411): every image is resized whole —
    shorter side to `image_size` (mask_dataset_size), `filter` bilinear — so a batch for ops.resize_normalize must be of one resized
    shape.  The loader reads the headers of at most `window` paths at a time, groups them with bucket_batches (a deterministic function
    of the path list, batch_size and window: batches come OUT OF INPUT ORDER and carry their indices) and decodes one batch ahead.
    An image outside the kernel's envelope (more than KMAX taps per output pixel — a source side over 75 times the target with
    bilinear's 3-tap support — or 3 w h >= 2^31) is resized by Pillow in its worker and packed as an identity image.  A missing or
    unreadable file raises in the step that reads its header or needs its batch, at the latest."""

    def __init__(self, paths: Sequence[str], image_size, batch_size: int, n_workers: int, window: int = 512, filter: str = "bilinear", pin=None):
        if image_size is not None and image_size < 1:
            raise ValueError("ShapeBucketLoader: image_size must be positive or None")
        if window < 1 or filter not in FILTERS:
            raise ValueError(f"ShapeBucketLoader: window must be positive and filter one of {sorted(FILTERS)}")
        super().__init__(paths, 1, batch_size, n_workers, None, pin)
        self.image_size, self.window, self.filter = image_size, int(window), filter

    def __len__(self):
        raise TypeError("ShapeBucketLoader: the number of batches depends on the files' shapes")

    def _groups(self, pool: ThreadPoolExecutor):
        """bucket_batches over the path list, its shape keys read from the headers `window` paths at a time: yields (indices, the files'
        (w, h), the resized (nw, nh))."""
        sizes = {}

        def keys():
            for start in range(0, len(self.paths), self.window):
                block = self.paths[start:start + self.window]
                for i, wh in enumerate(pool.map(self._size, block), start):
                    sizes[i] = wh
                for i in range(start, start + len(block)):
                    yield mask_dataset_size(*sizes[i], self.image_size)

        for idx in _buckets(keys(), self.batch_size, self.window):
            wh = [sizes.pop(i) for i in idx]
            yield idx, wh, mask_dataset_size(*wh[0], self.image_size)

    def _start(self, pool: ThreadPoolExecutor, slot: int, group):
        idx, sizes, (nw, nh) = group
        chunk = [self.paths[i] for i in idx]
        staging, packed, desc, kmax, n_host, futures = self._pack(pool, slot, chunk, sizes, [((nw, nh), (0, 0))] * len(idx), (nw, nh))
        return ShapeBatch(chunk, idx, [(h, w) for w, h in sizes], (nh, nw), staging, packed, desc, kmax, n_host), futures

    def __iter__(self):
        with ThreadPoolExecutor(max_workers=self.n_threads, thread_name_prefix="zutis-decode") as pool:
            groups = self._groups(pool)
            first = next(groups, None)
            pending = None if first is None else self._start(pool, 0, first)
            k = 0
            try:
                while pending is not None:
                    batch, futures = pending
                    pending = None
                    for f in futures:
                        f.result()              # raises what the worker raised
                    k += 1
                    nxt = next(groups, None)
                    if nxt is not None:
                        pending = self._start(pool, k % 2, nxt)
                    yield batch
            finally:
                if pending is not None:
                    for f in pending[1]:
                        f.cancel()


GT_MODES = {"u8": ("L", "P"), "rg16": ("RGB",)}      # Pillow modes np.array() turns into u8 [H, W] / u8 [H, W, 3]
GT_CHANNELS = {"u8": 1, "rg16": 3}

EvalBatch = collections.namedtuple("EvalBatch", "paths gt_paths indices size_hw out_hw staging packed_bytes gt kmax n_host")
EvalBatch.__doc__ = """One decoded evaluation batch: images of ONE file size that resize to ONE shape, with their ground truth.  paths /
gt_paths / indices: the files and their positions in the loader's lists; size_hw: the (H, W) every file of the batch has; out_hw: what
the images resize to; staging: u8 [32 * B + packed_bytes + ground-truth bytes] — descriptor rows, the packed images, then gt, the host
view u8 [B, H, W] ("u8") or [B, H, W, 3] ("rg16") of its tail; kmax, n_host as in Batch."""


def split_eval_staging(staging: torch.Tensor, B: int, packed_bytes: int, gt_shape):
    """(packed, desc, gt) views of an EvalBatch's staging tensor (host or device)."""
    head = B * DESC_INTS * 4 + packed_bytes
    packed, desc = split_staging(staging[:head], B)
    return packed, desc, staging[head:].view(gt_shape)


def eval_bucket_key(w: int, h: int, gw: int, gh: int, max_size):
    """The key EvalBatchLoader groups by: (the image's resized (nw, nh), the ground truth's (gw, gh)) — one launch of the resize and one of
    the scoring kernel serve a batch, so both shapes are shared."""
    return longer_edge_size(w, h, max_size), (gw, gh)


class EvalBatchLoader(ShapeBucketLoader):
    """ShapeBucketLoader for the validation datasets: image i is scored against the ground-truth PNG gt_paths[i] at the file's own size
    (trainer.py:322-325), so a batch shares the image file size as well as the resized shape (eval_bucket_key), and the ground truth is
    decoded by the same threads into the tail of the same staging buffer.  max_size: None (the image goes in as it is: coco2017.py,
    coco20k.py) or the cap of the longer edge (longer_edge_size, imagenet_s.py:71-76), Pillow BILINEAR.  gt_format "u8": an 8-bit
    grey or palette PNG, the byte is the label; "rg16": an RGB PNG, label R + 256 G (imagenet_s.py:93).  A ground-truth file of
    another mode, or of another size than its image, raises ValueError naming the file."""

    def __init__(self, paths: Sequence[str], gt_paths: Sequence[str], max_size, batch_size: int, n_workers: int, window: int = 512,
                 gt_format: str = "u8", pin=None):
        if gt_format not in GT_MODES:
            raise ValueError(f"EvalBatchLoader: gt_format {gt_format!r} is not one of {sorted(GT_MODES)}")
        if len(paths) != len(gt_paths):
            raise ValueError("EvalBatchLoader: one ground-truth file per image")
        super().__init__(paths, max_size, batch_size, n_workers, window=window, filter="bilinear", pin=pin)
        self.gt_paths, self.max_size, self.gt_format = list(gt_paths), max_size, gt_format

    def _gt_size(self, path: str):
        with Image.open(path) as im:            # header only
            if im.mode not in GT_MODES[self.gt_format]:
                raise ValueError(f"{path}: ground truth of mode {im.mode!r}, gt_format {self.gt_format!r} needs one of {GT_MODES[self.gt_format]}")
            return im.size

    def _decode_gt(self, path: str, dst: np.ndarray):
        with Image.open(path) as im:
            a = np.asarray(im)
        if a.dtype != np.uint8 or a.shape != dst.shape:
            raise ValueError(f"{path}: ground truth decodes to {a.dtype} {a.shape}, expected uint8 {dst.shape}")
        np.copyto(dst, a)

    def _groups(self, pool: ThreadPoolExecutor):
        sizes = {}

        def keys():
            for start in range(0, len(self.paths), self.window):
                block = self.paths[start:start + self.window]
                gts = list(pool.map(self._gt_size, self.gt_paths[start:start + self.window]))
                for i, wh in enumerate(pool.map(self._size, block), start):
                    if gts[i - start] != wh:
                        raise ValueError(f"{self.gt_paths[i]}: ground truth of size {gts[i - start]}, its image {self.paths[i]} is {wh}")
                    sizes[i] = wh
                for i in range(start, start + len(block)):
                    yield eval_bucket_key(*sizes[i], *sizes[i], self.max_size)

        for idx in _buckets(keys(), self.batch_size, self.window):
            wh = [sizes.pop(i) for i in idx]
            yield idx, wh, longer_edge_size(*wh[0], self.max_size)

    def _start(self, pool: ThreadPoolExecutor, slot: int, group):
        idx, sizes, (nw, nh) = group
        B, (w, h), ch = len(idx), sizes[0], GT_CHANNELS[self.gt_format]
        chunk, gts = [self.paths[i] for i in idx], [self.gt_paths[i] for i in idx]
        staging, packed, desc, kmax, n_host, futures = self._pack(pool, slot, chunk, sizes, [((nw, nh), (0, 0))] * B, (nw, nh), extra=B * h * w * ch)
        gt = staging[B * DESC_INTS * 4 + packed.numel():].view((B, h, w) if ch == 1 else (B, h, w, ch))
        gt_np = gt.numpy()
        futures += [pool.submit(self._decode_gt, p, gt_np[b]) for b, p in enumerate(gts)]
        return EvalBatch(chunk, gts, idx, (h, w), (nh, nw), staging, packed.numel(), gt, kmax, n_host), futures


PredictBatch = collections.namedtuple("PredictBatch", "paths indices size_hw out_hw staging packed desc kmax n_host host_paths")
PredictBatch.__doc__ = """One decoded batch of images of ONE file size that resize to ONE shape.  paths / indices: the files and their
positions in the loader's list; size_hw: the (H, W) every file of the batch has; out_hw: what the images resize to; staging / packed /
desc / kmax / n_host as in Batch; host_paths: the files that were resized on the host (their packed bytes are NOT at file size)."""


class PredictBatchLoader(ShapeBucketLoader):
    """EvalBatchLoader without ground truth: the prediction of image i is made at the file's own size (trainer.py:322-325), so a batch
    shares the file size as well as the resized shape.  It groups by the very key evaluation groups by, eval_bucket_key(w, h, w, h,
    max_size): for one path list, batch_size and window its batches are EvalBatchLoader's.  max_size as there."""

    def __init__(self, paths: Sequence[str], max_size, batch_size: int, n_workers: int, window: int = 512, pin=None):
        super().__init__(paths, max_size, batch_size, n_workers, window=window, filter="bilinear", pin=pin)
        self.max_size = max_size

    def _groups(self, pool: ThreadPoolExecutor):
        sizes = {}

        def keys():
            for start in range(0, len(self.paths), self.window):
                block = self.paths[start:start + self.window]
                for i, wh in enumerate(pool.map(self._size, block), start):
                    sizes[i] = wh
                for i in range(start, start + len(block)):
                    yield eval_bucket_key(*sizes[i], *sizes[i], self.max_size)

        for idx in _buckets(keys(), self.batch_size, self.window):
            wh = [sizes.pop(i) for i in idx]
            yield idx, wh, longer_edge_size(*wh[0], self.max_size)

    def _start(self, pool: ThreadPoolExecutor, slot: int, group):
        idx, sizes, (nw, nh) = group
        (w, h), chunk = sizes[0], [self.paths[i] for i in idx]
        staging, packed, desc, kmax, n_host, futures = self._pack(pool, slot, chunk, sizes, [((nw, nh), (0, 0))] * len(idx), (nw, nh))
        host = [p for p in chunk if not _taps_ok(w, h, nw, nh, self.filter)] if n_host else []
        return PredictBatch(chunk, idx, (h, w), (nh, nw), staging, packed, desc, kmax, n_host, host), futures
