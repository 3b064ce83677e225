"""Host side of every "from image files" driver: embedding extraction (csrc/preprocess.hip, ops.resize_crop_normalize), pseudo-labels,
evaluation and prediction (ops.resize_normalize) and, through synth.TrainBatchLoader, training samples.  ONE pipeline: threads decode one
batch ahead into one of two reused pinned buffers (prefetch, DoubleBuffer), one host-to-device copy and one kernel per batch
(device_batches), and, where files are written, two pinned output buffers whose writer threads work while the next batch is on the
device (WriterRing).

The reference feeds CLIP through SimpleDataset's transform (utils/extract_image_embeddings.py:97-103: Resize BICUBIC, CenterCrop,
ToTensor, Normalize) under a 16-worker DataLoader (:64-65).  Here the workers are THREADS that only open and decode (Pillow
releases the GIL while it decodes); the resize, crop and normalisation run in one kernel per batch on the decoded bytes, which
is also what crosses PCIe (3 bytes per source pixel instead of 12 per output pixel).

  pil_resize_reference  NumPy restatement of Pillow's 8-bit resampler (bicubic, bilinear) — the CPU oracle of the tests, not a product path
  normalise_table       the 3 x 256 fp32 table the kernel looks normalised values up in
  DoubleBuffer          two reused byte buffers, regrown by a quarter: every staging and output buffer of the pipeline
  prefetch              the "start item k + 1, wait for item k, yield it" loop over a pool of decoding threads — the only one
  BatchLoader           paths -> batches of (packed bytes + descriptor rows) in reused staging buffers, decoded one batch ahead
  ShapeBucketLoader     the same staging for MaskDataset's transform (datasets/index_dataset.py:405-411): batches of ONE resized shape,
                        gathered from a bounded window of paths ahead, so that the batched SelfMask + solver run batched; optionally
                        of one file size too, and with a ground-truth PNG per image in the tail of the same staging buffer
  EvalBatchLoader       its constructor for evaluation: one file size per batch, every image travels with its ground truth
  PredictBatchLoader    its constructor for prediction: EvalBatchLoader's batches without the ground truth
  device_batches        the per-batch device sequence of every driver: H2D, event, views, the resize kernel, clean-up
  WriterRing            two output slots (pinned buffer, event, writer futures) over a pool of writer threads; thread_split beside it
  (picture_out.py)      over WriterRing, the output side of the drivers that write pictures: Layout and PictureStage (take, fill, commit)

Threads, not processes: no child ever holds the device open, nothing is pickled, a worker's exception is raised by the caller.
"""
from __future__ import annotations

import collections
import contextlib
import itertools
import math
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, List, Sequence

import numpy as np
import torch
from PIL import Image

from . import _lib, jpeg_device

PRECISION_BITS = 32 - 8 - 2     # Pillow's fixed-point coefficients: src/libImaging/Resample.c
KMAX = _lib.constants()["ZH_RCN_KMAX"]      # taps per output pixel the kernel serves
MAX_THREADS = 16                # decoding and writing threads of one call, together
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


Batch = collections.namedtuple("Batch", "paths indices sizes_hw size_hw out_hw staging packed desc kmax n_host host_paths gt_paths gt packed_bytes "
                               "jpeg n_host_decoded host_decoded_paths", defaults=(None,) * 17)
Batch.__doc__ = """One decoded batch of any loader; a field that does not apply is None.  paths: its files; staging: u8 tensor [32 * B +
packed_bytes (+ ground-truth bytes)] (pinned when the loader pins), descriptor rows first — one host-to-device copy moves all of it;
packed / desc: its first two views (u8 [packed_bytes], int32 [B, 8]), offsets relative to `packed`; kmax: the batch's largest tap count;
n_host / host_paths: the images that were resized on the host (outside device_supported: their packed bytes are NOT at file size).
ShapeBucketLoader adds indices: the files' positions in the loader's path list; sizes_hw: the files' own (H, W); out_hw: the (out_h,
out_w) every image of the batch resizes to; size_hw: the (H, W) every file has, when the file size is part of the bucket key;
gt_paths / gt: the ground-truth files and the host view u8 [B, H, W] ("u8") or [B, H, W, 3] ("rg16") of the staging buffer's tail.
With decoder="device" the staging buffer holds file bytes, not pixels: descriptor rows, then jpeg.staged_bytes bytes — the arrays of one
zh_jpeg_decode launch (jpeg_device.pack) and, behind them, the pixels of the images the host decoded (n_host_decoded /
host_decoded_paths: files jpeg_device.parse does not serve, images resized on the host, table sets past a launch's limit) — then the
ground truth; `packed` is None, packed_bytes and desc still describe the decoded images at the offsets they have on the device once
device_batches has run the decoder (jpeg: a JpegStage).
Valid until the loader is advanced."""

JpegStage = collections.namedtuple("JpegStage", "staged_bytes images segments tables scan n_blocks max_image_blocks max_image_pixels kept host chunks",
                                   defaults=(None,))
JpegStage.__doc__ = """Where the file bytes of a decoder="device" batch lie in its staging buffer, offsets counted from the end of the
descriptor rows: images / segments / tables / scan = (offset, bytes) of the arrays of jpeg_device.pack; n_blocks, max_image_blocks,
max_image_pixels: its launch sizes; kept: the batch positions of the images the launch decodes, in the order of its rows; host:
(batch position, offset of its pixels in the staged bytes, bytes, offset of its slot in the decoded images) of every host-decoded image;
chunks: (offset, bytes) of the chunk rows of jpeg_device.chunk_rows at jpeg_device.CHUNK_BYTES, staged behind the scan bytes when the
loader's decoder is "device-split" (None otherwise): decode_staged then calls ops.jpeg_decode_split."""


class DoubleBuffer:
    """Two reused u8 buffers, pinned host memory (`pin`) or memory of `device`: take(slot, nbytes) is a view of nbytes bytes of buffer
    `slot`, which is replaced by one a quarter larger when the request exceeds it (from the calling thread)."""

    def __init__(self, pin: bool, device=None):
        self.pin, self.device = bool(pin), device
        self.buffers: List[torch.Tensor] = [torch.empty(0, dtype=torch.uint8), torch.empty(0, dtype=torch.uint8)]

    def take(self, slot: int, nbytes: int) -> torch.Tensor:
        if self.buffers[slot].numel() < nbytes:
            self.buffers[slot] = torch.empty(nbytes + nbytes // 4, dtype=torch.uint8, device=self.device, pin_memory=self.pin)
        return self.buffers[slot][:nbytes]


def prefetch(items, start: Callable, n_threads: int):
    """Decode one item ahead: over a pool of n_threads threads, `start(pool, slot, item)` -> (batch, futures) lays item k + 1 out in
    staging slot (k + 1) % 2 and submits its decodes, after the futures of item k have been waited for (a worker's exception is raised
    there, by the step that needs its batch) and before batch k is yielded.  items: an iterable of work items — none: no pool is made —
    or a function of the pool that returns one (a source that reads file headers with the same threads).  `start` runs on the calling
    thread, in item order.  When the generator is closed or fails, what is still pending is cancelled and the pool joined: no thread
    outlives it."""
    if not callable(items):
        rest = iter(items)
        first = next(rest, None)
        if first is None:
            return
        items = lambda pool: itertools.chain((first,), rest)       # noqa: E731
    with ThreadPoolExecutor(max_workers=n_threads, thread_name_prefix="zutis-decode") as pool:
        items, slot, pending = iter(items(pool)), 0, None
        try:
            item = next(items, None)
            if item is not None:
                pending = start(pool, slot, item)
            while pending is not None:
                batch, futures = pending
                pending = None
                for f in futures:
                    f.result()                  # raises what the worker raised
                item = next(items, None)
                if item is not None:
                    slot ^= 1
                    pending = start(pool, slot, item)
                yield batch
        finally:
            if pending is not None:
                for f in pending[1]:
                    f.cancel()


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

    def __init__(self, paths: Sequence[str], n_px: int, batch_size: int, n_workers: int, box: Callable, pin=None, decoder: str = "host"):
        if batch_size < 1 or n_px < 1:
            raise ValueError("BatchLoader: batch_size and n_px must be positive")
        self.decoder = jpeg_device.check_decoder(type(self).__name__, decoder)
        self.paths, self.n_px, self.batch_size, self.box = list(paths), int(n_px), int(batch_size), box
        self.n_threads = max(1, min(int(n_workers), MAX_THREADS))
        self.pin = torch.cuda.is_available() if pin is None else bool(pin)
        self.filter = "bicubic"
        self._staging = DoubleBuffer(self.pin)
        self._files = {}                # decoder="device": slot -> what _read gave for the batch being laid out, when _start read it

    def __len__(self):
        return (len(self.paths) + self.batch_size - 1) // self.batch_size

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

    def _read(self, path: str):
        """decoder="device": the file's bytes and its plan — (data, plan, (w, h)); (None, None, (w, h)) from the header as Pillow reads
        it for a file the device decoder does not serve."""
        data = np.fromfile(path, np.uint8)
        plan = jpeg_device.parse(data)
        if plan is None:
            return None, None, self._size(path)
        return data, plan, (plan.width, plan.height)

    def _pack_files(self, pool: ThreadPoolExecutor, slot: int, chunk, sizes, host_boxes, shapes, rows, kmax, off, out_wh, extra: int):
        """_pack for decoder="device": the staging buffer gets the descriptor rows, the arrays of one zh_jpeg_decode launch over the files
        the device serves and, compacted behind them, room for the pixels of the others, which Pillow decodes in the pool as ever."""
        B = len(chunk)
        files = self._files.pop(slot, None) or list(pool.map(self._read, chunk))
        for p, size, (_, _, wh) in zip(chunk, sizes, files):
            if wh != tuple(size):
                raise ValueError(f"{p}: size {wh} differs from its header's {tuple(size)}")
        want = [i for i in range(B) if files[i][1] is not None and host_boxes[i] is None]
        jp = jpeg_device.pack([files[i][1] for i in want], [files[i][0] for i in want], out_off=[shapes[i][0] for i in want], out_bytes=off,
                              skip_overflow=True, chunk_bytes=jpeg_device.CHUNK_BYTES if self.decoder == "device-split" else None)
        kept = [want[k] for k in jp.kept]
        arrays = [np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in (jp.images, jp.segments, jp.tables, jp.scan) + (() if jp.chunks is None else (jp.chunks,))]
        at, places = 0, []
        for a in arrays:
            places.append((at, a.size))
            at += -(-a.size // ALIGN) * ALIGN
        host = []
        for i in sorted(set(range(B)) - set(kept)):
            o, h, w = shapes[i]
            host.append((i, at, 3 * w * h, o))
            at += -(-3 * w * h // ALIGN) * ALIGN
        head = B * DESC_INTS * 4
        staging = self._staging.take(slot, head + at + extra)
        desc = staging[:head].view(torch.int32).view(B, DESC_INTS)
        desc.numpy()[...] = rows
        pay = staging[head:head + at].numpy()
        for (o, n), a in zip(places, arrays):
            pay[o:o + n] = a
        futures = [pool.submit(self._decode, chunk[i], pay[o:o + n].reshape(shapes[i][1], shapes[i][2], 3), sizes[i], host_boxes[i], out_wh)
                   for i, o, n, _ in host]
        stage = JpegStage(at, *places[:4], jp.n_blocks, jp.max_image_blocks, jp.max_image_pixels, kept, host, places[4] if len(places) > 4 else None)
        resized = [p for p, hb in zip(chunk, host_boxes) if hb is not None]
        return Batch(paths=chunk, staging=staging, desc=desc, kmax=kmax, n_host=len(resized), host_paths=resized, packed_bytes=off, jpeg=stage,
                     n_host_decoded=len(host), host_decoded_paths=[chunk[i] for i, _, _, _ in host]), futures

    def _pack(self, pool: ThreadPoolExecutor, slot: int, chunk, sizes, boxes, out_wh, extra: int = 0):
        """Lay `chunk` (files of `sizes` = (w, h), resized and cropped as `boxes` = ((nw, nh), (left, top)) say, to out_wh = (w, h) of the
        kernel's output) out in staging buffer `slot` and start its decodes: (Batch, futures).  extra: bytes the staging buffer holds
        behind the packed images (packed stops in front of them)."""
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
        if self.decoder != "host":
            return self._pack_files(pool, slot, chunk, sizes, host_boxes, shapes, rows, kmax, off, out_wh, extra)
        head = B * DESC_INTS * 4
        staging = self._staging.take(slot, head + off + extra)
        packed, desc = split_staging(staging[:head + off], B)
        desc.numpy()[...] = rows
        pix = packed.numpy()
        futures = [pool.submit(self._decode, p, pix[o:o + 3 * w * h].reshape(h, w, 3), size, hb, out_wh)
                   for p, (o, h, w), size, hb in zip(chunk, shapes, sizes, host_boxes)]
        host = [p for p, hb in zip(chunk, host_boxes) if hb is not None]
        return Batch(paths=chunk, staging=staging, packed=packed, desc=desc, kmax=kmax, n_host=len(host), host_paths=host, packed_bytes=off), futures

    def _start(self, pool: ThreadPoolExecutor, slot: int, k: int):
        """Fix batch k's layout from the headers and start its decodes: (Batch, futures)."""
        chunk = self.paths[k * self.batch_size:(k + 1) * self.batch_size]
        if self.decoder != "host":      # one read serves the header and the decoder
            self._files[slot] = list(pool.map(self._read, chunk))
            sizes = [wh for _, _, wh in self._files[slot]]
        else:
            sizes = list(pool.map(self._size, chunk))
        n = self.n_px
        return self._pack(pool, slot, chunk, sizes, [self.box(w, h, n) for w, h in sizes], (n, n))

    def __iter__(self):
        return prefetch(range(len(self)), self._start, self.n_threads)


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


GT_MODES = {"u8": ("L", "P"), "rg16": ("RGB",)}      # Pillow modes np.array() turns into u8 [H, W] / u8 [H, W, 3]
GT_CHANNELS = {"u8": 1, "rg16": 3}


class ShapeBucketLoader(BatchLoader):
    """BatchLoader's threads and staging for MaskDataset's transform (datasets/index_dataset.py:388-411): every image is resized whole —
    `size_rule(w, h, image_size)` gives its (nw, nh): mask_dataset_size (shorter side to image_size), `filter` bilinear — so a batch for
    ops.resize_normalize must be of one resized shape.  The loader reads the headers of at most `window` paths at a time, groups them
    with bucket_batches (a deterministic function of the path list, batch_size and window: batches come OUT OF INPUT ORDER and carry
    their indices) and decodes one batch ahead.  An image outside the kernel's envelope (more than KMAX taps per output pixel — a source
    side over 75 times the target with bilinear's 3-tap support — or 3 w h >= 2^31) is resized by Pillow in its worker and packed as an
    identity image.  A missing or unreadable file raises in the step that reads its header or needs its batch, at the latest.
    by_file_size: the file's (w, h) is part of the bucket key, (the resized (nw, nh), (w, h)) — with longer_edge_size the value of
    eval_bucket_key(w, h, w, h, image_size) — and the batch carries size_hw.
    gt_paths: one ground-truth PNG per image, of `gt_format` ("u8": an 8-bit grey or palette PNG, the byte is the label; "rg16": an RGB
    PNG, label R + 256 G, imagenet_s.py:93), decoded by the same threads into the tail of the same staging buffer.  A ground-truth file
    of another mode, or of another size than its image, raises ValueError naming the file."""

    def __init__(self, paths: Sequence[str], image_size, batch_size: int, n_workers: int, window: int = 512, filter: str = "bilinear", pin=None, *,
                 size_rule: Callable = mask_dataset_size, by_file_size: bool = False, gt_paths=None, gt_format: str = "u8", decoder: str = "host"):
        if image_size is not None and image_size < 1:
            raise ValueError("ShapeBucketLoader: image_size must be positive or None")
        if window < 1 or filter not in FILTERS:
            raise ValueError(f"ShapeBucketLoader: window must be positive and filter one of {sorted(FILTERS)}")
        super().__init__(paths, 1, batch_size, n_workers, None, pin, decoder)
        self.image_size, self.window, self.filter = image_size, int(window), filter
        self.size_rule, self.by_file_size = size_rule, bool(by_file_size)
        self.gt_paths, self.gt_format = None if gt_paths is None else list(gt_paths), gt_format

    def __len__(self):
        raise TypeError("ShapeBucketLoader: the number of batches depends on the files' shapes")

    def _gt_size(self, path: str):
        with Image.open(path) as im:            # header only
            if im.mode not in GT_MODES[self.gt_format]:
                raise ValueError(f"{path}: ground truth of mode {im.mode!r}, gt_format {self.gt_format!r} needs one of {GT_MODES[self.gt_format]}")
            return im.size

    @staticmethod
    def _decode_gt(path: str, dst: np.ndarray):
        with Image.open(path) as im:
            a = np.asarray(im)
        if a.dtype != np.uint8 or a.shape != dst.shape:
            raise ValueError(f"{path}: ground truth decodes to {a.dtype} {a.shape}, expected uint8 {dst.shape}")
        np.copyto(dst, a)

    def _groups(self, pool: ThreadPoolExecutor):
        """bucket_batches over the path list, its shape keys read from the headers `window` paths at a time: yields (indices, the files'
        (w, h), the resized (nw, nh))."""
        sizes = {}

        def keys():
            for start in range(0, len(self.paths), self.window):
                block = self.paths[start:start + self.window]
                gts = None if self.gt_paths is None else list(pool.map(self._gt_size, self.gt_paths[start:start + self.window]))
                for i, wh in enumerate(pool.map(self._size, block), start):
                    if gts is not None and gts[i - start] != wh:
                        raise ValueError(f"{self.gt_paths[i]}: ground truth of size {gts[i - start]}, its image {self.paths[i]} is {wh}")
                    sizes[i] = wh
                for i in range(start, start + len(block)):
                    resized = self.size_rule(*sizes[i], self.image_size)
                    yield (resized, sizes[i]) if self.by_file_size else resized

        for idx in _buckets(keys(), self.batch_size, self.window):
            wh = [sizes.pop(i) for i in idx]
            yield idx, wh, self.size_rule(*wh[0], self.image_size)

    def _start(self, pool: ThreadPoolExecutor, slot: int, group):
        idx, sizes, (nw, nh) = group
        B, (w, h) = len(idx), sizes[0]
        ch = 0 if self.gt_paths is None else GT_CHANNELS[self.gt_format]
        batch, futures = self._pack(pool, slot, [self.paths[i] for i in idx], sizes, [((nw, nh), (0, 0))] * B, (nw, nh), extra=B * h * w * ch)
        batch = batch._replace(indices=idx, sizes_hw=[(h_, w_) for w_, h_ in sizes], out_hw=(nh, nw), size_hw=(h, w) if self.by_file_size else None)
        if ch:
            gts = [self.gt_paths[i] for i in idx]
            gt = batch.staging[B * DESC_INTS * 4 + (batch.packed_bytes if batch.jpeg is None else batch.jpeg.staged_bytes):].view((B, h, w) if ch == 1 else (B, h, w, ch))
            gt_np = gt.numpy()
            futures += [pool.submit(self._decode_gt, p, gt_np[b]) for b, p in enumerate(gts)]
            batch = batch._replace(gt_paths=gts, gt=gt)
        return batch, futures

    def __iter__(self):
        return prefetch(self._groups, self._start, self.n_threads)


def split_eval_staging(staging: torch.Tensor, B: int, packed_bytes: int, gt_shape):
    """(packed, desc, gt) views of the staging tensor (host or device) of a batch with ground truth."""
    head = B * DESC_INTS * 4 + packed_bytes
    packed, desc = split_staging(staging[:head], B)
    return packed, desc, staging[head:].view(gt_shape)


def eval_bucket_key(w: int, h: int, gw: int, gh: int, max_size):
    """The key EvalBatchLoader groups by: (the image's resized (nw, nh), the ground truth's (gw, gh)) — one launch of the resize and one of
    the scoring kernel serve a batch, so both shapes are shared."""
    return longer_edge_size(w, h, max_size), (gw, gh)


class EvalBatchLoader(ShapeBucketLoader):
    """ShapeBucketLoader for the validation datasets: image i is scored against the ground-truth PNG gt_paths[i] at the file's own size
    (trainer.py:322-325), so a batch shares the image file size as well as the resized shape (eval_bucket_key), and the ground truth
    travels in the same staging buffer.  max_size: None (the image goes in as it is: coco2017.py, coco20k.py) or the cap of the longer
    edge (longer_edge_size, imagenet_s.py:71-76), Pillow BILINEAR.  gt_format as ShapeBucketLoader's."""

    def __init__(self, paths: Sequence[str], gt_paths: Sequence[str], max_size, batch_size: int, n_workers: int, window: int = 512,
                 gt_format: str = "u8", pin=None, decoder: str = "host"):
        if gt_format not in GT_MODES:
            raise ValueError(f"EvalBatchLoader: gt_format {gt_format!r} is not one of {sorted(GT_MODES)}")
        if len(paths) != len(gt_paths):
            raise ValueError("EvalBatchLoader: one ground-truth file per image")
        super().__init__(paths, max_size, batch_size, n_workers, window=window, filter="bilinear", pin=pin, size_rule=longer_edge_size,
                         by_file_size=True, gt_paths=gt_paths, gt_format=gt_format, decoder=decoder)


class PredictBatchLoader(ShapeBucketLoader):
    """EvalBatchLoader without ground truth: the prediction of image i is made at the file's own size (trainer.py:322-325), so a batch
    shares the file size as well as the resized shape.  It groups by the very key evaluation groups by, eval_bucket_key(w, h, w, h,
    max_size): for one path list, batch_size and window its batches are EvalBatchLoader's.  max_size as there."""

    def __init__(self, paths: Sequence[str], max_size, batch_size: int, n_workers: int, window: int = 512, pin=None, decoder: str = "host"):
        super().__init__(paths, max_size, batch_size, n_workers, window=window, filter="bilinear", pin=pin, size_rule=longer_edge_size,
                         by_file_size=True, decoder=decoder)


# ------------------------------------------------------------------------------------------------- the device side of a driver
def resize_normalize_of(lut: torch.Tensor):
    """The `transform` of device_batches for a ShapeBucketLoader: (the staging views — split_staging's, or split_eval_staging's with ground
    truth —, ops.resize_normalize of the batch: Pillow BILINEAR + to_tensor + normalize, the identity where nothing is resized)."""
    from . import ops

    def transform(batch: Batch, staged: torch.Tensor):
        B, (oh, ow) = len(batch.paths), batch.out_hw
        views = split_staging(staged, B) if batch.gt is None else split_eval_staging(staged, B, batch.packed_bytes, tuple(batch.gt.shape))
        return views, ops.resize_normalize(views[0], views[1], oh, ow, lut, filter="bilinear", kmax=batch.kmax)
    return transform


def decode_staged(batch: Batch, staged: torch.Tensor, full: torch.Tensor) -> torch.Tensor:
    """The device side of decoder="device": `staged` is the batch's staging buffer on the device (descriptor rows, file bytes, host-decoded
    pixels, ground truth); `full` receives what a host-decoded staging buffer would hold there — the rows, every image's RGB bytes at its
    row's offset, the ground truth — and is returned.  One zh_jpeg_decode launch sequence (ops.jpeg_decode; ops.jpeg_decode_split when the
    loader staged chunk rows: decoder="device-split") writes the served images
    straight into their slots, the host-decoded ones are copied into theirs on the device.  The status array is read once, here: the
    read waits for the batch's upload and its decode (the wait device_batches makes behind the driver's body then returns at once).  An
    image with a non-zero status is decoded by Pillow on the calling thread and written over its slot before anything reads it; whatever
    Pillow raises for it is raised here."""
    from . import ops
    B, j = len(batch.paths), batch.jpeg
    head = B * DESC_INTS * 4
    full[:head].copy_(staged[:head])
    if staged.numel() > head + j.staged_bytes:
        full[head + batch.packed_bytes:].copy_(staged[head + j.staged_bytes:])
    pay, rgb = staged[head:head + j.staged_bytes], full[head:head + batch.packed_bytes]
    status = None
    if j.kept:
        part = lambda place, dtype, cols: pay[place[0]:place[0] + place[1]].view(dtype).view(-1, cols)      # noqa: E731
        status = torch.empty(len(j.kept), dtype=torch.int32, device=staged.device)
        arrays = (pay[j.scan[0]:j.scan[0] + j.scan[1]], part(j.segments, torch.int32, jpeg_device.SEGMENT_WORDS),
                  part(j.images, torch.int32, jpeg_device.IMAGE_WORDS), part(j.tables, torch.uint8, jpeg_device.TABLE_SET_BYTES))
        if j.chunks is None:
            ops.jpeg_decode(*arrays, j.n_blocks, j.max_image_blocks, j.max_image_pixels, rgb, status)
        else:
            ops.jpeg_decode_split(*arrays[:2], part(j.chunks, torch.int32, jpeg_device.CHUNK_WORDS), *arrays[2:], j.n_blocks, j.max_image_blocks,
                                  j.max_image_pixels, rgb, status)
    for _, at, n, slot in j.host:
        rgb[slot:slot + n].copy_(pay[at:at + n])
    if status is not None:
        rows = batch.desc.numpy()
        for k in np.flatnonzero(status.cpu().numpy()).tolist():
            i = j.kept[k]
            a = np.array(Image.open(batch.paths[i]).convert("RGB"))
            o, w, h = int(rows[i, 0]) * ALIGN, int(rows[i, 1]), int(rows[i, 2])
            if a.shape != (h, w, 3):
                raise ValueError(f"{batch.paths[i]}: decoded size {a.shape[1::-1]} differs from its header's {(w, h)}")
            rgb[o:o + 3 * w * h].copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1))
    return full


@contextlib.contextmanager
def device_batches(loader, dev, transform: Callable):
    """The device loop every driver shares, `dev` the current device inside: `with device_batches(...) as steps: for batch, views, x in
    steps: <the driver's work on the batch>`.  Per batch: ONE non-blocking host-to-device copy of batch.staging (descriptors + decoded
    bytes + whatever rides behind them), an event behind it, `transform(batch, staged)` -> (views, x); after the driver's body, and before
    the loader is advanced, the event is waited for — the loader may then decode into that staging buffer again.  On the way out, whether
    the body, the loader or a kernel failed or nothing did: the device is synchronised (nothing in flight on the pinned buffers when they
    go) and the loader's generator closed (a failure outside the loader: its threads end here)."""
    copied = torch.cuda.Event()
    batches = iter(loader)
    decoded = DoubleBuffer(False, dev)          # decoder="device": the decoded batches, at the layout a host-decoded staging buffer has

    def steps():
        for k, batch in enumerate(batches):
            staged = batch.staging.to(dev, non_blocking=True)
            copied.record()
            if getattr(batch, "jpeg", None) is not None:          # (synth.TrainBatch has no such field: its loader decodes on the host)
                staged = decode_staged(batch, staged, decoded.take(k & 1, staged.numel() - batch.jpeg.staged_bytes + batch.packed_bytes))
            yield (batch, *transform(batch, staged))
            copied.synchronize()

    with torch.cuda.device(dev):
        try:
            yield steps()
        finally:
            torch.cuda.synchronize(dev)
            batches.close()


# ------------------------------------------------------------------------------------------------- the output side of a driver
def thread_split(n_workers: int, share: float):
    """(decoders, writers) of a driver that writes files: together min(n_workers, 16) threads but two at the least, the writers `share`
    of them (rounded down) but one at the least."""
    total = max(2, min(int(n_workers), MAX_THREADS))
    n_write = max(1, int(total * share))
    return total - n_write, n_write


class WriterRing:
    """Two output slots over a pool of `n_writers` threads named `prefix`: per slot a pinned host buffer (and its twin on `device`, when
    one is given), the event the driver records behind the copy into it, and the futures of the writers that read it.  take() hands a
    slot out again only after those writers are done.  Leaving the `with` block cancels what has not started and joins the pool."""

    def __init__(self, pin: bool, n_writers: int, prefix: str, device=None):
        self.host, self.dev = DoubleBuffer(pin), None if device is None else DoubleBuffer(False, device)
        self.events = [torch.cuda.Event(), torch.cuda.Event()] if torch.cuda.is_available() else [None, None]
        self.writers: List[list] = [[], []]
        self.pool = ThreadPoolExecutor(max_workers=n_writers, thread_name_prefix=prefix) if n_writers else None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.pool is not None:
            self.pool.shutdown(wait=True, cancel_futures=True)

    def submit(self, slot: int, fn: Callable, *args):
        self.writers[slot].append(self.pool.submit(fn, *args))

    def drain(self, slot=None):
        """Wait for EVERY writer of the slot (None: of both); the first failure is the one raised."""
        error = None
        for s in (0, 1) if slot is None else (slot,):
            futures, self.writers[s] = self.writers[s], []
            for f in futures:
                try:
                    f.result()
                except BaseException as e:
                    error = error or e
        if error is not None:
            raise error

    def take(self, slot: int, nbytes: int):
        """(host view, device view or None) of nbytes bytes of the slot, once its writers are done (drain)."""
        self.drain(slot)
        return self.host.take(slot, nbytes), None if self.dev is None else self.dev.take(slot, nbytes)
