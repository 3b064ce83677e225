"""Pseudo-label driver: SelfMask + bilateral solver + nearest resize + COCO-RLE JSON, with the mask
staying on the GPU between the stages.

Mirrors IndexDataset.generate_pseudo_masks (datasets/index_dataset.py:177-226): the reference runs batch 1, pulls the
mask to the host (`.cpu()`), converts the image tensor to PIL on the host, solves in NumPy/SciPy, re-uploads nothing and
resizes with F.interpolate on CPU tensors.  Here: SelfMaskEngine.forward(inference=True) -> device u8 mask ->
zh_denormalize_u8 + zh_bilateral_solve (device) -> `> 0.5` -> zh_resize_nearest_u8 (device) -> one D2H -> RLE.

`component=` (every driver here; None by default, and then every file is byte for byte what it was without the keyword):
"second_largest" replaces the `> 0.5` by the cleaning the reference's own bilateral_solver_output computes from the solver's soft
output (utils/bilateral_solver.py:185-193: holes filled, 4-connected components, the second largest under the key (count, label) —
the largest object while the background is larger still; zutis_amd/components.py states the tie rule), on the device
(zh_second_largest_component) at solver resolution, before the nearest resize.  It needs bilateral_solver=True.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops, preprocess, rle
from .engine import SelfMaskEngine

COMPONENTS = (None, "second_largest")


def check_component(component: Optional[str], bilateral_solver: bool) -> Optional[str]:
    """The `component=` keyword of the drivers: None or "second_largest", the latter on the solver's soft output only."""
    if component not in COMPONENTS:
        raise ValueError(f"component {component!r} is neither None nor 'second_largest'")
    if component is not None and not bilateral_solver:
        raise ValueError(f"component={component!r} works on the bilateral solver's soft output: it needs bilateral_solver=True")
    return component


def _binarise(soft: torch.Tensor, component: Optional[str]) -> torch.Tensor:
    """soft f64 [H,W] / [B,H,W] (device) -> u8 {0,1}: `> 0.5` (selfmask.py:231), or the second-largest component of it."""
    return ops.threshold_f64_u8(soft, 0.5) if component is None else ops.second_largest_component(soft, 0.5)


def _device_mask(engine: SelfMaskEngine, image: torch.Tensor, original_size: Optional[Tuple[int, int]],
                 bilateral_solver: bool, component: Optional[str] = None) -> torch.Tensor:
    """image f32 [3,H,W] (normalised, on the GPU) -> uint8 {0,1} mask [H0,W0] on the GPU, all on the current stream."""
    out = engine.forward(image[None].contiguous(), inference=True)
    dt = out["dts"][0]                                                     # u8 [H,W] on device (selfmask.py:216-222)
    if bilateral_solver:                                                   # selfmask.py:226-234
        rgb = ops.denormalize_u8(image.contiguous())
        soft, _ = ops.bilateral_solve(rgb, dt.contiguous())
        dt = _binarise(soft, component)                                    # `> 0.5` on the device result
    if original_size is not None and tuple(original_size) != tuple(dt.shape):
        dt = ops.resize_nearest_u8(dt.contiguous(), int(original_size[0]), int(original_size[1]))   # index_dataset.py:215
    return dt


@torch.no_grad()
def pseudo_mask(engine: SelfMaskEngine, image: torch.Tensor, original_size: Optional[Tuple[int, int]] = None,
                bilateral_solver: bool = True, component: Optional[str] = None) -> np.ndarray:
    """image f32 [3,H,W] (normalised, on the GPU) -> uint8 {0,1} mask [H0,W0] (original_size or H,W) on the host."""
    check_component(component, bilateral_solver)
    return _device_mask(engine, image, original_size, bilateral_solver, component).cpu().numpy()


def _device_masks_batch(engine: SelfMaskEngine, images: torch.Tensor, bilateral_solver: bool, component: Optional[str] = None,
                        **norm) -> torch.Tensor:
    """The device steps of pseudo_masks_batch up to the threshold: images f32 [B,3,H,W] -> u8 {0,1} [B,H,W], on the current stream.
    norm: mean= / std= the images were normalised with, when they are not ops.denormalize_u8's defaults."""
    B = images.shape[0]
    out = engine.forward(images.contiguous(), inference=True)
    dts = out["dts"]                                                       # u8 [B,H,W]
    if bilateral_solver:
        rgb = torch.stack([ops.denormalize_u8(images[b].contiguous(), **norm) for b in range(B)])
        soft, _ = ops.bilateral_solve(rgb, dts.contiguous())
        dts = _binarise(soft, component)
    return dts


@torch.no_grad()
def pseudo_masks_batch(engine: SelfMaskEngine, images: torch.Tensor, original_sizes: Optional[Sequence[Tuple[int, int]]] = None,
                       bilateral_solver: bool = True, component: Optional[str] = None) -> List[torch.Tensor]:
    """B images of ONE size in one pass (the reference loops batch 1, index_dataset.py:189-204): images f32 [B,3,H,W] on the
    GPU -> list of B uint8 {0,1} masks on the GPU.  SelfMask runs batched; the bilateral solver's ~110 launches are shared by
    the whole batch (zh_bilateral_solve_batch, blockIdx.y = image) — for one image it is launch/latency-bound."""
    check_component(component, bilateral_solver)
    dts = _device_masks_batch(engine, images, bilateral_solver, component)
    masks = []
    for b in range(images.shape[0]):
        dt = dts[b]
        if original_sizes is not None and tuple(original_sizes[b]) != tuple(dt.shape):
            dt = ops.resize_nearest_u8(dt.contiguous(), int(original_sizes[b][0]), int(original_sizes[b][1]))
        masks.append(dt)
    return masks


def save_rle_json(mask: np.ndarray, path: str) -> Dict:
    """index_dataset.py:219-224: RLE-encode (Fortran order), dump as JSON (counts as str, like ujson reject_bytes=False),
    read back and assert the round trip."""
    r = rle.encode(mask)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump({"size": r["size"], "counts": r["counts"].decode("ascii")}, f)
    back = json.load(open(path))
    assert (rle.decode_np(back) == mask).sum() == mask.size
    return r


@torch.no_grad()
def generate_pseudo_masks_batched(engine: SelfMaskEngine, images: Sequence[torch.Tensor], original_sizes: Sequence[Tuple[int, int]],
                                  out_paths: Sequence[str], bilateral_solver: bool = True, batch_size: int = 8,
                                  component: Optional[str] = None) -> List[str]:
    """generate_pseudo_masks with images grouped by shape (consecutive images of one H x W, up to batch_size) so that SelfMask
    and the solver run batched.  A group's files are bit for bit those of the batch-1 path when the group's size and one image fall on
    the same side of every batch-reading rule of zutis_amd/shape_rules.py.  They do not at the working shape: at 512x683 (T = 5505)
    the encoder's key split is 5 / 4 / 2 / 1 for groups of 1 / 2 / 4 / 8 (shape_rules.long_sequence_key_split), so the fp32 sums of an
    image are re-associated (~1e-7) with the size of its group — the ragged last group included — and a file then equals the batch-1
    file only while no soft mask value or objectness logit lies that close to its threshold (tests/test_bilateral_gpu.py)."""
    check_component(component, bilateral_solver)
    i, n = 0, len(images)
    while i < n:
        j = i + 1
        while j < n and j - i < batch_size and images[j].shape == images[i].shape:
            j += 1
        masks = pseudo_masks_batch(engine, torch.stack(list(images[i:j])), original_sizes[i:j], bilateral_solver, component)
        for m, path in zip(masks, out_paths[i:j]):
            save_rle_json(m.cpu().numpy(), path)
        i = j
    return list(out_paths)


@torch.no_grad()
def generate_pseudo_masks(engine: SelfMaskEngine, images: Sequence[torch.Tensor], original_sizes: Sequence[Tuple[int, int]],
                          out_paths: Sequence[str], bilateral_solver: bool = True, n_streams: int = 4,
                          component: Optional[str] = None) -> List[str]:
    """The loop of IndexDataset.generate_pseudo_masks (index_dataset.py:196-226) as a pipeline: image i runs SelfMask + solver +
    resize on HIP stream i % n_streams (one forked engine = one set of activation buffers per stream; the solver and the
    ViT of different images overlap — a single 512x683 image is launch/latency-bound: ~110 solver launches in 0.9 ms), the
    mask lands in pinned host memory by an async copy, and the host RLE-encodes / writes image i - n_streams meanwhile."""
    from collections import deque
    check_component(component, bilateral_solver)
    n_streams = max(1, min(n_streams, len(images)))
    if n_streams == 1:
        for img, size, path in zip(images, original_sizes, out_paths):
            save_rle_json(pseudo_mask(engine, img, size, bilateral_solver, component), path)
        return list(out_paths)
    dev = images[0].device
    streams = [torch.cuda.Stream(device=dev) for _ in range(n_streams)]
    engines = [engine] + [engine.fork() for _ in range(n_streams - 1)]
    pinned: List[Optional[torch.Tensor]] = [None] * n_streams
    pending = deque()

    def finish(item):
        ev, host, shape, path = item
        ev.synchronize()
        save_rle_json(host[: shape[0] * shape[1]].view(shape).numpy().copy(), path)

    for i, (img, size, path) in enumerate(zip(images, original_sizes, out_paths)):
        k = i % n_streams
        if len(pending) == n_streams:                                   # slot k's previous image: buffers free after this
            finish(pending.popleft())
        streams[k].wait_stream(torch.cuda.current_stream(dev))          # the image may have been produced on the caller's stream
        with torch.cuda.stream(streams[k]):
            dt = _device_mask(engines[k], img, size, bilateral_solver, component)
            n = dt.numel()
            if pinned[k] is None or pinned[k].numel() < n:
                pinned[k] = torch.empty((n,), dtype=torch.uint8, pin_memory=True)
            pinned[k][:n].copy_(dt.reshape(-1), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        pending.append((ev, pinned[k], tuple(dt.shape), path))
    while pending:
        finish(pending.popleft())
    return list(out_paths)


# ------------------------------------------------------------------------------------- files in, JSON out
def _write_masks(event, host: np.ndarray, items):
    """A writer task: once the batch's copy has landed, index_dataset.py:219-224 for some of its masks.  items: (offset, (H, W), path)."""
    event.synchronize()
    for off, (h, w), path in items:
        save_rle_json(host[off:off + h * w].reshape(h, w), path)


@torch.no_grad()
def generate_pseudo_masks_from_files(engine: SelfMaskEngine, p_images: Sequence[str], out_paths: Sequence[str], *, image_size: Optional[int] = 512,
                                     mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), bilateral_solver: bool = True,
                                     batch_size: int = 8, n_workers: int = 16, window: int = 512, decoder: str = "host",
                                     component: Optional[str] = None) -> List[str]:
    """IndexDataset.generate_pseudo_masks (datasets/index_dataset.py:177-226) from a list of image files to the RLE JSON files
    `out_paths`, MaskDataset's transform (:405-411) included, over the file pipeline of preprocess.py.  Threads decode into pinned
    staging one batch ahead (ShapeBucketLoader: batches of ONE resized shape out of a window of `window` paths, so SelfMask and the
    solver run batched on a corpus of mixed shapes); per batch (device_batches) one host-to-device copy of the decoded bytes and
    ops.resize_normalize (Pillow's BILINEAR + the normalisation, bit for bit); then the device steps of pseudo_masks_batch, every mask
    resized to its file's own size into one device buffer of a WriterRing slot, one copy to its pinned twin behind the slot's event; RLE
    encoding, the JSON write and its read-back check run on the ring's threads while the next batch is on the GPU.  n_workers (at most
    16) is split between decoders and writers (a quarter, at least one).
    Each file is what save_rle_json writes; returns out_paths (input order).  A missing or unreadable image and a writer's exception
    are raised here.  The grouping is preprocess.bucket_batches of the files' resized shapes."""
    check_component(component, bilateral_solver)
    p_images, out_paths = list(p_images), list(out_paths)
    if len(p_images) != len(out_paths):
        raise ValueError("generate_pseudo_masks_from_files: one output path per image")
    if not p_images:
        return out_paths
    dev = engine._device()
    n_decode, n_writers = preprocess.thread_split(n_workers, 0.25)
    lut = torch.from_numpy(preprocess.normalise_table(mean, std)).to(dev)
    loader = preprocess.ShapeBucketLoader(p_images, image_size, batch_size, n_decode, window=window, filter="bilinear", decoder=decoder)
    with preprocess.WriterRing(loader.pin, n_writers, "zutis-rle", device=dev) as ring, \
            preprocess.device_batches(loader, dev, preprocess.resize_normalize_of(lut)) as steps:
        for k, (batch, _, x) in enumerate(steps):
            B, (oh, ow) = len(batch.paths), batch.out_hw
            dts = _device_masks_batch(engine, x, bilateral_solver, component, mean=mean, std=std)
            offs = np.concatenate(([0], np.cumsum([h * w for h, w in batch.sizes_hw]))).tolist()
            host, out = ring.take(k % 2, offs[-1])                                      # the writers of batch k - 2 are done with its host buffer
            for b, (h, w) in enumerate(batch.sizes_hw):                                 # index_dataset.py:214-215
                dst = out[offs[b]:offs[b + 1]].view(h, w)
                if (h, w) == (oh, ow):
                    dst.copy_(dts[b])
                else:
                    ops.resize_nearest_u8(dts[b], h, w, out=dst)
            host.copy_(out, non_blocking=True)                                          # one D2H
            ring.events[k % 2].record()
            items, host_np = [(offs[b], batch.sizes_hw[b], out_paths[i]) for b, i in enumerate(batch.indices)], host.numpy()
            per = -(-B // n_writers)
            for j in range(0, B, per):
                ring.submit(k % 2, _write_masks, ring.events[k % 2], host_np, items[j:j + per])
        ring.drain()
    return out_paths


# ------------------------------------------------------------------------------------- the dataset method's own signature
def _image_size_hw(p_image: str) -> Tuple[int, int]:
    """(H, W) of the image file — `W, H = Image.open(p_image).size` (index_dataset.py:214)."""
    from PIL import Image
    with Image.open(p_image) as im:
        w, h = im.size
    return h, w


@torch.no_grad()
def dataset_generate_pseudo_masks(self, p_images: List[str], dir_dataset: str, n_workers: int = 4, bilateral_solver: bool = True, *,
                                  batch_size: int = 8, network=None, mask_dataset_cls=None, image_size_fn=None, loader: str = "dataset",
                                  component: Optional[str] = None) -> None:
    """`IndexDataset.generate_pseudo_masks(self, p_images, dir_dataset, n_workers, bilateral_solver)` (datasets/index_dataset.py:177-226;
    the same method exists in datasets/imagenet.py and datasets/pass.py) over the batched device path.  Bind it in place of the
    reference's method — `IndexDataset.generate_pseudo_masks = zutis_amd.pseudo_masks.dataset_generate_pseudo_masks` — and the
    unchanged caller (`_get_pseudo_masks`, :263) runs SelfMask + bilateral solver + nearest resize on the GPU, batched by image
    shape, and writes the same JSON files to the same paths.

    What it takes from `self`, exactly as the reference's method does: `self.device` and `self._convert_p_image_to_p_pseudo_mask`.
    The loader is the dataset module's own `MaskDataset` (same resize / normalisation); the network is the `selfmask` of
    `utils.utils.get_network` (the overlay's drop-in SelfMask when it is installed) unless `network=` is given.  The keyword-only
    arguments are not in the reference's signature: `batch_size` (images of one shape solved together; 1 = the reference's loop),
    the injection points the tests use, and `loader`: "dataset" (the default: the DataLoader over MaskDataset, groups of consecutive
    images of one shape) or "threads" (generate_pseudo_masks_from_files with image_size / mean / std of a MaskDataset instance and
    n_workers decoding and writing threads: shape-bucketed batches, the resize on the device), and `component` (the module docstring)."""
    import sys
    from torch.utils.data import DataLoader
    check_component(component, bilateral_solver)
    option = {} if component is None else {"component": component}     # without the option the drivers are called exactly as before
    if network is None:
        from utils.utils import get_network                       # the reference's factory (utils/utils.py), as :184 calls it
        network = get_network(network_name="selfmask")
    network = network.to(self.device)
    network.eval()
    engine = network._get_engine() if hasattr(network, "_get_engine") else network
    if not isinstance(engine, SelfMaskEngine):
        raise TypeError("dataset_generate_pseudo_masks needs the MI355X drop-in SelfMask (networks/selfmask/selfmask.py of the overlay) "
                        "or a SelfMaskEngine: there is no torch / CPU fallback")
    if loader not in ("dataset", "threads"):
        raise ValueError(f"dataset_generate_pseudo_masks: loader {loader!r} is neither 'dataset' nor 'threads'")
    if mask_dataset_cls is None:
        mask_dataset_cls = getattr(sys.modules[type(self).__module__], "MaskDataset")
    if loader == "threads":
        ds = mask_dataset_cls(p_images=p_images)
        generate_pseudo_masks_from_files(engine, p_images, [self._convert_p_image_to_p_pseudo_mask(p_image=p) for p in p_images],
                                         image_size=ds.image_size, mean=ds.mean, std=ds.std, bilateral_solver=bilateral_solver,
                                         batch_size=batch_size, n_workers=n_workers, **option)
        print(f"Pseudo-masks are saved in {dir_dataset}.")          # :226
        return
    size_of = image_size_fn or _image_size_hw
    loader = DataLoader(dataset=mask_dataset_cls(p_images=p_images), batch_size=1, num_workers=n_workers, pin_memory=True)   # :187-188

    images: List[torch.Tensor] = []
    sizes: List[Tuple[int, int]] = []
    paths: List[str] = []

    def flush():
        if images:
            generate_pseudo_masks_batched(engine, images, sizes, paths, bilateral_solver=bilateral_solver, batch_size=batch_size, **option)
            images.clear(); sizes.clear(); paths.clear()

    for dict_data in loader:                                        # :191-194: image 1 x 3 x H x W, p_image [str]
        image, p_image = dict_data["image"], dict_data["p_image"][0]
        if images and (tuple(image.shape[1:]) != tuple(images[0].shape) or len(images) >= batch_size):
            flush()                                                 # a group = consecutive images of one shape
        images.append(image[0].to(self.device, non_blocking=True).float())
        sizes.append(size_of(p_image))                              # :214 the file's own resolution
        paths.append(self._convert_p_image_to_p_pseudo_mask(p_image=p_image))   # :209
    flush()
    print(f"Pseudo-masks are saved in {dir_dataset}.")              # :226
