"""Drop-in replacement for the reference's utils/extract_image_embeddings.py on MI355X.

extract_image_embeddings(p_images, model_name, fp, device, batch_size, n_workers) -> Dict[basename, FloatTensor[E]]
keeps the reference signature and on-disk pickle format (utils/extract_image_embeddings.py:21-86).  The reference runs
third-party `clip`'s fp16 `encode_image` (`clip.load` leaves the model in half precision on a GPU, :43,72-76); here the ViT
tower runs in zutis_amd.engine.ClipImageEncoder.  `precision="exact"` (the default) computes every contraction in the fp32-class
f16x3 / f16x2 mode (fp16 split pairs, fp32 accumulate / residual / LayerNorm) — MORE precise than the reference's own run;
`precision="fast"` is the reference's arithmetic class for this path (fp16 MFMA operands in the transformer body, fp32 accumulate)
with the residual stream still fp32 — wider than the reference's; `precision="half"` (opt-in) also STORES the residual stream as fp16,
which is the reference's own storage class for this tower: the stream is rounded once after ln_pre and twice per residual update
(the Linear's output, then the sum — what an fp16 `x + linear(y)` does), LayerNorm statistics / accumulators / softmax / QuickGELU
stay fp32.  Every mode returns unit-norm fp32 embeddings.  Weights come from `clip.load` when the package is present, else from
`state_dict=`.
Pre-processing (bicubic resize of the shorter side, centre crop, CLIP mean/std; SimpleDataset :90-116): `n_workers` threads (at most
16; the reference's DataLoader workers, :64-65) open and decode the files one batch ahead (zutis_amd.preprocess.BatchLoader), the decoded
bytes cross to the device in one copy per batch (zutis_amd.preprocess.device_batches), and one kernel (ops.resize_crop_normalize)
resizes, crops and normalises them — the
very bytes of Pillow's resampler and the very fp32 values of `_preprocess`, which stays here as the host statement of the same
transform (the tests' reference), so the embeddings are bit for bit those of the host path.
`decoder="device"` (opt-in; "host" is the default): the threads only read the files and parse their headers, baseline JPEG files
cross to the device as file bytes and zh_jpeg_decode (zutis_amd/jpeg_device.py: byte for byte Pillow's pixels) decodes them in front
of the resize kernel; any other file, and any the device reports as damaged, is decoded by Pillow as before — the embeddings are the same.
`decoder="device-split"`: the same route with every file's scan split among lanes (zh_jpeg_decode_split: a file without restart markers
is one entropy segment, which "device" leaves to one lane); the same pixels, the same embeddings.
"""
import os
import pickle as pkl
from typing import Dict, List, Optional

import numpy as np
import torch
from PIL import Image

from zutis_amd import ops, preprocess
from zutis_amd.engine import ClipImageEncoder

_MEAN = np.array((0.48145466, 0.4578275, 0.40821073), np.float32)
_STD = np.array((0.26862954, 0.26130258, 0.27577711), np.float32)


def resize_crop_box(w: int, h: int, n_px: int):
    """CLIP's `_transform` (third-party clip, used at utils/extract_image_embeddings.py:43,98-103) =
    torchvision Resize(n_px, BICUBIC) + CenterCrop(n_px), with torchvision's integer conventions: the shorter side becomes
    n_px and the longer one int(n_px * long / short) (truncation); the crop offset is int(round((side - n_px) / 2.0))
    (Python's round-half-to-even).  Returns ((new_w, new_h), (left, top))."""
    if w <= h:
        nw, nh = n_px, int(n_px * h / w)
    else:
        nw, nh = int(n_px * w / h), n_px
    return (nw, nh), (int(round((nw - n_px) / 2.0)), int(round((nh - n_px) / 2.0)))


def _preprocess(p_image: str, n_px: int) -> np.ndarray:
    im = Image.open(p_image).convert("RGB")
    (nw, nh), (left, top) = resize_crop_box(*im.size, n_px)
    im = im.resize((nw, nh), Image.BICUBIC)
    a = np.asarray(im.crop((left, top, left + n_px, top + n_px)), np.float32) / 255.0
    return ((a - _MEAN) / _STD).transpose(2, 0, 1)


@torch.no_grad()
def extract_image_embeddings(
        p_images: List[str],
        model_name: str = "RN50",
        fp: Optional[str] = None,
        device: torch.device = torch.device("cuda:0"),
        batch_size: int = 256,
        n_workers: int = 16,
        *,
        state_dict: Optional[dict] = None,
        precision: str = "exact",
        decoder: str = "host",
) -> Dict[str, torch.Tensor]:
    if "ViT" not in model_name:
        raise NotImplementedError(f"{model_name}: only the CLIP-ViT towers are on the MI355X hot path")
    if state_dict is None:
        import clip                                                    # reference :43 (needs the package + weights)
        model, _ = clip.load(model_name, device="cpu")
        state_dict = model.state_dict()
    vis = {k: v.float().to(device) for k, v in state_dict.items() if k.startswith("visual.")}
    patch = vis["visual.conv1.weight"].shape[-1]
    enc = ClipImageEncoder(vis, patch, prefix="visual.", precision=precision)
    n_px = patch * enc.grid
    out: Dict[str, torch.Tensor] = {}
    lut = torch.from_numpy(preprocess.normalise_table(_MEAN, _STD)).to(device)
    loader = preprocess.BatchLoader(p_images, n_px, batch_size, n_workers, resize_crop_box, decoder=decoder)

    def transform(batch, staged):
        packed, desc = preprocess.split_staging(staged, len(batch.paths))
        return (packed, desc), ops.resize_crop_normalize(packed, desc, n_px, lut, kmax=batch.kmax)

    with preprocess.device_batches(loader, device, transform) as steps:
        for k, (batch, _, x) in enumerate(steps):
            i, chunk = k * batch_size, batch.paths
            emb = enc.encode_image(x).cpu()                                 # L2-normalised, fp32 (reference :72-76); the copy back completes
                                                                            # behind the batch's upload, so the loop's event wait never blocks
            for p, e in zip(chunk, emb):
                out[os.path.basename(p)] = e.clone()
            if fp is not None and ((i // batch_size) % max(1, (len(p_images) // batch_size) // 20) == 0 or i + batch_size >= len(p_images)):
                pkl.dump(out, open(fp, "wb"))                               # periodic checkpoint (reference :80-85)
    return out
