"""Instance predictions as pictures: what utils/visualiser.py:154-187 (trainer.py:368-372, coco20k_eval.py:271-276) asks detectron2 for,
without detectron2 or matplotlib — an id map and a colour overlay painted by zh_instance_paint where the masks already lie.

The picture, per pixel: among the predictions whose score is above min_score (strict, as convert_to_instances compares,
visualiser.py:139) the one of highest score that covers the pixel (ties: the earlier one) is its `top`; the id map holds its position + 1
(0: none); the overlay is the image where there is no top, the top's colour where a 4-neighbour inside the image has another top (the
outline), and elsewhere predict_files.blend of the image and that colour.  paint_reference states this in NumPy integers (the oracle of
the tests, the host arm of tools/instance_paint_bench.py); everything else here runs the kernel: paint_predictions for callers who hold
prediction dicts, visualise_instance_predictions as the method to bind onto the reference's Visualiser.  predict_from_files(...,
instance_map=True, instance_overlay=True) and ZUTIS.predict_instances_painted paint straight behind the NMS, with no RLE decode at all.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from .predict_files import blend

COLOUR_LEVELS = (255, 210, 165)      # the value (brightness) levels instance_colours cycles through
COLOUR_SATURATION = 230              # of 255
COLOUR_HUE_STEP = 137                # degrees: the golden angle, coprime to 360


def instance_colours(n: int) -> np.ndarray:
    """u8 [n, 3]: colour i has hue (137 i) mod 360 degrees (the golden angle: neighbours in the table lie far apart on the colour wheel),
    saturation 230 / 255 and value COLOUR_LEVELS[(i + i // 360) % 3], converted from HSV to RGB in integers (floor divisions):
    with v the value, s the saturation, region = hue // 60, rem = hue % 60,
        p = v (255 - s) // 255,  q = v (255 * 60 - s rem) // (255 * 60),  t = v (255 * 60 - s (60 - rem)) // (255 * 60),
    (r, g, b) = (v,t,p), (q,v,p), (p,v,t), (p,q,v), (t,p,v), (v,p,q) for region 0..5.  The first 1080 entries are pairwise distinct; the
    table repeats after them."""
    i = np.arange(int(n), dtype=np.int64)
    hue = (COLOUR_HUE_STEP * i) % 360
    v = np.asarray(COLOUR_LEVELS, np.int64)[(i + i // 360) % 3]
    s = COLOUR_SATURATION
    region, rem = hue // 60, hue % 60
    p = v * (255 - s) // 255
    q = v * (255 * 60 - s * rem) // (255 * 60)
    t = v * (255 * 60 - s * (60 - rem)) // (255 * 60)
    r = np.choose(region, [v, q, p, p, t, v])
    g = np.choose(region, [t, v, v, q, p, p])
    b = np.choose(region, [p, p, t, v, v, q])
    return np.ascontiguousarray(np.stack([r, g, b], axis=1).astype(np.uint8)).reshape(int(n), 3)


def paint_order(scores, min_score: float = 0.0):
    """The painted slots in paint rank: score > min_score in float64 (strict), by score descending, ties to the lower slot."""
    s = np.asarray(scores, np.float64).reshape(-1)
    return sorted((j for j in range(s.size) if s[j] > np.float64(min_score)), key=lambda j: (-s[j], j))


def paint_reference(image_u8, masks_u8, scores, colours, alpha: int = 128, outline: bool = True, min_score: float = 0.0):
    """zh_instance_paint for one image in NumPy integers: image u8 [H,W,3], masks [n,H,W] (non-zero = in the mask), scores [n], colours u8
    [n,3], slots in the order given -> (ids int64 [H,W]: slot + 1 of the pixel's top, 0 for none; overlay u8 [H,W,3])."""
    if int(alpha) != alpha or not 0 <= int(alpha) <= 256:
        raise ValueError(f"paint_reference: alpha {alpha!r} is not an integer in 0..256")
    image = np.asarray(image_u8)
    H, W = image.shape[:2]
    masks = np.asarray(masks_u8).reshape(-1, H, W)
    colours = np.asarray(colours, np.uint8).reshape(-1, 3)
    ids = np.zeros((H, W), np.int64)
    for j in paint_order(scores, min_score):
        ids[(ids == 0) & (masks[j] != 0)] = j + 1
    overlay = image.astype(np.uint8).copy()
    top = ids > 0
    if top.any():
        col = colours[np.maximum(ids, 1) - 1]                                  # [H,W,3]; meaningless where there is no top
        overlay[top] = blend(image[top], col[top], alpha)
        if outline:
            other = np.zeros((H, W), bool)                                       # a 4-neighbour INSIDE the image with another top (or none)
            other[:, 1:] |= ids[:, 1:] != ids[:, :-1]
            other[:, :-1] |= ids[:, :-1] != ids[:, 1:]
            other[1:, :] |= ids[1:, :] != ids[:-1, :]
            other[:-1, :] |= ids[:-1, :] != ids[1:, :]
            edge = other & top
            overlay[edge] = col[edge]
    return ids, overlay


def _image_bytes(image) -> np.ndarray:
    """u8 [H,W,3] of a PIL image, a u8 [H,W,3] array, or the normalised float array [3,H,W] converted as Visualiser.numpy_to_pil does
    (visualiser.py:17-28: float64 x * std + mean, * 255, clip to 0..255, truncate)."""
    if isinstance(image, np.ndarray):
        if image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3:
            return np.ascontiguousarray(image)
        if image.ndim != 3 or image.shape[0] != 3:
            raise TypeError(f"image: a float array [3, H, W] or a u8 array [H, W, 3] expected, got {image.dtype} {image.shape}")
        a = image * np.array((0.229, 0.224, 0.225))[:, None, None]
        a = a + np.array((0.485, 0.456, 0.406))[:, None, None]
        a = np.clip(a * 255.0, 0, 255)
        return np.ascontiguousarray(a.astype(np.uint8).transpose(1, 2, 0))
    from PIL import Image
    if not isinstance(image, Image.Image):
        raise TypeError(f"image: a PIL image or a NumPy array expected, got {type(image).__name__}")
    return np.ascontiguousarray(np.asarray(image.convert("RGB")))


def _align(n: int) -> int:
    return -(-n // 16) * 16


def paint_predictions(image, predictions: Sequence[dict], *, colours=None, alpha: int = 128, outline: bool = True, min_score: float = 0.0,
                      device=None):
    """The picture of one image's prediction dicts (what predict(mask_type="instance") returns): their RLEs are decoded on the host
    (rle.decode_np), image, masks, scores and colours go up in ONE copy, zh_instance_paint paints, and (ids int64 [H,W], overlay u8
    [H,W,3]) come back as NumPy; prediction i has id i + 1.  colours: u8 [n,3], one per prediction (None: instance_colours(n))."""
    import torch
    from . import ops, rle
    img = _image_bytes(image)
    H, W = img.shape[:2]
    n = len(predictions)
    Q = max(n, 1)
    col = instance_colours(n) if colours is None else np.asarray(colours)
    if col.shape != (n, 3) or (col.size and (col.min() < 0 or col.max() > 255)):
        raise ValueError(f"paint_predictions: colours [{n}, 3] in 0..255 expected, got {col.shape}")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    # one buffer, every part at a multiple of 16 bytes: [desc | score f64 | index int32 | count | colours | image | masks]
    o_desc, o_score = 0, 32
    o_index = o_score + _align(8 * Q)
    o_count = o_index + _align(4 * Q)
    o_col = o_count + 16
    o_img = o_col + _align(3 * Q)
    o_mask = o_img + _align(3 * H * W)
    host = np.zeros(o_mask + Q * H * W, np.uint8)
    host[o_desc:o_desc + 32].view(np.int32)[:] = (0, W, H, W, H, 0, 0, 0)
    host[o_score:o_score + 8 * n].view(np.float64)[:] = [float(p["score"]) for p in predictions]
    host[o_index:o_index + 4 * Q].view(np.int32)[:] = np.arange(Q)
    host[o_count:o_count + 4].view(np.int32)[:] = n
    host[o_col:o_col + 3 * n] = col.astype(np.uint8).reshape(-1)
    host[o_img:o_img + 3 * H * W] = img.reshape(-1)
    for j, p in enumerate(predictions):
        m = rle.decode_np(p["segmentation"])
        if m.shape != (H, W):
            raise ValueError(f"paint_predictions: prediction {j} is a {m.shape} mask, the image is {(H, W)}")
        host[o_mask + j * H * W:o_mask + (j + 1) * H * W] = m.reshape(-1)
    with torch.cuda.device(dev):
        buf = torch.from_numpy(host).to(dev)
        id_format = "u8" if Q <= 255 else "rg16"
        out = torch.empty((H * W * ((1 if id_format == "u8" else 3) + 3),), dtype=torch.uint8, device=dev)
        ids_out = out[:out.numel() - 3 * H * W].view((1, H, W) if id_format == "u8" else (1, H, W, 3))
        ops.instance_paint(buf[o_index:o_index + 4 * Q].view(torch.int32).view(1, Q), buf[o_score:o_score + 8 * Q].view(torch.float64).view(1, Q),
                           buf[o_count:o_count + 4].view(torch.int32), H, W, masks=buf[o_mask:].view(1, Q, H, W),
                           colours=buf[o_col:o_col + 3 * Q].view(1, Q, 3), alpha=alpha, outline=outline, min_score=min_score,
                           packed=buf[o_img:o_img + _align(3 * H * W)], desc=buf[:32].view(torch.int32).view(1, 8),
                           desc_host=torch.from_numpy(host[:32].view(np.int32).reshape(1, 8)), id_format=id_format, ids_out=ids_out,
                           overlay_out=out[out.numel() - 3 * H * W:].view(1, H, W, 3))
        back = out.cpu().numpy()
    raw = back[:back.size - 3 * H * W]
    ids = raw.astype(np.int64).reshape(H, W) if id_format == "u8" else \
        (raw.reshape(H, W, 3)[..., 0].astype(np.int64) + 256 * raw.reshape(H, W, 3)[..., 1].astype(np.int64))
    return ids, back[back.size - 3 * H * W:].reshape(H, W, 3).copy()


def visualise_instance_predictions(self, image, predictions, label_id_to_rgb=None, confidence_threshold: float = 0.75,
                                   fp: Optional[str] = None, instance_mode=None):
    """Visualiser.visualise_instance_predictions (utils/visualiser.py:154-187) over zh_instance_paint, to bind in its place:
        Visualiser.visualise_instance_predictions = zutis_amd.instance_paint.visualise_instance_predictions
    image: a PIL image, or the normalised float array [3,H,W] (converted as numpy_to_pil does); predictions: the coco-style dicts; a
    prediction is drawn when its score > confidence_threshold (visualiser.py:139), in label_id_to_rgb[category_id] when that is given
    (detectron2's ColorMode.SEGMENTATION), else in its instance_colours entry.  instance_mode is accepted and ignored.  Writes the PNG to
    fp when given and returns the overlay u8 [H,W,3].  No class names or scores are drawn (the dicts carry them)."""
    n = len(predictions)
    if label_id_to_rgb is not None:
        col = np.asarray([tuple(label_id_to_rgb[p["category_id"]]) for p in predictions], dtype=np.int64).reshape(n, 3)
    else:
        col = instance_colours(n)
    _, overlay = paint_predictions(image, predictions, colours=col, min_score=float(confidence_threshold))
    if fp is not None:
        from PIL import Image
        Image.fromarray(overlay).save(fp, format="PNG")
    return overlay
