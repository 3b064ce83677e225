"""Predictions from image files: the loop of coco20k_eval.py:241-268 (forward, instance predict, collect the COCO result dicts) and the
common case next to it — run the segmenter over a list of images, get label maps on disk — over the drop-in ZUTIS.

The label of a pixel is zutis.py:366-372 (arg-max over the bilinear up-sampling of the low-res logits, at the file's own size as
trainer.py:322-325 sizes it); it leaves the arg-max kernel as the bytes of the PNG it becomes (zh_upsample_argmax_bytes): one byte per
pixel ("u8"), or R = label & 255, G = label >> 8, B = 0 ("rg16": imagenet_s.py:93 read backwards) — the two formats evaluate_from_files
reads as ground truth.  The same launch can blend a palette colour over the decoded image, which is already on the device as the bytes
of the batch's staging buffer.  The file pipeline of preprocess.py: decoding threads fill a pinned staging buffer one batch ahead
(PredictBatchLoader: batches of one file size); per batch (device_batches) ONE host-to-device copy and ops.resize_normalize; then the
module's forward, the byte kernel, ONE device-to-host copy into one of the two pinned output buffers of a WriterRing, whose threads
encode and write batch k's PNGs while batch k + 1 is on the device.  png_encoder="device": the pictures stay on the device, zh_png_deflate
(png_device.py) turns each into the zlib stream of its PNG, and the one copy back carries the streams: a writer frames and writes.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import jpeg_device, picture_out, png_device, preprocess
from .evaluate import _require_dropin, collect_instance_predictions
from .preprocess import MAX_THREADS
LABEL_LIMIT = {"u8": 256, "rg16": 65536}
LABEL_CHANNELS = {"u8": 1, "rg16": 3}


def encode_labels(labels: np.ndarray, label_format: str) -> np.ndarray:
    """The bytes zh_upsample_argmax_bytes writes for an integer label map [..., H, W]: u8 [..., H, W] ("u8") or u8 [..., H, W, 3] =
    (label & 255, label >> 8, 0) ("rg16").  NumPy statement of the formats; not a product path."""
    v = np.asarray(labels).astype(np.int64)
    if v.size and (v.min() < 0 or v.max() >= LABEL_LIMIT[label_format]):
        raise ValueError(f"encode_labels: labels outside [0, {LABEL_LIMIT[label_format]}) do not fit {label_format!r}")
    if label_format == "u8":
        return v.astype(np.uint8)
    return np.stack([v & 255, v >> 8, np.zeros_like(v)], axis=-1).astype(np.uint8)


def decode_labels(raw: np.ndarray, label_format: str) -> np.ndarray:
    """int64 label map of the bytes of a label PNG, as EvalBatchLoader / zh_upsample_argmax_score read them (B is ignored)."""
    raw = np.asarray(raw)
    if label_format == "u8":
        return raw.astype(np.int64)
    return raw[..., 0].astype(np.int64) + 256 * raw[..., 1].astype(np.int64)


def blend(image_u8: np.ndarray, colours_u8: np.ndarray, alpha: int) -> np.ndarray:
    """The overlay of zh_upsample_argmax_bytes in NumPy integers: (image * (256 - alpha) + colours * alpha + 128) >> 8, alpha in 0..256."""
    if int(alpha) != alpha or not 0 <= int(alpha) <= 256:
        raise ValueError(f"blend: alpha {alpha!r} is not an integer in 0..256")
    a = int(alpha)
    return ((np.asarray(image_u8).astype(np.int64) * (256 - a) + np.asarray(colours_u8).astype(np.int64) * a + 128) >> 8).astype(np.uint8)


def normalise_palette(palette, n: int) -> np.ndarray:
    """u8 [n, 3] from a dict {label: (r, g, b)} (utils.get_palette) or an array-like [>= n, 3]: it must cover 0 .. n - 1 with integer
    colours in 0 .. 255 (entries beyond n - 1 are dropped)."""
    if isinstance(palette, dict):
        missing = [i for i in range(n) if i not in palette]
        if missing:
            raise ValueError(f"palette: no colour for label {missing[0]} ({len(missing)} of {n} labels missing)")
        a = np.asarray([tuple(palette[i]) for i in range(n)])
    else:
        a = np.asarray(palette)
        if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < n:
            raise ValueError(f"palette: [{n}, 3] expected (one colour per label), got {a.shape}")
        a = a[:n]
    if a.shape != (n, 3):
        raise ValueError(f"palette: every colour must be (r, g, b), got {a.shape}")
    if not np.issubdtype(a.dtype, np.integer):
        if not np.array_equal(a, np.round(a)):
            raise ValueError("palette: colours must be integers in 0..255 (get_palette's float form is for matplotlib)")
        a = a.astype(np.int64)
    if a.size and (a.min() < 0 or a.max() > 255):
        raise ValueError("palette: colours must lie in 0..255")
    return np.ascontiguousarray(a.astype(np.uint8))


def resolve_output_paths(p_images: Sequence[str], out_dir: Optional[str], out_paths: Optional[Sequence[str]], overlay: bool = False,
                         overlay_ext: str = ".png"):
    """(label paths, overlay paths or None): out_paths[i] as given, or {out_dir}/{stem of the image}.png; the overlay goes to
    {stem of the label map}_overlay.png (overlay_ext: ".jpg" for a JPEG overlay) beside it.  Exactly one of out_dir / out_paths; two
    outputs on one path: ValueError."""
    if (out_dir is None) == (out_paths is None):
        raise ValueError("predict_from_files: give exactly one of out_dir and out_paths")
    if out_paths is not None:
        labels = [os.fspath(p) for p in out_paths]
        if len(labels) != len(p_images):
            raise ValueError("predict_from_files: one output path per image")
    else:
        labels = [os.path.join(os.fspath(out_dir), os.path.splitext(os.path.basename(os.fspath(p)))[0] + ".png") for p in p_images]
    overlays = [os.path.splitext(p)[0] + "_overlay" + overlay_ext for p in labels] if overlay else None
    seen = {}
    for i, p in enumerate(labels + (overlays or [])):
        key = os.path.normpath(os.path.abspath(p))
        if key in seen:
            a, b = p_images[seen[key] % len(labels)], p_images[i % len(labels)]
            raise ValueError(f"predict_from_files: {a} and {b} map to one output path, {p}")
        seen[key] = i
    return labels, overlays


def resolve_instance_paths(p_images: Sequence[str], label_paths: Sequence[str], written: Sequence[Optional[Sequence[str]]], instance_map: bool,
                           instance_overlay: bool, overlay_ext: str = ".png"):
    """(id-map paths or None, instance-overlay paths or None): {stem of the label map}_instances.png and {stem}_instances_overlay.png (or
    overlay_ext in its place) beside
    where image i's label map goes (or would go: label_paths, resolve_output_paths' first result).  They take part in the
    one-path-one-output check together with `written`, the lists of files the call writes besides them (None entries are skipped)."""
    maps = [os.path.splitext(p)[0] + "_instances.png" for p in label_paths] if instance_map else None
    overlays = [os.path.splitext(p)[0] + "_instances_overlay" + overlay_ext for p in label_paths] if instance_overlay else None
    seen = {}
    for paths in list(written) + [maps, overlays]:
        for i, p in enumerate(paths or []):
            key = os.path.normpath(os.path.abspath(p))
            if key in seen:
                raise ValueError(f"predict_from_files: {p_images[seen[key]]} and {p_images[i]} map to one output path, {p}")
            seen[key] = i
    return maps, overlays


def _validate_instance_pictures(instance: bool, instance_map: bool, instance_overlay: bool, instance_colours, instance_min_score, palette, n: int):
    """The instance_* arguments of predict_from_files, before any work -> (colour mode, u8 colour table or None)."""
    if not (instance_map or instance_overlay):
        return None, None
    if not instance:
        raise ValueError("predict_from_files: instance_map / instance_overlay picture the instance predictions: they need instance=True")
    if isinstance(instance_min_score, bool) or not isinstance(instance_min_score, (int, float, np.integer, np.floating)) or instance_min_score != instance_min_score:
        raise ValueError(f"predict_from_files: instance_min_score {instance_min_score!r} is not a number")
    if isinstance(instance_colours, str):
        if instance_colours not in ("category", "instance"):
            raise ValueError(f"predict_from_files: instance_colours {instance_colours!r} is not \"category\", \"instance\" or an array [queries, 3]")
        if instance_colours == "category":
            if palette is None:
                raise ValueError("predict_from_files: instance_colours=\"category\" needs a palette (indexed by the network's category index)")
            return "category", normalise_palette(palette, n)
        return "instance", None
    a = np.asarray(instance_colours)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 1:
        raise ValueError(f"predict_from_files: instance_colours as an array is [queries, 3] (one colour per id), got {a.shape}")
    return "array", normalise_palette(a, a.shape[0])


def predictions_json_form(predictions: Sequence[dict]) -> List[dict]:
    """What trainer.py:393-398 dumps: every prediction without its "bbox", the RLE "counts" as a str; new dicts, the given ones stay whole."""
    out = []
    for p in predictions:
        q = {k: v for k, v in p.items() if k != "bbox"}
        seg = dict(q["segmentation"])
        if isinstance(seg["counts"], (bytes, bytearray)):
            seg["counts"] = bytes(seg["counts"]).decode("ascii")
        seg["size"] = [int(s) for s in seg["size"]]
        q["segmentation"] = seg
        out.append(q)
    return out


def _jsonable(o):
    if isinstance(o, np.generic):
        return o.item()
    if isinstance(o, np.ndarray):
        return o.tolist()
    raise TypeError(f"predictions_json: {type(o).__name__} is not JSON serialisable")


def _validate(n: int, n_images: int, semantic: bool, instance: bool, label_format: str, palette, overlay: bool, alpha, image_ids, compress_level):
    if not semantic and not instance:
        raise ValueError("predict_from_files: semantic=False and instance=False leave nothing to predict")
    if label_format not in LABEL_LIMIT:
        raise ValueError(f"predict_from_files: label_format {label_format!r} is not one of {sorted(LABEL_LIMIT)}")
    if n > 65536:
        raise ValueError(f"predict_from_files: {n} categories do not fit a label file (at most 65536, \"rg16\")")
    if semantic and n > LABEL_LIMIT[label_format]:
        raise ValueError(f"predict_from_files: {n} categories do not fit one byte per pixel: use label_format=\"rg16\"")
    if image_ids is not None and len(image_ids) != n_images:
        raise ValueError("predict_from_files: one image id per image")
    if overlay and not semantic:
        raise ValueError("predict_from_files: overlay=True colours the semantic labels: it needs semantic=True")
    if overlay and palette is None:
        raise ValueError("predict_from_files: overlay=True needs a palette")
    if int(alpha) != alpha or not 0 <= int(alpha) <= 256:
        raise ValueError(f"predict_from_files: alpha {alpha!r} is not an integer in 0..256")
    if int(compress_level) != compress_level or not 0 <= int(compress_level) <= 9:
        raise ValueError(f"predict_from_files: compress_level {compress_level!r} is not an integer in 0..9")
    return normalise_palette(palette, n) if (palette is not None and semantic) else None


def thread_split(n_workers: int, writers_needed: bool):
    """(decoders, writers): together min(n_workers, 16) threads, at least one of each kind that is needed (so two when n_workers is 1
    and files are written); writers get half, PNG encoding costing about what decoding costs."""
    if not writers_needed:
        return max(1, min(int(n_workers), MAX_THREADS)), 0
    return preprocess.thread_split(n_workers, 0.5)


@torch.no_grad()
def predict_from_files(network, p_images: Sequence[str], *, out_dir: Optional[str] = None, out_paths: Optional[Sequence[str]] = None,
                       semantic: bool = True, label_format: str = "u8", palette=None, overlay: bool = False, alpha: int = 128,
                       max_size: Optional[int] = None, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), batch_size: int = 4,
                       n_workers: int = 16, window: int = 512, compress_level: int = 1, instance: bool = False,
                       image_ids: Optional[Sequence] = None, new_label_id_to_old_label_id: Optional[Dict[int, int]] = None,
                       label_id_to_category: Optional[Dict[int, str]] = None, nms_type: Optional[str] = "hard",
                       predictions_json: Optional[str] = None, instance_map: bool = False, instance_overlay: bool = False,
                       instance_colours="instance", instance_min_score: float = 0.0, instance_outline: bool = True,
                       png_encoder: str = "host", decoder: str = "host", overlay_format: str = "png", jpeg_quality: int = 90,
                       jpeg_subsampling: str = "4:2:0", jpeg_encoder: str = "host") -> dict:
    """The segmenter over a list of image files: label PNGs (and overlays) on disk, and / or the instance predictions.

    network: the drop-in ZUTIS (zutis_amd/dropin/networks/zutis.py) on a GPU; its text embeddings are the n categories.
    semantic=True: the label map of image i (zutis.py:366-372 at the file's own (H, W)) is written to out_paths[i], or to
    {out_dir}/{stem of the image}.png — give exactly one of the two; directories are created; two images on one output path is a
    ValueError before any work.  label_format "u8" (n <= 256): a mode L PNG, the byte is the label; with a palette a mode P PNG that
    carries it — the exact label map and the coloured picture in one file.  "rg16" (n <= 65536): a mode RGB PNG, R = label & 255,
    G = label >> 8, B = 0 (imagenet_s.py:93 read backwards).  These are the files evaluate_from_files reads as ground truth.
    palette: {label: (r, g, b)} as utils.get_palette returns, or an array [n, 3]; integers 0..255 covering 0 .. n - 1.
    overlay=True (needs the palette): {stem}_overlay.png beside the label map, (image * (256 - alpha) + colour * alpha + 128) >> 8 per
    channel, alpha an integer in 0..256.  An image the loader had to resize on the host (a source side more than 75 times the target)
    is not on the device at file size: NotImplementedError naming the file.
    max_size None: the image goes in at its own size; else the longer edge is capped with Pillow BILINEAR (imagenet_s.py:71-76); the
    prediction is made at the file's size either way.  Batches: up to batch_size images of one file size out of a window of `window`
    paths, grouped as evaluate_from_files groups them.  Decoding and writing threads together: min(n_workers, 16) (two at the least).
    instance=True: predict(mask_type="instance", size=(H, W), ...) per batch as coco20k_eval.py:258-265 calls it; image_ids: one per
    image (None: 0, predict's default).  predictions_json: a path that receives what trainer.py:393-398 writes — the dicts without
    "bbox", RLE counts as str, in input-path order.
    instance_map / instance_overlay (need instance=True): a picture of the instance predictions per image, painted on the device behind
    the NMS (zh_instance_paint; what utils/visualiser.py:154-187 draws with detectron2) — {stem}_instances.png: per pixel the id of the
    prediction of highest score (ties: the lower id) among those with score > instance_min_score that cover it, 0 where none does, mode L
    (the byte is the id), or RGB (R = id & 255, G = id >> 8, B = 0) when the network has more than 255 queries;
    {stem}_instances_overlay.png: mode RGB, the image with every such pixel blended with its prediction's colour (alpha, as the semantic
    overlay) and, with instance_outline, in the pure colour where a 4-neighbour belongs to another prediction or to none.  Both sit beside
    where the label map goes or would go (out_dir / out_paths are accepted without semantic=True) and take part in the one-path check.
    instance_colours: "instance" (entry id - 1 of instance_paint.instance_colours), "category" (palette[the network's category index], needs
    the palette), or an array [>= queries, 3] with one colour per id.  The bytes share the batch's device buffer, its one copy back and the
    writer slot with the semantic outputs.  The result gains "instance_map_paths", "instance_overlay_paths" and "instance_ids": parallel to
    "instance_predictions", the id of each prediction in its image's map.
    png_encoder "host": the writer threads encode with Pillow (compress_level).  "device": every picture of the call — label map in any
    format, overlay, id map, instance overlay — is encoded on the device behind the kernels that made it (one zh_png_deflate per kind of
    picture and batch: png_device.py defines the stream — Up filter, run-length deflate with the fixed Huffman code); the batch's one copy
    back carries the streams at their worst-case stride and their lengths, and a writer only frames a stream (chunk CRCs) and writes the
    file.  The files decode to the same pixels, mode and palette; label and id maps come out at 1.14 - 1.19 x Pillow's level-1 size,
    photographic overlays at 2.0 x (1.05 of their raw bytes against 0.52; profiles/NOTES.md), which is why "host" is the default.
    compress_level is unused with "device".  Any other value: ValueError before any work.
    decoder "host": the decoding threads run Pillow.  "device": they read the files and parse the headers; baseline JPEG files cross to
    the device as their file bytes and are decoded there (zh_jpeg_decode: zutis_amd/jpeg_device.py defines the pixels, byte for byte
    Pillow's), everything else — and any file whose scan the device reports as damaged — is decoded by Pillow as ever, so the files
    written do not depend on it.  "device-split": as "device", with every file's scan split among lanes (zh_jpeg_decode_split), which is
    what a file without restart markers needs to be decoded in parallel.  Any other value: ValueError before any work.
    overlay_format "png": the two overlays are PNG files, as above.  "jpeg": {stem}_overlay.jpg and {stem}_instances_overlay.jpg take
    their place — baseline JPEG at jpeg_quality (1 .. 100) and jpeg_subsampling ("4:2:0" | "4:4:4") with the Annex K Huffman tables and a
    restart marker every 16 MCUs: the file zutis_amd/jpeg_device.encode_np defines, about a tenth of the PNG's bytes — under the same
    result keys and the same one-path check; label maps and id maps stay PNG under png_encoder whatever these say.  jpeg_encoder "host":
    the writer threads encode with Pillow (save(..., restart_marker_blocks=16); a Pillow without that option: RuntimeError before any
    work).  "device": the overlays are encoded on the device (one zh_jpeg_encode per kind of overlay and batch, behind the
    zh_png_deflate calls), their scans travel in the batch's one copy back at jpeg_device.scan_slot stride and a writer puts the header
    and FF D9 around them; the files are the same bytes either way.  A scan that does not fit its slot — the JPEG would be larger than
    the pixels: noise at quality 100 — is copied back raw and encoded by the host arm; the result then counts it in
    "jpeg_host_fallbacks" (a key of the result with overlay_format="jpeg" only).  Any other value of the four: ValueError naming the
    argument, before any work.
    Returns {"label_paths": [...] | None, "overlay_paths": [...] | None, "instance_predictions": the dicts predict gave (with "bbox"),
    in input-path order, "n_images": int}.
    A missing or unreadable image (FileNotFoundError / OSError / ValueError) and a directory or file that cannot be written (OSError)
    are raised here; no decoding or writing thread outlives the call and the device stays usable."""
    p_images = [os.fspath(p) for p in p_images]
    on_device = png_device.check_encoder("predict_from_files", png_encoder) == "device"
    jpeg_device.check_decoder("predict_from_files", decoder)
    as_jpeg = jpeg_device.check_overlay_format("predict_from_files", overlay_format) == "jpeg"
    jpeg_device.check_encode_args("predict_from_files", jpeg_quality, jpeg_subsampling)
    if jpeg_device.check_encoder("predict_from_files", jpeg_encoder) == "host" and as_jpeg:
        jpeg_device.require_host_encoder("predict_from_files")
    overlay_ext, overlay_kind = (".jpg", (3, "JPEG", None)) if as_jpeg else (".png", (3, "RGB", None))
    _require_dropin(network, "predict_from_files")
    n = int(network.text_embeddings.shape[0])
    pal = _validate(n, len(p_images), semantic, instance, label_format, palette, overlay, alpha, image_ids, compress_level)
    colour_mode, colour_table = _validate_instance_pictures(instance, instance_map, instance_overlay, instance_colours, instance_min_score, palette, n)
    paint = colour_mode is not None
    label_paths = overlay_paths = map_paths = iovl_paths = None
    if semantic or paint:
        would_be, overlay_paths = resolve_output_paths(p_images, out_dir, out_paths, overlay, overlay_ext)
        label_paths = would_be if semantic else None
        if paint:
            map_paths, iovl_paths = resolve_instance_paths(p_images, would_be, [label_paths, overlay_paths], instance_map, instance_overlay, overlay_ext)
        for d in sorted({os.path.dirname(p) or "." for paths in (label_paths, map_paths, iovl_paths) for p in (paths or [])}):
            os.makedirs(d, exist_ok=True)
    elif out_dir is not None and out_paths is not None:
        raise ValueError("predict_from_files: give exactly one of out_dir and out_paths")
    per_image: List[List[dict]] = [[] for _ in p_images]
    per_image_ids: List[List[int]] = [[] for _ in p_images]
    if p_images:
        eng = network._get_engine()
        dev = eng._device()
        n_decode, n_write = thread_split(n_workers, semantic or paint)
        ch = LABEL_CHANNELS[label_format]
        mode = "RGB" if label_format == "rg16" else ("P" if pal is not None else "L")
        pal_bytes = pal.tobytes() if mode == "P" else None
        lut = torch.from_numpy(preprocess.normalise_table(mean, std)).to(dev)
        pal_dev = torch.from_numpy(pal).to(dev) if (overlay and pal is not None) else None
        colour_dev = torch.from_numpy(colour_table).to(dev) if colour_table is not None else None
        loader = preprocess.PredictBatchLoader(p_images, max_size, batch_size, n_decode, window=window, decoder=decoder)
        # name -> (paths, (c, mode, palette bytes)) of the kinds of picture the call writes, in layout order; the id map's once Q is known
        kinds = {name: kind for name, kind in (("labels", (label_paths, (ch, mode, pal_bytes))), ("overlay", (overlay_paths, overlay_kind)),
                                               ("ids", (map_paths, None)), ("instance_overlay", (iovl_paths, overlay_kind))) if kind[0] is not None}
        with preprocess.device_batches(loader, dev, preprocess.resize_normalize_of(lut)) as steps, \
                picture_out.PictureStage(png_encoder, loader.pin, n_write, dev, compress_level=compress_level,
                                         error="predict_from_files: the device encoder left no stream for {path} ({h} x {w} x {c})",
                                         jpeg_encoder=jpeg_encoder if as_jpeg else "host", jpeg_quality=jpeg_quality, jpeg_subsampling=jpeg_subsampling) as stage:
            for k, (batch, (packed, desc), x) in enumerate(steps):
                B, (H, W) = len(batch.paths), batch.size_hw
                if (overlay or instance_overlay) and batch.n_host:
                    raise NotImplementedError(f"predict_from_files: {batch.host_paths[0]} was resized on the host (a side more than 75 times its "
                                              f"target): its decoded image is not on the device at file size, no overlay can be made")
                out = network(x)                                                           # the module's forward: its hipGraph replay applies
                if paint:
                    Q = int(out["mask_proposals"].shape[-3])
                    id_format = "u8" if Q <= 255 else "rg16"
                    if instance_map:
                        kinds["ids"] = (map_paths, (LABEL_CHANNELS[id_format], "L" if id_format == "u8" else "RGB", None))
                if kinds:
                    layout = picture_out.Layout([(H, W)] * B, [kind for _, kind in kinds.values()], stage.jpeg_encoder)
                    view = dict(zip(kinds, layout.views(stage.take(k, layout, [paths[i] for paths, _ in kinds.values() for i in batch.indices]))))
                if semantic:
                    eng.label_bytes(out["patch_tokens"], network.text_embeddings, (H, W), label_format=label_format, labels_out=view["labels"],
                                    palette=pal_dev, packed=packed if overlay else None, desc=desc if overlay else None, alpha=int(alpha),
                                    overlay_out=view.get("overlay"), desc_host=batch.desc)
                if kinds and not paint:
                    stage.commit()                                                         # labels + overlay: one D2H
                if instance and not paint:
                    collect_instance_predictions(network, out, batch, image_ids, per_image, label_id_to_category=label_id_to_category,
                                                 new_label_id_to_old_label_id=new_label_id_to_old_label_id, nms_type=nms_type)
                elif instance:
                    if colour_mode == "array" and colour_table.shape[0] < Q:
                        raise ValueError(f"predict_from_files: instance_colours holds {colour_table.shape[0]} colours, the network has {Q} queries")
                    # the paint rides the predict's stream behind the NMS: the pictures are complete when the predict returns, and go back
                    # with the semantic bytes of the batch in the one copy behind it
                    preds, ids = network.predict_instances_painted(
                        out, size=batch.size_hw, image_ids=list(batch.indices), label_id_to_category=label_id_to_category,
                        new_label_id_to_old_label_id=new_label_id_to_old_label_id, nms_type=nms_type, packed=packed, desc=desc, desc_host=batch.desc,
                        colours=colour_dev[:Q].unsqueeze(0).expand(B, Q, 3).contiguous() if colour_mode == "array" else None,
                        palette=colour_dev if colour_mode == "category" else None, alpha=int(alpha), outline=bool(instance_outline),
                        min_score=float(instance_min_score), id_format=id_format, ids_out=view.get("ids"), overlay_out=view.get("instance_overlay"))
                    for p, pid in zip(preds, ids):
                        i = p["image_id"]
                        p["image_id"] = image_ids[i] if image_ids is not None else 0
                        per_image[i].append(p)
                        per_image_ids[i].append(pid)
                    stage.commit()                                                         # labels + overlay + instance pictures: one D2H
        eng.check_finite()                                                                 # the forwards' status word: one read for the whole run
        fallbacks = stage.jpeg_host_fallbacks
    predictions = [p for ps in per_image for p in ps]
    if predictions_json is not None:
        d = os.path.dirname(os.fspath(predictions_json))
        if d:
            os.makedirs(d, exist_ok=True)
        with open(predictions_json, "w") as f:
            json.dump(predictions_json_form(predictions), f, default=_jsonable)
    result = {"label_paths": label_paths, "overlay_paths": overlay_paths, "instance_predictions": predictions, "n_images": len(p_images)}
    if paint:
        result.update(instance_map_paths=map_paths, instance_overlay_paths=iovl_paths, instance_ids=[i for ids in per_image_ids for i in ids])
    if as_jpeg:
        result["jpeg_host_fallbacks"] = fallbacks if p_images else 0
    return result


def predict_files_of(dataset):
    """(p_images, max_size, image_ids) for predict_from_files from one of the reference's dataset objects — the image half of
    evaluate.eval_files_of, so a split without ground truth (ImageNet-S test) is served:

      imagenet-s50 / -s300 / -s919 (datasets/imagenet_s.py:63-99): p_images as globbed, max_size = its max_size (1024), no image ids;
      coco2017, coco20k     (datasets/coco2017.py:121-149, coco20k.py:165-202): get_image_path(image_id) over image_ids, None, image_ids.

    TypeError for anything else."""
    name = getattr(dataset, "name", None)
    if isinstance(name, str) and name.startswith("imagenet-s"):
        return list(dataset.p_images), int(dataset.max_size), None
    if name in ("coco2017", "coco20k"):
        ids = list(dataset.image_ids)
        return [dataset.get_image_path(i) for i in ids], None, ids
    raise TypeError(f"predict_files_of: no path rules for the dataset {name!r} ({type(dataset).__name__})")
