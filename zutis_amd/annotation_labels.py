"""Semantic ground truth from COCO annotations: the label maps the reference's COCO datasets open at
{dir_dataset}/annotations/semantic_segmentation_masks/{stem}.png (datasets/coco2017.py:134, datasets/coco20k.py:178) and that neither the
reference nor a COCO download ships, painted from `instances_*.json`.

paint_plan() fixes, per image, which annotations are painted with which label byte and in which order; labels_np() is the definition
(dense masks of rle.from_polygons / the RLE's counts, painted on the host); LabelPainter paints on the device: the file's segmentations
become run lengths once (polygons through zh_polygon_runs with the counts left resident, RLE and crowd segmentations through
rle.counts_np and one upload), zh_rle_prefix turns them into run ends, and zh_runs_label_maps (csrc/label_paint.hip) paints the maps of
a batch of images in one launch, a gather per pixel.  write_semantic_masks() writes the PNG directory; evaluate.evaluate_from_annotations
scores against the painted maps without one.

The reference does not ship the script that made its PNGs: the order, the overlap rule and the treatment of crowds are this module's
choices (its defaults are what a loop over getAnnIds / annToMask that assigns mask pixels in file order gives) and cannot be pinned
against it.  The label numbering can: the default is old_label_id_to_new_label_id of datasets/coco2017.py:152-244.

No torch at import: paint_plan and labels_np are host code.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import picture_out, rle
from .coco_eval import _load

ORDERS = ("file", "area")
OVERLAPS = ("last", "ignore")
CROWDS = ("label", "ignore", "skip")
PAINT_BYTES = 64 << 20        # output bytes of one ragged launch of write_semantic_masks


class Plan:
    """What paint_plan() leaves: ground_truth (the annotation dict), images = [{"id", "h", "w", "file_name"}], lists = per image
    [(annotation index, label byte)] in paint order, overlap, ignore_value."""
    __slots__ = ("ground_truth", "images", "lists", "overlap", "ignore_value")

    def __init__(self, ground_truth, images, lists, overlap, ignore_value):
        self.ground_truth, self.images, self.lists, self.overlap, self.ignore_value = ground_truth, images, lists, overlap, ignore_value

    def __len__(self):
        return len(self.images)


def default_label_of(category_ids) -> Dict[int, int]:
    """{category id: rank among the sorted ids + 1}: for COCO's 80 ids old_label_id_to_new_label_id (datasets/coco2017.py:152-244);
    background is 0."""
    ids = sorted(set(category_ids))
    if len(ids) > 254:
        raise ValueError(f"paint_plan: {len(ids)} categories do not fit the labels 1 .. 254")
    return {c: k + 1 for k, c in enumerate(ids)}


def _segmentation_counts(a, image) -> np.ndarray:
    seg = a["segmentation"]
    if isinstance(seg, dict):
        return rle.counts_np(seg["counts"])
    return rle.counts_np(rle.from_polygons(seg, int(image["height"]), int(image["width"]))["counts"])


def paint_plan(ground_truth, image_ids: Optional[Sequence] = None, *, label_of: Optional[Dict[int, int]] = None, order: str = "file",
               overlap: str = "last", crowd: str = "label", ignore_value: int = 255) -> Plan:
    """Which annotation paints which label, image by image.

    ground_truth: a COCO annotation dict or the path of its JSON.  Images: those of image_ids, in that order, or every entry of `images`
    in file order; an image without annotations has an empty list (an all-zero map).  label_of: {category id: label in 1 .. 254}
    (default_label_of of the file's categories when None); a painted annotation whose category it lacks raises ValueError.
    order "file": the order of `annotations` in the file (what getAnnIds(imgIds=...) yields); "area": descending by the annotation's
    `area` field (its pixel count when absent), stable, so that small objects stay visible.
    crowd "label": a crowd is painted like any other annotation (annToMask does not distinguish); "ignore": crowds move to the end of the
    list and paint ignore_value; "skip": they are left out.
    overlap "last": a pixel takes the label of the last list entry that covers it; "ignore": the label of the only entry that covers it,
    ignore_value when two or more do.  An uncovered pixel is 0."""
    gt = _load(ground_truth)
    if order not in ORDERS or overlap not in OVERLAPS or crowd not in CROWDS:
        raise ValueError(f"paint_plan: order one of {ORDERS}, overlap one of {OVERLAPS}, crowd one of {CROWDS}; got {order!r}, {overlap!r}, {crowd!r}")
    if int(ignore_value) != ignore_value or not 0 <= int(ignore_value) <= 255:
        raise ValueError(f"paint_plan: ignore_value {ignore_value!r} is not a byte")
    if label_of is None:
        label_of = default_label_of(c["id"] for c in gt["categories"])
    else:
        label_of = dict(label_of)
        bad = {c: v for c, v in label_of.items() if int(v) != v or not 1 <= int(v) <= 254}
        if bad:
            raise ValueError(f"paint_plan: labels outside 1 .. 254: {bad}")
    by_id = {im["id"]: im for im in gt["images"]}
    if image_ids is None:
        chosen = list(gt["images"])
    else:
        missing = [i for i in image_ids if i not in by_id]
        if missing:
            raise ValueError(f"paint_plan: image ids the annotations do not list: {missing[:8]}")
        chosen = [by_id[i] for i in image_ids]
    anns_of: Dict = {}
    for j, a in enumerate(gt["annotations"]):
        anns_of.setdefault(a["image_id"], []).append(j)
    images, lists = [], []
    for im in chosen:
        h, w = int(im["height"]), int(im["width"])
        if h < 0 or w < 0 or h * w > 0x7fffffff:
            raise ValueError(f"paint_plan: image {im['id']!r} of {h} x {w} pixels")
        idx = list(anns_of.get(im["id"], ()))
        if crowd == "skip":
            idx = [j for j in idx if not gt["annotations"][j].get("iscrowd", 0)]
        if order == "area":
            area = [float(gt["annotations"][j]["area"]) if "area" in gt["annotations"][j]
                    else float(_segmentation_counts(gt["annotations"][j], im)[1::2].sum()) for j in idx]
            idx = [idx[k] for k in np.argsort(-np.asarray(area, dtype=np.float64), kind="mergesort")]
        entries, crowds = [], []
        for j in idx:
            a = gt["annotations"][j]
            if crowd == "ignore" and a.get("iscrowd", 0):
                crowds.append((j, int(ignore_value)))
                continue
            if a["category_id"] not in label_of:
                raise ValueError(f"paint_plan: annotation {a.get('id', j)!r} has the category {a['category_id']!r}, which label_of lacks")
            entries.append((j, int(label_of[a["category_id"]])))
        images.append({"id": im["id"], "h": h, "w": w, "file_name": im.get("file_name", f"{im['id']}.jpg")})
        lists.append(entries + crowds)
    return Plan(gt, images, lists, overlap, int(ignore_value))


def _dense(plan: Plan, j: int, h: int, w: int) -> np.ndarray:
    a = plan.ground_truth["annotations"][j]
    seg = a["segmentation"]
    if isinstance(seg, dict):
        if [int(v) for v in seg["size"]] != [h, w]:
            raise ValueError(f"annotation {a.get('id', j)!r}: an RLE of size {list(seg['size'])} on an image of {[h, w]}")
        cnts = rle.counts_np(seg["counts"])
        if (cnts < 0).any() or int(cnts.sum()) != h * w:
            raise ValueError(f"annotation {a.get('id', j)!r}: RLE counts that do not sum to height * width")
        return rle._dense(cnts, h, w).astype(bool)
    return rle.decode_np(rle.from_polygons(seg, h, w)).astype(bool)


def labels_np(plan: Plan) -> List[np.ndarray]:
    """The definition: [uint8 [h, w]] per image of the plan, each annotation's dense mask painted by the plan's rules.  Host only, not
    optimised."""
    out = []
    for im, entries in zip(plan.images, plan.lists):
        h, w = im["h"], im["w"]
        m = np.zeros((h, w), np.uint8)
        cover = np.zeros((h, w), np.int64)
        for j, label in entries:
            d = _dense(plan, j, h, w)
            m[d] = label                                    # the last entry that covers a pixel stays
            cover += d
        if plan.overlap == "ignore":
            m[cover >= 2] = plan.ignore_value
        out.append(m)
    return out


def stem_of(file_name: str) -> str:
    """{file name without .jpg}, as coco2017.py:134 / evaluate.eval_files_of form it."""
    return str(file_name).split("/")[-1].split(".jpg")[0]


class LabelPainter:
    """The plan's label maps on the device.  Construction converts the segmentations of every annotation the plan paints, once:
    polygons through polygons.runs_resident (zh_polygon_runs; the counts stay on the device, compacted to the runs written), RLE and crowd
    segmentations through rle.counts_np on the host, uploaded together with the polygons the kernel left to the host
    (stats["host_fallback"] of them, filled from rle.from_polygons); then ONE zh_rle_prefix over all of them.  Resident afterwards:
    counts / run_end int32 [R], run_off int32 [n + 1], status, and the paint lists of all images.  A mask whose counts do not sum to its
    image's h * w raises ValueError naming the annotation (check()).
    paint() / paint_ragged() are one launch of zh_runs_label_maps each and copy nothing back."""

    def __init__(self, plan: Plan, device=None, events=None):
        import torch
        from . import _lib, polygons
        if device is None:
            if not torch.cuda.is_available():
                raise _lib.ZutisHipError("LabelPainter paints on the GPU (labels_np is the host form)")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.ZutisHipError("LabelPainter paints on the GPU (labels_np is the host form)")
        self.plan, self.events = plan, events
        anns = plan.ground_truth["annotations"]
        size_of = {}                                                     # annotation index -> (h, w) of the image that paints it
        for im, entries in zip(plan.images, plan.lists):
            for j, _ in entries:
                size_of[j] = (im["h"], im["w"])
        used = sorted(size_of)
        poly = [j for j in used if not isinstance(anns[j]["segmentation"], dict)]
        chunks, fallback, pstats = polygons.runs_resident([(anns[j]["segmentation"], *size_of[j]) for j in poly], self.device, events)
        # mask order: per chunk the polygons the kernel converted, then everything that comes from the host
        self.mask_of: Dict[int, int] = {}
        self.names: List[int] = []                                       # mask -> annotation index
        lens: List[int] = []
        at = 0
        for counts, n_runs in chunks:
            for a, n in enumerate(n_runs.tolist()):
                if n >= 0:
                    self.mask_of[poly[at + a]] = len(self.names)
                    self.names.append(poly[at + a])
                    lens.append(n)
            at += len(n_runs)
        host_counts = []
        poly_pos = {j: k for k, j in enumerate(poly)}
        for j in used:
            if j in self.mask_of:
                continue
            seg = anns[j]["segmentation"]
            if isinstance(seg, dict):
                if [int(v) for v in seg["size"]] != list(size_of[j]):
                    raise ValueError(f"annotation {anns[j].get('id', j)!r}: an RLE of size {list(seg['size'])} on an image of {list(size_of[j])}")
                c = rle.counts_np(seg["counts"])
            else:
                c = fallback[poly_pos[j]]
            self.mask_of[j] = len(self.names)
            self.names.append(j)
            lens.append(len(c))
            host_counts.append(np.clip(c, -1, 0x7fffffff).astype(np.int32))
        n = len(self.names)
        run_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        if run_off[-1] > 0x7fffffff:
            raise ValueError("LabelPainter: more than 2^31 - 1 runs in one annotation file (paint it in parts: image_ids)")
        hw = np.asarray([size_of[j][0] * size_of[j][1] for j in self.names], dtype=np.int32)
        list_off = np.concatenate(([0], np.cumsum([len(e) for e in plan.lists]))).astype(np.int32)
        list_mask = np.asarray([self.mask_of[j] for e in plan.lists for j, _ in e], dtype=np.int32)
        list_label = np.asarray([lab for e in plan.lists for _, lab in e], dtype=np.uint8)
        self.list_off_host, self.list_mask_host, self.list_label_host = list_off, list_mask, list_label
        self.stats = {"images": len(plan), "annotations": len(used), "polygon_annotations": len(poly), "polygons": pstats["polygons"],
                      "host_fallback": pstats["host_fallback"], "rle_annotations": len(used) - len(poly), "runs": int(run_off[-1])}
        with torch.cuda.device(self.device):
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            parts = [c for c, _ in chunks] + ([up(np.concatenate(host_counts))] if host_counts else [])
            self.counts = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int32, device=self.device)
            if not self.counts.numel():
                self.counts = torch.zeros(1, dtype=torch.int32, device=self.device)     # no run at all: one slot no mask owns, never a null address
            self.run_off, self.hw = up(run_off.astype(np.int32)), up(hw)
            self.run_end = torch.empty_like(self.counts)
            self.status = torch.zeros(max(1, (n + 31) // 32), dtype=torch.int32, device=self.device)
        self.prefix()

    def prefix(self, check: bool = True):
        """zh_rle_prefix over the resident counts (run_end and status are rewritten) and, with check, check()."""
        import torch
        from . import ops
        with torch.cuda.device(self.device):
            self.status.zero_()
            run_fg, area = torch.empty_like(self.counts), torch.empty(len(self.names), dtype=torch.int32, device=self.device)
            e = self._event()
            ops.rle_prefix(self.counts, self.run_off, self.hw, self.run_end, run_fg, area, self.status)
            self._event(e, "zh_rle_prefix")
        if check:
            self.check()

    def check(self):
        """ValueError naming the annotations whose counts do not sum to their image's height * width (one small copy back)."""
        n = len(self.names)
        status = self.status.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero((status[np.arange(n) >> 5] >> (np.arange(n) & 31).astype(np.uint32)) & 1)
        if bad.size:
            anns = self.plan.ground_truth["annotations"]
            names = [f"annotation {anns[self.names[m]].get('id', self.names[m])!r}" for m in bad[:8]]
            raise ValueError(f"RLE counts that do not sum to height * width: {', '.join(names)}" + (" ..." if bad.size > 8 else ""))

    def _event(self, e0=None, name=None):
        import torch
        if self.events is None:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        if e0 is not None:
            self.events.append((name, e0, e))
        return e

    def _lists(self, image_indices):
        """The batch's own (list_off, list_mask, list_label, hw, out_off, max_tiles) as host arrays."""
        from . import ops
        idx = [int(i) for i in image_indices]
        for i in idx:
            if not 0 <= i < len(self.plan):
                raise IndexError(f"LabelPainter: image index {i} outside the plan's {len(self.plan)} images")
        lo, hi = self.list_off_host[idx], self.list_off_host[[i + 1 for i in idx]]
        sel = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)] + [np.zeros(0, np.int64)]).astype(np.int64)
        hw = np.asarray([(self.plan.images[i]["h"], self.plan.images[i]["w"]) for i in idx], dtype=np.int32).reshape(-1, 2)
        out_off = np.concatenate(([0], np.cumsum(hw[:, 0].astype(np.int64) * hw[:, 1]))).astype(np.int64)
        return (np.concatenate(([0], np.cumsum(hi - lo))).astype(np.int32), self.list_mask_host[sel], self.list_label_host[sel], hw, out_off,
                max([ops.label_tiles(h, w) for h, w in hw.tolist()] + [0]))

    def _launch(self, image_indices, out):
        """ONE host-to-device copy of the batch's lists and ONE launch into `out` (u8 on the device, out_off[-1] bytes)."""
        import torch
        from . import ops
        from .coco_eval import _sections
        list_off, list_mask, list_label, hw, out_off, max_tiles = self._lists(image_indices)
        host, lay = _sections([("out_off", out_off), ("list_off", list_off), ("list_mask", list_mask), ("hw", hw), ("list_label", list_label)])
        with torch.cuda.device(self.device):
            dbuf = torch.from_numpy(host).to(self.device)                                   # the batch's lists: a few bytes an entry
            view = lambda n, dt: dbuf[lay[n][0]:lay[n][0] + max(lay[n][1].nbytes, 16)].view(dt)[:lay[n][1].size]
            e = self._event()
            ops.runs_label_maps(self.run_end, self.run_off, self.status, view("list_off", torch.int32), view("list_mask", torch.int32),
                                view("list_label", torch.uint8), view("hw", torch.int32), view("out_off", torch.int64), out, max_tiles,
                                overlap=self.plan.overlap, ignore_value=self.plan.ignore_value)
            self._event(e, "zh_runs_label_maps")
        return out_off

    def paint(self, image_indices: Sequence[int], out=None):
        """u8 [B, H, W] on the device: the maps of the plan's images `image_indices`, which must be of one size (ValueError otherwise).
        out: the caller's contiguous u8 buffer of B * H * W bytes."""
        import torch
        from . import ops
        idx = list(image_indices)
        sizes = {(self.plan.images[int(i)]["h"], self.plan.images[int(i)]["w"]) for i in idx}
        if len(sizes) > 1:
            raise ValueError(f"LabelPainter.paint: images of {len(sizes)} sizes in one batch ({sorted(sizes)[:4]}): paint_ragged takes those")
        H, W = sizes.pop() if sizes else (0, 0)
        shape = (len(idx), H, W)
        with torch.cuda.device(self.device):
            out = torch.empty(shape, dtype=torch.uint8, device=self.device) if out is None else ops._caller_buffer(out, torch.uint8, shape, "LabelPainter.paint out")
        if len(idx) and H * W:
            self._launch(idx, out)
        return out

    def paint_ragged(self, image_indices: Sequence[int], out=None):
        """(u8 [bytes] on the device, int64 offsets [B + 1] on the host): image k's row-major [h, w] map at offsets[k]."""
        import torch
        idx = list(image_indices)
        total = sum(self.plan.images[int(i)]["h"] * self.plan.images[int(i)]["w"] for i in idx)
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty(total, dtype=torch.uint8, device=self.device)
            elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != total:
                raise ValueError(f"LabelPainter.paint_ragged: out must be {total} contiguous bytes")
        if idx:
            out_off = self._launch(idx, out)
        else:
            out_off = np.zeros(1, np.int64)
        return out, out_off


def write_semantic_masks(ground_truth, out_dir: str, *, image_ids: Optional[Sequence] = None, route: str = "device", n_workers: int = 16,
                         compress_level: int = 1, device=None, paint_bytes: int = PAINT_BYTES, label_of: Optional[Dict[int, int]] = None,
                         order: str = "file", overlap: str = "last", crowd: str = "label", ignore_value: int = 255, events=None,
                         png_encoder: str = "host") -> dict:
    """Write {out_dir}/{file_name without .jpg}.png, mode L, for the plan's images: the files coco2017.py:134 / coco20k.py:178 open and
    evaluate_from_files(gt_format="u8") reads.

    route "device": LabelPainter, ragged launches of at most paint_bytes output bytes (a larger image goes alone); per launch ONE copy
    back into a pinned buffer of a preprocess.WriterRing, whose n_workers (at most 16) threads encode launch k's PNGs while launch k + 1
    is painted.  route "host": labels_np and Image.save in this thread; needs no GPU.  label_of / order / overlap / crowd / ignore_value:
    paint_plan's.  png_encoder "host": the writer threads encode with Pillow (compress_level).  "device" (route "device" only: ValueError
    with route "host"): zh_png_deflate behind each ragged launch turns the maps into the zlib streams of their PNGs (png_device.py); the
    copy back carries the streams at their worst-case strides and their lengths, a writer frames a stream and writes the file;
    compress_level is unused.  The files decode to the same maps.  Returns {"paths": one per image, in the plan's order, "stats"}."""
    from . import png_device
    if route not in ("device", "host"):
        raise ValueError(f"write_semantic_masks: route {route!r} is not 'device' or 'host'")
    on_device = png_device.check_encoder("write_semantic_masks", png_encoder) == "device"
    if on_device and route == "host":
        raise ValueError("write_semantic_masks: png_encoder=\"device\" encodes behind the device's paint: it needs route=\"device\"")
    plan = paint_plan(ground_truth, image_ids, label_of=label_of, order=order, overlap=overlap, crowd=crowd, ignore_value=ignore_value)
    os.makedirs(out_dir, exist_ok=True)
    paths = [os.path.join(out_dir, stem_of(im["file_name"]) + ".png") for im in plan.images]
    if len(set(paths)) != len(paths):
        raise ValueError("write_semantic_masks: two images of the plan share a file name")
    if route == "host":
        for p, m in zip(paths, labels_np(plan)):
            picture_out.write_png(p, m, "L", None, int(compress_level))
        return {"paths": paths, "stats": {"images": len(plan), "annotations": sum(len(e) for e in plan.lists), "launches": 0}}
    import torch
    from . import preprocess
    painter = LabelPainter(plan, device, events)
    dev = painter.device
    groups, cur, used = [], [], 0
    for i, im in enumerate(plan.images):
        n = im["h"] * im["w"]
        if cur and (used + n > paint_bytes or len(cur) == 65535):
            groups.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += n
    if cur:
        groups.append(cur)
    n_write = max(1, min(int(n_workers), preprocess.MAX_THREADS))
    with torch.cuda.device(dev):
        try:
            with picture_out.PictureStage(png_encoder, True, n_write, dev, compress_level=compress_level, events=events,
                                          error="write_semantic_masks: the device encoder left no stream for {path} ({h} x {w})") as stage:
                for k, idx in enumerate(groups):
                    sizes = [(plan.images[i]["h"], plan.images[i]["w"]) for i in idx]
                    if on_device and min(min(s) for s in sizes) < 1:
                        raise ValueError("write_semantic_masks: an image without pixels has no PNG")
                    painter.paint_ragged(idx, out=stage.take(k, picture_out.Layout(sizes, [(1, "L", None)]), [paths[i] for i in idx]))
                    stage.commit()                                                 # the one copy back of the launch
        finally:
            torch.cuda.synchronize(dev)
    return {"paths": paths, "stats": dict(painter.stats, launches=len(groups))}
