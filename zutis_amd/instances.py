"""Instance post-processing of predict (zutis.py:211-299,423-469) behind the candidates: popcount IoU, the greedy per-category NMS loop,
run / RLE extraction of the kept masks and their picture, all on the device, and the host decode of the ONE buffer that comes back.
Two device paths give the same results — fused (runs, boxes, areas and strings from ONE launch, zh_mask_rle_fused_kept: masks up to
1024 columns whose bits + tables fit the LDS) and chain (run extraction, two launches, + string kernel) — and differ only in which
kernels run (_launch_*) and in how a slot's string, box and area are read out of the buffer (read_*).  The kernels: csrc/instance.hip
(statistics, masked mean, classification, IoU counts, NMS) and csrc/mask_rle.hip (run extraction, the string kernel, the fused kernel);
the string format both paths and the host encoder (csrc/rle_host.hip) write is csrc/rle_codec.h's."""
import collections
import functools
import math
from typing import Dict, Optional

import numpy as np
import torch

from . import ops, rle

# ints of the packed transition list that ride along with the small tables, per image (256 KB; a quarter of it per image in batches
# above 4): the 17 kept masks of the config-3 fixture (480x640, noisy: ~1750 transitions each) are 29.8 k
PACK_HEAD = 65536

# kept: (batch index, category, query index, score) in the reference's emission order; per kept entry its COCO RLE dict, xyxy box, area
# and slot (its position in the kernel's kept list = its id in a painted map minus 1); status: ops.STATUS_* as the NMS kernel read it
Instances = collections.namedtuple("Instances", "kept rles boxes areas status slots")


def to_host(t: torch.Tensor, cache: Optional[Dict[int, torch.Tensor]]) -> np.ndarray:
    """A 1-D uint8 device tensor on the host: one asynchronous copy into a cached PINNED buffer + one stream synchronisation (`.cpu()`
    goes through pageable memory: an allocation, a staged copy and its own synchronisation).  `cache` belongs to ONE engine instance
    (forks — one per stream / thread — have their own: a shared buffer would be overwritten by a sibling's predict; None: not cached).
    The array is a view of the cached buffer: valid until that engine's next call with the same size (callers take what they need out
    of it before they return); a buffer that falls out of the cache stays alive as long as a view of it does."""
    n = t.numel()
    if cache is None:
        cache = {}
    buf = cache.get(n)
    if buf is None:
        while len(cache) >= 8:
            cache.pop(next(iter(cache)))
        buf = cache[n] = torch.empty((n,), dtype=torch.uint8, pin_memory=True)
    buf.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return buf.numpy()


def reference_category_rank(all_categories_row) -> Dict[int, int]:
    """The kernel walks the categories in ascending id; the reference walks a set of the image's category ids (zutis.py:237-238), i.e.
    CPython's iteration order of a set of numpy int64 scalars — ascending only while every id is below the hash table's size.  This
    re-creates that very set (Q ids of one image, in query order) and ranks the ids by it."""
    return {int(c): i for i, c in enumerate(set(np.asarray(all_categories_row).astype(np.int64)))}


def iou_counts(masks_u8: torch.Tensor, bits: Optional[torch.Tensor] = None):
    """Exact popcount intersection / union counts, int32 [B,Q,Q] each, of contiguous masks u8 [B,Q,H,W] (zh_mask_iou_counts per image).
    bits (int64 [B,Q,(H*W + 63) // 64]): the step's workspace, which holds the masks bit-packed afterwards."""
    B, Q, H, W = masks_u8.shape
    inter = torch.empty((B, Q, Q), dtype=torch.int32, device=masks_u8.device)
    uni = torch.empty((B, Q, Q), dtype=torch.int32, device=masks_u8.device)
    for b in range(B):
        ops.mask_iou_counts(masks_u8[b], Q, H * W, inter[b], uni[b], workspace=None if bits is None else bits[b])
    return inter, uni


def mask_iou_matrix(masks_u8: torch.Tensor, return_areas: bool = False):
    """Pairwise IoU of one image's [Q,H,W] u8 masks: exact popcounts on device, float64 divide on the host
    (= utils/iou.py:30-32 on boolean masks).  The diagonal of the intersection counts is each mask's area."""
    inter, uni = iou_counts(masks_u8.contiguous()[None])
    ih = inter[0].cpu().numpy()
    iou = ih / (uni[0].cpu().numpy() + 1e-7)
    return (iou, np.diag(ih).copy()) if return_areas else iou


def nms(masks_u8, scores, category_ids, nms_type="hard", nms_threshold=0.3, sigma=0.5, threshold=0.001):
    """zutis.py:211-299 for a batch, entirely on the device: masks u8 [B,Q,H,W], scores f32 [B,Q], category_ids int64 [B,Q] -> list of
    (batch index, category, query index, score) in the reference's emission order.  Popcount IoU counts per image, then one launch of
    the greedy per-category loop (zh_mask_nms, one workgroup per image); only the kept triples and their count cross PCIe."""
    B, Q = scores.shape
    inter, uni = iou_counts(masks_u8.contiguous())
    idx, sc, cat, cnt = ops.mask_nms(inter, uni, scores.contiguous(), category_ids.contiguous(), nms_type, nms_threshold, sigma, threshold)
    # ONE device -> host copy for the five small results (every copy synchronises the stream), laid out as the kernel's own `pk`:
    # indices, categories and counts are small integers, exact in float64 next to the float64 scores
    f64 = torch.float64
    pk = torch.cat([idx.to(f64), sc.to(f64), cat.to(f64), category_ids.to(f64), cnt.to(f64).view(B, 1)], dim=1).cpu().numpy()
    return assemble(pk, [[({}, None, None)] * int(n) for n in pk[:, 4 * Q]], Q)[0]


def encode_masks(masks_u8: torch.Tensor, sel: np.ndarray, max_runs: int = 8192):
    """COCO RLE dicts, xyxy boxes and areas of the masks `sel` (flat indices into [n,H,W]) without moving the masks
    to the host: zh_mask_runs extracts the column-major run boundaries on the device; only those cross PCIe."""
    n, H, W = masks_u8.shape
    if len(sel) == 0:
        return [], [], []
    sel_dev = torch.from_numpy(np.ascontiguousarray(sel, dtype=np.int32)).to(masks_u8.device)
    pos, nr, ba = ops.mask_runs(masks_u8.contiguous(), sel_dev, max_runs)
    nb_h = torch.cat([nr, ba], dim=1).cpu().numpy()           # one copy (= one stream synchronisation) for both small tables
    nr_h, ba_h = nb_h[:, :2], nb_h[:, 2:]
    keep = int(min(max_runs, max(1, nr_h[:, 0].max())))
    pos_h = pos[:, :keep].cpu().numpy()
    rles = rle.rles_from_transitions(pos_h, nr_h, H, W)      # all strings in one C call
    for j, q in enumerate(sel):
        if rles[j] is None:                                  # pathological mask (> max_runs transitions): the host encoder
            rles[j] = rle.encode(masks_u8[int(q)].cpu().numpy())
    boxes = [[float(v) for v in row[:4]] for row in ba_h]
    areas = [int(row[4]) for row in ba_h]
    return rles, boxes, areas


# ---------------------------------------------------------------------------------------- the one result buffer
# ONE buffer = one copy (= the one synchronisation of the predict) for everything the host needs, as [(name, dtype, shape)] sections
# back to back; the kernels' contracts depend on the byte layout.  pk, as zh_mask_nms packs it: per image the kept (index | score |
# category) triples, every query's category, the count, the status word.  Per kept slot (row b * Q + j; rows past the count are not
# written): info / nr, ba as ops.mask_rle_fused_kept / ops.mask_runs_kept document them, slen the string's length or -1.  cursor: zeroed
# by the NMS kernel, places the fused strings.  The chain's packed transition list of `head` ints itself stays on the device.
F64, I32, U8 = np.dtype(np.float64), np.dtype(np.int32), np.dtype(np.uint8)
_TORCH = {F64: torch.float64, I32: torch.int32, U8: torch.uint8}


def fused_layout(B: int, Q: int, cap: int):
    return [("pk", F64, (B, 4 * Q + 2)), ("info", I32, (B * Q, 8)), ("cursor", I32, (2,)), ("chars", U8, (cap,))]


def chain_layout(B: int, Q: int, head: int):
    return [("pk", F64, (B, 4 * Q + 2)), ("nr", I32, (B * Q, 2)), ("ba", I32, (B * Q, 5)), ("slen", I32, (B * Q,)), ("chars", U8, (5 * head + 16 * B * Q,))]


def layout_bytes(sections) -> int:
    return sum(math.prod(shape) * dtype.itemsize for _, dtype, shape in sections)


def carve(buf, sections) -> dict:
    """The named views of a flat uint8 buffer, a device tensor or its host copy (ndarray): the same offsets for both.  (On the predict's
    critical path, each tensor view costs microseconds: none is made that changes nothing.)"""
    views, at, on_device = {}, 0, isinstance(buf, torch.Tensor)
    for name, dtype, shape in sections:
        end = at + math.prod(shape) * dtype.itemsize
        v = buf[at:end]
        if dtype is not U8:
            v = v.view(_TORCH[dtype] if on_device else dtype)
        views[name] = v if len(shape) == 1 else v.reshape(shape)
        at = end
    return views


def _launch_fused(m, bits, v, nms_loop, max_runs):
    """The NMS loop + ONE launch for runs, boxes, areas and strings into the device views v -> the loop's device outputs."""
    kept = idx, _, _, cnt = nms_loop(packed=v["pk"], zero_word=v["cursor"])
    ops.mask_rle_fused_kept(m, idx, cnt, max_runs, v["chars"], v["cursor"], v["info"], bits=bits)
    return kept


def _launch_chain(m, v, nms_loop, max_runs, head):
    """The NMS loop, run extraction (two launches) into a packed list of `head` ints and the string kernel over that list."""
    B, Q, H, W = m.shape
    pos_head = torch.empty((head,), dtype=torch.int32, device=m.device)
    kept = idx, _, _, cnt = nms_loop(packed=v["pk"])
    ops.mask_runs_kept(m, idx, cnt, max_runs, pos_head, v["nr"], v["ba"], packed=True)
    ops.mask_rle_kept(pos_head, v["nr"], cnt, B, Q, max_runs, H * W, v["chars"], v["slen"])
    return kept


# ---------------------------------------------------------------------------------------- host decode (numpy / Python only)
def read_fused(v: dict, counts, size):
    """Per image the list, by kept slot j, of (rle dict or None, box, area) from the host views of a fused_layout buffer.  None: over
    max_runs transitions, or the strings outgrew the buffer."""
    Q, chars = v["info"].shape[0] // len(counts), v["chars"]
    return [[({"size": size, "counts": chars[c0:c0 + ln].tobytes()} if ln >= 0 else None, [float(x0), float(y0), float(x1), float(y1)], ar)
             for c0, ln, x0, y0, x1, y1, ar, _ in v["info"][b * Q:b * Q + n].tolist()] for b, n in enumerate(counts)]


def read_chain(v: dict, counts, lens, size, max_runs: int, second_list: Optional[np.ndarray] = None):
    """read_fused for a chain_layout buffer.  lens: per image the length of every kept mask's entry in the packed list, min(transitions,
    max_runs); mask j's string lies at 5 * (start of its entry) + 16 * (kept masks before it), both counted across the batch.  With
    second_list (the whole packed list, copied when it outgrew the head) the strings are built here instead."""
    Q, chars, per = v["nr"].shape[0] // len(counts), v["chars"], []
    at = rank_all = 0
    for b, n in enumerate(counts):
        if second_list is not None and n:
            r = rle.rles_from_transitions(second_list[at:], v["nr"][b * Q:b * Q + n], size[0], size[1], packed_max_runs=max_runs)
            at += sum(lens[b])
        else:
            r, sl = [], v["slen"][b * Q:b * Q + n].tolist()
            for j in range(n):
                c0 = 5 * at + 16 * rank_all
                r.append({"size": size, "counts": chars[c0:c0 + sl[j]].tobytes()} if sl[j] >= 0 else None)
                at += lens[b][j]
                rank_all += 1
        per.append([(r[j], [float(x) for x in row[:4]], row[4]) for j, row in enumerate(v["ba"][b * Q:b * Q + n].tolist())])
    return per


def assemble(pk: np.ndarray, per, Q: int):
    """pk + the readers' per-slot triples -> kept, rles, boxes, areas, slots in the reference's emission order — the per-category groups
    ordered by reference_category_rank, stable inside a category (the kernel's = the reference's selection order) — and redo: (position
    in these lists, flat mask index) of the strings that are None."""
    kept, rles, boxes, areas, slots, redo = [], [], [], [], [], []
    for b, triples in enumerate(per):
        if not triples:
            continue
        row = pk[b].tolist()
        rank = reference_category_rank(pk[b, 3 * Q:4 * Q])
        for j in sorted(range(len(triples)), key=lambda j: rank[int(row[2 * Q + j])]):
            q, (r, box, area) = int(row[j]), triples[j]
            if r is None:
                redo.append((len(kept), b * Q + q))
            kept.append((b, int(row[2 * Q + j]), q, row[Q + j]))
            slots.append(j); rles.append(r); boxes.append(box); areas.append(area)
    return kept, rles, boxes, areas, slots, redo


def nms_encode(masks_u8, scores, category_ids, nms_type="hard", nms_threshold=0.3, sigma=0.5, threshold=0.001, range_flag=None,
               max_runs: int = 8192, pack_head: Optional[int] = None, fused: Optional[bool] = None, paint: Optional[dict] = None,
               pinned: Optional[dict] = None, colour_cache: Optional[dict] = None) -> Instances:
    """nms + encode_masks chained on the device: popcount IoU counts, the greedy per-category loop, then runs, boxes, areas and COCO RLE
    strings of the kept masks straight from the loop's device outputs — the NMS result does not visit the host in between — and ONE
    device -> host copy (to_host with the cache `pinned`) of the path's result buffer.  The host encodes only when the chain path's
    packed list outgrows its PACK_HEAD (pack_head) ints per image (a second copy) or a string was not written.  range_flag: the status
    word (int32 [1]) the NMS kernel reads.  fused: None = where ops.mask_rle_fused_supported.  paint (the keyword arguments of
    paint_kept): the picture of the kept masks is launched behind the NMS loop, from its device outputs and the bit-packed masks of the
    IoU step (zh_instance_paint: no copy, no synchronisation of its own)."""
    B, Q, H, W = masks_u8.shape
    m = masks_u8.contiguous()
    bits = torch.empty((B, Q, (H * W + 63) // 64), dtype=torch.int64, device=m.device)     # the IoU step's bit-packed masks, read again below
    inter, uni = iou_counts(m, bits)
    nms_loop = functools.partial(ops.mask_nms, inter, uni, scores.contiguous(), category_ids.contiguous(), nms_type, nms_threshold, sigma,
                                 threshold, range_flag=range_flag)
    per_image = (PACK_HEAD if B <= 4 else PACK_HEAD // 4) if pack_head is None else pack_head
    if fused is None:
        fused = ops.mask_rle_fused_supported(H, W, max_runs)
    head = int(min(B * Q * max_runs, B * per_image))
    # fused: the bytes of strings that ride along (a string is ~2.2 B per transition)
    sections = fused_layout(B, Q, int(max(64, 4 * B * per_image))) if fused else chain_layout(B, Q, head)
    buf = torch.empty((layout_bytes(sections),), dtype=torch.uint8, device=m.device)
    dv = carve(buf, sections)
    idx, sc, kcat, cnt = _launch_fused(m, bits, dv, nms_loop, max_runs) if fused else _launch_chain(m, dv, nms_loop, max_runs, head)
    if paint is not None:
        paint_kept(m, idx, sc, kcat, cnt, bits=bits, colour_cache=colour_cache, **paint)
    v = carve(to_host(buf, pinned), sections)
    pk = v["pk"]
    counts = pk[:, 4 * Q].astype(np.int64).tolist()
    status = int(pk[:, 4 * Q + 1].max()) if range_flag is not None else 0
    size = [int(H), int(W)]
    if fused:
        per = read_fused(v, counts, size)
    else:
        lens = [np.minimum(v["nr"][b * Q:b * Q + n, 0], max_runs).tolist() for b, n in enumerate(counts)]
        second_list = None
        if sum(map(sum, lens)) > head:                         # the lists outgrew the head: the whole packed list in a second copy
            big = torch.empty((sum(map(sum, lens)),), dtype=torch.int32, device=m.device)
            ops.mask_runs_kept(m, idx, cnt, max_runs, big, dv["nr"], dv["ba"], packed=True)
            second_list = big.cpu().numpy()
        per = read_chain(v, counts, lens, size, max_runs, second_list)
    kept, rles, boxes, areas, slots, redo = assemble(pk, per, Q)
    if redo:
        # one batched launch for the strings the device did not write, on either path (encode_masks itself falls back to rle.encode for
        # a mask over its max_runs): identical strings for one extra small launch, in the pathological case only
        r2, _, _ = encode_masks(m.view(B * Q, H, W), np.array([f for _, f in redo], dtype=np.int32))
        for (at, _), r in zip(redo, r2):
            rles[at] = r
    return Instances(kept, rles, boxes, areas, status, slots)


def paint_kept(masks_u8, index, score, category, count, *, colour_cache: Optional[dict] = None, colours=None, palette=None, overlay_out=None,
               **paint):
    """The picture of a kept list (ops.instance_paint, which takes **paint: bits, ids_out, id_format, packed, desc, desc_host, alpha,
    outline, min_score) on the current stream: index / score / category / count as zh_mask_nms writes them ([B,Q] int32 / f64 / int64,
    [B] int32), on the device.  The colour of slot j of image b: colours[b, j] (u8 [B,Q,3]), or palette[category[b, j]] (palette u8
    [n,3] by the network's category index; gathered on the device), or — both None — entry j of instance_paint.instance_colours (kept
    on the device in colour_cache, one table per engine)."""
    B, Q, H, W = masks_u8.shape
    if overlay_out is not None and colours is None:
        if palette is not None:
            colours = palette[category.clamp(0, palette.shape[0] - 1)].contiguous()      # entries past count are not read by the kernel
        else:
            from .instance_paint import instance_colours
            key, cache = (Q, str(masks_u8.device)), {} if colour_cache is None else colour_cache
            if key not in cache:
                cache.clear()
                cache[key] = torch.from_numpy(instance_colours(Q)).to(masks_u8.device)
            colours = cache[key].unsqueeze(0).expand(B, Q, 3).contiguous()
    return ops.instance_paint(index, score, count, H, W, masks=masks_u8, colours=colours, overlay_out=overlay_out, **paint)


def slot_table(kept, B: int, Q: int, device):
    """A host-built kept list [(batch index, category, query index, score)] as the slot table paint_kept reads — image b's j-th entry
    is slot j — uploaded: ((index int32 [B,Q], score f64 [B,Q], category int64 [B,Q], count int32 [B]), per entry its slot)."""
    table = np.zeros((B, Q, 3), np.float64)
    count = np.zeros((B,), np.int32)
    slots = []
    for bi, c, q, s in kept:
        table[bi, count[bi]] = (q, s, c)
        slots.append(int(count[bi]))
        count[bi] += 1
    t = torch.from_numpy(table).to(device)
    return (t[..., 0].to(torch.int32).contiguous(), t[..., 1].contiguous(), t[..., 2].to(torch.int64).contiguous(),
            torch.from_numpy(count).to(device)), slots
