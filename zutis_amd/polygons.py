"""Polygon annotations to COCO run lengths for a whole annotation file at once: rle.from_polygons (pycocotools' rleFrPoly + merge,
restated in zutis_amd/rle.py) in its parallel form.  pack() flattens the annotations into arrays, runs_np() is the NumPy statement of
the algorithm the kernel runs (csrc/polygon.hip, zh_polygon_runs), runs_device() runs it on the GPU.  The yardstick of all three is
rle.from_polygons, count for count.

The parallel form.  _polygon_boundary's walk has no serial dependence: point j of a polygon's walk is a closed-form function of its
edge (found in the prefix of the edges' step counts) and of its place on it, so the crossing between the points j - 1 and j is
computed from those two alone, seams between edges included.  The serial tail of _polygon_counts (sort, differences, merging what a
zero-length run separates) keeps a position exactly when it occurs an odd number of times, and closes the last run at h * w.  Put
per pixel: position x lies inside the polygon exactly when an odd number of its crossings lie at or before x.  So after a sort per
polygon the crossing of rank r is a start (+1) when r is even and an end (-1) when r is odd; equal positions cancel in pairs when
equal positions are taken together; crossings at h * w or beyond never change a pixel and are dropped.  The union of an annotation's
polygons (from_polygons ORs dense masks) is then the coverage scan over its merged events: a run boundary wherever the coverage
moves between 0 and positive across one position, and the counts are the differences of the boundaries from 0 to h * w — the run of
zeros first (of length 0 when pixel 0 is covered), no other empty run: rle._counts' canonical form.

No torch at import: pack and runs_np are host code.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, rle

SCALE = 5                     # rleFrPoly's upsampling
LDS_CROSSINGS = _lib.constants()["ZH_POLYGON_LDS_CROSSINGS"]          # crossings of one annotation the kernel sorts in LDS
MAX_COORD = 1 << 24           # scaled coordinates beyond this, and walks of more than MAX_STEPS points, take the host path
MAX_STEPS = 1 << 22
CHUNK_ANNOTATIONS = 16384     # annotations per launch of runs_device: at most 16384 * 4097 runs (256 MB) of output capacity


def _polys(polys):
    if len(polys) and not isinstance(polys[0], (list, tuple, np.ndarray)):
        return [polys]
    return polys


def pack(annotations: Sequence[Tuple]) -> Dict[str, np.ndarray]:
    """annotations = [(polys, h, w)], polys = [[x0, y0, x1, y1, ...], ...] or one flat list -> flat arrays over all of them:

    xs, ys      int32 [V]      the vertices scaled as rleFrPoly scales them, int(5 * v + .5) with C truncation
    steps       int32 [V]      points on the edge that starts at the vertex (it ends at the polygon's next one): max(|dx|, |dy|) + 1
    step_pref   int32 [V + P]  per polygon the exclusive prefix of its steps, k + 1 entries at vert_off[p] + p
    vert_off    int32 [P + 1]  polygon p's vertices; poly_off int32 [A + 1]: annotation a's polygons
    hw          int32 [A, 2]   (h, w)
    bound       int64 [P]      at least the polygon's kept crossings: sum over its edges of |dx| // 5 + 2
    out_off     int32 [A + 1]  annotation a's slice of the output: its bounds' sum + 1 runs (1 for an annotation left to the host)
    host        bool [A]       left to rle.from_polygons: over_cap (its bounds sum to more than LDS_CROSSINGS) or unsafe
    unsafe      bool [A]       outside what the arrays hold: a polygon of no vertex, a coordinate that is not finite or scales beyond
                               MAX_COORD, a walk of more than MAX_STEPS points, an image without pixels
    """
    A = len(annotations)
    flat, n_vert, n_poly, hw = [], [], np.zeros(A, np.int64), np.zeros((A, 2), np.int64)
    unsafe = np.zeros(A, bool)
    for a, (polys, h, w) in enumerate(annotations):
        h, w = int(h), int(w)
        if h * w > 0x7fffffff:
            raise ValueError("polygons.pack: an image of more than 2^31 - 1 pixels")
        hw[a] = h, w
        polys = _polys(polys)
        n_poly[a] = len(polys)
        if h < 1 or w < 1:
            unsafe[a] = True
        for p in polys:
            v = np.asarray(p, dtype=np.float64).reshape(-1)
            k = v.size // 2
            if k == 0:
                unsafe[a] = True
            n_vert.append(k)
            flat.append(v[:2 * k])
    P = len(n_vert)
    n_vert = np.asarray(n_vert, dtype=np.int64)
    vert_off = np.concatenate(([0], np.cumsum(n_vert)))
    poly_off = np.concatenate(([0], np.cumsum(n_poly)))
    V = int(vert_off[-1])
    ann_of_poly = np.repeat(np.arange(A), n_poly)
    poly_of_vert = np.repeat(np.arange(P), n_vert)
    xy = np.concatenate(flat + [np.zeros(0)]).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        sc = np.trunc(SCALE * xy + .5)                                  # int(scale * v + .5): C truncates toward zero
    wild = ~(np.abs(sc) <= MAX_COORD).all(axis=1)                       # NaN and infinities included
    np.logical_or.at(unsafe, ann_of_poly[poly_of_vert[wild]], True)
    sc = np.where(wild[:, None], 0.0, sc).astype(np.int64)
    xs, ys = sc[:, 0], sc[:, 1]
    nxt = np.arange(V) + 1
    last = vert_off[1:][n_vert > 0] - 1
    nxt[last] = vert_off[:-1][n_vert > 0]                               # the edge from a polygon's last vertex closes it
    dx, dy = np.abs(xs[nxt] - xs), np.abs(ys - ys[nxt])
    steps = np.maximum(dx, dy) + 1
    cs = np.concatenate(([0], np.cumsum(steps)))
    walk = cs[vert_off[1:]] - cs[vert_off[:-1]]                         # points per polygon
    bound = np.concatenate(([0], np.cumsum(dx // SCALE + 2)))
    bound = bound[vert_off[1:]] - bound[vert_off[:-1]]
    np.logical_or.at(unsafe, ann_of_poly[walk > MAX_STEPS], True)
    step_pref = np.zeros(V + P, np.int64)
    if V:
        step_pref[np.arange(V) + poly_of_vert + 1] = cs[1:] - cs[vert_off[:-1]][poly_of_vert]
    ann_bound = np.zeros(A, np.int64)
    np.add.at(ann_bound, ann_of_poly, bound)
    over_cap = ann_bound > LDS_CROSSINGS
    host = over_cap | unsafe
    out_off = np.concatenate(([0], np.cumsum(np.where(host, 1, ann_bound + 1))))
    if out_off[-1] > 0x7fffffff:
        raise ValueError("polygons.pack: more than 2^31 - 1 runs of capacity in one call (convert the file in parts)")
    i32 = lambda v: np.ascontiguousarray(np.clip(v, -0x80000000, 0x7fffffff), dtype=np.int32)
    return {"xs": i32(xs), "ys": i32(ys), "steps": i32(steps), "step_pref": i32(step_pref), "vert_off": i32(vert_off),
            "poly_off": i32(poly_off), "hw": i32(hw), "bound": bound, "out_off": i32(out_off), "host": host, "unsafe": unsafe,
            "over_cap": over_cap}


def _points(pk, edge, d):
    """(u, v) of point d on `edge` (arrays), in closed form as _polygon_boundary steps it: the flip rule (dx == dy goes with dx > dy),
    t = n - d under flip, s = 0 on an edge of no length, int() by truncation; one float64 operation at a time."""
    xs, ys, vert_off = pk["xs"].astype(np.int64), pk["ys"].astype(np.int64), pk["vert_off"].astype(np.int64)
    poly = np.searchsorted(vert_off, edge, side="right") - 1
    nxt = np.where(edge + 1 == vert_off[poly + 1], vert_off[poly], edge + 1)
    x0, x1, y0, y1 = xs[edge], xs[nxt], ys[edge], ys[nxt]
    dx, dy = np.abs(x1 - x0), np.abs(y0 - y1)
    major = dx >= dy
    flip = np.where(major, x0 > x1, y0 > y1)
    x0, x1 = np.where(flip, x1, x0), np.where(flip, x0, x1)
    y0, y1 = np.where(flip, y1, y0), np.where(flip, y0, y1)
    n = np.where(major, dx, dy)
    t = np.where(flip, n - d, d)
    num = np.where(major, y1 - y0, x1 - x0).astype(np.float64)
    s = np.where(n > 0, num / np.maximum(n, 1).astype(np.float64), 0.0)
    along = t + np.where(major, x0, y0)
    across = np.trunc(np.where(major, y0, x0).astype(np.float64) + s * t.astype(np.float64) + .5).astype(np.int64)
    return np.where(major, along, across), np.where(major, across, along)


def crossings_np(pk):
    """(annotation, polygon, position) of every kept crossing of every annotation that is not `unsafe`, positions at h * w included
    (pack's bound counts them), in walk order."""
    vert_off, poly_off = pk["vert_off"].astype(np.int64), pk["poly_off"].astype(np.int64)
    P = vert_off.size - 1
    ann_of_poly = np.repeat(np.arange(poly_off.size - 1), np.diff(poly_off))
    steps = pk["steps"].astype(np.int64).copy()
    steps[np.repeat(pk["unsafe"][ann_of_poly], np.diff(vert_off))] = 0
    edge = np.repeat(np.arange(steps.size), steps)                          # the edge of every point of every walk
    start = np.concatenate(([0], np.cumsum(steps)))[:-1]
    d = np.arange(edge.size) - start[edge]
    u, v = _points(pk, edge, d)
    poly = np.searchsorted(vert_off, edge, side="right") - 1
    ann = ann_of_poly[poly]
    j = np.flatnonzero(poly[1:] == poly[:-1]) + 1                           # pairs (j - 1, j) within one polygon's walk
    u0, u1, v0, v1 = u[j - 1], u[j], v[j - 1], v[j]
    h, w = pk["hw"][ann[j], 0].astype(np.int64), pk["hw"][ann[j], 1].astype(np.int64)
    xd = np.where(u1 < u0, u1, u1 - 1).astype(np.float64)
    xd = (xd + .5) / SCALE - .5
    keep = (u1 != u0) & (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)    # the walk changes column at a pixel-column centre
    yd = np.minimum(v0, v1).astype(np.float64)
    yd = (yd + .5) / SCALE - .5
    yd = np.clip(yd, 0.0, h.astype(np.float64))
    pos = xd.astype(np.int64) * h + np.ceil(yd).astype(np.int64)
    return ann[j][keep], poly[j][keep], pos[keep]


def runs_np(pk) -> List[Optional[np.ndarray]]:
    """The int64 run counts of every annotation of pack()'s arrays, as the kernel computes them (the module's docstring); None for an
    `unsafe` annotation, whose walk the arrays do not hold."""
    A = pk["hw"].shape[0]
    hw = pk["hw"][:, 0].astype(np.int64) * pk["hw"][:, 1].astype(np.int64)
    ann, poly, pos = crossings_np(pk)
    inside = pos < hw[ann]                                                  # a crossing at h * w changes no pixel
    ann, poly, pos = ann[inside], poly[inside], pos[inside]
    o = np.lexsort((pos, poly))                                             # the sort per polygon
    ann, poly, pos = ann[o], poly[o], pos[o]
    first = np.flatnonzero(np.concatenate(([True], poly[1:] != poly[:-1]))) if pos.size else np.zeros(0, np.int64)
    rank = np.arange(pos.size) - np.repeat(first, np.diff(np.concatenate((first, [pos.size]))))
    sign = 1 - 2 * (rank & 1)                                               # even rank: the polygon starts, odd: it ends
    o = np.lexsort((pos, ann))                                              # the merge of an annotation's events
    ann, pos, sign = ann[o], pos[o], sign[o]
    cs = np.cumsum(sign)
    a_first = np.searchsorted(ann, np.arange(A), side="left")
    cov = cs - np.concatenate(([0], cs))[a_first][ann] if pos.size else cs  # coverage after each event, within its annotation
    end = np.concatenate(((ann[1:] != ann[:-1]) | (pos[1:] != pos[:-1]), [True])) if pos.size else np.zeros(0, bool)
    g_ann, g_pos, after = ann[end], pos[end], cov[end]                      # equal positions taken together
    before = np.concatenate(([0], after[:-1]))
    if g_ann.size:
        before[np.concatenate(([True], g_ann[1:] != g_ann[:-1]))] = 0
    b = (before > 0) != (after > 0)
    b_ann, b_pos = g_ann[b], g_pos[b]
    lo = np.searchsorted(b_ann, np.arange(A), side="left")
    hi = np.searchsorted(b_ann, np.arange(A), side="right")
    return [None if pk["unsafe"][a] else np.diff(np.concatenate(([0], b_pos[lo[a]:hi[a]], [hw[a]]))).astype(np.int64) for a in range(A)]


def _host_counts(annotation) -> np.ndarray:
    polys, h, w = annotation
    return rle.counts_np(rle.from_polygons(polys, int(h), int(w))["counts"])


def runs_device(annotations: Sequence[Tuple], device=None, events=None):
    """([int64 run counts per annotation], stats) on the GPU: per CHUNK_ANNOTATIONS annotations (one chunk for most files) ONE
    host-to-device copy of pack()'s arrays, zh_polygon_runs, ONE copy back.  Annotations pack() leaves to the host, and any the kernel
    refuses, are filled from rle.from_polygons and counted: stats = {"annotations", "polygons", "host_fallback"}.  events (a list):
    gets (entry name, start, end) HIP events of each launch."""
    import torch
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.ZutisHipError("polygons.runs_device runs on the GPU (rle.from_polygons is the host form)")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.ZutisHipError("polygons.runs_device runs on the GPU (rle.from_polygons is the host form)")
    annotations = list(annotations)
    res, stats = [], {"annotations": len(annotations), "polygons": 0, "host_fallback": 0}
    for lo in range(0, len(annotations), CHUNK_ANNOTATIONS):
        _runs_chunk(annotations[lo:lo + CHUNK_ANNOTATIONS], device, events, res, stats)
    return res, stats


def _launch_chunk(annotations, device, events, stats):
    """pack() of one chunk, ONE host-to-device copy of its arrays and zh_polygon_runs: (pk, out) with out int32 [cap + A] on the device,
    the counts in out[:cap] at pk["out_off"], n_runs in out[cap:].  Adds the chunk's polygons to `stats`."""
    import torch
    from . import ops
    from .coco_eval import _sections
    pk = pack(annotations)
    A = len(annotations)
    stats["polygons"] += int(pk["vert_off"].size - 1)
    names = ("xs", "ys", "step_pref", "vert_off", "poly_off", "hw", "out_off")
    host, lay = _sections([(n, pk[n]) for n in names] + [("flags", pk["host"].astype(np.int32))])
    cap = int(pk["out_off"][-1])
    with torch.cuda.device(device):
        dbuf = torch.from_numpy(host).to(device)                                         # the one host-to-device copy
        out = torch.empty(cap + A, dtype=torch.int32, device=device)                     # counts [cap], n_runs [A]
        view = lambda n: dbuf[lay[n][0]:lay[n][0] + max(lay[n][1].nbytes, 4)].view(torch.int32)[:lay[n][1].size]
        if events is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        ops.polygon_runs(*(view(n) for n in names), view("flags"), out[:cap], out[cap:])
        if events is not None:
            e1.record()
            events.append(("zh_polygon_runs", e0, e1))
    return pk, out


def _runs_chunk(annotations, device, events, res, stats):
    """One launch of runs_device: appends the chunk's counts to `res` and adds to `stats`."""
    pk, out = _launch_chunk(annotations, device, events, stats)
    A, cap = len(annotations), int(pk["out_off"][-1])
    h_out = out.cpu().numpy()                                                            # the one copy back
    n_runs, off = h_out[cap:], pk["out_off"]
    for a in range(A):
        if n_runs[a] < 0:
            stats["host_fallback"] += 1
            res.append(_host_counts(annotations[a]))
        else:
            res.append(h_out[off[a]:off[a] + n_runs[a]].astype(np.int64))


def runs_resident(annotations: Sequence[Tuple], device=None, events=None):
    """runs_device with the counts left on the device: ([(counts int32 [R_c] on the device, n_runs int64 [A_c] on the host)] per chunk of
    CHUNK_ANNOTATIONS annotations, {chunk-wide annotation index: int64 host counts} of those left to the host, stats).  Per chunk pack()
    and the launch of runs_device, then only n_runs crosses to the host (4 bytes an annotation) and the capacity-sized output is
    compacted to the runs actually written — annotation a's n_runs[a] counts follow those of a - 1, an annotation left to the host
    (n_runs -1, filled from rle.from_polygons in the dict) takes no place — so what stays resident is the runs, not out_off[-1] slots."""
    import torch
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.ZutisHipError("polygons.runs_resident runs on the GPU (rle.from_polygons is the host form)")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.ZutisHipError("polygons.runs_resident runs on the GPU (rle.from_polygons is the host form)")
    annotations = list(annotations)
    chunks, host, stats = [], {}, {"annotations": len(annotations), "polygons": 0, "host_fallback": 0}
    for lo in range(0, len(annotations), CHUNK_ANNOTATIONS):
        part = annotations[lo:lo + CHUNK_ANNOTATIONS]
        pk, out = _launch_chunk(part, device, events, stats)
        A, cap = len(part), int(pk["out_off"][-1])
        n_runs = out[cap:].cpu().numpy().astype(np.int64)                                # 4 bytes an annotation: the counts stay
        for a in np.flatnonzero(n_runs < 0):
            stats["host_fallback"] += 1
            host[lo + int(a)] = _host_counts(part[a])
        kept = np.maximum(n_runs, 0)
        start = np.concatenate(([0], np.cumsum(kept)))[:-1]
        with torch.cuda.device(device):                                                  # the gather that compacts: index plumbing, no arithmetic on the counts
            shift = torch.repeat_interleave(torch.from_numpy(pk["out_off"][:-1].astype(np.int64) - start).to(device),
                                            torch.from_numpy(kept).to(device), output_size=int(kept.sum()))
            src = torch.arange(shift.numel(), dtype=torch.int64, device=device) + shift
            chunks.append((out[:cap][src] if src.numel() else torch.zeros(0, dtype=torch.int32, device=device), n_runs))
    return chunks, host, stats


def to_rles(annotations: Sequence[Tuple], device=None) -> List[Dict]:
    """The COCO RLE dicts of polygon annotations [(polys, h, w)]: mask.frPyObjects + mask.merge per annotation, for a whole file."""
    counts, _ = runs_device(annotations, device)
    return [{"size": [int(h), int(w)], "counts": rle._to_string(c)} for c, (_, h, w) in zip(counts, annotations)]
