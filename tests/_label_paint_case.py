"""Small COCO annotation dicts for tests/test_annotation_labels_cpu.py and tests/test_annotation_labels_gpu.py: the rectangles whose label
maps are written out by hand, the edge set, a seeded corpus of one size, and the NumPy restatement of the per-pixel walk that
csrc/label_paint.hip runs.  CPU only."""
import numpy as np

from tests import _cocoeval_case as CC
from tests import _polygon_case as PC
from zutis_amd import polygons, rle

CATEGORIES = (1, 3, 7, 90)            # non-contiguous ids: the default labels are 1, 2, 3, 4
LABEL = {1: 1, 3: 2, 7: 3, 90: 4}
IGN = 255


def rect(x0, y0, x1, y1):
    """The polygon that covers columns x0 .. x1 - 1 and rows y0 .. y1 - 1 (tests/_polygon_case.hand_cases)."""
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def rle_segmentation(mask, form):
    """The RLE dict of a dense mask as tests/_cocoeval_case.to_coco writes it: form "bytes" / "str" (compressed) or "list" (uncompressed)."""
    h, w = mask.shape
    ann, _ = CC.to_coco({0: (h, w)}, [1], [CC.gt(0, 1, mask)], [], counts_form=form)
    return ann["annotations"][0]["segmentation"]


class Builder:
    def __init__(self):
        self.images, self.annotations = [], []

    def image(self, h, w, file_name=None):
        i = 100 + 7 * len(self.images)                              # ids that are not positions
        self.images.append({"id": i, "height": h, "width": w, "file_name": file_name or f"dir/{i:012d}.jpg"})
        return i

    def add(self, image_id, category_id, segmentation, iscrowd=0, area=None):
        a = {"id": 1000 + len(self.annotations), "image_id": image_id, "category_id": category_id, "segmentation": segmentation,
             "iscrowd": int(iscrowd)}
        if area is not None:
            a["area"] = float(area)
        self.annotations.append(a)

    def done(self, categories=CATEGORIES):
        return {"images": self.images, "categories": [{"id": c, "name": f"c{c}"} for c in categories], "annotations": self.annotations}


# ---- rectangles by hand: a 4 x 6 image; A (category 3 -> 2) rows 0-2, columns 0-3, area 12; C, a crowd without an `area` field (category
# 1 -> 1; 6 pixels) rows 0-2, columns 3-4; B (category 90 -> 4) rows 2-3, columns 2-5, area 8.  File order A, C, B; by area A, B, C.
# Pixel (2, 3) lies under all three.
def hand_dict():
    b = Builder()
    i = b.image(4, 6)
    b.add(i, 3, [rect(0, 0, 4, 3)], area=12)
    b.add(i, 1, rle_segmentation(CC.box(4, 6, 0, 3, 3, 5), "list"), iscrowd=1)
    b.add(i, 90, [rect(2, 2, 6, 4)], area=8)
    return b.done()


_SKIP_LAST = [[2, 2, 2, 2, 0, 0], [2, 2, 2, 2, 0, 0], [2, 2, 4, 4, 4, 4], [0, 0, 4, 4, 4, 4]]
_CROWD_ON_TOP = [[2, 2, 2, IGN, IGN, 0], [2, 2, 2, IGN, IGN, 0], [2, 2, 4, IGN, IGN, 4], [0, 0, 4, 4, 4, 4]]
HAND = {  # (order, overlap, crowd) -> the map
    ("file", "last", "label"): [[2, 2, 2, 1, 1, 0], [2, 2, 2, 1, 1, 0], [2, 2, 4, 4, 4, 4], [0, 0, 4, 4, 4, 4]],      # B over C over A
    ("file", "last", "ignore"): _CROWD_ON_TOP,                                                                          # A, B, then C as 255
    ("file", "last", "skip"): _SKIP_LAST,
    ("area", "last", "label"): [[2, 2, 2, 1, 1, 0], [2, 2, 2, 1, 1, 0], [2, 2, 4, 1, 1, 4], [0, 0, 4, 4, 4, 4]],      # C over B over A
    ("area", "last", "ignore"): _CROWD_ON_TOP,
    ("area", "last", "skip"): _SKIP_LAST,
}
for _o in ("file", "area"):                                          # "ignore" does not depend on the order
    HAND[(_o, "ignore", "label")] = [[2, 2, 2, IGN, 1, 0], [2, 2, 2, IGN, 1, 0], [2, 2, IGN, IGN, IGN, 4], [0, 0, 4, 4, 4, 4]]
    HAND[(_o, "ignore", "ignore")] = [[2, 2, 2, IGN, IGN, 0], [2, 2, 2, IGN, IGN, 0], [2, 2, IGN, IGN, IGN, 4], [0, 0, 4, 4, 4, 4]]
    HAND[(_o, "ignore", "skip")] = [[2, 2, 2, 2, 0, 0], [2, 2, 2, 2, 0, 0], [2, 2, IGN, IGN, 4, 4], [0, 0, 4, 4, 4, 4]]


def hand_cases():
    """[((order, overlap, crowd), uint8 [4, 6])] over hand_dict()."""
    return [(k, np.asarray(v, np.uint8)) for k, v in HAND.items()]


# ---- the edge set
def edge_dict(zigzags=1):
    """One annotation dict: images of 1 x 1, 1 x 7, 7 x 1, 9 x 11 and 33 x 65 (one past a wave, one past a 32-wide tile), an image without
    annotations, annotations of no pixel ([h * w]) and of every pixel ([0, h * w]), three annotations stacked on one pixel, two entries
    of one label that overlap, crowds as uncompressed and as compressed RLE, an annotation of several polygons, one image with 300
    annotations, and `zigzags` annotations over ZH_POLYGON_LDS_CROSSINGS (the host fallback)."""
    rng = np.random.default_rng(5)
    b = Builder()
    i = b.image(1, 1)
    b.add(i, 1, {"size": [1, 1], "counts": [0, 1]})
    i = b.image(1, 7)
    b.add(i, 3, [rect(2, 0, 5, 1)])
    b.add(i, 7, {"size": [1, 7], "counts": [7]})                                          # no pixel
    b.add(i, 90, rle_segmentation(CC.box(1, 7, 0, 4, 1, 7), "str"), iscrowd=1)
    i = b.image(7, 1)
    b.add(i, 90, {"size": [7, 1], "counts": [0, 7]})                                      # every pixel
    b.add(i, 1, [rect(0, 2, 1, 5)])
    b.add(i, 7, rle_segmentation(CC.box(7, 1, 5, 0, 7, 1), "list"), iscrowd=1)
    i = b.image(9, 11)
    b.add(i, 1, [rect(1, 1, 8, 6)], area=35)
    b.add(i, 3, [rect(3, 2, 10, 8)], area=42)
    b.add(i, 7, [rect(4, 3, 6, 9)], area=12)                                              # (4, 4) lies under all three
    b.add(i, 7, [rect(5, 7, 11, 9)], area=12)                                             # the same label again, over the one before
    b.add(i, 90, [rect(0, 0, 2, 2), rect(9, 0, 11, 3), [0.0, 8.0, 3.0, 8.0, 0.0, 5.0]], area=13)      # several polygons
    b.add(i, 3, rle_segmentation(CC.box(9, 11, 6, 0, 9, 4) & (rng.random((9, 11)) > .3), "bytes"), iscrowd=1)
    b.image(20, 24)                                                                       # no annotation
    i = b.image(33, 65)
    b.add(i, 1, {"size": [33, 65], "counts": [0, 33 * 65]})                               # every pixel, under the rest
    b.add(i, 3, {"size": [33, 65], "counts": [33 * 65]})
    for k, (polys, h, w) in enumerate(PC.coco_like(11, 6, 33, 65, polys=(1, 3))):
        b.add(i, CATEGORIES[k % 4], polys)
    b.add(i, 7, rle_segmentation(rng.random((33, 65)) > .6, "list"), iscrowd=1)           # 1000-odd runs
    b.add(i, 90, rle_segmentation(CC.box(33, 65, 30, 60, 33, 65), "str"), iscrowd=1)      # the last pixel
    b.add(i, 3, [rect(31, 0, 34, 9)])                                                     # across the 32-column tile edge, rows 0 .. 8
    i = b.image(40, 56)
    for k in range(300):                                                                  # more than one staging pass of the list
        x0, y0 = int(rng.integers(0, 52)), int(rng.integers(0, 36))
        if k % 25 == 7:
            m = CC.box(40, 56, y0, x0, y0 + 4, x0 + 4)
            b.add(i, CATEGORIES[k % 4], rle_segmentation(m, ("list", "str")[k & 1]), iscrowd=1)
        else:
            b.add(i, CATEGORIES[k % 4], [rect(x0, y0, x0 + int(rng.integers(1, 6)), y0 + int(rng.integers(1, 6)))])
    for _ in range(zigzags):
        polys, h, w = PC.zigzag(polygons.LDS_CROSSINGS)
        i = b.image(h, w)
        b.add(i, 3, [rect(0, 0, 40, 8)])
        b.add(i, 7, polys)
        b.add(i, 1, [rect(w - 3, 2, w, 5)])
    return b.done()


def same_size_dict(seed=3, n=40, h=40, w=56):
    """n images of h x w with 0 - 12 star and rectangle annotations each, some of them crowds as RLE."""
    rng = np.random.default_rng(seed)
    b = Builder()
    for _ in range(n):
        i = b.image(h, w)
        for k in range(int(rng.integers(0, 13))):
            c = CATEGORIES[int(rng.integers(0, 4))]
            kind = int(rng.integers(0, 4))
            if kind == 0:
                x0, y0 = int(rng.integers(-3, w - 2)), int(rng.integers(-3, h - 2))
                b.add(i, c, [rect(x0, y0, x0 + int(rng.integers(1, 30)), y0 + int(rng.integers(1, 30)))])
            elif kind == 3:
                b.add(i, c, rle_segmentation(rng.random((h, w)) > .8, ("list", "str")[k & 1]), iscrowd=1)
            else:
                b.add(i, c, [PC.star(rng, h, w) for _ in range(kind)])
    return b.done()


# ---- the kernel's walk, per pixel, in NumPy
def run_ends(plan):
    """{annotation index: int64 run ends} of the plan's annotations from the host counts (what zh_rle_prefix leaves as run_end)."""
    anns = plan.ground_truth["annotations"]
    ends = {}
    for im, entries in zip(plan.images, plan.lists):
        for j, _ in entries:
            seg = anns[j]["segmentation"]
            c = rle.counts_np(seg["counts"] if isinstance(seg, dict) else rle.from_polygons(seg, im["h"], im["w"])["counts"])
            ends[j] = np.cumsum(c)
    return ends


def walk_np(plan, forward=False, parity=1, row_major=False):
    """csrc/label_paint.hip restated: per pixel the column-major position p = x * h + y, in each list entry the index of the first run end
    greater than p by binary search, covered when that index is odd; the list walked from its last entry to its first, stopping at the
    first hit ("last") or the second ("ignore").  forward / parity / row_major: the three ways to get it wrong."""
    ends = run_ends(plan)
    out = []
    for im, entries in zip(plan.images, plan.lists):
        h, w = im["h"], im["w"]
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        p = (ys * w + xs) if row_major else (xs * h + ys)
        label = np.zeros((h, w), np.int64)
        hits = np.zeros((h, w), np.int64)
        for j, lab in (entries if forward else entries[::-1]):
            covered = (np.searchsorted(ends[j], p, side="right") & 1) == parity
            covered &= np.searchsorted(ends[j], p, side="right") < len(ends[j])
            live = hits < (1 if plan.overlap == "last" else 2)                            # lanes that have not stopped
            first = covered & live & (hits == 0)
            label[first] = lab
            label[covered & live & (hits == 1)] = plan.ignore_value
            hits += covered & live
        out.append(label.astype(np.uint8))
    return out
