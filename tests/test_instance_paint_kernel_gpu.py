"""-m gpu: zh_instance_paint — the id map and the colour overlay of the kept instance masks — against instance_paint.paint_reference, the
definition in NumPy integers.  Exact equality of both outputs, for the byte form and the bit form of the masks; the outputs sit in a
guard-band arena (tests/_guard.py), so a byte written outside [B,H,W] / [B,H,W,3] is reported.  The shapes are the smallest at which the
kernel can go wrong: a wave owns one 64-pixel word of every mask, so the edges are at 63 / 64 / 65 pixels, a row that crosses a word,
and a width that is no multiple of 64 (words straddle rows, the vertical neighbours of the outline lie in other words)."""
import numpy as np
import pytest
import torch

from tests._guard import OUT_FILL, Arena, assert_equal, assert_untouched

pytestmark = pytest.mark.gpu

u8, i32, i64, f64 = torch.uint8, torch.int32, torch.int64, torch.float64


class Case:
    """Seeded inputs: masks u8 [B,Q,H,W] (non-zero bytes of several values), a slot table whose slot j shows query index[b,j] (a permutation:
    slot != query), scores f64, colours u8 [B,Q,3] per slot, images u8 [B,H,W,3].  Entries past count[b] hold what a kept list may hold
    there — -1, a huge index, a NaN or a winning score — and must never be read."""

    def __init__(self, seed, B, Q, H, W, counts=None, density=0.35):
        rng = np.random.default_rng(seed)
        self.B, self.Q, self.H, self.W = B, Q, H, W
        self.masks = (rng.random((B, Q, H, W)) < density).astype(np.uint8) * rng.choice(np.array([1, 1, 2, 255], np.uint8), (B, Q, H, W))
        self.index = np.stack([rng.permutation(Q) for _ in range(B)]).astype(np.int32)
        self.score = rng.random((B, Q))
        self.count = np.full((B,), Q, np.int32) if counts is None else np.asarray(counts, np.int32)
        self.colours = rng.integers(0, 256, (B, Q, 3), dtype=np.uint8)
        self.images = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        for b in range(B):
            c = int(self.count[b])
            self.index[b, c:] = np.resize(np.array([-1, 10 ** 6, -(2 ** 31)], np.int32), Q - c)
            self.score[b, c:] = np.resize(np.array([np.nan, 9.0, np.inf]), Q - c)

    def reference(self, alpha=128, outline=True, min_score=0.0):
        ids, ovl = [], []
        for b in range(self.B):
            c = int(self.count[b])
            i, o = paint_reference(self.images[b], self.masks[b][self.index[b, :c]], self.score[b, :c], self.colours[b, :c], alpha=alpha,
                                   outline=outline, min_score=min_score)
            ids.append(i)
            ovl.append(o)
        return np.stack(ids), np.stack(ovl)


def paint_reference(*a, **k):
    from zutis_amd.instance_paint import paint_reference as ref
    return ref(*a, **k)


def _staging(dev, images):
    """(packed, desc, desc_host) as a loader lays a batch out: every image HWC at a 16-byte aligned offset, desc rows (offset / 16, w, h, ...)."""
    B, H, W, _ = images.shape
    step = -(-3 * H * W // 16) * 16
    packed = np.full((B * step + 16,), 0xEE, np.uint8)
    desc = np.zeros((B, 8), np.int32)
    for b in range(B):
        packed[16 + b * step:16 + b * step + 3 * H * W] = images[b].reshape(-1)
        desc[b] = ((16 + b * step) // 16, W, H, W, H, 0, 0, 0)
    return torch.from_numpy(packed).to(dev), torch.from_numpy(desc).to(dev), torch.from_numpy(desc)


def _bits(dev, masks_dev):
    """The bit-packed masks as the product path makes them: the workspace zh_mask_iou_counts leaves behind."""
    from zutis_amd import ops
    B, Q, H, W = masks_dev.shape
    bits = torch.empty((B, Q, (H * W + 63) // 64), dtype=i64, device=dev)
    inter = torch.empty((Q, Q), dtype=i32, device=dev)
    for b in range(B):
        ops.mask_iou_counts(masks_dev[b], Q, H * W, inter, torch.empty_like(inter), workspace=bits[b])
    return bits


def _decode_ids(raw, id_format):
    raw = raw.astype(np.int64)
    if id_format == "u8":
        return raw
    assert not raw[..., 2].any()
    return raw[..., 0] + 256 * raw[..., 1]


def _paint(dev, case, form, *, alpha=128, outline=True, min_score=0.0, id_format="u8", want_ids=True, want_overlay=True, table=None):
    """One launch into a guard-band arena -> (ids int64 [B,H,W] or None, overlay u8 [B,H,W,3] or None).  table: (index, score, count) device
    tensors to use instead of the case's (the chained test)."""
    from zutis_amd import ops
    B, Q, H, W = case.B, case.Q, case.H, case.W
    arena = Arena(OUT_FILL, dev)
    ch = 1 if id_format == "u8" else 3
    v_ids = arena.add("ids", u8, 1, B * H * W * ch, tail_rows=1) if want_ids else None
    v_ovl = arena.add("overlay", u8, 1, B * H * W * 3, tail_rows=1) if want_overlay else None
    v_ws = arena.workspace("workspace", ops.instance_paint_workspace_size(B, Q, H, W))
    masks = torch.from_numpy(case.masks).to(dev)
    packed, desc, desc_host = _staging(dev, case.images)
    index, score, count = table if table is not None else (torch.from_numpy(case.index).to(dev), torch.from_numpy(case.score).to(dev),
                                                           torch.from_numpy(case.count).to(dev))
    ops.instance_paint(index, score, count, H, W, masks=masks if form == "bytes" else None, bits=_bits(dev, masks) if form == "bits" else None,
                       colours=torch.from_numpy(case.colours).to(dev), alpha=alpha, outline=outline, min_score=min_score, packed=packed, desc=desc,
                       desc_host=desc_host, id_format=id_format,
                       ids_out=v_ids.m2.view((B, H, W) if ch == 1 else (B, H, W, 3)) if want_ids else None,
                       overlay_out=v_ovl.m2.view(B, H, W, 3) if want_overlay else None, workspace=v_ws.m2.view(-1))
    torch.cuda.synchronize()
    assert_untouched(arena)
    ids = _decode_ids(v_ids.get().numpy().reshape((B, H, W) if ch == 1 else (B, H, W, 3)), id_format) if want_ids else None
    ovl = v_ovl.get().numpy().reshape(B, H, W, 3) if want_overlay else None
    return ids, ovl


def _check(dev, case, **kw):
    """Both mask forms against the reference; returns the reference's (ids, overlay)."""
    ref_kw = {k: kw[k] for k in ("alpha", "outline", "min_score") if k in kw}
    want_ids, want_ovl = case.reference(**ref_kw)
    for form in ("bits", "bytes"):
        ids, ovl = _paint(dev, case, form, **kw)
        assert_equal(ids, want_ids, f"{form}: id map")
        assert_equal(ovl, want_ovl, f"{form}: overlay")
    return want_ids, want_ovl


# 1 x 1; one row / one column crossing a word; 63, 64 and 65 pixels; W % 64 != 0 with several words per image and more than one workgroup
WORD_EDGES = [(1, 1), (1, 70), (70, 1), (7, 9), (8, 8), (5, 13), (33, 67)]


@pytest.mark.parametrize("H,W", WORD_EDGES)
def test_word_edges(dev, H, W):
    want_ids, _ = _check(dev, Case(100 + H * W, 2, 5, H, W, density=0.4))
    if H * W > 1:
        assert want_ids.max() > 0 and (want_ids == 0).any()


def test_many_overlapping_masks(dev):
    case = Case(2, 1, 100, 24, 40, density=0.12)               # every pair of masks overlaps somewhere; a pixel lies under 12 of them
    want_ids, _ = _check(dev, case)
    assert len(np.unique(want_ids)) > 20                       # the walk goes deep into the ranks before every lane has its top
    m = (case.masks[0].reshape(100, -1) != 0).astype(np.int64)
    assert (m @ m.T > 0).all()


def test_an_empty_mask_among_the_kept(dev):
    case = Case(3, 1, 6, 9, 11)
    case.masks[0, case.index[0, 2]] = 0
    case.score[0, 2] = 2.0                                     # the empty mask ranks first and claims nothing
    want_ids, _ = _check(dev, case)
    assert not (want_ids == 3).any() and want_ids.max() > 0


def test_a_full_mask_has_no_outline_but_against_other_instances(dev):
    case = Case(4, 1, 2, 12, 70, density=0.0)
    full, blob = case.index[0, 0], case.index[0, 1]
    case.masks[0, full] = 1
    case.masks[0, blob, 3:8, 60:68] = 1                        # the blob's rows cross a word boundary
    case.score[0] = (0.25, 0.75)
    want_ids, want_ovl = _check(dev, case)
    inner = np.ones((12, 70), bool)
    inner[2:9, 59:69] = False                                  # away from the blob: the full mask meets only itself and the image border
    from zutis_amd.predict_files import blend
    assert np.array_equal(want_ovl[0][inner], blend(case.images[0][inner], np.broadcast_to(case.colours[0, 0], (inner.sum(), 3)), 128))
    case.count[:] = 1                                          # the full mask alone: a pure blend, border pixels included
    _, alone = _check(dev, case)
    assert np.array_equal(alone[0], blend(case.images[0], np.broadcast_to(case.colours[0, 0], (12, 70, 3)), 128))


def test_a_batch_with_counts_zero_some_and_all(dev):
    Q = 7
    case = Case(5, 3, Q, 10, 23, counts=(0, 5, Q))
    want_ids, want_ovl = _check(dev, case)
    assert not want_ids[0].any() and np.array_equal(want_ovl[0], case.images[0])
    assert want_ids[1].max() <= 5 and want_ids[2].max() > 0


def test_min_score_is_strict_and_can_remove_the_top_ranked_slot(dev):
    case = Case(6, 1, 5, 9, 15, density=0.6)
    case.score[0] = (0.9, 0.5, 0.5000000000000001, 0.2, 0.7)
    unfiltered, _ = case.reference()
    ids, _ = _check(dev, case, min_score=0.5)                  # slot 1 (== min_score) goes, slot 2 (one ulp above) stays
    assert (unfiltered == 2).any() and not (ids == 2).any() and (ids == 3).any()
    case.score[0] = (0.2, 0.9, 0.5, 0.3, 0.7)
    case2_ids, _ = _check(dev, case, min_score=-1.0)
    assert (case2_ids == 2).any()
    case.score[0, 1] = -2.0                                    # now the filter removes what was the top-ranked slot
    ids, _ = _check(dev, case, min_score=-1.0)
    assert not (ids == 2).any() and ids.max() > 0


def test_equal_scores_go_to_the_lower_slot(dev):
    case = Case(7, 2, 8, 9, 14, density=0.7)
    case.score[:] = np.array([0.5, 0.25, 0.5, 0.5, 0.25, 0.75, 0.75, 0.5])
    want_ids, _ = _check(dev, case)
    both = (case.masks[0, case.index[0, 5]] != 0) & (case.masks[0, case.index[0, 6]] != 0)
    assert both.any() and (want_ids[0][both] == 6).all()      # slots 5 and 6 tie at the top: slot 5 (id 6) wins where both cover


@pytest.mark.parametrize("alpha", [0, 128, 256])
@pytest.mark.parametrize("outline", [True, False])
def test_alpha_and_outline(dev, alpha, outline):
    _check(dev, Case(8, 2, 4, 11, 19), alpha=alpha, outline=outline)


def test_rg16_ids_above_255_and_u8_refuses_them(dev):
    from zutis_amd._lib import ZutisHipError
    Q = 300
    case = Case(9, 1, Q, 4, 4, density=0.02)
    case.score[0] = np.linspace(0.1, 0.9, Q)                   # the high slots win: ids above 255 appear
    want_ids, _ = _check(dev, case, id_format="rg16")
    assert want_ids.max() > 255
    with pytest.raises(ZutisHipError, match="rg16"):
        _paint(dev, case, "bytes", id_format="u8")
    _paint(dev, case, "bytes", id_format="u8", want_ids=False)  # an overlay alone does not need the byte format to fit


def test_the_slot_table_comes_straight_from_mask_nms(dev):
    """The chained layout: index / score / count are the tensors zh_mask_nms wrote, handed on without a host visit; what lies past
    count[b] is whatever the launch left there."""
    from zutis_amd import ops
    B, Q, H, W = 2, 12, 17, 29
    case = Case(10, B, Q, H, W, density=0.3)
    rng = np.random.default_rng(11)
    masks = torch.from_numpy(case.masks).to(dev)
    inter = torch.empty((B, Q, Q), dtype=i32, device=dev)
    uni = torch.empty_like(inter)
    for b in range(B):
        ops.mask_iou_counts(masks[b], Q, H * W, inter[b], uni[b])
    scores = torch.from_numpy(rng.random((B, Q)).astype(np.float32)).to(dev)
    cats = torch.from_numpy(rng.integers(0, 4, (B, Q))).to(dev)
    idx, sc, _, cnt = ops.mask_nms(inter, uni, scores, cats, "hard", nms_threshold=0.9)
    got = {form: _paint(dev, case, form, table=(idx, sc, cnt)) for form in ("bits", "bytes")}
    case.count = cnt.cpu().numpy()
    assert case.count.min() >= 2
    for b in range(B):
        c = int(case.count[b])
        case.index[b, :c] = idx[b, :c].cpu().numpy()
        case.score[b, :c] = sc[b, :c].cpu().numpy()
    want_ids, want_ovl = case.reference()
    for form, (ids, ovl) in got.items():
        assert_equal(ids, want_ids, f"{form}: id map")
        assert_equal(ovl, want_ovl, f"{form}: overlay")


@pytest.mark.parametrize("outline", [True, False])
def test_only_one_of_the_two_outputs(dev, outline):
    case = Case(12, 2, 5, 9, 15)
    want_ids, want_ovl = case.reference(outline=outline)
    for form in ("bits", "bytes"):
        ids, none = _paint(dev, case, form, outline=outline, want_overlay=False)
        assert none is None
        assert_equal(ids, want_ids, f"{form}: id map alone")
        none, ovl = _paint(dev, case, form, outline=outline, want_ids=False)
        assert none is None
        assert_equal(ovl, want_ovl, f"{form}: overlay alone")
