"""GPU: the five entry points of csrc/criterion.hip (zh_mask_match_cost, zh_mask_match_grad, zh_upsample_ce_fwd / _bwd,
zh_gemm_f32_strided) called directly through zutis_amd.ops, against the kernel-level float64 oracles of tests/_criterion_ref.py.
Covered: the ViT-B/32 and ViT-B/16 training geometries, non-square / identity / downsampled / size-1 axes, planes narrower than a
workgroup and shorter than a 48-row band, 1 and odd query counts, the 16-instance group boundary, empty images, saturated and
out-of-range proposals, edge and out-of-range labels, ignore_index values, large logits, every GEMM layout, bitwise repeatability and
the kernels' refusals.

Forward tolerances come from the length of each fixed-order fp32 sum (u = 2^-24): a sum of k terms, rounded once per add, is off by
at most (k - 1) u sum |terms| (Higham, recursive summation), and k is the longest add chain of the kernel's reduction tree."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from tests._criterion_case import make_case
from tests._criterion_ref import ce_ref, gemm_strided_ref, mask_cost_ref, mask_grad_ref, up_f32

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BAND = 48                     # full-resolution rows per workgroup of the cost kernel (MC_BAND)


def _ops():
    from zutis_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------------------------------- costs
def run_cost(props, gts, dev, wd=1.0, wb=1.0):
    from zutis_amd.criterion import _pack_gt
    ops = _ops()
    B, L, Q = props.shape[:3]
    inst_off, gt_u8, off, H, W = _pack_gt(list(gts), dev)
    n_tot, n_max = int(off[-1]), int(np.diff(off).max())
    nan = float("nan")
    costs = torch.full((max(1, L * n_tot * Q),), nan, device=dev)
    stat_pg = torch.full_like(costs, nan)
    stat_p = torch.full((B, L, Q), nan, device=dev)
    stat_g = torch.full((max(1, n_tot),), nan, device=dev)
    skip = torch.full((B,), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.mask_match_cost(props.contiguous(), gt_u8, inst_off, n_max, H, W, costs, stat_p, stat_pg, stat_g, skip, status, wd, wb)
    return {"costs": costs, "stat_p": stat_p, "stat_pg": stat_pg, "stat_g": stat_g, "skip": skip, "status": int(status.item()),
            "inst_off": inst_off, "gt_u8": gt_u8, "off": off, "H": H, "W": W}


def per_image(flat, off, b, L, Q):
    """image b's [L, n_b, Q] block of the flat cost / stat_pg layout (at L * inst_off[b] * Q)."""
    n_b = int(off[b + 1] - off[b])
    s = L * int(off[b]) * Q
    return flat[s:s + L * n_b * Q].reshape(L, n_b, Q)


def check_cost(out, ref, props, gts):
    B, L, Q, h, w = props.shape
    H, W = out["H"], out["W"]
    off = out["off"]
    assert out["status"] == 0
    assert out["skip"].cpu().tolist() == [int(s) for s in ref["skip"]]
    # sum g of an instance: integers below 2^24 are summed exactly in fp32
    if off[-1]:
        assert torch.equal(out["stat_g"][:int(off[-1])].double().cpu(), ref["stat_g"].cpu())
    # sum p over H*W pixels in [0, 1]: per thread a chain of ceil(BAND W / 256) adds, a 6-level wave tree, 3 adds over the waves,
    # NB - 1 over the bands; the kernel's p is the oracle's fp32 p (a rare double rounding of the emulated fma moves one pixel by
    # one ulp, u < u H W on the sum)
    k = -(-min(BAND, H) * W // 256) + 6 + 3 + -(-H // BAND)
    sp64 = ref["stat_p"]
    err = (out["stat_p"].double() - sp64).abs()
    assert (err <= (k + 1) * U * sp64 + U).all(), float(err.max())
    for b in range(B):
        n_b = int(off[b + 1] - off[b])
        if n_b == 0:
            continue
        c = per_image(out["costs"], off, b, L, Q).double()
        pg = per_image(out["stat_pg"], off, b, L, Q).double()
        # costs: the suite's end-to-end bound, saturated planes included
        dc = (c - ref["costs"][b]).abs()
        assert float(dc.max()) <= 1e-5, (b, float(dc.max()))
        # sum g.p: the chain of sum p over a subset of its terms
        pg64 = ref["stat_pg"][b]
        assert ((pg - pg64).abs() <= (k + 1) * U * pg64 + U).all(), (b, float((pg - pg64).abs().max()))


def hungarian_pairs(ref, skip, L):
    """(b, l, q, i) of the float64 optimum of every (image, layer) that is not skipped."""
    pairs = []
    for b, cm in ref["costs"].items():
        if skip[b]:
            continue
        for l in range(L):
            rows, cols = linear_sum_assignment(cm[l].cpu().numpy())
            pairs += [(b, l, int(q), int(i)) for i, q in zip(rows, cols)]
    return pairs


def run_grad(props, out, pairs, dev, grad_out=1.0, wd=1.0, wb=1.0, scale=1.0):
    ops = _ops()
    pt = torch.tensor(pairs, dtype=torch.int32, device=dev).reshape(-1, 4)
    g = torch.full_like(props, float("nan"))           # every element must be written: matched planes, and 0 elsewhere
    go = torch.tensor([grad_out], dtype=torch.float32, device=dev)
    ops.mask_match_grad(props.contiguous(), out["gt_u8"], out["inst_off"], pt, out["stat_p"], out["stat_pg"], out["stat_g"], go,
                        out["H"], out["W"], wd, wb, scale, out=g)
    return g


def check_grad(g, gref, pairs):
    """Each paired plane to 1e-4 of its own largest value; every other plane exactly 0."""
    B, L, Q = g.shape[:3]
    done = torch.zeros(B, L, Q, dtype=torch.bool)
    for b, l, q, _ in pairs:
        done[b, l, q] = True
        r = gref[b, l, q]
        d = float((g[b, l, q].double() - r).abs().max())
        assert d <= 1e-4 * float(r.abs().max()), ((b, l, q), d, float(r.abs().max()))
    rest = g[~done.to(g.device)]
    assert rest.numel() == 0 or bool((rest == 0).all())


def cost_and_grad(props, gts, dev, pairs=None, wd=1.0, wb=1.0, grad_out=1.0):
    L = props.shape[1]
    ref = mask_cost_ref(props, gts, wd, wb)
    out = run_cost(props, gts, dev, wd, wb)
    check_cost(out, ref, props, gts)
    if pairs is None:
        pairs = hungarian_pairs(ref, ref["skip"], L)
    scale = 1.0 / props.shape[0]
    g = run_grad(props, out, pairs, dev, grad_out, wd, wb, scale)
    gref = mask_grad_ref(props, gts, pairs, wd, wb, grad_out * scale)
    check_grad(g, gref, pairs)
    return out, g


def _props_gts(B, L, Q, h, w, H, W, seed, n_range=(1, 10), dev="cpu"):
    props, gts, _, _, _ = make_case(B, L, Q, h, w, H, W, 2, 4, 1, 1, seed=seed, n_range=n_range)
    return props.to(dev), gts


GEOMETRIES = {
    "vitb32_24to384": (8, 6, 100, 24, 24, 384, 384),     # configs/*_vit_b_32.yaml: 384 crops, 24x24 proposals, 16x
    "vitb16_48to384": (8, 6, 100, 48, 48, 384, 384),
    "nonsquare_20x28to90x130": (2, 2, 7, 20, 28, 90, 130),   # W < 256, W % 4 == 2, H not a multiple of the band
    "identity_h_40x24to40x100": (2, 2, 5, 40, 24, 40, 100),
    "down_40to30_x_20to70": (2, 2, 5, 40, 20, 30, 70),
    "h1_1x13to37x52": (2, 1, 3, 1, 13, 37, 52),             # H < 48: one partial band
    "w1_9x1to45x17": (2, 1, 4, 9, 1, 45, 17),
    "q1_16x12to100x61": (3, 2, 1, 16, 12, 100, 61),
}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_cost_and_grad_geometries(dev, name):
    B, L, Q, h, w, H, W = GEOMETRIES[name]
    props, gts = _props_gts(B, L, Q, h, w, H, W, seed=31, dev=dev)
    cost_and_grad(props, gts, dev)


def test_cost_and_grad_weights_and_grad_out(dev):
    props, gts = _props_gts(2, 2, 9, 24, 24, 96, 96, seed=5, dev=dev)
    cost_and_grad(props, gts, dev, wd=0.6, wb=1.7, grad_out=0.7)


@pytest.mark.parametrize("counts", [(16, 0, 17), (33,)])
def test_instance_group_boundaries(dev, counts):
    """16 instances fill one workgroup's group exactly, 17 and 33 spill one instance into the next; an image with 0 instances sits
    between two that have some."""
    B = len(counts)
    props, gts = _props_gts(B, 2, 11, 24, 24, 120, 96, seed=7, n_range=(33, 33), dev=dev)
    gts = [g[:n] for g, n in zip(gts, counts)]
    out, _ = cost_and_grad(props, gts, dev)
    assert out["skip"].cpu().tolist() == [int(n == 0) for n in counts]


def test_every_image_empty(dev):
    props, _ = _props_gts(3, 2, 5, 12, 12, 60, 60, seed=1, dev=dev)
    gts = [torch.zeros(0, 60, 60, dtype=torch.uint8)] * 3
    out = run_cost(props, gts, dev)
    assert out["off"][-1] == 0 and out["status"] == 0
    assert out["skip"].cpu().tolist() == [1, 1, 1]
    ref = mask_cost_ref(props, gts)
    assert torch.allclose(out["stat_p"].double(), ref["stat_p"], rtol=30 * U, atol=0)
    g = run_grad(props, out, [], dev)
    assert bool((g == 0).all())


def saturated_case(dev):
    """ViT-B/32 geometry (24 -> 384).  Image 0: one instance over all but a 4-pixel frame, and queries that are exactly 1.0 except for
    a few interior holes: wherever g = 1 and p = 1 the 1 - p side of the BCE is the -100 clamp, and the cost's BCE sum must not
    cancel +-100 per pixel; query 36 is exactly 0.0 over a corner of the instance.  Image 1: three boxes; query 0 is exactly 1.0 on
    a box one low-res pixel larger than box 0 (p = 1, g = 0 on its rim), query 1 exactly 0.0 on box 1, query 2 exactly 1.0 away
    from every box.  Returns props, gts and explicit pairs: saturated planes paired with their own GT and with others."""
    g = torch.Generator().manual_seed(17)
    B, L, Q, h, w, H, W = 2, 3, 41, 24, 24, 384, 384
    props = torch.sigmoid(torch.randn(B, L, Q, h, w, generator=g) - 1.0)
    gt0 = torch.zeros(1, H, W, dtype=torch.uint8)
    gt0[0, 4:380, 4:380] = 1
    for l in range(L):
        for q in range(36):
            props[0, l, q] = 1.0
            holes = torch.randint(1, 23, (2, 24), generator=g)
            props[0, l, q, holes[0], holes[1]] = torch.rand(24, generator=g) * 0.9 + 0.05
    props[0, :, 36, 2:10, 2:10] = 0.0
    gt1 = torch.zeros(3, H, W, dtype=torch.uint8)
    gt1[0, 64:160, 64:192] = 1
    gt1[1, 200:300, 40:120] = 1
    gt1[2, 220:330, 250:340] = 1
    props[1, :, 0, 3:11, 3:13] = 1.0            # full-res [56, 168) x [56, 200): box 0 plus a rim
    props[1, :, 1, 12:19, 2:8] = 0.0
    props[1, :, 2, 0:3, 18:24] = 1.0
    pairs = [(0, l, q, 0) for l in range(L) for q in (0, 1, 35, 40)] + [(0, 1, 36, 0)]
    pairs += [(1, l, 0, 0) for l in range(L)] + [(1, 0, 1, 1), (1, 1, 1, 2), (1, 2, 2, 1), (1, 0, 3, 2), (1, 2, 4, 0)]
    return props.to(dev), [gt0, gt1], pairs


def test_saturated_proposals(dev):
    props, gts, pairs = saturated_case(dev)
    p = up_f32(props, 384, 384)
    assert bool((p == 1.0).any()) and bool((p == 0.0).any())     # exact 0 and 1 reach full resolution
    cost_and_grad(props, gts, dev, pairs=pairs)


@pytest.mark.parametrize("bad", [float("nan"), 1.0000001, -1e-30])
def test_out_of_range_proposal_sets_status(dev, bad):
    props, gts = _props_gts(2, 2, 5, 12, 12, 60, 60, seed=3, dev=dev)
    assert run_cost(props, gts, dev)["status"] == 0
    props = props.clone()
    props[1, 1, 4, 11, 0] = bad
    assert run_cost(props, gts, dev)["status"] & _ops().STATUS_RANGE


# ------------------------------------------------------------------------------------------------------------------------------ CE
def lowres_logits(B, n_cat, h, w, D, seed, scale, dev):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randn(B, h, w, D, generator=g)
    te = torch.randn(n_cat, D, generator=g)
    tok, te = tok / tok.norm(dim=-1, keepdim=True), te / te.norm(dim=-1, keepdim=True) * scale
    return tok.to(dev), te.to(dev)


def text_gemm(te, tok):
    """lo [B, n_cat, h, w] = te . tok, the criterion's call of zh_gemm_f32_strided (A k-contiguous, B k-contiguous)."""
    ops = _ops()
    B, h, w, D = tok.shape
    n_cat, hw = te.shape[0], h * w
    lo = torch.empty(B, n_cat, h, w, device=tok.device)
    ops.gemm_f32_strided(te, (0, D, 1), tok, (hw * D, D, 1), lo, (n_cat * hw, hw, 1), B, n_cat, hw, D)
    return lo


def run_ce(lo, labels, ignore_index, grad_out=1.0):
    ops = _ops()
    dev = lo.device
    out = torch.full((2,), float("nan"), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    lab = labels.to(dev).to(torch.int64).contiguous()
    lse = ops.upsample_ce_fwd(lo, lab, ignore_index, out, status)
    go = torch.tensor([grad_out], dtype=torch.float32, device=dev)
    dlo = ops.upsample_ce_bwd(lo, lab, lse, out, go, ignore_index, out=torch.full_like(lo, float("nan")))
    return out, int(status.item()), lse, dlo


def check_ce(lo, labels, ignore_index, te=None, grad_out=1.0):
    """Forward against the oracle with derived bounds; dlogits (and the token gradient through zh_gemm_f32_strided when te is given)
    per image to 1e-4 of the image's largest value."""
    out, status, lse, dlo = run_ce(lo, labels, ignore_index, grad_out)
    ref = ce_ref(lo, labels, ignore_index, grad_out)
    n_cat = lo.shape[1]
    count = ref["count"]
    assert int(out[1].item()) == count                      # integers: exact
    # lse: each upsampled logit v is 3 roundings off the float64 bilinear value (<= 3 u max|lo| after the softmax weighting);
    # the online sum s >= 1 takes n_cat adds / rescales, each with a rounding and an exp argument error (x e^-x <= 1/e), plus
    # __expf's own ~2 u: relative error of s <= n_cat (1 + 1/e + 2) u; then __logf and the add to the max: u (|lse| + 4)
    amax = float(lo.abs().max())
    ref_lse = ref["lse"]
    tol_lse = U * (3 * amax + 3.4 * n_cat + ref_lse.abs() + 4)
    d = (lse.double() - ref_lse).abs()
    assert bool((d <= tol_lse).all()), float((d - tol_lse).max())
    if count == 0:
        assert np.isnan(float(out[0].item()))
        assert bool((dlo == 0).all())
    else:
        # mean NLL: each pixel's nll = lse - v is off by tol_lse + 3 u amax; the fp32 block sum (6-level wave tree, 3 wave adds)
        # adds 9 u sum |nll| / count; the float64 reduction of the block partials does not count
        nll_tol = float(tol_lse.max()) + 3 * U * amax
        assert abs(float(out[0].item()) - ref["mean"]) <= nll_tol + 10 * U * (abs(ref["mean"]) + 2 * amax)
        for b in range(lo.shape[0]):
            r = ref["dlogits"][b]
            m = float(r.abs().max())
            assert float((dlo[b].double() - r).abs().max()) <= 1e-4 * m, b
            if m == 0:                                      # an image whose pixels are all ignored
                assert bool((dlo[b] == 0).all())
    if te is not None and count:
        ops = _ops()
        B, _, h, w = lo.shape
        D = te.shape[1]
        hw = h * w
        dtok = torch.empty(B, h, w, D, device=lo.device)
        ops.gemm_f32_strided(dlo, (n_cat * hw, 1, hw), te, (0, 1, D), dtok, (hw * D, D, 1), B, hw, D, n_cat)
        tref = torch.einsum("bnhw,nd->bhwd", ref["dlogits"], te.double())
        for b in range(B):
            m = float(tref[b].abs().max())
            assert float((dtok[b].double() - tref[b]).abs().max()) <= 1e-4 * m, b
    return out, status


def _labels(B, H, W, n_cat, seed, ignore_index=255, p_ignore=0.05):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, n_cat, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < p_ignore] = ignore_index
    return lab


@pytest.mark.parametrize("n_cat", [81, 920])
def test_ce_vitb32_training_shape(dev, n_cat):
    """B = 8, 24x24x512 tokens -> 384^2, the text GEMM of the criterion included."""
    tok, te = lowres_logits(8, n_cat, 24, 24, 512, seed=n_cat, scale=1.0, dev=dev)
    lo = text_gemm(te, tok)
    c64, bound = gemm_strided_ref(te, (0, 512, 1), tok, (576 * 512, 512, 1), 8, n_cat, 576, 512)
    assert bool(((lo.reshape(8, n_cat, 576).double() - c64).abs() <= 513 * U * bound).all())
    lab = _labels(8, 384, 384, n_cat, seed=2)
    lab[3, :5, :] = n_cat - 1
    _, status = check_ce(lo, lab, 255, te=te)
    assert status == 0


CE_GEOMETRIES = {
    "vitb16_48to384": (2, 81, 48, 48, 384, 384),
    "nonsquare_20x28to90x130": (2, 33, 20, 28, 90, 130),
    "identity_h_40x24to40x100": (2, 17, 40, 24, 40, 100),
    "down_40to30_x_20to70": (2, 17, 40, 20, 30, 70),
    "h1_1x13to37x52": (2, 17, 1, 13, 37, 52),
    "w1_9x1to45x17": (3, 16, 9, 1, 45, 17),
}


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("name", list(CE_GEOMETRIES))
def test_ce_geometries(dev, name, scale):
    B, n_cat, h, w, H, W = CE_GEOMETRIES[name]
    tok, te = lowres_logits(B, n_cat, h, w, 64, seed=4, scale=scale, dev=dev)
    lo = text_gemm(te, tok)
    _, status = check_ce(lo, _labels(B, H, W, n_cat, seed=5), 255, te=te)
    assert status == 0


@pytest.mark.parametrize("ignore_index", [255, -100, 0])
def test_ce_ignore_index_and_edge_labels(dev, ignore_index):
    """Labels at n_cat - 1, one image fully ignored among valid ones; with ignore_index = 0 class 0 is never a target."""
    B, n_cat = 3, 21
    tok, te = lowres_logits(B, n_cat, 12, 15, 32, seed=9, scale=30.0, dev=dev)
    lo = text_gemm(te, tok)
    lab = _labels(B, 70, 77, n_cat, seed=6, ignore_index=ignore_index, p_ignore=0.2)
    lab[0, 10:30, :] = n_cat - 1
    lab[1] = ignore_index
    out, status = check_ce(lo, lab, ignore_index, te=te, grad_out=0.5)
    assert status == 0


def test_ce_label_equal_to_n_cat_is_flagged_and_ignored(dev):
    B, n_cat = 2, 11
    tok, te = lowres_logits(B, n_cat, 10, 10, 16, seed=2, scale=1.0, dev=dev)
    lo = text_gemm(te, tok)
    lab = _labels(B, 50, 50, n_cat, seed=3)
    assert run_ce(lo, lab, 255)[1] == 0
    lab[1, 7, 9] = n_cat
    lab[0, 0, 0] = -1
    out, status = check_ce(lo, lab, 255)                    # the oracle ignores both pixels: so must the kernels
    assert status & _ops().STATUS_LABEL


def test_ce_all_labels_ignored(dev):
    tok, te = lowres_logits(2, 7, 8, 8, 16, seed=1, scale=1.0, dev=dev)
    lo = text_gemm(te, tok)
    out, status = check_ce(lo, torch.full((2, 40, 40), 255), 255)
    assert status == 0 and float(out[1].item()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------- GEMM
def _operand(batch, rows, K, kcontig, shared, g, dev):
    """A [batch or 1, rows, K] operand in a padded buffer, k-contiguous (row stride K + 3) or not (k stride rows + 5); returns
    (buffer, (batch stride, row stride, k stride))."""
    if kcontig:
        rs, ks = K + 3, 1
        plane = rows * rs
    else:
        rs, ks = 1, rows + 5
        plane = K * ks
    nb = 1 if shared else batch
    buf = torch.randn(nb * plane + 7, generator=g).to(dev)
    return buf, (0 if shared else plane, rs, ks)


@pytest.mark.parametrize("a_kc,b_kc", [(True, True), (True, False), (False, True), (False, False)])
def test_gemm_f32_strided_layouts_and_edges(dev, a_kc, b_kc):
    """C[t](m, n) = sum_k A[t](m, k) B[t](n, k) into a column-major view of a larger sentinel-filled buffer; B shared across the batch
    or A (batch stride 0).  Per element |C - C64| <= (K + 1) u sum_k |a b| (a chain of K fmas from 0)."""
    ops = _ops()
    g = torch.Generator().manual_seed(int(a_kc) * 2 + int(b_kc))
    batch = 2
    for M in (1, 63, 64, 65, 130):
        for N in (1, 63, 64, 65, 130):
            for K in (1, 15, 16, 17, 920):
                A, sa = _operand(batch, M, K, a_kc, a_kc and b_kc, g, dev)
                Bm, sb = _operand(batch, N, K, b_kc, not (a_kc and b_kc), g, dev)
                sc = ((M + 3) * N + 5, 1, M + 3)                # C[t](m, n) at t sc0 + m + n (M + 3): gaps between columns
                C = torch.full((batch * sc[0] + 5,), -7.25e30, device=dev)
                ops.gemm_f32_strided(A, sa, Bm, sb, C, sc, batch, M, N, K)
                c64, bound = gemm_strided_ref(A, sa, Bm, sb, batch, M, N, K)
                view = torch.as_strided(C, (batch, M, N), (sc[0], sc[1], sc[2]))
                err = (view.double() - c64).abs()
                assert bool((err <= (K + 1) * U * bound).all()), (M, N, K, float(err.max()))
                mask = torch.ones_like(C, dtype=torch.bool)
                torch.as_strided(mask, (batch, M, N), (sc[0], sc[1], sc[2])).fill_(False)
                assert bool((C[mask] == -7.25e30).all()), (M, N, K)


# ------------------------------------------------------------------------------------------------------------- reproducibility
def test_every_entry_point_is_bitwise_repeatable(dev):
    """The header promises fixed-order sums: two runs of each entry point at the ViT-B/32 training shape are bitwise equal."""
    props, gts = _props_gts(8, 6, 100, 24, 24, 384, 384, seed=11, dev=dev)
    tok, te = lowres_logits(8, 81, 24, 24, 512, seed=3, scale=1.0, dev=dev)
    lab = _labels(8, 384, 384, 81, seed=4)
    runs = []
    for _ in range(2):
        o = run_cost(props, gts, dev)
        ref_pairs = []
        for b in range(8):
            n_b = int(o["off"][b + 1] - o["off"][b])
            ref_pairs += [(b, l, i, i) for l in range(6) for i in range(n_b)]
        gm = run_grad(props, o, ref_pairs, dev, scale=1.0 / 8)
        lo = text_gemm(te, tok)
        ce, _, lse, dlo = run_ce(lo, lab, 255)
        runs.append([o["costs"], o["stat_p"], o["stat_pg"], o["stat_g"], o["skip"], gm, lo, ce, lse, dlo])
    for k, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), k


# ----------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(dev):
    from zutis_amd import _lib
    ops = _ops()
    # cost kernel: two 96x96 planes do not fit the 64 KiB LDS
    props, gts = _props_gts(1, 1, 2, 96, 96, 192, 192, seed=1, dev=dev)
    with pytest.raises(_lib.ZutisHipError, match="proposal plane 96x96 too large for LDS"):
        run_cost(props, gts, dev)
    # CE backward: 16 full-resolution rows of W = 1100 do not fit
    lo = torch.zeros(1, 3, 4, 10, device=dev)
    lab = torch.zeros(1, 8, 1100, dtype=torch.int64, device=dev)
    out = torch.zeros(2, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    lse = ops.upsample_ce_fwd(lo, lab, 255, out, st)
    with pytest.raises(_lib.ZutisHipError, match="W = 1100 too large for LDS"):
        ops.upsample_ce_bwd(lo, lab, lse, out, torch.ones(1, device=dev), 255)
    # a workspace one float short
    L = _lib.load()
    from zutis_amd.criterion import _pack_gt
    props, gts = _props_gts(2, 1, 3, 12, 12, 60, 60, seed=2, dev=dev)
    inst_off, gt_u8, off, H, W = _pack_gt(gts, dev)
    n_max = int(np.diff(off).max())
    need = int(L.zh_mask_match_cost_workspace_size(2, 1, 3, H, n_max))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    f = torch.empty(64, device=dev)
    sk = torch.empty(2, dtype=torch.int32, device=dev)
    p = ops._p
    rc = L.zh_mask_match_cost(p(props), p(gt_u8), p(inst_off), p(f), p(f), p(f), p(f), p(sk), p(st), 2, 1, 3, 12, 12, H, W, n_max,
                              1.0, 1.0, ops.lin_scale(12, H), ops.lin_scale(12, W), p(ws), need - 4, ops._stream())
    with pytest.raises(_lib.ZutisHipError, match="workspace too small"):
        _lib.check(rc, "zh_mask_match_cost")
    need = int(L.zh_upsample_ce_workspace_size(1, 8, 1100))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = L.zh_upsample_ce_fwd(p(lo), p(lab), p(lse), p(out), p(st), 1, 3, 4, 10, 8, 1100, 255, ops.lin_scale(4, 8),
                              ops.lin_scale(10, 1100), p(ws), need - 4, ops._stream())
    with pytest.raises(_lib.ZutisHipError, match="workspace too small"):
        _lib.check(rc, "zh_upsample_ce_fwd")
