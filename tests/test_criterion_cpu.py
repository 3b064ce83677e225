"""CPU: the float64 restatement of the training criterion (tests/_criterion_ref.py) against the reference's recorded outputs
(tests/golden/criterion.npz, tools/gen_criterion_golden.py), the drop-in's signatures, and the drop-in's refusal of CPU tensors.
The kernel-level oracles of tests/_criterion_ref.py (used by tests/test_criterion_kernels_gpu.py) are pinned here to torch autograd of
the reference's formulas, to oracle.resample.bilinear_nchw, to an adjoint dot-product test and to the recorded outputs."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

from tests._criterion_ref import (adjoint, ce_ref, criterion_ref, lin_matrix, mask_cost_ref, mask_grad_ref, match_grad, match_terms,
                                  up_f32)

WEIGHTS = {"default": {}, "custom": dict(weight_ce_loss=0.7, weight_mask_loss=1.3, weight_dice_loss=0.6, weight_bce_loss=1.7)}


def load_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "criterion.npz"))
    counts = z["gt_counts"].tolist()
    gt = torch.from_numpy(z["gt_u8"])
    gts = list(torch.split(gt, counts))
    return z, torch.from_numpy(z["props"]), gts, torch.from_numpy(z["tokens"]), torch.from_numpy(z["sem"]).long(), torch.from_numpy(z["te"])


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("tag", list(WEIGHTS))
def test_restatement_matches_reference_golden(golden_dir, tag):
    z, props, gts, tok, sem, te = load_golden(golden_dir)
    r = criterion_ref(props, gts, tok, sem, te, **WEIGHTS[tag])
    keys = sorted(k for k in z.files if k.startswith(f"{tag}_cost_"))
    assert len(keys) == 4 and sorted(r["costs"]) == sorted(tuple(int(v) for v in k.split("_")[-2:]) for k in keys)
    for k in keys:
        b, l = (int(v) for v in k.split("_")[-2:])
        assert np.abs(r["costs"][(b, l)] - z[k]).max() <= 1e-5, k
        rows, cols = r["matches"][(b, l)]
        assert np.array_equal(rows, z[f"{tag}_rows_{b}_{l}"]) and np.array_equal(cols, z[f"{tag}_cols_{b}_{l}"]), k
    assert abs(r["ce"] - float(z[f"{tag}_ce_loss"])) <= 1e-5
    assert abs(r["mask"] - float(z[f"{tag}_mask_loss"])) <= 1e-5
    assert abs(r["loss"] - float(z[f"{tag}_loss"])) <= 1e-5
    assert rel(r["grad_props"], z[f"{tag}_grad_props"]) <= 1e-5
    assert rel(r["grad_tokens"], z[f"{tag}_grad_tokens"]) <= 1e-5


def test_dropin_signatures_equal_the_reference(golden_dir):
    from zutis_amd.dropin.criterion import Criterion
    z = np.load(os.path.join(golden_dir, "criterion.npz"))
    want = json.loads(str(z["signatures"]))
    for fn in ("__init__", "__call__"):
        ps = inspect.signature(getattr(Criterion, fn)).parameters.values()
        got = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)] for p in ps]
        assert got == want[fn], fn


def test_dropin_refuses_cpu_tensors(golden_dir):
    from zutis_amd import _lib
    from zutis_amd.dropin.criterion import Criterion
    z, props, gts, tok, sem, te = load_golden(golden_dir)
    crit = Criterion(te)
    assert crit.text_embeddings is te and crit.ignore_index == 255
    with pytest.raises(_lib.ZutisHipError, match="no CPU fallback"):
        crit(props, gts, [[0] * int(g.shape[0]) for g in gts], tok, sem)


def test_dropin_refuses_batch_mismatches_before_any_launch(golden_dir):
    """Every per-image input must cover the proposals' batch: the kernels index GT offsets, tokens and labels by image.  The checks
    run on the host before the device check, so they hold for CPU tensors too."""
    from zutis_amd import _lib
    from zutis_amd.dropin.criterion import Criterion
    z, props, gts, tok, sem, te = load_golden(golden_dir)
    crit = Criterion(te)
    cats = [[0] * int(g.shape[0]) for g in gts]
    with pytest.raises(_lib.ZutisHipError, match="ground-truth instance mask tensors for a batch of 3"):
        crit(props, gts[:-1], cats, tok, sem)
    with pytest.raises(_lib.ZutisHipError, match="patch tokens must be"):
        crit(props, gts, cats, tok[:-1], sem)
    with pytest.raises(_lib.ZutisHipError, match="patch tokens must be"):
        crit(props, gts, cats, tok[0], sem)
    with pytest.raises(_lib.ZutisHipError, match="semantic masks must be"):
        crit(props, gts, cats, tok, sem[:-1])
    with pytest.raises(_lib.ZutisHipError, match="text embeddings must be"):
        Criterion(te[None])(props, gts, cats, tok, sem)
    with pytest.raises(_lib.ZutisHipError, match="text embeddings must be"):
        Criterion(te[:, :-1])(props, gts, cats, tok, sem)


# ------------------------------------------------------------------------------------------------- pins of the kernel-level oracles
def _dice_loss(dt, gt):
    """The reference's dice_loss (criterion.py): dt [Q, HW], gt [n, HW] -> [Q, n]."""
    numerator = 2 * torch.einsum("nc,mc->nm", dt, gt)
    denominator = dt.sum(-1)[:, None] + gt.sum(-1)[None, :]
    return 1 - (numerator + 1) / (denominator + 1)


def _bce_loss(dt, gt):
    """The reference's binary_cross_entropy_loss: [Q, n] mean over the pixels of F.binary_cross_entropy(reduction="none")."""
    return F.binary_cross_entropy(dt[:, None].repeat(1, gt.shape[0], 1), gt[None].repeat(dt.shape[0], 1, 1), reduction="none").mean(-1)


@pytest.mark.parametrize("wd,wb", [(1.0, 1.0), (0.6, 1.7)])
def test_match_terms_equal_autograd_of_the_reference_formulas(wd, wb):
    """Full resolution, float64, proposals with exact 0.0 and 1.0 on and off the GT: values and gradients of the oracle's closed
    forms equal torch autograd of the reference's dice + BCE (the -100 log clamp, the 1e-12 clamp of BCE's backward)."""
    g = torch.Generator().manual_seed(0)
    Q, n, HW = 7, 4, 300
    p = torch.rand(Q, HW, generator=g, dtype=torch.float64)
    p[0, :120], p[1, 60:200], p[2, ::3] = 1.0, 0.0, 1.0
    p[3, ::5] = 0.0
    gt = (torch.rand(n, HW, generator=g) < 0.4).to(torch.float64)
    gt[0, :100] = 1.0
    gt[1, 60:200] = 1.0
    pr = p.clone().requires_grad_(True)
    cost = (wd * _dice_loss(pr, gt) + wb * _bce_loss(pr, gt)).T
    c, sp, spg, sg = match_terms(p, gt, wd, wb)
    assert torch.allclose(c, cost.detach(), rtol=1e-13, atol=1e-13)
    assert torch.equal(sp, p.sum(-1)) and torch.equal(sg, gt.sum(-1)) and torch.allclose(spg, gt @ p.T, rtol=1e-15, atol=0)
    rows, cols = [0, 1, 2, 3], [0, 1, 2, 5]                   # saturated planes on and off their GT, and an unsaturated one
    cost[rows, cols].sum().backward()
    gr = match_grad(p, gt, rows, cols, wd, wb)
    assert float(pr.grad.abs().max()) > 0.5e12 / HW           # 1 / 1e-12 where p is exactly 0 or 1 against the other label
    assert torch.allclose(gr, pr.grad, rtol=1e-12, atol=1e-12 * float(pr.grad.abs().max()))
    assert bool((gr[[4, 6]] == 0).all())


@pytest.mark.parametrize("ignore_index", [255, -100, 0])
def test_ce_oracle_equals_torch_cross_entropy(ignore_index):
    g = torch.Generator().manual_seed(1)
    B, n, h, w, H, W = 2, 6, 5, 7, 23, 31
    lo = torch.randn(B, n, h, w, generator=g, dtype=torch.float64) * 4
    lab = torch.randint(0, n, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < 0.3] = ignore_index
    lab[1, :4] = n - 1
    Ty, Tx = lin_matrix(h, H), lin_matrix(w, W)
    lr = lo.clone().requires_grad_(True)
    up = Ty @ lr @ Tx.T
    loss = F.cross_entropy(up, lab, ignore_index=ignore_index)
    (0.7 * loss).backward()
    r = ce_ref(lo, lab, ignore_index, grad_out=0.7)
    assert r["count"] == int((lab != ignore_index).sum())
    assert abs(r["mean"] - float(loss.detach())) <= 1e-13 * abs(float(loss.detach()))
    assert torch.allclose(r["lse"], torch.logsumexp(up.detach(), 1), rtol=1e-14, atol=0)
    assert torch.allclose(r["dlogits"], lr.grad, rtol=1e-12, atol=1e-14)
    allign = torch.full_like(lab, ignore_index)
    lr.grad = None
    F.cross_entropy(Ty @ lr @ Tx.T, allign, ignore_index=ignore_index).backward()
    r = ce_ref(lo, allign, ignore_index)
    assert r["count"] == 0 and np.isnan(r["mean"]) and np.isnan(float(F.cross_entropy(up.detach(), allign, ignore_index=ignore_index)))
    assert bool((r["dlogits"] == 0).all()) and bool((lr.grad == 0).all())


def _up64(x, H, W):
    """Float64 bilinear upsample by gathering the two taps of linear_index_weights along each axis (no matrix)."""
    from oracle.resample import linear_index_weights
    y0, y1, ly0, ly1 = linear_index_weights(x.shape[-2], H)
    x0, x1, lx0, lx1 = linear_index_weights(x.shape[-1], W)
    ly0, ly1, lx0, lx1 = (torch.from_numpy(a).double() for a in (ly0, ly1, lx0, lx1))
    r = x[..., y0, :] * ly0[:, None] + x[..., y1, :] * ly1[:, None]
    return r[..., x0] * lx0 + r[..., x1] * lx1


AXES = [(24, 384, 24, 384), (40, 40, 24, 100), (40, 30, 20, 70), (1, 13, 9, 1), (20, 90, 28, 130)]


@pytest.mark.parametrize("h,H,w,W", AXES)
def test_adjoint_dot_product(h, H, w, W):
    """<My x Mx^T, G> = <x, My^T G Mx> for ratios 16, 1 (identity), 0.75 (downsampling) and a low-res size of 1; the forward is
    the two-tap gather, the adjoint the dense matrices."""
    g = torch.Generator().manual_seed(h * 1000 + W)
    x = torch.randn(3, h, w, generator=g, dtype=torch.float64)
    G = torch.randn(3, H, W, generator=g, dtype=torch.float64)
    My, Mx = lin_matrix(h, H), lin_matrix(w, W)
    up = _up64(x, H, W)
    assert torch.allclose(up, My @ x @ Mx.T, rtol=0, atol=1e-14)
    lhs = float((up * G).sum())
    rhs = float((x * adjoint(G, My, Mx)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    assert torch.allclose(My.sum(1), torch.ones(H, dtype=torch.float64), rtol=0, atol=1e-7)   # fp32 weights: l0 + l1 == 1 to 1 ulp


@pytest.mark.parametrize("h,H,w,W", AXES)
def test_up_f32_is_bitwise_bilinear_nchw(h, H, w, W):
    """up_f32 (torch, any device) is oracle.resample.bilinear_nchw, bit for bit, exact 0.0 and 1.0 included."""
    from oracle.resample import bilinear_nchw
    g = torch.Generator().manual_seed(h + W)
    x = torch.rand(2, 3, h, w, generator=g)
    x[0, 0] = 1.0
    x[1, 1, : max(1, h // 2)] = 0.0
    want = bilinear_nchw(x.numpy(), H, W)
    got = up_f32(x, H, W).numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("tag", list(WEIGHTS))
def test_kernel_oracles_reproduce_reference_golden(golden_dir, tag):
    """mask_cost_ref + Hungarian + mask_grad_ref + ce_ref, composed as the criterion, meet the golden file within the bounds of
    test_restatement_matches_reference_golden."""
    z, props, gts, tok, sem, te = load_golden(golden_dir)
    kw = dict(weight_ce_loss=1.0, weight_mask_loss=1.0, weight_dice_loss=1.0, weight_bce_loss=1.0)
    kw.update(WEIGHTS[tag])
    B, L = props.shape[:2]
    ref = mask_cost_ref(props, gts, kw["weight_dice_loss"], kw["weight_bce_loss"])
    keys = sorted(k for k in z.files if k.startswith(f"{tag}_cost_"))
    assert sorted((b, l) for b in range(B) if not ref["skip"][b] for l in range(L)) == \
        sorted(tuple(int(v) for v in k.split("_")[-2:]) for k in keys)
    pairs, mask = [], 0.0
    for k in keys:
        b, l = (int(v) for v in k.split("_")[-2:])
        cm = ref["costs"][b][l].numpy()
        assert np.abs(cm - z[k]).max() <= 1e-5, k
        rows, cols = linear_sum_assignment(cm)
        assert np.array_equal(rows, z[f"{tag}_rows_{b}_{l}"]) and np.array_equal(cols, z[f"{tag}_cols_{b}_{l}"]), k
        mask += float(cm[rows, cols].sum())
        pairs += [(b, l, int(q), int(i)) for i, q in zip(rows, cols)]
    mask /= B
    gp = mask_grad_ref(props, gts, pairs, kw["weight_dice_loss"], kw["weight_bce_loss"], kw["weight_mask_loss"] / B)
    te64 = te.double()
    lo = torch.einsum("nc,bhwc->bnhw", te64, tok.double())
    ce = ce_ref(lo, sem, 255, grad_out=kw["weight_ce_loss"])
    gt_ = torch.einsum("bnhw,nc->bhwc", ce["dlogits"], te64)
    assert abs(ce["mean"] - float(z[f"{tag}_ce_loss"])) <= 1e-5
    assert abs(mask - float(z[f"{tag}_mask_loss"])) <= 1e-5
    assert abs(kw["weight_mask_loss"] * mask + kw["weight_ce_loss"] * ce["mean"] - float(z[f"{tag}_loss"])) <= 1e-5
    assert rel(gp, z[f"{tag}_grad_props"]) <= 1e-5
    assert rel(gt_, z[f"{tag}_grad_tokens"]) <= 1e-5
