"""float64 restatement of the training criterion (dice + BCE Hungarian-matched mask loss, CE on upsampled text logits), in the
contraction form: per (image, layer) only [Q, H*W] upsampled proposals exist, never [Q, n, H*W] copies, and the CE logits are
upsampled per image from the low-res einsum.  Gradients come from torch autograd, one (image, layer) / image at a time so that
the peak memory stays at one such slice.  Runs on whatever device the inputs are on."""
from __future__ import annotations

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment


def interp_matrix(n_in: int, n_out: int, device) -> torch.Tensor:
    """[n_out, n_in] float64 matrix of F.interpolate(size=, bilinear, align_corners=False) along one axis, with the sample positions
    of an fp32 tensor (scale = float32(in) / float32(out), src = max(scale * (d + 0.5) - 0.5, 0) in float32, as ATen)."""
    M = np.zeros((n_out, n_in), np.float64)
    if n_in == n_out:
        return torch.eye(n_in, dtype=torch.float64, device=device)
    scale = np.float32(n_in) / np.float32(n_out)
    d = np.arange(n_out, dtype=np.float32)
    src = np.maximum(scale * (d + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = np.clip(src - i0.astype(np.float32), 0, 1).astype(np.float32)
    l0 = np.float32(1) - l1
    np.add.at(M, (np.arange(n_out), i0), l0.astype(np.float64))
    np.add.at(M, (np.arange(n_out), i1), l1.astype(np.float64))
    return torch.from_numpy(M).to(device)


def upsample(x: torch.Tensor, My: torch.Tensor, Mx: torch.Tensor) -> torch.Tensor:
    """[..., h, w] -> [..., H, W] bilinear (the contraction My x Mx^T)."""
    return My @ x @ Mx.T


def costs_of(p_up, g, wd, wb):
    """p_up [Q, HW] in [0, 1], g [n, HW] binary -> [n, Q] weighted dice + BCE cost."""
    HW = p_up.shape[-1]
    sp, sg = p_up.sum(-1), g.sum(-1)
    spg = g @ p_up.T
    A = torch.clamp(torch.log(p_up), min=-100.0)
    Bv = torch.clamp(torch.log1p(-p_up), min=-100.0)
    dice = 1.0 - (2.0 * spg + 1.0) / (sp[None, :] + sg[:, None] + 1.0)
    bce = -(Bv.sum(-1)[None, :] + g @ (A - Bv).T) / HW
    return wd * dice + wb * bce


def criterion_ref(props, gts, tokens, sem, te, weight_ce_loss=1.0, weight_mask_loss=1.0, weight_dice_loss=1.0,
                  weight_bce_loss=1.0, ignore_index=255, grads=True, images_for_grads=None):
    """props [b, (L,) Q, h, w]; gts list of [n_i, H, W]; tokens [b, h2, w2, D]; sem [b, H, W]; te [n_cat, D].
    Returns dict(costs {(b, l): float64 [n, Q]}, matches {(b, l): (rows, cols)}, ce, mask, loss, grad_props, grad_tokens).
    images_for_grads: restrict the backward passes to these images (the values still cover the whole batch)."""
    dev = props.device
    p = props.detach().to(torch.float64)
    p5 = p.unsqueeze(1) if p.dim() == 4 else p
    B, L, Q, h, w = p5.shape
    tok = tokens.detach().to(torch.float64)
    te64 = te.detach().to(device=dev, dtype=torch.float64)
    H, W = gts[0].shape[-2:]
    sem = sem.to(dev).to(torch.int64)
    gp = torch.zeros_like(p5)
    gt_ = torch.zeros_like(tok)
    gsel = range(B) if images_for_grads is None else images_for_grads

    h2, w2 = tok.shape[1:3]
    Ty, Tx, My, Mx = interp_matrix(h2, H, dev), interp_matrix(w2, W, dev), interp_matrix(h, H, dev), interp_matrix(w, W, dev)
    # CE: mean over the non-ignored pixels of the whole batch
    count = int((sem != ignore_index).sum())
    nll_total = 0.0
    for b in range(B):
        t = tok[b].clone().requires_grad_(grads and b in gsel)
        lo = torch.einsum("nc,hwc->nhw", te64, t)
        up = upsample(lo, Ty, Tx)
        lab = sem[b]
        valid = lab != ignore_index
        lsm = torch.log_softmax(up, dim=0)
        nll = -(lsm.gather(0, torch.where(valid, lab, 0)[None])[0] * valid).sum()
        nll_total += float(nll.detach())
        if grads and b in gsel and count > 0:
            (weight_ce_loss * nll / count).backward()
            gt_[b] = t.grad
        del lo, up, lsm
    ce = nll_total / count if count > 0 else float("nan")

    costs, matches = {}, {}
    mask_total = 0.0
    for b in range(B):
        g = gts[b].to(dev).to(torch.float64).reshape(gts[b].shape[0], -1)
        if g.sum() == 0:
            continue
        for l in range(L):
            pl = p5[b, l].clone().requires_grad_(grads and b in gsel)
            up = upsample(pl, My, Mx).reshape(Q, -1)
            cm = costs_of(up, g, weight_dice_loss, weight_bce_loss)
            cmh = cm.detach().cpu().numpy()
            r, c = linear_sum_assignment(cmh)
            costs[(b, l)], matches[(b, l)] = cmh, (r, c)
            term = cm[torch.as_tensor(r, device=dev), torch.as_tensor(c, device=dev)].sum()
            mask_total += float(term.detach())
            if grads and b in gsel:
                (weight_mask_loss / B * term).backward()
                gp[b, l] = pl.grad
            del up, cm
    mask = mask_total / B
    return {"costs": costs, "matches": matches, "ce": ce, "mask": mask, "loss": weight_mask_loss * mask + weight_ce_loss * ce,
            "grad_props": gp.reshape(props.shape), "grad_tokens": gt_}


def unique_margin(cm: np.ndarray) -> float:
    """How much worse the second-best assignment of cost matrix cm is than the best (every other assignment drops a best pair)."""
    r, c = linear_sum_assignment(cm)
    best = cm[r, c].sum()
    gap = np.inf
    for i, q in zip(r, c):
        alt = cm.astype(np.float64).copy()
        alt[i, q] = 1e9
        r2, c2 = linear_sum_assignment(alt)
        gap = min(gap, alt[r2, c2].sum() - best)
    return float(gap)
