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


# ---------------------------------------------------------------------------------------------------------------------------------
# Kernel-level float64 oracles: one per entry point of csrc/criterion.hip, on the kernels' own fp32 sample weights and positions
# (oracle.resample.linear_index_weights, the fma included).  Every full-resolution proposal value is the fp32 value the kernels
# interpolate (bilinear_nchw's arithmetic), taken to float64 only afterwards: at saturation the BCE gradient
# (p - g) / max(p (1 - p), 1e-12) is defined by that fp32 value alone.
# ---------------------------------------------------------------------------------------------------------------------------------

def lin_matrix(n_in: int, n_out: int, device="cpu") -> torch.Tensor:
    """[n_out, n_in] float64 matrix of the kernels' bilinear weights along one axis (linear_index_weights)."""
    from oracle.resample import linear_index_weights
    i0, i1, l0, l1 = linear_index_weights(n_in, n_out)
    M = np.zeros((n_out, n_in), np.float64)
    np.add.at(M, (np.arange(n_out), i0), l0.astype(np.float64))
    np.add.at(M, (np.arange(n_out), i1), l1.astype(np.float64))
    return torch.from_numpy(M).to(device)


def adjoint(G: torch.Tensor, My: torch.Tensor, Mx: torch.Tensor) -> torch.Tensor:
    """[..., H, W] -> [..., h, w]: the adjoint of the bilinear upsample, My^T G Mx."""
    return My.T @ G @ Mx


def _fma(a, b, c):
    # oracle.resample.fma on torch tensors: the product of two fp32 values is exact in float64
    return (a.double() * b.double() + c.double()).float()


def up_f32(x: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """[..., h, w] fp32 -> [..., H, W] fp32 with the arithmetic of oracle.resample.bilinear_nchw (pinned bitwise to it by
    tests/test_criterion_cpu.py), on the tensor's device."""
    from oracle.resample import linear_index_weights
    dev = x.device
    y0, y1, ly0, ly1 = (torch.from_numpy(a).to(dev) for a in linear_index_weights(x.shape[-2], H))
    x0, x1, lx0, lx1 = (torch.from_numpy(a).to(dev) for a in linear_index_weights(x.shape[-1], W))
    x = x.to(torch.float32)
    top, bot = x[..., y0, :], x[..., y1, :]
    r0 = _fma(top[..., x0], lx0, top[..., x1] * lx1)
    r1 = _fma(bot[..., x0], lx0, bot[..., x1] * lx1)
    return _fma(r0, ly0[:, None], r1 * ly1[:, None])


def match_terms(p: torch.Tensor, g: torch.Tensor, wd: float = 1.0, wb: float = 1.0):
    """Full resolution, float64: p [Q, HW] in [0, 1], g [n, HW] binary -> (cost [n, Q], sum p [Q], sum g.p [n, Q], sum g [n]).
    cost = wd * dice + wb * mean BCE with torch's -100 log clamp, each pixel's loss taken whole (g ? log p : log(1 - p))."""
    HW = p.shape[-1]
    sp, sg, spg = p.sum(-1), g.sum(-1), g @ p.T
    A = torch.clamp(torch.log(p), min=-100.0)
    Bv = torch.clamp(torch.log(1.0 - p), min=-100.0)
    dice = 1.0 - (2.0 * spg + 1.0) / (sp[None, :] + sg[:, None] + 1.0)
    bce = -(g @ A.T + (1.0 - g) @ Bv.T) / HW
    return wd * dice + wb * bce, sp, spg, sg


BCE_EPS = float(np.float32(1e-12))


def match_grad(p: torch.Tensor, g: torch.Tensor, rows, cols, wd: float = 1.0, wb: float = 1.0) -> torch.Tensor:
    """Full resolution, float64: d/dp of sum over the pairs (instance rows[k], query cols[k]) of match_terms' cost -> [Q, HW].
    The BCE part is torch's binary_cross_entropy_backward, (p - g) / max(p (1 - p), eps) / HW (the -100 log clamp does not enter),
    with torch's eps, the fp32 value of 1e-12 (as the kernel's 1e-12f), in every dtype."""
    HW = p.shape[-1]
    out = torch.zeros_like(p)
    sp, sg = p.sum(-1), g.sum(-1)
    for i, q in zip(rows, cols):
        gi, pq = g[i], p[q]
        D = sp[q] + sg[i] + 1.0
        N = 2.0 * (gi @ pq) + 1.0
        out[q] += wd * (N - 2.0 * gi * D) / (D * D) + wb * (pq - gi) / torch.clamp((1.0 - pq) * pq, min=BCE_EPS) / HW
    return out


def mask_cost_ref(props: torch.Tensor, gts, wd: float = 1.0, wb: float = 1.0):
    """zh_mask_match_cost in float64.  props fp32 [B, L, Q, h, w]; gts list of [n_b, H, W] -> dict(costs {b: [L, n_b, Q]},
    stat_p [B, L, Q], stat_pg {b: [L, n_b, Q]}, stat_g [n_tot], skip [B] bool (an image whose masks are all empty))."""
    B, L, Q = props.shape[:3]
    H, W = gts[0].shape[-2:]
    dev = props.device
    stat_p = torch.zeros(B, L, Q, dtype=torch.float64, device=dev)
    costs, stat_pg, stat_g, skip = {}, {}, [], []
    for b in range(B):
        g = gts[b].to(dev).flatten(1).ne(0).to(torch.float64)
        stat_g.append(g.sum(-1))
        skip.append(bool(g.sum() == 0))
        cs, pgs = [], []
        for l in range(L):
            p = up_f32(props[b, l], H, W).reshape(Q, -1).double()
            c, sp, spg, _ = match_terms(p, g, wd, wb)
            stat_p[b, l] = sp
            cs.append(c)
            pgs.append(spg)
        costs[b], stat_pg[b] = torch.stack(cs), torch.stack(pgs)
    return {"costs": costs, "stat_p": stat_p, "stat_pg": stat_pg, "stat_g": torch.cat(stat_g), "skip": skip}


def mask_grad_ref(props: torch.Tensor, gts, pairs, wd: float = 1.0, wb: float = 1.0, scale: float = 1.0) -> torch.Tensor:
    """zh_mask_match_grad in float64: pairs (b, l, q, i) -> scale * d/dprops of the sum of their costs, [B, L, Q, h, w]
    (0 outside the paired planes)."""
    B, L, Q, h, w = props.shape
    H, W = gts[0].shape[-2:]
    dev = props.device
    My, Mx = lin_matrix(h, H, dev), lin_matrix(w, W, dev)
    out = torch.zeros(B, L, Q, h, w, dtype=torch.float64, device=dev)
    by = {}
    for b, l, q, i in pairs:
        by.setdefault((int(b), int(l)), []).append((int(i), int(q)))
    for (b, l), iq in by.items():
        g = gts[b].to(dev).flatten(1).ne(0).to(torch.float64)
        p = up_f32(props[b, l], H, W).reshape(Q, -1).double()
        rows, cols = zip(*iq)
        G = match_grad(p, g, rows, cols, wd, wb).reshape(Q, H, W)
        out[b, l] = adjoint(G, My, Mx) * scale
    return out


def ce_ref(logits_lo: torch.Tensor, labels: torch.Tensor, ignore_index: int = 255, grad_out: float = 1.0):
    """zh_upsample_ce_fwd / _bwd in float64.  logits_lo [B, n_cat, h, w]; labels int [B, H, W] -> dict(lse [B, H, W], mean, count,
    dlogits [B, n_cat, h, w] = d (grad_out * mean) / d logits_lo).  A label is used when it is not ignore_index and lies in
    [0, n_cat) (the kernels flag any other one and skip it); with no such label the mean is NaN and the count 0 (torch's mean over
    an empty set) and dlogits is 0."""
    B, n, h, w = logits_lo.shape
    H, W = labels.shape[-2:]
    dev = logits_lo.device
    Ty, Tx = lin_matrix(h, H, dev), lin_matrix(w, W, dev)
    lab = labels.to(dev).to(torch.int64)
    valid = (lab != ignore_index) & (lab >= 0) & (lab < n)
    count = int(valid.sum())
    lse = torch.empty(B, H, W, dtype=torch.float64, device=dev)
    dlo = torch.zeros(B, n, h, w, dtype=torch.float64, device=dev)
    total = 0.0
    for b in range(B):
        up = Ty @ logits_lo[b].double() @ Tx.T
        lse[b] = torch.logsumexp(up, 0)
        li = torch.where(valid[b], lab[b], 0)
        total += float(((lse[b] - up.gather(0, li[None])[0]) * valid[b]).sum())
        if count:
            G = torch.exp(up - lse[b])
            G.scatter_add_(0, li[None], -torch.ones_like(G[:1]))
            dlo[b] = adjoint(G * valid[b] * (grad_out / count), Ty, Tx)
        del up
    return {"lse": lse, "mean": total / count if count else float("nan"), "count": count, "dlogits": dlo}


def gemm_strided_ref(A: torch.Tensor, a_strides, Bm: torch.Tensor, b_strides, batch: int, M: int, N: int, K: int):
    """zh_gemm_f32_strided in float64: C[t](m, n) = sum_k A[t](m, k) B[t](n, k), strides (batch, row, k) in elements from the
    start of A / Bm.  Returns (C [batch, M, N], sum_k |A B| [batch, M, N], the scale of fp32 rounding errors)."""
    a = torch.as_strided(A.double(), (batch, M, K), a_strides)
    b = torch.as_strided(Bm.double(), (batch, N, K), b_strides)
    return a @ b.transpose(1, 2), a.abs() @ b.abs().transpose(1, 2)
