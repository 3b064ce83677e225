"""The training criterion (criterion.py::Criterion, called by every Trainer.fit step, trainer.py:105-160) on HIP kernels.

The reference materialises the upsampled patch tokens (8 x 512 x 384^2 fp32 at the shipped configs), the full-resolution logits
and, per (image, decoder layer), BCE on repeat()-ed [Q, n, H*W] copies of proposals and GT masks that autograd keeps until
backward.  Here (csrc/criterion.hip):

  * the matching costs of every (image, layer) come from one launch of zh_mask_match_cost, which interpolates the low-res
    proposals on the fly and reduces four sums per (instance, query);
  * the CE term is upsample(te . tok): a low-res GEMM (zh_gemm_f32_strided), then zh_upsample_ce_fwd (upsample -> log-sum-exp
    -> NLL, ignore_index) with a deterministic final reduction;
  * the host does ONE device -> host copy (status word, CE mean and count, skip flags, all cost matrices), solves the
    assignments with scipy exactly as the reference does, and does ONE host -> device copy (mask loss value + matched pairs);
  * backward: zh_mask_match_grad / zh_upsample_ce_bwd push the full-resolution gradients through the adjoint of the bilinear
    upsample into the low-res inputs (never writing them at full resolution), then the transposed GEMM gives d tokens.

HipCriterion(..., assignment="device") keeps the step on the device between those two groups of kernels (csrc/assign.hip): ground
truth that is already on the GPU is packed there (zh_pack_masks_u8, or not at all when it lies packed already), zh_linear_assignment
solves every (image, layer) exactly as scipy does and writes the pairs and the mask loss where the backward reads them, and the host
does ONE small device -> host copy (status word, CE mean and count, mask loss, pair count, pairs) and no host -> device copy.

The text embeddings are constants of the criterion (the frozen CLIP text features of the reference): no gradient flows into them.
There is no CPU fallback: CPU tensors raise ZutisHipError.
"""
from __future__ import annotations

from typing import Dict, List, Union

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from . import _lib, ops


class _MaskTerm(torch.autograd.Function):
    """mask_loss = sum over (image, layer) of the matched costs / batch_size (criterion.py:97-150).  The tensors the backward reads go
    through save_for_backward: an in-place change of the proposals between forward and backward raises, as it does in torch."""

    @staticmethod
    def forward(ctx, proposals, p5, gt_u8, inst_off, pairs, stat_p, stat_pg, stat_g, mask_loss, meta):
        ctx.save_for_backward(p5, gt_u8, inst_off, pairs, stat_p, stat_pg, stat_g)
        ctx.meta = meta
        return mask_loss.clone()

    @staticmethod
    def backward(ctx, grad):
        p5, gt_u8, inst_off, pairs, stat_p, stat_pg, stat_g = ctx.saved_tensors
        m = ctx.meta
        g = grad.detach().reshape(1).to(torch.float32).contiguous()
        out = ops.mask_match_grad(p5, gt_u8, inst_off, pairs, stat_p, stat_pg, stat_g, g, m["H"], m["W"], m["wd"], m["wb"], m["loss_scale"])
        return (out.reshape(m["shape"]).to(m["dtype"]),) + (None,) * 9


class _CETerm(torch.autograd.Function):
    """ce_loss = F.cross_entropy(einsum(te, upsample(tok)), labels, ignore_index) (criterion.py:77-95)."""

    @staticmethod
    def forward(ctx, tokens, logits_lo, te, labels, lse, ce_out, meta):
        ctx.save_for_backward(logits_lo, te, labels, lse, ce_out)
        ctx.meta = meta
        return ce_out[0].clone()

    @staticmethod
    def backward(ctx, grad):
        lo, te, labels, lse, ce_out = ctx.saved_tensors
        m = ctx.meta
        g = grad.detach().reshape(1).to(torch.float32).contiguous()
        B, n, h, w = lo.shape
        D = te.shape[1]
        dlo = ops.upsample_ce_bwd(lo, labels, lse, ce_out, g, m["ignore_index"])
        dtok = torch.empty((B, h, w, D), dtype=torch.float32, device=lo.device)
        hw = h * w
        # d tok[b](pix, d) = sum_c dlo[b](c, pix) te(c, d)
        ops.gemm_f32_strided(dlo, (n * hw, 1, hw), te, (0, 1, D), dtok, (hw * D, D, 1), B, hw, D, n)
        return (dtok.to(m["dtype"]),) + (None,) * 6


def _check_batch(props, gts, tokens, te, sem):
    """Host-side shape checks before anything is packed or launched: every per-image input must cover the proposals' batch
    (the kernels index the GT offsets, tokens and labels by the proposals' image index)."""
    bad = _lib.ZutisHipError
    if not isinstance(props, torch.Tensor) or props.dim() not in (4, 5):
        raise bad(f"HipCriterion: proposals must be a [b, Q, h, w] or [b, L, Q, h, w] tensor, got "
                  f"{tuple(props.shape) if isinstance(props, torch.Tensor) else type(props).__name__}")
    B = int(props.shape[0])
    if B < 1:
        raise bad("HipCriterion: empty batch")
    if len(gts) != B:
        raise bad(f"HipCriterion: {len(gts)} ground-truth instance mask tensors for a batch of {B} proposals")
    if not isinstance(tokens, torch.Tensor) or tokens.dim() != 4 or int(tokens.shape[0]) != B:
        raise bad(f"HipCriterion: patch tokens must be [{B}, h, w, D], got "
                  f"{tuple(tokens.shape) if isinstance(tokens, torch.Tensor) else type(tokens).__name__}")
    if not isinstance(te, torch.Tensor) or te.dim() != 2 or te.shape[0] < 1 or te.shape[1] != tokens.shape[3]:
        raise bad(f"HipCriterion: text embeddings must be [n_categories, {int(tokens.shape[3])}], got "
                  f"{tuple(te.shape) if isinstance(te, torch.Tensor) else type(te).__name__}")
    if not isinstance(sem, torch.Tensor) or sem.dim() != 3 or int(sem.shape[0]) != B:
        raise bad(f"HipCriterion: semantic masks must be [{B}, H, W], got "
                  f"{tuple(sem.shape) if isinstance(sem, torch.Tensor) else type(sem).__name__}")


def _pack_gt(gts, dev, on_device=False):
    """The ragged GT list -> ONE host buffer [inst_off int32 (B + 1, padded to 16 bytes) | masks u8 [n_tot, H, W]], copied once.
    on_device (assignment="device"): when every GT tensor is on `dev` already, nothing goes to the host — ops.pack_masks_u8 packs
    them there (bool views of one allocation in order, as zutis_amd.synth delivers them, are used where they lie)."""
    B = len(gts)
    for g in gts:
        assert len(g.shape) == 3, f"Invalid ground truth instance masks shape: {len(g.shape)} != 3"
    H, W = (int(s) for s in gts[0].shape[-2:])
    for g in gts:
        if tuple(g.shape[-2:]) != (H, W):
            raise _lib.ZutisHipError(f"HipCriterion: every image's GT masks must be {H}x{W} (got {tuple(g.shape)})")
    counts = [int(g.shape[0]) for g in gts]
    off = np.zeros(B + 1, dtype=np.int32)
    off[1:] = np.cumsum(counts)
    if on_device and all(isinstance(g, torch.Tensor) and g.device == dev for g in gts):
        src = [g.detach() for g in gts]
        if not (all(g.dtype in (torch.bool, torch.uint8) for g in src) or all(g.dtype == torch.int64 for g in src)):
            src = [g != 0 for g in src]                         # any other dtype: compared on the device
        gt_u8, inst_off, _ = ops.pack_masks_u8(src, H, W)
        return inst_off, gt_u8, off, H, W
    head = (4 * (B + 1) + 15) // 16 * 16
    buf = torch.zeros(head + int(off[-1]) * H * W, dtype=torch.uint8)
    buf[:4 * (B + 1)] = torch.from_numpy(off.view(np.uint8))
    if off[-1]:
        buf[head:] = torch.cat([(g.detach().cpu() != 0).to(torch.uint8).reshape(-1) for g in gts], 0)
    d = buf.to(dev)
    return d[:4 * (B + 1)].view(torch.int32), d[head:].view(-1, H, W), off, H, W


class HipCriterion:
    """Same constructor, call and return contract as the reference's criterion.py::Criterion (:8-23, :63-161)."""

    def __init__(
            self,
            text_embeddings: torch.Tensor,
            weight_ce_loss: float = 1.0,
            weight_mask_loss: float = 1.0,
            weight_dice_loss: float = 1.0,
            weight_bce_loss: float = 1.0,
            ignore_index: int = 255,
            *,
            assignment: str = "host"
    ):
        """assignment (keyword-only, after the reference's arguments): "host" solves the assignments with scipy on the host, as the
        reference does.  "device" solves them on the GPU (zh_linear_assignment: scipy's algorithm, scan order and tie rule in
        float64 — the same matches, ties included), packs ground truth that is already on the GPU there, and makes one small
        device -> host copy per call and no host -> device copy.  In device mode `last_costs` stays empty (use host mode to look
        at the costs), a non-finite cost raises ValueError (scipy would accept +inf entries; the cost kernel cannot produce one
        without the range assert firing first), and a call with more than ops.ASSIGN_MAX_DIM (1024) queries or instances of one
        image — the solver's LDS state — is solved on the host as in "host" mode.  Bool ground-truth views of one allocation are
        read where they lie, forward and backward: like the proposals, they must not be overwritten between the two."""
        self.assignment = assignment
        self.text_embeddings: torch.Tensor = text_embeddings  # n_categories x n_dims
        self.weight_ce_loss: float = weight_ce_loss
        self.weight_mask_loss: float = weight_mask_loss
        self.weight_dice_loss: float = weight_dice_loss
        self.weight_bce_loss: float = weight_bce_loss
        self.ignore_index: int = ignore_index
        self.last_costs: Dict = {}          # (image, layer) -> float32 [n_i, Q] cost matrix of the last call (tests / inspection; host mode)
        self.last_matches: Dict = {}        # (image, layer) -> (instance indices, query indices)

    @property
    def assignment(self) -> str:
        """"host" or "device" (see __init__); may be set between calls."""
        return self._assignment

    @assignment.setter
    def assignment(self, value: str):
        if value not in ("host", "device"):
            raise ValueError(f"HipCriterion: assignment must be 'host' or 'device', got {value!r}")
        self._assignment = value

    def __call__(
            self,
            batch_mask_proposals: torch.Tensor,  # b (x n_layers) x n_queries x h x w
            batch_ground_truth_instance_masks: List[torch.Tensor],  # b x n_instances (variable) x H x W, {0, 1}
            batch_category_ids: List[List[int]],  # unused, as in the reference
            batch_patch_tokens: torch.Tensor,  # b x h x w x text_dims
            batch_ground_truth_semantic_masks,  # b x H x W
    ) -> Dict[str, Union[float, np.ndarray, torch.Tensor]]:
        props, tokens = batch_mask_proposals, batch_patch_tokens
        _check_batch(props, batch_ground_truth_instance_masks, tokens, self.text_embeddings, batch_ground_truth_semantic_masks)
        if not (props.is_cuda and tokens.is_cuda):
            raise _lib.ZutisHipError("HipCriterion needs the mask proposals and patch tokens on the GPU (no CPU fallback)")
        dev = props.device
        with torch.cuda.device(dev):
            return self._call(props, batch_ground_truth_instance_masks, tokens, batch_ground_truth_semantic_masks, dev)

    def _call(self, props, gts, tokens, sem, dev):
        B = len(props)
        p5 = props.detach().to(torch.float32)
        p5 = (p5.unsqueeze(1) if props.dim() == 4 else p5).contiguous()
        _, L, Q, h, w = p5.shape
        n_inst = max((int(g.shape[0]) for g in gts if len(g.shape)), default=0)
        on_device = self.assignment == "device" and max(n_inst, Q) <= ops.ASSIGN_MAX_DIM     # above the cap: the host solve
        inst_off, gt_u8, off, H, W = _pack_gt(list(gts), dev, on_device)
        n_tot, n_max = int(off[-1]), int(np.diff(off).max()) if B else 0
        labels = sem.to(dev).to(torch.int64).contiguous()
        if tuple(labels.shape) != (B, H, W):
            raise _lib.ZutisHipError(f"HipCriterion: semantic masks must be [{B}, {H}, {W}], got {tuple(labels.shape)}")

        if on_device:
            # ONE readback buffer: [status, n_pairs, ce mean, ce count, mask loss, -, -, -, pairs [cap, 4]]; skip and costs stay on the device
            cap = ops.assignment_pairs_capacity(B, L, Q, n_max, n_tot)
            rb = torch.zeros(8 + 4 * cap, dtype=torch.int32, device=dev)
            status, ce_out = rb[0:1], rb[2:4].view(torch.float32)
            skip = torch.empty(B, dtype=torch.int32, device=dev)
            costs = torch.empty(max(1, L * n_tot * Q), dtype=torch.float32, device=dev)
        else:
            # ONE readback buffer: [status, -, ce mean, ce count, skip [B], costs [L * n_tot * Q]]
            rb = torch.zeros(4 + B + L * n_tot * Q, dtype=torch.int32, device=dev)
            status, ce_out, skip = rb[0:1], rb[2:4].view(torch.float32), rb[4:4 + B]
            costs = rb[4 + B:].view(torch.float32)

        # CE: low-res logits [B, n_cat, h2, w2] = te . tok, then upsample -> LSE -> NLL
        te = self.text_embeddings.detach().to(device=dev, dtype=torch.float32).contiguous()
        tok = tokens.detach().to(torch.float32).contiguous()
        _, h2, w2, D = tok.shape
        n_cat = te.shape[0]
        hw2 = h2 * w2
        lo = torch.empty((B, n_cat, h2, w2), dtype=torch.float32, device=dev)
        ops.gemm_f32_strided(te, (0, D, 1), tok, (hw2 * D, D, 1), lo, (n_cat * hw2, hw2, 1), B, n_cat, hw2, D)
        lse = ops.upsample_ce_fwd(lo, labels, self.ignore_index, ce_out, status)

        # matching costs of every (image, layer)
        stat_p = torch.empty((B, L, Q), dtype=torch.float32, device=dev)
        stat_pg = torch.empty((max(1, L * n_tot * Q),), dtype=torch.float32, device=dev)
        stat_g = torch.empty((max(1, n_tot),), dtype=torch.float32, device=dev)
        ops.mask_match_cost(p5, gt_u8, inst_off, n_max, H, W, costs, stat_p, stat_pg, stat_g, skip, status,
                            self.weight_dice_loss, self.weight_bce_loss)

        if on_device:                                           # the assignments of every (image, layer): one call, no host trip
            ops.linear_assignment_batched(costs, inst_off, skip, B, L, Q, n_max, n_tot, rb[8:], rb[1:2], rb[4:5].view(torch.float32), status)
        host = rb.cpu().numpy()                                 # the one device -> host copy (synchronises)
        word = int(host[0])
        if word & ops.STATUS_RANGE:                             # the reference's asserts, criterion.py:71-72 (error path only)
            mn, mx = props.min(), props.max()
            assert 0 <= mn <= 1, f"unexpected value: {mn}"
            assert 0 <= mx <= 1, f"unexpected value: {mx}"
        if word & ops.STATUS_LABEL:
            raise ValueError(f"HipCriterion: a semantic label is neither in [0, {n_cat}) nor ignore_index={self.ignore_index}")
        ce_value = float(host[2:4].view(np.float32)[0])
        meta_m = {"H": H, "W": W, "wd": self.weight_dice_loss, "wb": self.weight_bce_loss, "loss_scale": 1.0 / B,
                  "shape": props.shape, "dtype": props.dtype}
        if on_device:
            if word & ops.STATUS_NONFINITE:
                raise ValueError("HipCriterion: a matching cost is not finite (assignment='device' needs finite costs)")
            n_pairs = int(host[1])
            pairs_h = host[8:8 + 4 * n_pairs].reshape(-1, 4)
            mask_value = host[4:5].view(np.float32)[0]
            self.last_costs, self.last_matches = {}, {}
            instance_indices = query_indices = None
            # the pairs are in (b, l, i) order: one run per matched (image, layer)
            cuts = np.flatnonzero(np.any(pairs_h[1:, :2] != pairs_h[:-1, :2], axis=1)) + 1 if n_pairs else np.zeros(0, dtype=np.int64)
            for run in np.split(pairs_h, cuts) if n_pairs else []:
                instance_indices, query_indices = run[:, 3].astype(np.int64), run[:, 2].astype(np.int64)
                self.last_matches[(int(run[0, 0]), int(run[0, 1]))] = (instance_indices, query_indices)
            mask_loss = _MaskTerm.apply(props, p5, gt_u8, inst_off, rb[8:8 + 4 * n_pairs].view(-1, 4), stat_p, stat_pg, stat_g,
                                        rb[4:5].view(torch.float32)[0], meta_m)
            return self._finish(mask_loss, tokens, lo, te, labels, lse, ce_out, ce_value, mask_value, instance_indices, query_indices)
        skip_h = host[4:4 + B]
        cost_h = host[4 + B:].view(np.float32)

        # host Hungarian per (image, layer), as the reference (criterion.py:133)
        pairs: List[int] = []
        total = 0.0
        self.last_costs, self.last_matches = {}, {}
        instance_indices = query_indices = None
        for b in range(B):
            if skip_h[b]:
                continue
            n_b = int(off[b + 1] - off[b])
            for l in range(L):
                base = (L * int(off[b]) + l * n_b) * Q
                cm = cost_h[base:base + n_b * Q].reshape(n_b, Q)
                instance_indices, query_indices = linear_sum_assignment(cost_matrix=cm)
                self.last_costs[(b, l)] = cm.copy()
                self.last_matches[(b, l)] = (instance_indices, query_indices)
                total += float(cm[instance_indices, query_indices].astype(np.float64).sum())
                for i, q in zip(instance_indices, query_indices):
                    pairs += [b, l, int(q), int(i)]
        mask_value = np.float32(total / B)
        hb = np.zeros(4 + len(pairs), dtype=np.int32)
        hb[0] = mask_value.view(np.int32)
        hb[4:] = pairs
        db = torch.from_numpy(hb).to(dev)                       # the one host -> device copy
        mask_loss = _MaskTerm.apply(props, p5, gt_u8, inst_off, db[4:].view(-1, 4), stat_p, stat_pg, stat_g,
                                    db[0:1].view(torch.float32)[0], meta_m)
        return self._finish(mask_loss, tokens, lo, te, labels, lse, ce_out, ce_value, mask_value, instance_indices, query_indices)

    def _finish(self, mask_loss, tokens, lo, te, labels, lse, ce_out, ce_value, mask_value, instance_indices, query_indices):
        ce_loss = _CETerm.apply(tokens, lo, te, labels, lse, ce_out, {"ignore_index": self.ignore_index, "dtype": tokens.dtype})
        loss = self.weight_mask_loss * mask_loss + self.weight_ce_loss * ce_loss
        return {
            "ce_loss": ce_value,
            "mask_loss": float(mask_value),
            "loss": loss,
            "instance_indices": instance_indices,  # of the last (image, layer) processed, as in the reference
            "query_indices": query_indices
        }
