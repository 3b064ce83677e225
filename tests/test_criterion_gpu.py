"""GPU: the HIP training criterion (zutis_amd/criterion.py, drop-in zutis_amd/dropin/criterion.py) against the reference's
recorded outputs (tests/golden/criterion.npz) and against the float64 restatement (tests/_criterion_ref.py) at the training
shape of the shipped configs (batch 8, 384^2 crops, 6 decoder layers x 100 queries on 48x48, 1-10 instances, 81 / 920 classes)."""
import numpy as np
import pytest
import torch

from tests._criterion_case import make_case
from tests._criterion_ref import criterion_ref, unique_margin
from tests.test_criterion_cpu import WEIGHTS, load_golden, rel

pytestmark = pytest.mark.gpu


def _run(crit, props, gts, tok, sem, dev, five=True):
    p = props.to(dev).clone().requires_grad_(True)
    t = tok.to(dev).clone().requires_grad_(True)
    out = crit(p, gts, [[0] * int(g.shape[0]) for g in gts], t, sem)
    out["loss"].backward()
    return out, p.grad, t.grad


@pytest.mark.parametrize("tag", list(WEIGHTS))
def test_golden_case_through_the_dropin(golden_dir, dev, tag):
    from zutis_amd.dropin.criterion import Criterion
    z, props, gts, tok, sem, te = load_golden(golden_dir)
    crit = Criterion(te.to(dev), **WEIGHTS[tag])
    out, gp, gt = _run(crit, props, gts, tok, sem, dev)
    assert abs(out["ce_loss"] - float(z[f"{tag}_ce_loss"])) <= 1e-5
    assert abs(out["mask_loss"] - float(z[f"{tag}_mask_loss"])) <= 1e-5
    assert abs(float(out["loss"]) - float(z[f"{tag}_loss"])) <= 1e-5
    keys = sorted(k for k in z.files if k.startswith(f"{tag}_cost_"))
    assert sorted(crit.last_costs) == sorted(tuple(int(v) for v in k.split("_")[-2:]) for k in keys)
    for k in keys:
        b, l = (int(v) for v in k.split("_")[-2:])
        assert np.abs(crit.last_costs[(b, l)] - z[k]).max() <= 1e-5, k
        rows, cols = crit.last_matches[(b, l)]
        assert np.array_equal(rows, z[f"{tag}_rows_{b}_{l}"]) and np.array_equal(cols, z[f"{tag}_cols_{b}_{l}"]), k
    last = keys[-1].split("_")[-2:]
    assert np.array_equal(out["query_indices"], z[f"{tag}_cols_{last[0]}_{last[1]}"])
    assert rel(gp.cpu(), z[f"{tag}_grad_props"]) <= 1e-4
    assert rel(gt.cpu(), z[f"{tag}_grad_tokens"]) <= 1e-4


@pytest.mark.parametrize("n_cat,five,hw", [(81, True, 48), (920, True, 48), (81, False, 48), (920, True, 24)],
                         ids=["81-True", "920-True", "81-False", "vitb32-920-True"])
def test_training_shape_against_float64(dev, n_cat, five, hw):
    """hw = 48: ViT-B/16 (16-pixel patches of the 384 crop); hw = 24: ViT-B/32 (configs/*_vit_b_32.yaml), proposals and tokens
    24x24, upsampled 16x."""
    from zutis_amd.criterion import HipCriterion
    L = 6 if five else 1
    props, gts, tok, te, sem = make_case(8, L, 100, hw, hw, 384, 384, n_cat, 512, hw, hw, seed=11)
    if not five:
        props = props[:, 0]
    props, tok, te = props.to(dev), tok.to(dev), te.to(dev)
    ref = criterion_ref(props, gts, tok, sem, te, images_for_grads=(0, 1))
    assert len(ref["costs"]) == 8 * L
    for key, cm in ref["costs"].items():
        assert unique_margin(cm) > 1e-4, key           # the seeded optimum is unique by a margin fp32 cannot bridge
    crit = HipCriterion(te)
    out, gp, gt = _run(crit, props, gts, tok, sem, dev)
    for key, cm in ref["costs"].items():
        assert np.abs(crit.last_costs[key] - cm).max() <= 1e-5, key
        assert all(np.array_equal(a, b) for a, b in zip(crit.last_matches[key], ref["matches"][key])), key
    assert abs(float(out["loss"]) - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    assert abs(out["ce_loss"] - ref["ce"]) <= 1e-5 * abs(ref["ce"])
    assert abs(out["mask_loss"] - ref["mask"]) <= 1e-5 * abs(ref["mask"])
    assert rel(gp[:2].cpu(), ref["grad_props"][:2].cpu()) <= 1e-4
    assert rel(gt[:2].cpu(), ref["grad_tokens"][:2].cpu()) <= 1e-4


def test_gradients_are_bitwise_reproducible(dev):
    from zutis_amd.criterion import HipCriterion
    props, gts, tok, te, sem = make_case(8, 6, 100, 48, 48, 384, 384, 81, 512, 48, 48, seed=11)
    crit = HipCriterion(te.to(dev))
    o1, gp1, gt1 = _run(crit, props, gts, tok, sem, dev)
    c1 = dict(crit.last_costs)
    o2, gp2, gt2 = _run(crit, props, gts, tok, sem, dev)
    assert torch.equal(gp1, gp2) and torch.equal(gt1, gt2)
    assert o1["ce_loss"] == o2["ce_loss"] and o1["mask_loss"] == o2["mask_loss"]
    assert all(np.array_equal(c1[k], crit.last_costs[k]) for k in c1)


def test_bad_label_raises_and_the_next_call_is_right(golden_dir, dev):
    from zutis_amd.dropin.criterion import Criterion
    z, props, gts, tok, sem, te = load_golden(golden_dir)
    crit = Criterion(te.to(dev))
    bad = sem.clone()
    bad[1, 5, 7] = 7                                   # == n_cat, not ignore_index
    with pytest.raises(ValueError):
        _run(crit, props, gts, tok, bad, dev)
    out, gp, _ = _run(crit, props, gts, tok, sem, dev)
    assert abs(out["ce_loss"] - float(z["default_ce_loss"])) <= 1e-5
    assert abs(out["mask_loss"] - float(z["default_mask_loss"])) <= 1e-5


def test_range_assert_skip_and_all_ignored(golden_dir, dev):
    from zutis_amd.dropin.criterion import Criterion
    z, props, gts, tok, sem, te = load_golden(golden_dir)
    crit = Criterion(te.to(dev))
    with pytest.raises(AssertionError, match="unexpected value"):
        _run(crit, props * 1.5, gts, tok, sem, dev)
    out, _, _ = _run(crit, props, gts, tok, torch.full_like(sem, 255), dev)
    assert np.isnan(out["ce_loss"]) and abs(out["mask_loss"] - float(z["default_mask_loss"])) <= 1e-5
    assert not any(b == 1 for b, _ in crit.last_costs)  # image 1's GT is all zero: skipped


def test_adamw_steps_track_float64(dev):
    from zutis_amd.criterion import HipCriterion
    props, gts, tok, te, sem = make_case(2, 2, 8, 24, 24, 96, 96, 7, 32, 12, 12, seed=3, n_range=(2, 4))
    te = te.to(dev)
    p0 = torch.logit(props).to(dev)
    t0 = tok.to(dev)
    runs = {}
    for kind in ("hip", "f64"):
        dt = torch.float32 if kind == "hip" else torch.float64
        pp = torch.nn.Parameter(p0.clone().to(dt))
        tp = torch.nn.Parameter(t0.clone().to(dt))
        opt = torch.optim.AdamW([pp, tp], lr=1e-2, eps=1e-4)
        crit = HipCriterion(te)
        for _ in range(4):
            opt.zero_grad()
            prop = torch.sigmoid(pp)
            tk = tp / tp.norm(dim=-1, keepdim=True)
            if kind == "hip":
                crit(prop, gts, [[0]] * 2, tk, sem)["loss"].backward()
            else:
                r = criterion_ref(prop, gts, tk, sem, te)
                torch.autograd.backward([prop, tk], [r["grad_props"], r["grad_tokens"]])
            opt.step()
        runs[kind] = (pp.detach().double(), tp.detach().double())
    assert (runs["hip"][0] - runs["f64"][0]).abs().max() <= 1e-4
    assert (runs["hip"][1] - runs["f64"][1]).abs().max() <= 1e-4


def test_batch_mismatches_raise_before_any_launch(golden_dir, dev):
    from zutis_amd import _lib
    from zutis_amd.dropin.criterion import Criterion
    z, props, gts, tok, sem, te = load_golden(golden_dir)
    crit = Criterion(te.to(dev))
    with pytest.raises(_lib.ZutisHipError, match="ground-truth instance mask tensors"):
        _run(crit, props, gts[:-1], tok, sem, dev)
    with pytest.raises(_lib.ZutisHipError, match="patch tokens must be"):
        _run(crit, props, gts, tok[:-1], sem, dev)
    out, _, _ = _run(crit, props, gts, tok, sem, dev)          # and the criterion still answers right afterwards
    assert abs(out["ce_loss"] - float(z["default_ce_loss"])) <= 1e-5
    assert abs(out["mask_loss"] - float(z["default_mask_loss"])) <= 1e-5


def test_in_place_change_of_the_proposals_before_backward_raises(golden_dir, dev):
    from zutis_amd.dropin.criterion import Criterion
    z, props, gts, tok, sem, te = load_golden(golden_dir)
    crit = Criterion(te.to(dev))
    p = props.to(dev).clone().requires_grad_(True)
    out = crit(p, gts, None, tok.to(dev), sem)
    with torch.no_grad():
        p.mul_(1.0)                                            # bumps the version counter the backward checks
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out["loss"].backward()


def test_more_than_16_instances_and_an_odd_query_count(dev):
    """Image 1 has 20 instances (two instance groups of the cost kernel), image 0 has 5 (its second group is empty), Q = 31 is odd
    (the last query pair of a workgroup has one query), 24^2 -> 90 x 110."""
    from zutis_amd.criterion import HipCriterion
    props, gts, tok, te, sem = make_case(2, 2, 31, 24, 24, 90, 110, 7, 32, 12, 12, seed=21, n_range=(20, 20))
    gts[0] = gts[0][:5]
    props, tok, te = props.to(dev), tok.to(dev), te.to(dev)
    ref = criterion_ref(props, gts, tok, sem, te)
    assert len(ref["costs"]) == 4
    for key, cm in ref["costs"].items():
        assert unique_margin(cm) > 1e-4, key
    crit = HipCriterion(te)
    out, gp, gt = _run(crit, props, gts, tok, sem, dev)
    for key, cm in ref["costs"].items():
        assert crit.last_costs[key].shape == cm.shape, key
        assert np.abs(crit.last_costs[key] - cm).max() <= 1e-5, key
        assert all(np.array_equal(a, b) for a, b in zip(crit.last_matches[key], ref["matches"][key])), key
    assert abs(float(out["loss"]) - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    assert rel(gp.cpu(), ref["grad_props"].cpu()) <= 1e-4
    assert rel(gt.cpu(), ref["grad_tokens"].cpu()) <= 1e-4
