"""HipCriterion(assignment="device") against assignment="host" (the scipy solve) on the same inputs: equal matches, bitwise equal
gradients and CE loss, the mask loss within one float32 ulp (both are float32 roundings of float64 sums of the same matched costs,
associated differently)."""
import functools

import numpy as np
import pytest
import torch

from tests._criterion_case import make_case
from zutis_amd.criterion import HipCriterion

SMALL = (2, 2, 7, 6, 6, 24, 24, 5, 8, 6, 6)          # B, L, Q, h, w, H, W, n_cat, D, h2, w2 (1..10 instances: n > Q occurs)
LARGE = (3, 6, 100, 12, 12, 48, 48, 5, 8, 12, 12)    # the training step's L and Q


@functools.lru_cache(maxsize=None)
def _case(shape, seed, variant):
    props, gts, tok, te, sem = make_case(*shape, seed)
    if variant == "duplicate":                       # random_duplicate: identical GT masks, bit-identical cost rows
        gts[0] = gts[0].repeat(2, 1, 1)
    elif variant == "zero":                          # an all-zero image is skipped; the mask loss is still divided by B
        gts[1] = torch.zeros_like(gts[1])
    return props, tuple(gts), tok, te, sem


def _run(mode, case, dev, gt_as="cpu_u8"):
    props, gts, tok, te, sem = case
    if gt_as == "dev_bool":                          # as zutis_amd.synth delivers them: bool views of one allocation
        gts = list(torch.split(torch.cat(gts, 0).to(dev).bool(), [int(g.shape[0]) for g in gts], 0))
    elif gt_as == "dev_i64":
        gts = [g.to(dev).to(torch.int64) for g in gts]
    else:
        gts = list(gts)
    crit = HipCriterion(te.to(dev), assignment=mode)
    p = props.to(dev).clone().requires_grad_(True)
    t = tok.to(dev).clone().requires_grad_(True)
    out = crit(p, gts, None, t, sem.to(dev))
    out["loss"].backward()
    return out, p.grad.clone(), t.grad.clone(), crit


@functools.lru_cache(maxsize=None)
def _host(shape, seed, variant):
    return _run("host", _case(shape, seed, variant), torch.device("cuda:0"))


def _assert_same(got, want):
    out, gp, gt_, crit = got
    wout, wgp, wgt, wcrit = want
    assert list(crit.last_matches) == list(wcrit.last_matches) and len(crit.last_matches) > 0
    for k, (ii, qq) in wcrit.last_matches.items():
        assert np.array_equal(crit.last_matches[k][0], ii) and np.array_equal(crit.last_matches[k][1], qq), k
        assert crit.last_matches[k][0].dtype == crit.last_matches[k][1].dtype == np.int64
    assert np.array_equal(out["instance_indices"], wout["instance_indices"]) and np.array_equal(out["query_indices"], wout["query_indices"])
    assert torch.equal(gp, wgp) and torch.equal(gt_, wgt)                                    # bitwise
    assert isinstance(out["ce_loss"], float) and isinstance(out["mask_loss"], float)
    assert np.float32(out["ce_loss"]).tobytes() == np.float32(wout["ce_loss"]).tobytes()
    a, b = np.float32(out["mask_loss"]), np.float32(wout["mask_loss"])
    assert abs(float(a) - float(b)) <= float(np.spacing(max(abs(a), abs(b))))
    assert crit.last_costs == {}                                                             # documented: host mode keeps the costs
    lo, wlo = float(out["loss"].detach()), float(wout["loss"].detach())
    assert abs(lo - wlo) <= 2 * float(np.spacing(np.float32(abs(wlo))))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,seed", [(SMALL, 0), (SMALL, 1), (SMALL, 2), (LARGE, 4)])
@pytest.mark.parametrize("gt_as", ["cpu_u8", "dev_bool", "dev_i64"])
def test_device_mode_equals_host_mode(dev, shape, seed, gt_as):
    _assert_same(_run("device", _case(shape, seed, "plain"), dev, gt_as), _host(shape, seed, "plain"))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,seed", [(SMALL, 0), (SMALL, 3), (LARGE, 4)])
@pytest.mark.parametrize("gt_as", ["cpu_u8", "dev_bool"])
def test_duplicated_masks_tie_the_rows(dev, shape, seed, gt_as):
    want = _host(shape, seed, "duplicate")
    n0 = _case(shape, seed, "duplicate")[1][0].shape[0]
    c = want[3].last_costs[(0, 0)]
    assert np.array_equal(c[:n0 // 2], c[n0 // 2:])                                          # the tie is real
    _assert_same(_run("device", _case(shape, seed, "duplicate"), dev, gt_as), want)


@pytest.mark.gpu
@pytest.mark.parametrize("gt_as", ["cpu_u8", "dev_bool"])
def test_all_zero_image_is_skipped_and_loss_divided_by_batch(dev, gt_as):
    want = _host(SMALL, 0, "zero")
    got = _run("device", _case(SMALL, 0, "zero"), dev, gt_as)
    _assert_same(got, want)
    assert not any(b == 1 for b, _ in got[3].last_matches) and any(b == 0 for b, _ in got[3].last_matches)
    # divided by B = 2, not by the one image that was matched: the same image alone gives twice the mask loss
    props, gts, tok, te, sem = _case(SMALL, 0, "zero")
    alone = _run("device", (props[:1], gts[:1], tok[:1], te, sem[:1]), dev, gt_as)[0]
    assert abs(alone["mask_loss"] - 2 * got[0]["mask_loss"]) <= 2 * float(np.spacing(np.float32(alone["mask_loss"])))


@pytest.mark.gpu
def test_out_of_range_proposal_raises_the_reference_assert(dev):
    props, gts, tok, te, sem = _case(SMALL, 0, "plain")
    with pytest.raises(AssertionError, match="unexpected value"):
        _run("device", (props * 1.5, gts, tok, te, sem), dev, "dev_bool")
    _assert_same(_run("device", _case(SMALL, 0, "plain"), dev, "dev_bool"), _host(SMALL, 0, "plain"))     # and the next call is right


@pytest.mark.gpu
def test_device_mode_with_device_ground_truth_stays_on_the_device(dev, monkeypatch):
    """No host -> device copy and exactly one device -> host copy in the forward.  The project counts library calls, not hipMemcpy
    records, so the copies are watched where torch makes them: Tensor.cpu / .numpy-bound reads, Tensor.to / .cuda from the host,
    torch.tensor / as_tensor / from_numpy (whose result would be sent up)."""
    props, gts, tok, te, sem = _case(SMALL, 1, "plain")
    gts_d = list(torch.split(torch.cat(gts, 0).to(dev).bool(), [int(g.shape[0]) for g in gts], 0))
    crit = HipCriterion(te.to(dev), assignment="device")
    p, t, s = props.to(dev).requires_grad_(True), tok.to(dev).requires_grad_(True), sem.to(dev)
    crit(p, gts_d, None, t, s)                                               # warm: library load, workspaces
    down, up = [], []
    real_cpu, real_to = torch.Tensor.cpu, torch.Tensor.to

    def spy_cpu(self, *a, **k):
        if self.is_cuda:
            down.append(tuple(self.shape))
        return real_cpu(self, *a, **k)

    def spy_to(self, *a, **k):
        r = real_to(self, *a, **k)
        if r.is_cuda != self.is_cuda:
            (up if r.is_cuda else down).append(tuple(self.shape))
        return r

    def no_host_tensor(*a, **k):
        raise AssertionError("a host tensor was built in the device-mode forward")

    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "cpu", spy_cpu)
        m.setattr(torch.Tensor, "to", spy_to)
        m.setattr(torch.Tensor, "cuda", no_host_tensor)
        m.setattr(torch.Tensor, "item", no_host_tensor)
        m.setattr(torch.Tensor, "tolist", no_host_tensor)
        m.setattr(torch, "from_numpy", no_host_tensor)
        m.setattr(torch, "tensor", no_host_tensor)
        m.setattr(torch, "as_tensor", no_host_tensor)
        out = crit(p, gts_d, None, t, s)
    assert up == [] and len(down) == 1, (up, down)
    n_pairs = sum(len(ii) for ii, _ in crit.last_matches.values())
    assert down[0][0] <= 8 + 4 * 2 * 2 * 10 and n_pairs > 0                  # the one small buffer: header + at most B * L * 10 pairs
    assert all(g.dtype == torch.bool and g.is_cuda for g in gts_d)
    want = _host(SMALL, 1, "plain")
    assert out["mask_loss"] == pytest.approx(want[0]["mask_loss"], rel=1e-6) and list(crit.last_matches) == list(want[3].last_matches)
    # host mode on the same inputs does go through the host: the spy sees its copies
    crit_h = HipCriterion(te.to(dev))
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "cpu", spy_cpu)
        m.setattr(torch.Tensor, "to", spy_to)
        down.clear(), up.clear()
        crit_h(p, gts_d, None, t, s)
    assert len(up) >= 2 and len(down) >= 1 + len(gts_d)
