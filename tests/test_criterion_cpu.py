"""CPU: the float64 restatement of the training criterion (tests/_criterion_ref.py) against the reference's recorded outputs
(tests/golden/criterion.npz, tools/gen_criterion_golden.py), the drop-in's signatures, and the drop-in's refusal of CPU tensors."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from tests._criterion_ref import criterion_ref

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
