"""-m gpu: ZUTIS over a ViT-L/14 tower (width 1024, patch 14, embed 768; 16 encoder heads at dh = 64, the decoder's 8 heads at dh = 128)
on the HIP engine and through the drop-in module, at the shallow geometry detgen.VIT_L14_SHALLOW (2 + 2 layers at the full width),
against the CPU oracle (oracle.zutis_ref) on the same seeded weights and inputs.

Tolerances are those of tests/test_e2e_gpu.py (TOLS: `fast` 2.5e-4 on logits / 1e-3 on the sigmoid mask proposals, `exact` 2e-5 / 2e-4; the
drop-in's `exact` instance bounds of test_dropin_module_matches_reference_golden); labels go through oracle.parity (no unexplained pixel).
The weights are drawn and the oracle is evaluated once per shape for the whole module.

Observed on an MI355X (a record, not a threshold; low-res logits / mask proposals, max abs error against the fp32 oracle):
  3 x 75 x 123         exact 8.6e-08 / 6.0e-07     fast 5.2e-05 / 1.7e-04
  224 x 224, split 1   exact 1.1e-07 / 4.8e-07     fast 4.6e-05 / 1.8e-04
  224 x 224, split 12  exact 1.1e-07 / 4.8e-07     fast 4.6e-05 / 1.8e-04
No bound of the ViT-B geometries had to move at width 1024."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from tests.test_e2e_gpu import TOLS

pytestmark = pytest.mark.gpu

N_CAT = 7
RAGGED = (3, 75, 123)          # 5 x 8 patches, M = 160 keys: a ragged fp16 key tile (64), an exact split-pair one (32); not a multiple of 14
SQUARE = (1, 224, 224)         # M = 1024: the threshold from which the cross-attention's keys are split


@functools.lru_cache(maxsize=None)
def _weights():
    from zutis_amd import detgen
    return detgen.zutis_state_dict(detgen.VIT_L14_SHALLOW)


@functools.lru_cache(maxsize=None)
def _text():
    from zutis_amd import detgen
    return torch.from_numpy(detgen.text_embeddings(N_CAT, detgen.VIT_L14_SHALLOW.embed_dim))


@functools.lru_cache(maxsize=None)
def _oracle(shape, seed=0):
    """The fp32 CPU oracle's forward for detgen.images(*shape, seed): mask proposals, patch tokens, low-res logits (read-only)."""
    from oracle import zutis_ref as O
    from zutis_amd import detgen
    cfg = detgen.VIT_L14_SHALLOW
    P = O.to_torch_params(_weights())
    with torch.no_grad():
        ref = O.zutis_forward(P, torch.from_numpy(detgen.images(*shape, seed=seed)), cfg.patch, cfg.dec_heads)
        lo = O.semantic_logits_lowres(ref["patch_tokens"], _text()).numpy()
    return ref["mask_proposals"], ref["patch_tokens"], lo


@functools.lru_cache(maxsize=None)
def _params(dev):
    return {k: torch.from_numpy(v).to(dev) for k, v in _weights().items()}


def _engine(dev, precision):
    from zutis_amd import detgen
    from zutis_amd.engine import ZutisEngine
    cfg = detgen.VIT_L14_SHALLOW
    eng = ZutisEngine(_params(dev), cfg.patch, cfg.dec_heads, precision=precision)
    assert (eng.D, eng.heads, eng.dec_dh, eng.E, eng.layers, eng.dec_layers, eng.Q) == (1024, 16, 128, 768, 2, 2, 100)
    return eng


def _check_forward(eng, dev, shape, precision, what):
    from oracle import zutis_ref as O
    from oracle.parity import unexplained_label_mismatches
    from zutis_amd import detgen
    logit_tol, mask_tol = TOLS[precision]
    mp_ref, pt_ref, lo_ref = _oracle(shape)
    out = eng.forward(torch.from_numpy(detgen.images(*shape)).to(dev))
    assert out["mask_proposals"].shape == mp_ref.shape and out["patch_tokens"].shape == pt_ref.shape
    text = _text().to(dev)
    lo = eng.semantic_logits_lowres(out["patch_tokens"], text).cpu().numpy()
    mp = out["mask_proposals"].cpu().numpy()
    e_lo, e_mp = float(np.abs(lo - lo_ref).max()), float(np.abs(mp - mp_ref.numpy()).max())
    print(f"{what}[{precision}]: logits maxerr {e_lo:.2e} (tol {logit_tol:g}), mask proposals {e_mp:.2e} (tol {mask_tol:g})")
    assert e_lo < logit_tol, e_lo
    assert e_mp < mask_tol, e_mp
    size = shape[1:]
    labels = eng.predict_semantic(out["patch_tokens"], text, size).cpu().numpy()
    n_mis, n_bad, worst = unexplained_label_mismatches(labels, O.predict_semantic(pt_ref, _text(), size), lo_ref, e_lo, size)
    assert n_bad == 0, (n_mis, n_bad, worst, e_lo)
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("precision", ["exact", "fast"])
def test_engine_vs_oracle_ragged_batch(dev, precision):
    """Three 75 x 123 images: 5 x 8 patches, 160 decoder keys."""
    _check_forward(_engine(dev, precision), dev, RAGGED, precision, "vit-l 3x75x123")


@pytest.mark.parametrize("precision", ["exact", "fast"])
def test_engine_vs_oracle_at_the_key_split_threshold(dev, precision):
    """One 224 x 224 image: M = 1024 keys, with the cross-attention unsplit and under the drop-in's setting of 12; the two settings agree
    with each other to the `exact` tolerance."""
    from zutis_amd import shape_rules
    eng = _engine(dev, precision)
    outs = {}
    for setting in (1, 12):
        eng.cross_ksplit = setting
        outs[setting] = _check_forward(eng, dev, SQUARE, precision, f"vit-l 224x224 cross_ksplit={setting}")
    assert shape_rules.cross_attention_key_split(12, 1, 8, 100, 1024, False) > 1 and shape_rules.cross_attention_key_split(1, 1, 8, 100, 1024, False) == 1
    logit_tol, mask_tol = TOLS["exact"]
    assert float((outs[1]["patch_tokens"] - outs[12]["patch_tokens"]).abs().max()) < logit_tol
    assert float((outs[1]["mask_proposals"] - outs[12]["mask_proposals"]).abs().max()) < mask_tol


def test_forward_graphed_matches_eager(dev):
    """hipGraph replay returns bitwise what the eager launch sequence returns at the ViT-L geometry."""
    from zutis_amd import detgen
    eng = _engine(dev, "exact")
    for seed in (0, 1, 2):
        x = torch.from_numpy(detgen.images(1, 75, 123, seed=seed)).to(dev)
        a = {k: v.clone() for k, v in eng.forward(x).items()}
        b = eng.forward_graphed(x)
        assert torch.equal(a["mask_proposals"], b["mask_proposals"]) and torch.equal(a["patch_tokens"], b["patch_tokens"])


def _dropin(dev, clip_arch="ViT-L/14"):
    from zutis_amd import detgen
    cfg = detgen.VIT_L14_SHALLOW
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zutis_amd", "dropin")
    if d not in sys.path:
        sys.path.insert(0, d)
    from networks.zutis import ZUTIS
    net = ZUTIS(categories=[f"c{i}" for i in range(N_CAT)], clip_arch=clip_arch, n_queries=cfg.n_queries, n_decoder_layers=cfg.dec_layers,
                n_heads=cfg.dec_heads, device=dev, text_embeddings=_text(), vision_config=(cfg.width, cfg.layers, cfg.patch, cfg.grid, cfg.embed_dim))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in _weights().items()}, strict=True)
    return net.to(dev).eval()


def test_dropin_module_matches_the_oracle(dev):
    """ZUTIS(clip_arch="ViT-L/14").forward / .predict (semantic, instance) on the HIP path at the module's defaults (`exact`, hipGraph
    replay for batches <= 4, cross_attention_key_split = 12), with the oracle where test_dropin_module_matches_reference_golden has the
    reference's golden outputs.  At random init every query proposes nearly the same mask: hard NMS keeps one per image, no NMS all 100."""
    from oracle import resample as R
    from oracle import zutis_ref as O
    from oracle.parity import unexplained_label_mismatches
    from zutis_amd import detgen, rle
    cfg = detgen.VIT_L14_SHALLOW
    b, H, W = RAGGED
    logit_tol, t_score, t_pix = TOLS["exact"][0], 2e-3, 5e-4
    net = _dropin(dev)
    assert net.precision == "exact" and net.cross_attention_key_split == 12 and net.use_hip_graph
    assert len(net.state_dict()) == len(detgen.zutis_param_shapes(cfg))
    x = torch.from_numpy(detgen.images(b, H, W)).to(dev)
    with pytest.raises(NotImplementedError):
        net(x)
    with torch.no_grad():
        out = {k: v.clone() for k, v in net(x).items()}
        again = net(x)                           # the second occurrence of the shape: captured and replayed
        assert all(torch.equal(out[k], again[k]) for k in out)
        assert [k for k, v in net._get_engine()._graphs.items() if v["graph"] is not None]
    eng_out = _engine(dev, "exact").forward(x)
    assert all(torch.equal(out[k], eng_out[k]) for k in out)          # the module returns the engine's outputs
    mp_ref, pt_ref, lo_ref = _oracle(RAGGED)
    labels = net.predict(out, mask_type="semantic", size=(H, W))
    assert labels.dtype == np.int64 and labels.shape == (b, H, W)
    logits = net.predict(out, mask_type="semantic", size=(H, W), return_logits=True)
    e_full = float(np.abs(logits.cpu().numpy() - O.predict_semantic(pt_ref, _text(), (H, W), return_logits=True).numpy()).max())
    assert e_full < logit_tol, e_full
    assert unexplained_label_mismatches(labels, O.predict_semantic(pt_ref, _text(), (H, W)), lo_ref, e_full, (H, W))[1] == 0
    binary, cats, scores = O.instance_scores(mp_ref, pt_ref, _text())
    up = R.bilinear_nchw(mp_ref[:, -1].numpy(), H, W) > 0.5
    for nms in ("hard", None):
        want = []
        for i in range(b):
            if nms is None:
                want += [(i, int(c), q, float(s)) for q, (c, s) in enumerate(zip(cats[i], scores[i])) if c != 0 and up[i, q].sum() > 0]
            else:
                want += [(i, c, q, s) for (c, q, s) in O.mask_nms(up[i], scores[i], cats[i], nms)]
        preds = net.predict(out, mask_type="instance", size=(H, W), image_ids=list(range(b)), nms_type=nms)
        assert len(preds) == len(want) > 0, (nms, len(preds), len(want))
        for p, (i, c, q, s) in zip(preds, want):
            assert p["image_id"] == i and p["category_id"] == c
            assert abs(p["score"] - s) < t_score
            assert (rle.decode(p["segmentation"]).astype(bool) != up[i, q]).mean() <= t_pix
            assert np.abs(np.array(p["bbox"]) - np.array(rle.mask_to_box(up[i, q]))).max() <= 1.0
            assert tuple(p["image_size"]) == (H, W)
    for nms in ("linear", "gaussian"):           # the soft forms run too; their first emission per image is the hard form's
        preds = net.predict(out, mask_type="instance", size=(H, W), image_ids=list(range(b)), nms_type=nms)
        assert len(preds) >= b and {p["image_id"] for p in preds} == set(range(b))


def test_dropin_accepts_the_336px_tower(dev):
    """clip_arch="ViT-L/14@336px" (pos-embed grid 24) constructs from its table entry and runs a forward at batch 1, key split 12."""
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zutis_amd", "dropin")
    if d not in sys.path:
        sys.path.insert(0, d)
    from networks.zutis import _VIT_ARCHS, ZUTIS
    from zutis_amd import detgen
    width, _, patch, grid, embed = _VIT_ARCHS["ViT-L/14@336px"]
    assert (width, patch, grid, embed) == (1024, 14, 24, 768)
    net = ZUTIS(categories=[f"c{i}" for i in range(N_CAT)], clip_arch="ViT-L/14@336px", n_decoder_layers=1, device=dev, text_embeddings=_text(),
                vision_config=(width, 1, patch, grid, embed)).to(dev).eval()
    x = torch.from_numpy(detgen.images(1, 224, 224)).to(dev)
    with torch.no_grad():
        out = net(x)
        labels = net.predict(out, mask_type="semantic", size=(224, 224))
    assert out["mask_proposals"].shape == (1, 1, 100, 32, 32) and out["patch_tokens"].shape == (1, 32, 32, 768)
    assert labels.shape == (1, 224, 224) and bool(torch.isfinite(out["mask_proposals"]).all())
