"""-m gpu: the HIP engine end to end against (a) the reference's golden outputs and (b) the CPU oracle."""
import math
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# north_star: fp32 logits within 1e-3.  Tolerances per engine precision (zutis_amd/engine.py): the default "fast" engine is
# held to a quarter of that on logits / unit-norm tokens and to 1e-3 on the sigmoid mask proposals; "exact" (every
# contraction in the reference-equivalent x3 mode) to fp32-reordering-class errors.
LOGIT_TOL = 2.5e-4
MASK_TOL = 1e-3
TOLS = {"fast": (LOGIT_TOL, MASK_TOL), "exact": (2e-5, 2e-4)}
# Labels: no agreement threshold.  Every pixel whose label differs from the reference's must be EXPLAINED by the logit error
# (oracle/parity.py: the reference's own top-1 / chosen-label margin at that pixel is <= 2 x the measured logit error).


def _engine(cfg, dev, precision="fast"):
    from zutis_amd import detgen
    from zutis_amd.engine import ZutisEngine
    P = {k: torch.from_numpy(v).to(dev) for k, v in detgen.zutis_state_dict(cfg).items()}
    return ZutisEngine(P, cfg.patch, cfg.dec_heads, precision=precision)


@pytest.mark.parametrize("precision", ["fast", "exact"])
@pytest.mark.parametrize("tag,cfgname", [("tiny", "TINY"), ("vitb32_224", "VIT_B32"), ("vitb16_336", "VIT_B16")])
def test_engine_vs_reference_golden(dev, golden_dir, tag, cfgname, precision):
    from zutis_amd import detgen
    cfg = getattr(detgen, cfgname)
    g = np.load(f"{golden_dir}/e2e_{tag}.npz")
    b, H, W, n = int(g["b"]), int(g["H"]), int(g["W"]), int(g["n_cat"])
    eng = _engine(cfg, dev, precision)
    LOGIT_TOL, MASK_TOL = TOLS[precision]
    x = torch.from_numpy(detgen.images(b, H, W)).to(dev)
    text = torch.from_numpy(detgen.text_embeddings(n, cfg.embed_dim)).to(dev)
    out = eng.forward(x)
    lo = eng.semantic_logits_lowres(out["patch_tokens"], text).cpu().numpy()
    err = np.abs(lo - g["logits_lo"]).max()
    assert err < LOGIT_TOL, err
    labels = eng.predict_semantic(out["patch_tokens"], text, tuple(g["size"])).cpu().numpy()
    agree = (labels == g["labels"]).mean()
    from oracle.parity import unexplained_label_mismatches
    n_mis, n_bad, worst = unexplained_label_mismatches(labels, g["labels"], g["logits_lo"], err, tuple(g["size"]))
    assert n_bad == 0, (n_mis, n_bad, worst, err)
    mp, pt = out["mask_proposals"].cpu().numpy(), out["patch_tokens"].cpu().numpy()
    assert mp.min() >= 0 and mp.max() <= 1
    if "mask_proposals" in g:
        assert np.abs(mp - g["mask_proposals"]).max() < MASK_TOL
        assert np.abs(pt - g["patch_tokens"]).max() < LOGIT_TOL
        lf = eng.predict_semantic(out["patch_tokens"], text, tuple(g["size"]), return_logits=True).cpu().numpy()
        assert np.abs(lf - g["logits_full"]).max() < LOGIT_TOL
    else:
        assert np.abs(mp[:, :, ::9, ::3, ::3] - g["mask_proposals_sub"]).max() < MASK_TOL
        assert np.abs(pt[:, ::3, ::3, ::4] - g["patch_tokens_sub"]).max() < LOGIT_TOL
    print(f"{tag}[{precision}]: logits maxerr {err:.2e}, label agreement {agree:.6f} ({n_mis} pixels differ, all with a reference "
          f"top-2 margin <= 2 err; largest {worst:.2e})")


@pytest.mark.parametrize("precision", ["exact", "fast"])
def test_engine_vs_oracle_ragged_batch(dev, precision):
    """Non-square, non-multiple-of-patch input, batch 3, against the CPU oracle on the same seeded inputs — at the product default
    (`exact`, fp32-reordering-class tolerances) and at `fast`."""
    from zutis_amd import detgen
    from oracle import zutis_ref as O
    cfg = detgen.TINY
    eng = _engine(cfg, dev, precision)
    LOGIT_TOL, MASK_TOL = TOLS[precision]
    P = O.to_torch_params(detgen.zutis_state_dict(cfg))
    x = torch.from_numpy(detgen.images(3, 75, 123))
    text = torch.from_numpy(detgen.text_embeddings(5, cfg.embed_dim))
    with torch.no_grad():
        ref = O.zutis_forward(P, x, cfg.patch, cfg.dec_heads)
        ref_lo = O.semantic_logits_lowres(ref["patch_tokens"], text).numpy()
    out = eng.forward(x.to(dev))
    assert out["mask_proposals"].shape == ref["mask_proposals"].shape
    lo = eng.semantic_logits_lowres(out["patch_tokens"], text.to(dev)).cpu().numpy()
    assert np.abs(lo - ref_lo).max() < LOGIT_TOL
    assert np.abs(out["mask_proposals"].cpu().numpy() - ref["mask_proposals"].numpy()).max() < MASK_TOL
    # argmax kernel is bit-exact GIVEN the same low-res logits (integer output)
    from oracle import resample as R
    lab = torch.empty((3, 75, 123), dtype=torch.int64, device=dev)
    from zutis_amd import ops
    ops.upsample_argmax(torch.from_numpy(ref_lo).to(dev), lab, 3, 5, ref_lo.shape[2], ref_lo.shape[3], 75, 123)
    assert np.array_equal(lab.cpu().numpy(), R.bilinear_argmax_nchw(ref_lo, 75, 123))


def test_engine_repack_on_weight_change(dev):
    from zutis_amd import detgen
    cfg = detgen.TINY
    eng = _engine(cfg, dev)
    x = torch.from_numpy(detgen.images(1, 64, 64)).to(dev)
    a = eng.forward(x)["patch_tokens"].clone()
    with torch.no_grad():
        eng.params["encoder.proj"].mul_(-1.0)
    b = eng.forward(x)["patch_tokens"]
    assert not torch.allclose(a, b)


def _dropin_zutis(cfg, dev, n_cat):
    import os, sys
    from zutis_amd import detgen
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zutis_amd", "dropin")
    if d not in sys.path:
        sys.path.insert(0, d)
    from networks.zutis import ZUTIS
    net = ZUTIS(categories=[f"c{i}" for i in range(n_cat)], clip_arch="ViT-B/16", n_queries=cfg.n_queries,
                n_decoder_layers=cfg.dec_layers, n_heads=cfg.dec_heads, device=dev,
                text_embeddings=torch.from_numpy(detgen.text_embeddings(n_cat, cfg.embed_dim)),
                vision_config=(cfg.width, cfg.layers, cfg.patch, cfg.grid, cfg.embed_dim))
    sd = {k: torch.from_numpy(v) for k, v in detgen.zutis_state_dict(cfg).items()}
    net.load_state_dict(sd, strict=True)          # same 275-key contract as the reference
    return net.to(dev).eval()


def test_dropin_replays_a_graph_from_the_second_occurrence_of_a_shape(dev):
    """The drop-in's forward of a batch <= 4: the first call of a shape runs eagerly (a shape seen once must not pay a capture), the
    second captures a hipGraph, later ones replay it — all bitwise equal; use_hip_graph = False never captures."""
    from zutis_amd import detgen
    cfg = detgen.TINY
    net = _dropin_zutis(cfg, dev, 7)
    xa = torch.from_numpy(detgen.images(1, 64, 96, seed=1)).to(dev)
    xb = torch.from_numpy(detgen.images(1, 64, 96, seed=2)).to(dev)
    graphs = lambda: [k for k, v in net._get_engine()._graphs.items() if v["graph"] is not None]
    with torch.no_grad():
        o1 = {k: v.clone() for k, v in net(xa).items()}
        assert graphs() == []
        o2 = {k: v.clone() for k, v in net(xa).items()}
        assert len(graphs()) == 1
        o3 = net(xa)
        ob = net(xb)
        assert len(graphs()) == 1
        for k in o1:
            assert torch.equal(o1[k], o2[k]) and torch.equal(o1[k], o3[k]) and not torch.equal(o1[k], ob[k])
        net.use_hip_graph = False
        net._engine = None
        net(xa); net(xa); net(xa)
        assert graphs() == []


@pytest.mark.parametrize("precision,t_score,t_pix", [("fast", 2e-2, 1e-2), ("exact", 2e-3, 5e-4)])
def test_dropin_module_matches_reference_golden(dev, golden_dir, precision, t_score, t_pix):
    """The reference's call surface (ZUTIS.forward / .predict semantic + instance, all NMS types) on the HIP path,
    against the reference's own outputs for the tiny config."""
    from zutis_amd import detgen
    cfg = detgen.TINY
    g = np.load(f"{golden_dir}/e2e_tiny.npz")
    b, H, W, n = int(g["b"]), int(g["H"]), int(g["W"]), int(g["n_cat"])
    net = _dropin_zutis(cfg, dev, n)
    net.precision = precision
    LOGIT_TOL = TOLS[precision][0]
    assert len(net.state_dict()) == len(detgen.zutis_param_shapes(cfg))
    x = torch.from_numpy(detgen.images(b, H, W)).to(dev)
    with pytest.raises(NotImplementedError):
        net(x)                                   # grad enabled + trainable params => training is refused, not faked
    with torch.no_grad():
        out = net(x)
    labels = net.predict(out, mask_type="semantic", size=(H, W))
    assert labels.dtype == np.int64 and labels.shape == (b, H, W)
    logits = net.predict(out, mask_type="semantic", size=(H, W), return_logits=True)
    e_full = float(np.abs(logits.cpu().numpy() - g["logits_full"]).max())
    assert e_full < LOGIT_TOL
    from oracle.parity import unexplained_label_mismatches
    assert unexplained_label_mismatches(labels, g["labels"], g["logits_lo"], e_full, (H, W))[1] == 0
    for nms in ("hard", "linear", "gaussian", None):
        key = str(nms).lower()
        preds = net.predict(out, mask_type="instance", size=(H, W), image_ids=list(range(b)), nms_type=nms)
        assert len(preds) == int(g[f"inst_{key}_n"]), (nms, len(preds))
        ref_masks = np.unpackbits(g[f"inst_{key}_masks"], axis=-1)[..., :W].astype(bool) if len(preds) else []
        from zutis_amd import rle
        for j, p in enumerate(preds):
            assert p["image_id"] == g[f"inst_{key}_img"][j] and p["category_id"] == g[f"inst_{key}_cat"][j]
            # score = mean(p inside p>0.5) * class prob: one low-res pixel crossing 0.5 moves it by ~1/mask_size (a 10x14 mask
            # here); the kernel itself is checked to 1e-6 on identical inputs in test_instance_kernels_vs_oracle_exact_inputs
            assert abs(p["score"] - g[f"inst_{key}_score"][j]) < t_score
            m = rle.decode(p["segmentation"]).astype(bool)
            assert (m != ref_masks[j]).mean() <= t_pix        # proposals thresholded at 0.5
            assert np.abs(np.array(p["bbox"]) - g[f"inst_{key}_bbox"][j]).max() <= 1.0
            assert tuple(p["image_size"]) == (H, W)


def test_instance_kernels_vs_oracle_exact_inputs(dev, golden_dir):
    """Feed the reference's own mask_proposals / patch_tokens to the instance kernels: integer outputs
    (binary masks, sizes, categories, IoU counts) must be bit-exact; scores within fp32 rounding."""
    from zutis_amd import detgen
    from zutis_amd.engine import ZutisEngine
    from oracle import zutis_ref as O, resample as R
    cfg = detgen.TINY
    g = np.load(f"{golden_dir}/e2e_tiny.npz")
    b, H, W, n = int(g["b"]), int(g["H"]), int(g["W"]), int(g["n_cat"])
    eng = _engine(cfg, dev)
    mp, pt = torch.from_numpy(g["mask_proposals"]), torch.from_numpy(g["patch_tokens"])
    text = torch.from_numpy(detgen.text_embeddings(n, cfg.embed_dim))
    binary, cats, scores = O.instance_scores(mp, pt, text)
    masks, sc, ct = eng.instance_candidates(mp[:, -1].to(dev), pt.to(dev), text.to(dev), 0.5, 5.0, (H, W))
    assert np.array_equal(ct.cpu().numpy(), cats)
    assert np.abs(sc.cpu().numpy() - scores).max() < 1e-6
    up = R.bilinear_nchw(mp[:, -1].numpy(), H, W) > 0.5
    assert np.array_equal(masks.cpu().numpy().astype(bool), up)
    iou = eng.mask_iou_matrix(masks[0])
    for i in range(up.shape[1]):
        for j in range(up.shape[1]):
            assert iou[i, j] == O.compute_iou(up[0, i], up[0, j])


# fast: the DINO body runs on fp16 operands and the mask logits are un-normalised (|logit| ~ 30): 1e-3 relative on the logit
@pytest.mark.parametrize("precision,t_obj,t_mask,t_dts", [("fast", 2e-3, 2e-2, 5e-3), ("exact", 2e-5, 4e-4, 2e-4)])
def test_selfmask_engine_vs_reference_golden(dev, golden_dir, precision, t_obj, t_mask, t_dts):
    """SelfMask (DINO ViT-S/8 + decoder + objectness) on the HIP path against the reference's outputs."""
    from zutis_amd import detgen
    from zutis_amd.engine import SelfMaskEngine
    g = np.load(f"{golden_dir}/selfmask.npz")
    eng = SelfMaskEngine({k: torch.from_numpy(v).to(dev) for k, v in detgen.selfmask_state_dict().items()}, precision=precision)
    for tag in ("small", "full"):
        b, H, W = (int(v) for v in g[f"{tag}_shape"])
        x = torch.from_numpy(detgen.images(b, H, W, seed=11)).to(dev)
        out = eng.forward(x)
        mp = out["mask_pred"].cpu().numpy()
        if tag == "full":
            mp = mp[:, :, :, ::2, ::2]
        e_obj = np.abs(out["objectness"].cpu().numpy() - g[f"{tag}_objectness"]).max()
        e_mask = np.abs(mp - g[f"{tag}_mask_pred"]).max()     # un-normalised queries: |logit| ~ 30
        print(f"selfmask {tag}[{precision}]: objectness {e_obj:.2e} mask_pred {e_mask:.2e}")
        assert e_obj < t_obj and e_mask < t_mask
        inf = eng.forward(x, inference=True)
        ref = np.unpackbits(g[f"{tag}_dts"], axis=-1)[..., :W].astype(bool)
        got = inf["dts"].cpu().numpy().astype(bool)
        assert got.shape == (b, H, W)
        assert (got != ref).mean() <= t_dts, (got != ref).mean()
        # and every differing pixel is explained: the oracle's own upsampled probability of the selected query lies within the
        # measured mask error of the 0.5 threshold there (x4 bilinear is a convex combination of mask_pred values)
        from oracle import selfmask_ref as S, zutis_ref as O
        with torch.no_grad():
            Po = O.to_torch_params(detgen.selfmask_state_dict())
            dts_o, idx_o, up_o = S.selfmask_inference(Po, x.cpu())
            e_full = float((out["mask_pred"].cpu() - S.selfmask_forward(Po, x.cpu())["mask_pred"]).abs().max())   # every pixel, not the sub-sample
        assert np.array_equal(np.stack(dts_o).astype(bool), ref)            # the oracle reproduces the reference's masks exactly
        if np.array_equal(inf["index"].cpu().numpy(), idx_o):
            sel = np.stack([up_o[i, idx_o[i]] for i in range(b)])
            unexplained = int(((got != ref) & (np.abs(sel - 0.5) > e_full + 2e-6)).sum())
            assert unexplained == 0, (tag, precision, unexplained, int((got != ref).sum()))


@pytest.mark.parametrize("precision,t_obj,t_mask", [("exact", 2e-5, 4e-4), ("fast", 2e-3, 2e-2)])
def test_selfmask_at_its_working_shape_512x683(dev, precision, t_obj, t_mask):
    """SelfMask at the shape the pseudo-label pipeline runs it (datasets/index_dataset.py:189-204 resizes to 512 on the short
    side: 512x683 -> 64x86 tokens padded to T = 5505 + cls, the flash-attention regime) against the CPU oracle, batch 1
    (selfmask.py:204-237).  Mask pixels may differ from the oracle's only where the oracle's own upsampled probability is
    within the measured mask error of the 0.5 threshold."""
    from zutis_amd import detgen
    from zutis_amd.engine import SelfMaskEngine
    from oracle import selfmask_ref as S, zutis_ref as O
    H, W = 512, 683
    sd = detgen.selfmask_state_dict()
    x = torch.from_numpy(detgen.images(1, H, W, seed=11))
    with torch.no_grad():
        ref = S.selfmask_forward(O.to_torch_params(sd), x)
        dts_ref, idx_ref, up_ref = S.selfmask_inference(O.to_torch_params(sd), x)
    eng = SelfMaskEngine({k: torch.from_numpy(v).to(dev) for k, v in sd.items()}, precision=precision)
    out = eng.forward(x.to(dev))
    e_obj = float((out["objectness"].cpu() - ref["objectness"]).abs().max())
    e_mask = float((out["mask_pred"].cpu() - ref["mask_pred"]).abs().max())
    assert out["mask_pred"].shape == ref["mask_pred"].shape
    assert e_obj < t_obj and e_mask < t_mask, (e_obj, e_mask)
    inf = eng.forward(x.to(dev), inference=True)
    got = inf["dts"].cpu().numpy().astype(bool)
    assert got.shape == (1, H, W)
    ol = ref["objectness_logits"][0].numpy()
    srt = np.sort(ol)
    if srt[-1] - srt[-2] > 4 * t_obj * 4:           # the winning query is unambiguous (sigmoid' <= 1/4): it must be the same one
        diff = got[0] != dts_ref[0].astype(bool)
        unexplained = int((diff & (np.abs(up_ref[0, idx_ref[0]] - 0.5) > e_mask + 2e-6)).sum())
        print(f"selfmask 512x683[{precision}]: objectness {e_obj:.2e} mask_pred {e_mask:.2e}, {int(diff.sum())} of {H * W} mask pixels "
              f"differ, unexplained {unexplained}")
        assert unexplained == 0


def test_selfmask_dropin_module(dev, golden_dir):
    import os, sys
    from zutis_amd import detgen
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zutis_amd", "dropin")
    if d not in sys.path:
        sys.path.insert(0, d)
    from networks.selfmask.selfmask import SelfMask
    net = SelfMask()
    assert len(net.state_dict()) == 267
    net.load_state_dict({k: torch.from_numpy(v) for k, v in detgen.selfmask_state_dict().items()}, strict=True)
    net = net.to(dev).eval()
    g = np.load(f"{golden_dir}/selfmask.npz")
    b, H, W = (int(v) for v in g["small_shape"])
    x = torch.from_numpy(detgen.images(b, H, W, seed=11)).to(dev)
    with torch.no_grad():
        out = net(x, inference=True)
    assert isinstance(out["dts"], list) and out["dts"][0].dtype == torch.uint8 and out["dts"][0].device.type == "cpu"
    ref = np.unpackbits(g["small_dts"], axis=-1)[..., :W].astype(bool)
    assert (torch.stack(out["dts"]).numpy().astype(bool) != ref).mean() < 5e-3
    # bilateral_solver=True (selfmask.py:226-237): "dts_bi" = solver(de-normalised image, dts) > 0.5, here from one batched
    # device solve; must equal the oracle's NumPy/SciPy solver applied to the module's own dts
    from oracle import bilateral_ref as B
    with torch.no_grad():
        out2 = net(x, inference=True, bilateral_solver=True)
    assert len(out2["dts_bi"]) == b and out2["dts_bi"][0].dtype == torch.uint8 and out2["dts_bi"][0].device.type == "cpu"
    for i in range(b):
        soft, _ = B.bilateral_solver_output(B.denormalize_to_u8(x[i].cpu().numpy()), out2["dts"][i].numpy())
        assert np.array_equal(out2["dts_bi"][i].numpy().astype(bool), soft > 0.5)


@pytest.mark.parametrize("width,layers,patch,grid,embed,B", [(128, 2, 14, 3, 64, 3), (1024, 2, 14, 24, 768, 2)])
def test_clip_encode_image_vs_oracle(dev, width, layers, patch, grid, embed, B):
    """CLIP encode_image (utils/extract_image_embeddings.py:72-73): CLS -> ln_post -> @proj -> L2, fixed pos-embed.
    Second case = ViT-L/14@336 geometry (D=1024, K=588 padded to 640, T=577) with 2 layers."""
    from zutis_amd import detgen
    from zutis_amd.engine import ClipImageEncoder
    from oracle import zutis_ref as O
    cfg = detgen.ZutisConfig(width=width, layers=layers, patch=patch, grid=grid, embed_dim=embed)
    sd = {k: v for k, v in detgen.zutis_state_dict(cfg).items() if k.startswith("encoder.")}
    x = torch.from_numpy(detgen.images(B, patch * grid, patch * grid, seed=5))
    with torch.no_grad():
        ref = O.clip_encode_image(O.to_torch_params(sd), x, patch).numpy()
    enc = ClipImageEncoder({k.replace("encoder.", "visual."): torch.from_numpy(v).to(dev) for k, v in sd.items()}, patch)
    got = enc.encode_image(x.to(dev)).cpu().numpy()
    assert got.shape == (B, embed)
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-5
    assert np.abs(got - ref).max() < 1e-3
    with pytest.raises(Exception):
        enc.encode_image(torch.zeros((1, 3, patch * (grid + 1), patch * grid), device=dev))   # CLIP needs its native grid


def test_running_score_dropin(dev, golden_dir):
    import os, sys
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zutis_amd", "dropin")
    if d not in sys.path:
        sys.path.insert(0, d)
    from utils.running_score import RunningScore
    g = np.load(f"{golden_dir}/ops.npz")
    rs = RunningScore(7, device=dev)
    rs.update(g["rs_gt"], g["rs_pred"])                               # numpy in, as trainer.py:347
    assert np.array_equal(rs.confusion_matrix, g["rs_hist"])
    sc, _ = rs.get_scores()
    assert np.allclose([sc["Pixel Acc"], sc["Mean Acc"], sc["FreqW Acc"], sc["Mean IoU"]], g["rs_scores"], rtol=0, atol=1e-12)
    rs.reset()
    rs.update(torch.from_numpy(g["rs_gt"]).to(dev), torch.from_numpy(g["rs_pred"]).to(dev))   # device tensors
    assert np.array_equal(rs.confusion_matrix, g["rs_hist"])


@pytest.mark.parametrize("precision", ["exact", "fast"])
def test_c4_geometry_518px_920_classes(dev, precision):
    """BASELINE config 4 geometry: ViT-B/16 @518 px (conv floor => 32x32 grid, T=1025, M=4096), 920 classes, b=1,
    against the CPU oracle — logits AND the 920-class label map; plus size-independent properties (unit-norm tokens, sigmoid
    range, argmax idempotence)."""
    from zutis_amd import detgen
    from oracle import zutis_ref as O
    cfg = detgen.VIT_B16
    eng = _engine(cfg, dev, precision)
    x = torch.from_numpy(detgen.images(1, 518, 518, seed=2))
    text = torch.from_numpy(detgen.text_embeddings(920, cfg.embed_dim))
    out = eng.forward(x.to(dev))
    assert out["mask_proposals"].shape == (1, 6, 100, 64, 64) and out["patch_tokens"].shape == (1, 64, 64, 512)
    pt = out["patch_tokens"]
    assert (pt.norm(dim=-1) - 1).abs().max().item() < 1e-5
    assert 0 <= out["mask_proposals"].min().item() and out["mask_proposals"].max().item() <= 1
    lo = eng.semantic_logits_lowres(pt, text.to(dev))
    labels = eng.predict_semantic(pt, text.to(dev), (518, 518))
    assert labels.shape == (1, 518, 518) and int(labels.max()) < 920
    full = eng.predict_semantic(pt, text.to(dev), (518, 518), return_logits=True)
    assert torch.equal(full.argmax(dim=1), labels)                    # fused upsample+argmax == argmax of the materialised logits
    with torch.no_grad():
        ref = O.zutis_forward(O.to_torch_params(detgen.zutis_state_dict(cfg)), x, cfg.patch, cfg.dec_heads)
        ref_lo = O.semantic_logits_lowres(ref["patch_tokens"], text).numpy()
    err = float(np.abs(lo.cpu().numpy() - ref_lo).max())
    assert err < TOLS[precision][0]
    # the 920-class labels against the ORACLE's (zutis.py:366-372: F.interpolate(bilinear) -> argmax over 920 classes at 518x518)
    from oracle import resample as R
    from oracle.parity import unexplained_label_mismatches
    lab_ref = R.bilinear_argmax_nchw(ref_lo, 518, 518)
    n_mis, n_bad, worst = unexplained_label_mismatches(labels.cpu().numpy(), lab_ref, ref_lo, err, (518, 518))
    print(f"c4[{precision}]: logits {err:.2e}; {n_mis} of {518 * 518} labels differ from the oracle's, unexplained {n_bad} (margin <= {worst:.2e})")
    assert n_bad == 0, (n_mis, n_bad, worst, err)
    # and bit-exact given the oracle's own low-res logits
    lab2 = torch.empty((1, 518, 518), dtype=torch.int64, device=dev)
    from zutis_amd import ops
    ops.upsample_argmax(torch.from_numpy(ref_lo).to(dev), lab2, 1, 920, 64, 64, 518, 518)
    assert np.array_equal(lab2.cpu().numpy(), lab_ref)


def test_forward_graphed_matches_eager(dev):
    """hipGraph replay (batch-1 latency path) returns exactly what the eager launch sequence returns, across replays and
    for a second input shape."""
    from zutis_amd import detgen
    cfg = detgen.TINY
    eng = _engine(cfg, dev)
    for (H, W) in [(80, 112), (64, 96)]:
        for seed in (0, 1, 2):
            x = torch.from_numpy(detgen.images(1, H, W, seed=seed)).to(dev)
            a = eng.forward(x)
            a = {k: v.clone() for k, v in a.items()}
            b = eng.forward_graphed(x)
            assert torch.equal(a["mask_proposals"], b["mask_proposals"]) and torch.equal(a["patch_tokens"], b["patch_tokens"])


def test_forward_graphed_shape_a_b_a_and_fork(dev):
    """A graph bakes in pointers to its shape's scratch buffers.  The engine's buffer cache drops a name's buffers when
    another shape arrives, so shape A, then B, then A again must not replay A into freed memory: between the two A
    replays a pile of fresh tensors is allocated (they would land in the freed blocks) and must survive untouched.
    fork() must not inherit the parent's captured graphs."""
    from zutis_amd import detgen
    cfg = detgen.TINY
    eng = _engine(cfg, dev)
    xa = torch.from_numpy(detgen.images(1, 80, 112, seed=3)).to(dev)
    xb = torch.from_numpy(detgen.images(1, 96, 64, seed=4)).to(dev)
    ref_a = {k: v.clone() for k, v in eng.forward(xa).items()}
    ref_b = {k: v.clone() for k, v in eng.forward(xb).items()}
    ga = eng.forward_graphed(xa)
    assert torch.equal(ga["patch_tokens"], ref_a["patch_tokens"])
    gb = eng.forward_graphed(xb)                         # evicts shape A's buffers from the cache
    assert torch.equal(gb["patch_tokens"], ref_b["patch_tokens"])
    canaries = [torch.full((1 << 16,), float(i), device=dev) for i in range(64)]   # occupy whatever was freed
    ga2 = eng.forward_graphed(xa)
    torch.cuda.synchronize()
    assert torch.equal(ga2["patch_tokens"], ref_a["patch_tokens"]) and torch.equal(ga2["mask_proposals"], ref_a["mask_proposals"])
    assert all(bool((c == float(i)).all()) for i, c in enumerate(canaries))
    f = eng.fork()
    assert len(f._graphs) == 0 and len(eng._graphs) == 2
    assert torch.equal(f.forward(xa)["patch_tokens"], ref_a["patch_tokens"])
    # a parameter update invalidates the captured graph (it holds the old packed weights)
    with torch.no_grad():
        eng.params["encoder.proj"].mul_(-1.0)
    upd = eng.forward_graphed(xa)                        # (the version check runs behind the replay: the stale replay is dropped, not returned)
    assert not torch.equal(upd["patch_tokens"], ref_a["patch_tokens"])
    assert torch.equal(upd["patch_tokens"], eng.forward(xa)["patch_tokens"].clone())
    assert torch.equal(eng.forward_graphed(xa)["patch_tokens"], upd["patch_tokens"])


def test_dropin_behind_a_pinned_dataloader_across_the_first_capture(dev):
    """The reference's validation loaders run with pin_memory=True (configs/*.yaml val_dataloader_kwargs, index_dataset.py:189): their
    pin-memory thread allocates pinned host memory and records events WHILE the drop-in captures its hipGraph on the second occurrence of
    a shape.  The capture is thread-local, so neither the loader thread nor the capture breaks; every output equals the eager one bit for
    bit; and the graphs live in their own small LRU (not in the geometry cache)."""
    from torch.utils.data import DataLoader, TensorDataset
    from zutis_amd import detgen
    cfg = detgen.TINY
    net = _dropin_zutis(cfg, dev, 5).requires_grad_(False)
    imgs = torch.cat([torch.from_numpy(detgen.images(1, 80, 112, seed=s)) for s in range(10)])
    net.use_hip_graph = False
    want = [net(imgs[i:i + 1].to(dev))["patch_tokens"].clone() for i in range(10)]
    net.use_hip_graph = True
    loader = DataLoader(TensorDataset(imgs), batch_size=1, num_workers=2, pin_memory=True)
    got = []
    for (xb,) in loader:                                  # image 0 eager, image 1 captures (loader threads busy), 2.. replay
        assert xb.is_pinned()
        got.append(net(xb.to(dev, non_blocking=True))["patch_tokens"].clone())
    assert len(got) == 10 and all(torch.equal(a, b) for a, b in zip(got, want))
    eng = net._get_engine()
    assert len(eng._graphs) == 1 and next(iter(eng._graphs.values()))["graph"] is not None
    # LRU of its own: more shapes than the cap keep only the newest, and the geometry tables are not evicted by graphs
    for k, (H, W) in enumerate([(64, 96), (96, 64), (64, 64), (80, 96), (96, 80), (64, 112), (112, 64)]):
        xk = torch.from_numpy(detgen.images(1, H, W, seed=k)).to(dev)
        for _ in range(3):
            o = net(xk)
        net.use_hip_graph = False
        assert torch.equal(o["patch_tokens"], net(xk)["patch_tokens"])
        net.use_hip_graph = True
    assert len(eng._graphs) == eng._GRAPH_CAP and not any(isinstance(k, tuple) and k and k[0] == "graph" for k in eng._geo)
    assert torch.equal(net(imgs[3:4].to(dev))["patch_tokens"], want[3])       # an evicted shape: eager / re-captured, same bits


@pytest.mark.parametrize("precision,t_mask,t_tok", [("exact", 2e-5, 2e-6), ("fast", 2e-3, 2e-4)])
def test_batch_invariance_full_size(dev, precision, t_mask, t_tok):
    """Size-independent property at the BASELINE geometry (ViT-B/16 @336): images are independent, and every reduction runs over K /
    keys / one image in an order fixed by the shape, so image i's outputs are BITWISE the same at any position of a batch and in
    batches of different sizes that select the same kernels (here 5 and 6 images: what makes rank-sharded evaluation with equal
    shards reproduce the single-GPU result exactly).  Kernel selection has four batch-reading rules — split-K of the
    N = D GEMMs up to 2048 token rows, the key split of self-attention up to 128 (image, head, query block) items, the long-sequence key split
    (T >= 2048: not at this geometry), the few-row GEMM kernel up to 128 rows and 512 workgroups (shape_rules.gemm_k_split / self_attention_key_split /
    long_sequence_key_split, gemm_skinny.h) — plus the engine's cross_ksplit setting, which reads the batch only as "auto"; across them (one image alone) the sums are re-associated: fp32-class
    agreement at `exact` (measured 1e-7 tokens / 5e-7 masks), the precision's own rounding level at `fast`."""
    from zutis_amd import detgen
    cfg = detgen.VIT_B16
    eng = _engine(cfg, dev, precision)
    x = torch.from_numpy(detgen.images(6, 336, 336, seed=4)).to(dev)
    text = torch.from_numpy(detgen.text_embeddings(81, cfg.embed_dim)).to(dev)
    full = {k: v.clone() for k, v in eng.forward(x).items()}
    lab_full = eng.predict_semantic(full["patch_tokens"], text, (336, 336)).clone()
    perm = [2, 0, 5, 1, 4]                                             # five of the six, in another order (5 and 6 images: the batch side of every threshold)
    sub = {k: v.clone() for k, v in eng.forward(x[perm].contiguous()).items()}
    lab_sub = eng.predict_semantic(sub["patch_tokens"], text, (336, 336)).clone()
    for j, i in enumerate(perm):
        assert torch.equal(sub["mask_proposals"][j], full["mask_proposals"][i])
        assert torch.equal(sub["patch_tokens"][j], full["patch_tokens"][i])
        assert torch.equal(lab_sub[j], lab_full[i])
    again = eng.forward(x)
    assert torch.equal(again["mask_proposals"], full["mask_proposals"]) and torch.equal(again["patch_tokens"], full["patch_tokens"])
    for i in (0, 5):                                                   # one image alone: other kernels, the same numbers to fp32 re-association
        one = eng.forward(x[i:i + 1].contiguous())
        assert float((one["mask_proposals"][0] - full["mask_proposals"][i]).abs().max()) < t_mask
        assert float((one["patch_tokens"][0] - full["patch_tokens"][i]).abs().max()) < t_tok
        lab = eng.predict_semantic(one["patch_tokens"], text, (336, 336))[0]
        assert float((lab != lab_full[i]).float().mean()) < (1e-4 if precision == "exact" else 2e-3)   # argmax flips only on near-ties between two classes
    pt = full["patch_tokens"]
    assert (pt.norm(dim=-1) - 1).abs().max().item() < 1e-5
    assert 0 <= full["mask_proposals"].min().item() and full["mask_proposals"].max().item() <= 1


def test_cross_attention_key_split_by_the_batch_is_opt_in_and_fp32_class(dev):
    """`engine.cross_ksplit = "auto"` (bench.py's config-4 runs: fewer (image, head) pairs than CUs) splits the cross-attention keys by the
    batch: 2 images x 8 heads -> a split of 8 (1024 keys); the outputs are those of the default (unsplit) engine to fp32 re-association,
    and the default engine is untouched (equal rank shards must reproduce a batch bit for bit)."""
    from zutis_amd import detgen
    cfg = detgen.VIT_B16
    eng = _engine(cfg, dev, "exact")
    assert eng.cross_ksplit == 1
    x = torch.from_numpy(detgen.images(2, 256, 256, seed=12)).to(dev)            # 16 x 16 patches -> 1024 memory tokens: the split's threshold
    from zutis_amd import _lib

    def counted(e):
        counts = {}
        _lib.COUNTER = counts
        try:
            o = {k: v.clone() for k, v in e.forward(x).items()}
        finally:
            _lib.COUNTER = None
        return o, counts.get("zh_attention_f16_splitk", 0)
    ref, n_ref = counted(eng)
    auto = eng.fork()
    auto.cross_ksplit = "auto"
    out, n_auto = counted(auto)
    assert n_auto - n_ref == cfg.dec_layers        # every decoder layer's cross-attention took the split form (the two-image encoder splits its keys either way)
    assert float((out["mask_proposals"] - ref["mask_proposals"]).abs().max()) < 2e-5
    assert float((out["patch_tokens"] - ref["patch_tokens"]).abs().max()) < 2e-6
    again = eng.forward(x)
    assert torch.equal(again["patch_tokens"], ref["patch_tokens"])             # the parent engine keeps its own (unsplit) arithmetic


def test_launch_plan_refuses_stale_weights(dev):
    from zutis_amd import detgen, _lib
    cfg = detgen.TINY
    eng = _engine(cfg, dev)
    text = torch.from_numpy(detgen.text_embeddings(5, cfg.embed_dim)).to(dev)
    p = eng.build_plan((1, 3, 64, 64), text, (64, 64))
    eng.run_plan(p, torch.from_numpy(detgen.images(1, 64, 64)).to(dev))
    with torch.no_grad():
        eng.params["encoder.proj"].mul_(-1.0)
    with pytest.raises(_lib.ZutisHipError, match="parameters changed"):
        eng.run_plan(p)


def test_launch_plan_replay_matches_eager(dev):
    """Native launch plan (zh_plan_run): bitwise the eager result, across replays with new inputs, and with two plans
    interleaved on two streams (zh_plan_run2)."""
    from zutis_amd import detgen, plan as zplan
    cfg = detgen.TINY
    text = torch.from_numpy(detgen.text_embeddings(7, cfg.embed_dim)).to(dev)
    eng, ref_eng = _engine(cfg, dev), _engine(cfg, dev)
    p = eng.build_plan((2, 3, 80, 112), text, (80, 112))
    assert p["plan"].n > 20, p["plan"].n
    for seed in (0, 1, 2):
        x = torch.from_numpy(detgen.images(2, 80, 112, seed=seed)).to(dev)
        out, labels = eng.run_plan(p, x)
        ref = ref_eng.forward(x)
        assert torch.equal(out["mask_proposals"], ref["mask_proposals"]) and torch.equal(out["patch_tokens"], ref["patch_tokens"])
        assert torch.equal(labels, ref_eng.predict_semantic(ref["patch_tokens"], text, (80, 112)))
    # two engines / two plans / two streams, interleaved from C
    eng_b = _engine(cfg, dev)
    pb = eng_b.build_plan((2, 3, 80, 112), text, (80, 112))
    xa = torch.from_numpy(detgen.images(2, 80, 112, seed=5)).to(dev)
    xb = torch.from_numpy(detgen.images(2, 80, 112, seed=6)).to(dev)
    p["x"].copy_(xa); pb["x"].copy_(xb)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    zplan.run2(p["plan"], sa.cuda_stream, pb["plan"], sb.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(p["labels"], ref_eng.predict_semantic(ref_eng.forward(xa)["patch_tokens"], text, (80, 112)))
    assert torch.equal(pb["labels"], ref_eng.predict_semantic(ref_eng.forward(xb)["patch_tokens"], text, (80, 112)))


@pytest.mark.parametrize("tag,cfgname,n", [("tiny", "TEXT_TINY", 9), ("b", "TEXT_B", 6)])
def test_text_tower_matches_reference_golden(dev, golden_dir, tag, cfgname, n):
    """ClipTextEncoder.encode_text vs CLIP.encode_text of the real reference (clip_arch.py:534-547, golden) and the oracle;
    prompt ensembling vs the reference's extract_text_embeddings loop.  fp32 logits tolerance 1e-3 applies to the unit-norm
    embeddings; raw (un-normalised) embeddings are O(1..10) and are compared relatively."""
    from zutis_amd import detgen
    from zutis_amd.engine import ClipTextEncoder
    from oracle import zutis_ref as O
    g = np.load(f"{golden_dir}/text.npz")
    tc = getattr(detgen, cfgname)
    sd = detgen.clip_text_state_dict(tc)
    eng = ClipTextEncoder({k: torch.from_numpy(v).to(dev) for k, v in sd.items()})
    tok = torch.from_numpy(detgen.text_tokens(n, tc))
    e = eng.encode_text(tok.to(dev)).cpu().numpy()
    ref = g[f"{tag}_encode_text"]
    un = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
    assert np.abs(un(e) - un(ref)).max() < 1e-3
    assert np.abs(e - ref).max() < 2e-3 * np.abs(ref).max()
    if tag == "tiny":
        toks = torch.from_numpy(detgen.text_tokens(15, tc, seed=23)).view(3, 5, -1)
        pe = eng.prompt_ensemble(toks.to(dev)).cpu().numpy()
        assert np.abs(pe - g["tiny_prompt_ensemble"]).max() < 1e-3
        assert np.abs(np.linalg.norm(pe, axis=1) - 1).max() < 1e-6
        # chunked == unchunked, and the drop-in model object through a reference-shaped loop
        eng2 = ClipTextEncoder({k: torch.from_numpy(v).to(dev) for k, v in sd.items()}, chunk=4)
        assert torch.equal(eng2.encode_text(tok.to(dev)).cpu(), torch.from_numpy(e))
        from zutis_amd.dropin.networks.clip_text import HipClipText, prompt_engineering_batched
        m = HipClipText({k: torch.from_numpy(v) for k, v in sd.items()}, device=dev)
        table = {f"t{t}|cat{c}|": toks[c, t] for c in range(3) for t in range(5)}
        res = prompt_engineering_batched(m, lambda texts: torch.stack([table[s] for s in texts]), [f"cat{c}" for c in range(3)],
                                         [f"t{t}|{{}}|" for t in range(5)])
        assert np.abs(np.stack([res[f"cat{c}"].cpu().numpy() for c in range(3)]) - g["tiny_prompt_ensemble"]).max() < 1e-3
        with pytest.raises(IndexError):
            eng.encode_text(torch.full((1, tc.context_length), tc.vocab_size, dtype=torch.int64))


def test_causal_attention_kernel(dev):
    from zutis_amd import ops
    for (B, H, dh, T) in [(2, 2, 64, 77), (1, 3, 64, 200), (2, 1, 96, 130)]:
        D = H * dh
        g = torch.Generator().manual_seed(T)
        q, k, v = (torch.randn((B, T, D), generator=g).half() for _ in range(3))
        qh, kh, vh = (t.float().view(B, T, H, dh).transpose(1, 2) for t in (q, k, v))
        s = qh @ kh.transpose(-1, -2) / math.sqrt(dh) + torch.full((T, T), float("-inf")).triu_(1)
        ref = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, T, D)
        o = torch.empty((B, T, D), dtype=torch.float16, device=dev)
        ops.attention(q.to(dev), k.to(dev), v.to(dev), o, batch=B, heads=H, Tq=T, Tk=T, head_dim=dh, ldq=D, ldk=D, ldv=D, ldo=D,
                      strideQ=T * D, strideK=T * D, strideV=T * D, strideO=T * D, causal=True)
        assert (o.float().cpu() - ref).abs().max().item() < 4e-3


def test_rank_sharded_evaluation_equals_full_batch(dev):
    """BASELINE config 2 at its full batch (32 x 336^2, 81 classes): evaluating the two contiguous rank shards [0,16) and
    [16,32) (what world_size 2 does, zutis_amd/distributed.shard_range) and concatenating in rank order gives BITWISE the
    logits and labels of the single-GPU batch — the all-gather in bench.py reproduces the single-GPU result exactly."""
    from zutis_amd import detgen
    from zutis_amd.distributed import shard_range
    cfg = detgen.VIT_B16
    eng = _engine(cfg, dev)
    x = torch.from_numpy(detgen.images(32, 336, 336, seed=9)).to(dev)
    text = torch.from_numpy(detgen.text_embeddings(81, cfg.embed_dim)).to(dev)
    full = eng.forward(x)
    lo_full = eng.semantic_logits_lowres(full["patch_tokens"], text).clone()
    lab_full = eng.predict_semantic(full["patch_tokens"], text, (336, 336)).clone()
    parts_lo, parts_lab = [], []
    for r in range(2):
        a, b = shard_range(32, r, 2)
        out = eng.forward(x[a:b].contiguous())
        parts_lo.append(eng.semantic_logits_lowres(out["patch_tokens"], text).clone())
        parts_lab.append(eng.predict_semantic(out["patch_tokens"], text, (336, 336)).clone())
    assert torch.equal(torch.cat(parts_lo), lo_full) and torch.equal(torch.cat(parts_lab), lab_full)
    assert int(lab_full.min()) >= 0 and int(lab_full.max()) < 81


def test_forked_engine_eager_predict(dev):
    """fork(): same weights, own buffers — a fork's first eager predict must not trust the parent's cached f16 copies."""
    from zutis_amd import detgen
    cfg = detgen.TINY
    eng = _engine(cfg, dev)
    text = torch.from_numpy(detgen.text_embeddings(7, cfg.embed_dim)).to(dev)
    x = torch.from_numpy(detgen.images(2, 80, 112, seed=3)).to(dev)
    out = eng.forward(x)
    ref = eng.predict_semantic(out["patch_tokens"], text, (80, 112)).clone()
    f = eng.fork()
    out2 = f.forward(x)
    assert torch.equal(out2["patch_tokens"], out["patch_tokens"])
    assert torch.equal(f.predict_semantic(out2["patch_tokens"], text, (80, 112)), ref)
    # tokens that did not come from the engine's last forward are re-cast
    other = torch.nn.functional.normalize(torch.randn_like(out["patch_tokens"]), dim=-1)
    a = eng.predict_semantic(other, text, (80, 112)).clone()
    eng.forward(x)
    assert torch.equal(eng.predict_semantic(other, text, (80, 112)), a)
