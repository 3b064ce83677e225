"""CPU: the oracle (oracle/) against the golden vectors produced by the REAL reference (oracle/gen_golden.py)."""
import numpy as np
import pytest
import torch

from oracle import resample as R
from oracle import zutis_ref as O
from zutis_amd import detgen


@pytest.mark.parametrize("tag,cfgname", [("tiny", "TINY"), ("vitb32_224", "VIT_B32"), ("vitb16_336", "VIT_B16")])
def test_oracle_e2e_matches_reference(golden_dir, tag, cfgname):
    cfg = getattr(detgen, cfgname)
    g = np.load(f"{golden_dir}/e2e_{tag}.npz")
    b, H, W, n = int(g["b"]), int(g["H"]), int(g["W"]), int(g["n_cat"])
    P = O.to_torch_params(detgen.zutis_state_dict(cfg))
    x = torch.from_numpy(detgen.images(b, H, W))
    text = torch.from_numpy(detgen.text_embeddings(n, cfg.embed_dim))
    with torch.no_grad():
        enc, _, _ = O.clip_vit_forward(P, x, cfg.patch)
        out = O.zutis_forward(P, x, cfg.patch, cfg.dec_heads)
        lo = O.semantic_logits_lowres(out["patch_tokens"], text).numpy()
        labels = O.predict_semantic(out["patch_tokens"], text, size=tuple(g["size"]))
    assert np.abs(lo - g["logits_lo"]).max() < 2e-6
    assert (labels == g["labels"]).mean() > 0.9995
    mp, pt = out["mask_proposals"].numpy(), out["patch_tokens"].numpy()
    if "mask_proposals" in g:
        assert np.abs(enc.numpy() - g["enc_tokens"]).max() < 2e-5
        assert np.abs(mp - g["mask_proposals"]).max() < 2e-6
        assert np.abs(pt - g["patch_tokens"]).max() < 2e-6
        lf = O.predict_semantic(out["patch_tokens"], text, size=tuple(g["size"]), return_logits=True).numpy()
        assert np.abs(lf - g["logits_full"]).max() < 2e-6
    else:
        assert np.abs(enc.numpy()[:, ::7, ::5] - g["enc_tokens_sub"]).max() < 5e-5
        assert np.abs(mp[:, :, ::9, ::3, ::3] - g["mask_proposals_sub"]).max() < 2e-6
        assert np.abs(pt[:, ::3, ::3, ::4] - g["patch_tokens_sub"]).max() < 2e-6


def test_oracle_instance_predict_matches_reference(golden_dir):
    """Instance branch (zutis.py:374-470): same masks / categories / scores as the reference for every NMS type."""
    cfg = detgen.TINY
    g = np.load(f"{golden_dir}/e2e_tiny.npz")
    b, H, W, n = int(g["b"]), int(g["H"]), int(g["W"]), int(g["n_cat"])
    mp = torch.from_numpy(g["mask_proposals"])
    pt = torch.from_numpy(g["patch_tokens"])
    text = torch.from_numpy(detgen.text_embeddings(n, cfg.embed_dim))
    binary, cats, scores = O.instance_scores(mp, pt, text)
    up = R.bilinear_nchw(mp[:, -1].numpy(), H, W) > 0.5
    for nms in ("hard", "linear", "gaussian", None):
        key = str(nms).lower()
        got = []
        for i in range(b):
            if nms is None:
                got += [(i, int(c), q, float(s)) for q, (c, s) in enumerate(zip(cats[i], scores[i])) if c != 0 and up[i, q].sum() > 0]
            else:
                got += [(i, c, q, s) for (c, q, s) in O.mask_nms(up[i], scores[i], cats[i], nms)]
        assert len(got) == int(g[f"inst_{key}_n"])
        if not got:
            continue
        ref_masks = np.unpackbits(g[f"inst_{key}_masks"], axis=-1)[..., :W].astype(bool)
        for j, (i, c, q, s) in enumerate(got):
            assert i == g[f"inst_{key}_img"][j] and c == g[f"inst_{key}_cat"][j]
            assert abs(s - g[f"inst_{key}_score"][j]) < 1e-6
            assert np.array_equal(up[i, q], ref_masks[j])


@pytest.mark.parametrize("thr", [0.5, 0.7, 0.3])
def test_float64_instance_scores_agree_with_the_fp32_oracle(thr):
    """instance_scores on .double() inputs with threshold = fp32(thr) is the float64 reference of the GPU scoring tests: the same
    binary masks as the fp32 form (torch compares an fp32 tensor with a Python scalar in fp32), the same categories wherever the
    float64 top-two probabilities are more than 1e-6 apart, scores within 1e-6."""
    g = torch.Generator().manual_seed(int(thr * 10))
    B, Q, h, w, E, n = 2, 20, 12, 15, 64, 30
    t = np.float32(thr)
    mp = torch.rand((B, Q, h, w), generator=g)
    mp.view(-1)[::7] = float(t)                                     # proposals equal to fp32(thr): off in both forms
    mp.view(-1)[3::14] = float(np.nextafter(t, np.float32(1)))
    pt = torch.randn((B, h, w, E), generator=g) + torch.randn((B, 1, 1, E), generator=g)
    text = torch.from_numpy(detgen.text_embeddings(n, E))
    b32, cat32, score32 = O.instance_scores(mp, pt, text, threshold=thr)
    b64, cat64, score64 = O.instance_scores(mp.double(), pt.double(), text.double(), threshold=float(t))
    assert torch.equal(b32, b64) and b32.view(-1)[::7].sum() == 0
    if thr == 0.3:
        assert bool((mp.double().view(-1)[::7] > thr).all())      # a float64 compare with 0.3 itself would set them
    assert score64.dtype == np.float64 and np.abs(score64 - score32).max() < 1e-6
    bf = b64.flatten(2).double()
    avg = torch.einsum("bqn,bnc->bqc", bf, pt.double().flatten(1, 2)) / (bf.sum(-1, keepdim=True) + 1e-7)
    prob = torch.sigmoid(torch.einsum("nc,bqc->bqn", text.double(), avg / (avg.norm(dim=-1, keepdim=True) + 1e-7)) * 5.0)
    top2 = prob.topk(2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1] > 1e-6).numpy()
    assert clear.mean() > 0.9 and np.array_equal(cat64[clear], cat32[clear])
    assert np.array_equal(cat64, prob.argmax(-1).numpy())


def test_oracle_ops_match_reference(golden_dir):
    g = np.load(f"{golden_dir}/ops.npz")
    for gr, (h, w) in [(14, (21, 21)), (14, (32, 32)), (7, (7, 7)), (14, (30, 40)), (4, (5, 7))]:
        pe = torch.from_numpy(detgen.det_normal(f"pe_{gr}", (gr * gr + 1, 48)))
        got = O.interpolate_positional_embedding(pe, h, w).numpy()
        assert np.abs(got - g[f"posembed_g{gr}_{h}x{w}"]).max() < 5e-6
    assert np.abs(O.sine_pe(10, 14, 96).numpy() - g["sine_10x14"]).max() < 1e-6
    assert np.abs(O.sine_pe(12, 17, 768).numpy() - g["sine_12x17"]).max() < 1e-6
    assert np.abs(R.bilinear_up2_cl(detgen.det_normal("up2", (2, 5, 7, 24))) - g["up2"]).max() < 1e-6
    for (H, W) in [(80, 112), (77, 145)]:   # ATen generic kernel (H+W > 128): bit-exact incl. exact ties
        assert np.array_equal(R.bilinear_argmax_nchw(g["argmax_lo"], H, W), g[f"argmax_labels_{H}x{W}"])
    hist = O.confusion_hist(g["rs_gt"], g["rs_pred"], 7)
    assert np.array_equal(hist, g["rs_hist"].astype(np.int64))
    sc, _ = O.scores_from_hist(hist)
    assert np.allclose([sc["Pixel Acc"], sc["Mean Acc"], sc["FreqW Acc"], sc["Mean IoU"]], g["rs_scores"], rtol=0, atol=1e-12)
    assert abs(O.compute_iou(g["iou_m1"], g["iou_m2"]) - float(g["iou"])) < 1e-12


def test_oracle_bilinear_is_bit_exact_vs_aten():
    """Pins oracle/resample.py to ATen's generic CPU kernel (the one the reference reaches for H+W > 128)."""
    import torch.nn.functional as F
    x = torch.from_numpy(detgen.det_normal("bil", (2, 5, 21, 21)))
    for (H, W) in [(336, 336), (427, 640), (100, 63), (375, 500)]:
        assert np.array_equal(R.bilinear_nchw(x.numpy(), H, W), F.interpolate(x, size=(H, W), mode="bilinear").numpy())


def test_detgen_is_deterministic_and_complete():
    sd = detgen.zutis_state_dict(detgen.VIT_B16)
    assert len(sd) == 275                                 # 275 keys for ViT-B/16
    assert sd["encoder.transformer.resblocks.3.attn.in_proj_weight"].shape == (2304, 768)
    a = detgen.det_normal("x", (1000,), seed=3)
    assert np.array_equal(a, detgen.det_normal("x", (1000,), seed=3))
    assert abs(a.mean()) < 0.15 and abs(a.std() - 1) < 0.1
    assert abs(float(a[0]) - float(detgen.det_normal("x", (1,), seed=3)[0])) == 0


def test_selfmask_oracle_matches_reference(golden_dir):
    from oracle import selfmask_ref as S
    g = np.load(f"{golden_dir}/selfmask.npz")
    P = O.to_torch_params(detgen.selfmask_state_dict())
    b, H, W = (int(v) for v in g["small_shape"])
    x = torch.from_numpy(detgen.images(b, H, W, seed=11))
    with torch.no_grad():
        o = S.selfmask_forward(P, x)
        dts, idx, _ = S.selfmask_inference(P, x)
    assert np.abs(o["objectness"].numpy() - g["small_objectness"]).max() < 2e-6
    assert np.abs(o["mask_pred"].numpy() - g["small_mask_pred"]).max() < 5e-5
    assert np.array_equal(np.stack(dts).astype(bool), np.unpackbits(g["small_dts"], axis=-1)[..., :W].astype(bool))


def test_bilateral_oracle_matches_reference(golden_dir):
    """Grid size, nnz of every blur matrix, bistochastisation vectors (bit-exact), CG iteration count, soft output and
    post-processed component against utils/bilateral_solver.py run in the authoring container."""
    from oracle import bilateral_ref as B
    g = np.load(f"{golden_dir}/bilateral.npz")
    ramp = np.repeat(np.arange(0, 256, 16, dtype=np.uint8)[None, :, None], 3, axis=2)
    c = B.grid_coords(ramp)
    assert c[:, 2].tolist() == [0, 0, 1, 3, 3, 5, 6, 7, 7, 9, 10, 10, 12, 12, 14, 15]      # SURVEY.md §8c known answer
    assert np.array_equal(c[:, 2], g["ramp_luma_bins"]) and np.array_equal(c[:, 3:], g["ramp_chroma_bins"])
    for tag in "abc":
        h, w, seed = (int(v) for v in g[f"{tag}_hw"])
        rgb = detgen.selfmask_like_rgb(h, w, seed=seed)
        grid = B.Grid(rgb)
        assert grid.nvertices == int(g[f"{tag}_nvertices"])
        assert [(grid.nbr[:, d, :] >= 0).sum() for d in range(5)] == g[f"{tag}_nnz"].tolist()
        t = g[f"{tag}_target"].reshape(-1).astype(np.double)
        xhat, its, n, m = B.solve(grid, t, np.ones(t.size) * 0.999)
        assert np.array_equal(n, g[f"{tag}_n"]) and np.array_equal(m, g[f"{tag}_m"])
        assert its == int(g[f"{tag}_cg_iters"])
        soft = xhat.reshape(h, w)
        assert np.abs(soft - g[f"{tag}_soft"]).max() < 1e-12
        assert np.array_equal(B.postprocess(soft), g[f"{tag}_binary"])
    # the EMPTY target (the pseudo-labeller found nothing): the reference's scipy cg returns zeros without iterating (`bnrm2 == 0`) and
    # the post-processing falls back to the all-True mask (bilateral_solver.py:188-193) — not 0 / 0
    soft0, bin0 = B.bilateral_solver_output(detgen.selfmask_like_rgb(96, 128, seed=3), np.zeros((96, 128), np.uint8))
    assert int(g["z_cg_iters"]) == 0 and np.array_equal(soft0, g["z_soft"]) and not soft0.any() and np.array_equal(bin0, g["z_binary"]) and bin0.all()
    x = detgen.det_normal("denorm", (3, 40, 56))
    x[0, 0, :16] = ((np.arange(16) * 16 / 255.0 - 0.485) / 0.229).astype(np.float32)
    assert np.array_equal(B.denormalize_to_u8(x), g["denorm_u8"])


@pytest.mark.parametrize("tag,cfgname,n", [("tiny", "TEXT_TINY", 9), ("b", "TEXT_B", 6)])
def test_text_oracle_matches_reference(golden_dir, tag, cfgname, n):
    """oracle clip_encode_text vs CLIP.encode_text of the real reference class (clip_arch.py:534-547); the prompt
    ensembling vs the reference's own extract_text_embeddings loop (utils/extract_text_embeddings.py:98-115)."""
    g = np.load(f"{golden_dir}/text.npz")
    tc = getattr(detgen, cfgname)
    P = O.to_torch_params(detgen.clip_text_state_dict(tc))
    tok = torch.from_numpy(detgen.text_tokens(n, tc))
    assert (tok.max(dim=1).values == tc.vocab_size - 1).all() and (tok[:, 0] == tc.vocab_size - 2).all()
    with torch.no_grad():
        e = O.clip_encode_text(P, tok).numpy()
    assert np.abs(e - g[f"{tag}_encode_text"]).max() < 1e-5      # 12 fp32 layers; values O(1)
    if tag == "tiny":
        toks = torch.from_numpy(detgen.text_tokens(15, tc, seed=23)).view(3, 5, -1)
        with torch.no_grad():
            pe = O.prompt_ensemble(P, toks).numpy()
        assert np.abs(pe - g["tiny_prompt_ensemble"]).max() < 1e-6
        assert np.abs(np.linalg.norm(pe, axis=1) - 1).max() < 1e-6


def test_a4_build_model_convert_weights_vs_reference(golden_dir):
    """build_model / convert_weights (clip_arch.py:566-627) as executed by the reference constructor: architecture inferred
    from the state_dict keys, conv / Linear / attention / proj values rounded through fp16, LayerNorm + class / positional
    embeddings untouched.  The drop-in's restatement (convert_weight_like_reference + its key-based inference) must
    reproduce the reference's resulting encoder parameters bit for bit, and the oracle forward on them its tokens."""
    import os, sys
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zutis_amd", "dropin")
    if d not in sys.path:
        sys.path.insert(0, d)
    from networks.zutis import ZUTIS
    cfg = detgen.A4_TINY
    g = np.load(f"{golden_dir}/a4_build_model.npz")
    csd = {k: torch.from_numpy(v) for k, v in detgen.clip_full_state_dict(cfg).items()}
    net = ZUTIS(categories=[f"c{i}" for i in range(7)], clip_arch="ViT-B/16", n_queries=cfg.n_queries, n_decoder_layers=cfg.dec_layers,
                n_heads=cfg.dec_heads, device=torch.device("cpu"), text_embeddings=torch.from_numpy(detgen.text_embeddings(7, cfg.embed_dim)),
                clip_state_dict=csd)
    enc = net.encoder
    assert [enc.width, enc.transformer.layers, enc.patch_size, enc.input_resolution, enc.output_dim] == list(g["arch"])
    sd = enc.state_dict()
    assert sorted("fp_" + k for k in sd) == sorted(k for k in g.files if k.startswith("fp_"))
    n_rounded = 0
    for k, v in sd.items():
        a = v.numpy().astype(np.float64).reshape(-1)
        fp = np.concatenate([[a.sum(), np.abs(a).sum(), (a * a).sum()], a[:8], [1.0]])
        assert np.array_equal(fp, g["fp_" + k]), k
        n_rounded += int(not torch.equal(v, csd["visual." + k].float()))
    assert n_rounded == 2 + 8 * cfg.layers            # conv1, proj, and per block 4 weights + 4 biases; LN / embeddings untouched
    P = {"encoder." + k: v for k, v in sd.items()}
    P.update({k: torch.from_numpy(v) for k, v in detgen.zutis_state_dict(cfg).items() if not k.startswith("encoder.")})
    x = torch.from_numpy(detgen.images(2, 80, 112))
    with torch.no_grad():
        tok, _, _ = O.clip_vit_forward(P, x, cfg.patch)
        out = O.zutis_forward(P, x, cfg.patch, cfg.dec_heads)
    assert np.abs(tok.numpy() - g["enc_tokens"]).max() < 2e-5
    assert np.abs(out["mask_proposals"].numpy() - g["mask_proposals"]).max() < 2e-6
    assert np.abs(out["patch_tokens"].numpy() - g["patch_tokens"]).max() < 2e-6


def test_c3_oracle_matches_reference_at_native_resolution(golden_dir):
    """Config 3's shape (ViT-B/16, 480x640, batch 1; weights detgen.c3_state_dict, threshold C3_THRESHOLD, the fixture's text
    rows): oracle forward + instance scoring + greedy NMS vs the reference's outputs — 9 categories, 100 candidates, 17 hard /
    57 linear survivors, emitted in the reference's set() order (33, 2, 67, 73, 80, 50, 20, 54, 31: not ascending)."""
    cfg = detgen.VIT_B16
    g = np.load(f"{golden_dir}/c3_vitb16.npz")
    H, W, thr = 480, 640, detgen.C3_THRESHOLD
    assert int(g["480x640_n"]) >= 5 and len(set(g["480x640_cat"].tolist())) >= 3
    assert list(dict.fromkeys(g["480x640_cat"].tolist())) != sorted(set(g["480x640_cat"].tolist()))
    P = O.to_torch_params(detgen.c3_state_dict(cfg))
    x = torch.from_numpy(detgen.images(1, H, W, seed=21))
    text = torch.from_numpy(g["text"])
    with torch.no_grad():
        out = O.zutis_forward(P, x, cfg.patch, cfg.dec_heads)
    mp, pt = out["mask_proposals"].numpy(), out["patch_tokens"].numpy()
    assert np.abs(mp[:, -1, :, ::3, ::3] - g["480x640_mask_proposals_last_sub"]).max() < 2e-5   # sharpened decoder attention (c3_state_dict): fp32 reordering noise x4
    assert np.abs(pt[:, ::3, ::3, ::4] - g["480x640_patch_tokens_sub"]).max() < 2e-6
    binary, cats, scores = O.instance_scores(out["mask_proposals"], out["patch_tokens"], text, threshold=thr)
    keep = cats[0] != 0
    assert list(cats[0][keep]) == list(g["480x640_all_cat"])
    assert np.abs(scores[0][keep] - g["480x640_all_score"]).max() < 1e-5
    up = R.bilinear_nchw(mp[:, -1], H, W) > thr
    assert np.abs(up[0][keep].reshape(keep.sum(), -1).sum(1) - g["480x640_all_area"]).max() <= 4
    for nms, key in (("hard", ""), ("linear", "linear_")):
        sel = O.mask_nms(up[0], scores[0], cats[0], nms)
        assert len(sel) == int(g[f"480x640_{key}n"]) and [c for c, _, _ in sel] == list(g[f"480x640_{key}cat"])
        # linear: every survivor's score carries products of (1 - IoU) of full-resolution masks that differ by a pixel or two
        assert np.abs(np.array([s for _, _, s in sel]) - g[f"480x640_{key}score"]).max() < (1e-5 if nms == "hard" else 2e-4)
        assert np.abs(np.array([up[0][q].sum() for _, q, _ in sel]) - g[f"480x640_{key}area"]).max() <= 4


def _e1_case(g, tag):
    B, R, width, layers, patch, grid, embed = (int(v) for v in g[f"{tag}_shape"])
    cfg = detgen.ZutisConfig(width=width, layers=layers, patch=patch, grid=grid, embed_dim=embed)
    sd = {k: v for k, v in detgen.zutis_state_dict(cfg).items() if k.startswith("encoder.")}
    return cfg, sd, torch.from_numpy(detgen.images(B, R, R, seed=5))


@pytest.mark.parametrize("tag", ["small", "l14_336"])
def test_oracle_encode_image_matches_reference(golden_dir, tag):
    """E1 pin: O.clip_encode_image against embeddings produced by the reference's own VisionTransformer submodules run in the
    order of CLIP's original forward (clip_arch.py:413-431) + the normalisation of utils/extract_image_embeddings.py:73
    (oracle/gen_golden.py::gen_encode_image).  Second case: ViT-L/14@336 geometry (24x24 grid, D = 1024), 2 layers."""
    g = np.load(f"{golden_dir}/encode_image.npz")
    cfg, sd, x = _e1_case(g, tag)
    with torch.no_grad():
        e = O.clip_encode_image(O.to_torch_params(sd), x, cfg.patch).numpy()
    ref = g[f"{tag}_embeddings"]
    assert e.shape == ref.shape
    assert np.abs(e - ref).max() < 5e-7, np.abs(e - ref).max()


def test_oracle_nms_walks_categories_in_the_references_set_order():
    """zutis.py:237-238 iterates set(category_ids_per_image): CPython's slot order for numpy int64 ids, not ascending once ids
    wrap the table ({33, 2, 40, 3} -> 40, 33, 2, 3).  The oracle and the drop-in's host NMS must emit in that order."""
    import os, sys
    rng = np.random.default_rng(3)
    Q, H, W = 24, 16, 16
    masks = np.zeros((Q, H, W), bool)
    for q in range(Q):
        y0, x0 = rng.integers(0, H - 4), rng.integers(0, W - 4)
        masks[q, y0:y0 + 4, x0:x0 + 4] = True
    cats = np.array([33, 2, 40, 3], np.int64)[np.arange(Q) % 4]
    scores = (rng.random(Q) * 0.9 + 0.05).astype(np.float32)
    want = [int(c) for c in set(cats)]
    assert want != sorted(want)
    got = O.mask_nms(masks, scores, cats, "hard")
    seen = []
    for c, _, _ in got:
        if c not in seen:
            seen.append(c)
    assert seen == want
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zutis_amd", "dropin")
    if d not in sys.path:
        sys.path.insert(0, d)
    from networks.zutis import ZUTIS
    host = ZUTIS.non_maximum_suppression_indices(masks, scores, cats, "hard")
    assert [(c, q) for c, q, _ in host] == [(c, q) for c, q, _ in got]
