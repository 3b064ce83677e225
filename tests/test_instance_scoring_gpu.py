"""-m gpu: the instance-scoring kernels (zh_instance_mask_stats, zh_masked_mean_tokens, zh_instance_classify), the NMS's pairwise
mask counts (zh_mask_iou_counts) and the text-tower glue (zh_embed_tokens_f32, zh_eot_rows_f32, zh_group_mean_l2norm) on identical
inputs against float64 references, at the evaluation's shapes and at the edges of each kernel's tiling.

Tiling the cases reach (zutis_amd/csrc/instance.hip): the masked mean runs QT = 10 queries x MCH = 64 pixels per workgroup with
CPT = 1 / 2 / 4 channels per thread (E <= 256 / 512 / 1024); the classifier walks classes wave, wave + 4, ... in passes of
4 x CPP = 24; the statistics take a 4-wide path only when M % 4 == 0 and the proposal row is 16-byte aligned; the mask packer reads
16-byte pieces only for a full, aligned 64-pixel word."""
import numpy as np
import pytest
import torch

from oracle import zutis_ref as O
from zutis_amd import detgen

pytestmark = pytest.mark.gpu

f32 = torch.float32
MARGIN = 1e-6          # float64 top-two probabilities closer than this may resolve either way in fp32


def _inputs(B, Q, h, w, E, thr, seed, L=None):
    """Proposals that threshold into region-shaped masks over tokens with a per-region direction (unit-norm rows, as the
    text-space patch tokens are), plus proposals at fp32(thr) and its two neighbours.  When Q >= 3, query Q-1 is empty and
    query Q-2 is full.  L: also return the [B, L, Q, h, w] tensor whose last layer is the proposals."""
    g = torch.Generator().manual_seed(seed)
    seg = ((torch.arange(h) * 4) // h)[:, None] * 2 + ((torch.arange(w) * 2) // w)[None, :]          # 8 regions
    mu = torch.randn((B, 8, E), generator=g)
    pt = mu[:, seg] + 0.5 * torch.randn((B, h, w, E), generator=g)
    pt = pt / pt.norm(dim=-1, keepdim=True)
    wq = torch.rand((B, Q, 8), generator=g)
    mp = (wq[:, :, seg] + 0.3 * (torch.rand((B, Q, h, w), generator=g) - 0.5)).clamp(0, 1)
    t = np.float32(thr)
    edge = torch.tensor([t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))], dtype=f32)
    pick = torch.rand((B, Q, h, w), generator=g)
    mp = torch.where(pick < 0.06, edge[(pick * 50).long() % 3], mp)
    if Q >= 3:
        mp[:, Q - 1] = 0.0
        mp[:, Q - 2] = 1.0
    if L is None:
        return mp.contiguous(), pt.contiguous()
    mp5 = torch.rand((B, L, Q, h, w), generator=g)
    mp5[:, -1] = mp
    return mp5, pt.contiguous()


def _f64(mp, pt, text, thr, T):
    """float64 statistics of the fp32 inputs.  The binary masks are torch's fp32 compare `mp > thr` (what the reference computes);
    everything after them is float64.  Category and score are the oracle's own instance_scores on .double() inputs."""
    mpl = mp[:, -1] if mp.dim() == 5 else mp
    binary = mpl > thr
    b64 = binary.flatten(2).double()
    sizes = b64.sum(-1)
    tk = pt.double().flatten(1, 2)
    avg = b64 @ tk / (sizes[..., None] + 1e-7)
    v = avg / (avg.norm(dim=-1, keepdim=True) + 1e-7)
    bin2, cat, score = O.instance_scores(mp.double(), pt.double(), text.double(), threshold=float(np.float32(thr)), temperature=T)
    assert torch.equal(bin2, binary)
    return dict(binary=binary, sizes=sizes, conf=(mpl.double().flatten(2) * b64).sum(-1) / (sizes + 1e-7), avg=avg,
                absmean=b64 @ tk.abs() / (sizes[..., None] + 1e-7), prob=torch.sigmoid((v @ text.double().t()) * T),
                cat=torch.from_numpy(cat), score=torch.from_numpy(score))


def _run(dev, mp, pt, text, thr, T):
    """The three scoring kernels as ZutisEngine.instance_candidates chains them; a 5-D mp goes in as its [:, -1] view with
    stride_image = L*Q*M (the drop-in's layout)."""
    from zutis_amd import ops
    mpd = mp.to(dev)
    if mp.dim() == 5:
        B, L, Q, h, w = mp.shape
        mpl, stride = mpd[:, -1], L * Q * h * w
    else:
        B, Q, h, w = mp.shape
        mpl, stride = mpd, Q * h * w
    M, E, n = h * w, pt.shape[-1], text.shape[0]
    sizes, conf = torch.empty((B * Q,), device=dev), torch.empty((B * Q,), device=dev)
    binary = torch.empty((B, Q, h, w), dtype=torch.uint8, device=dev)
    flag = torch.zeros((1,), dtype=torch.int32, device=dev)
    ops.instance_mask_stats(mpl, stride, thr, B, Q, M, sizes, conf, binary, flag)
    avg = torch.empty((B * Q, E), device=dev)
    ops.masked_mean_tokens(pt.to(dev), binary, sizes, avg, B, Q, M, E)
    cat = torch.empty((B, Q), dtype=torch.int64, device=dev)
    score = torch.empty((B, Q), device=dev)
    ops.instance_classify(avg, text.to(dev), conf, T, B * Q, n, E, cat, score)
    return dict(binary=binary.cpu(), sizes=sizes.cpu().view(B, Q), conf=conf.cpu().view(B, Q), avg=avg.cpu().view(B, Q, E),
                cat=cat.cpu(), score=score.cpu(), flag=int(flag.item()))


def _direction(ref, b, q):
    """fp32 unit vector along the float64 masked mean of (b, q): a text row equal to it is that query's clear best class."""
    a = ref["avg"][b, q]
    return (a / a.norm()).float()


def _check(got, ref, what=""):
    assert got["flag"] == 0
    assert torch.equal(got["binary"], ref["binary"].to(torch.uint8)), what
    assert torch.equal(got["sizes"].double(), ref["sizes"]), what
    e_conf = float((got["conf"].double() - ref["conf"]).abs().max())
    assert e_conf <= 2e-6, (what, e_conf)
    # one 64-term chunk sum plus at most 75 chunk sums, each rounding at 6e-8 of the masked sum of |tokens|
    e_avg = (got["avg"].double() - ref["avg"]).abs() - 1e-5 * ref["absmean"]
    assert float(e_avg.max()) <= 0.0, (what, float(e_avg.max()))
    e_score = (got["score"].double() - ref["score"]).abs() - 4e-6 * ref["score"].abs()
    assert float(e_score.max()) <= 0.0, (what, float(e_score.max()))
    prob = ref["prob"]
    top = prob.max(dim=-1).values
    second = prob.topk(2, dim=-1).values[..., 1] if prob.shape[-1] > 1 else torch.full_like(top, -1.0)
    picked = prob.gather(-1, got["cat"][..., None])[..., 0]
    ok = (got["cat"] == ref["cat"]) | ((top - second <= MARGIN) & (picked >= top - MARGIN))
    assert bool(ok.all()), (what, torch.nonzero(~ok)[:8].tolist())
    empty = ref["sizes"] == 0
    assert bool((got["conf"][empty] == 0).all() and (got["avg"][empty] == 0).all())
    assert bool((got["cat"][empty] == 0).all() and (got["score"][empty] == 0).all())
    return e_conf, float(((got["score"].double() - ref["score"]).abs() / ref["score"].abs().clamp_min(1e-30)).max())


# (B, Q, h, w, E, n, thr, T, L): L = layers of a 5-D proposal tensor passed as its [:, -1] view (None: a contiguous [B, Q, h, w])
CASES = {
    "eval_60x80_n81_thr07": (1, 100, 60, 80, 512, 81, 0.7, 5.0, None),       # the COCO-20K evaluation: 75 pixel chunks, 4 passes
    "eval_54x80_n80_thr05": (1, 100, 54, 80, 512, 80, 0.5, 5.0, None),
    "batch8": (8, 100, 60, 80, 512, 81, 0.7, 5.0, None),                      # blockIdx.y, partial rows b*Q + q
    "q1": (1, 1, 60, 80, 512, 81, 0.7, 5.0, None),                            # one query: a tile of 1
    "q13": (2, 13, 60, 80, 512, 81, 0.5, 5.0, None),                          # tile remainder of 3
    "m35": (2, 13, 5, 7, 512, 81, 0.5, 5.0, None),                            # one partial chunk; scalar stats path
    "m91": (2, 13, 7, 13, 512, 81, 0.3, 5.0, None),                           # partial second chunk; scalar path; fp32(0.3) > 0.3
    "strided_5d": (2, 13, 7, 13, 512, 81, 0.5, 5.0, 3),                       # offset base, stride L*Q*M, Q*M = 1183
    "e64": (2, 13, 12, 20, 64, 81, 0.5, 5.0, None),                           # CPT 1, three quarters of the threads idle
    "e300": (2, 13, 12, 20, 300, 81, 0.5, 5.0, None),                         # CPT 2 with a 44-channel tail
    "e768": (2, 13, 12, 20, 768, 81, 0.5, 5.0, None),                         # CPT 4, last quarter idle
    "e1024": (2, 13, 12, 20, 1024, 81, 0.5, 5.0, None),                       # CPT 4, full
    "n1": (2, 13, 12, 20, 512, 1, 0.5, 5.0, None),                            # three waves with no class
    "n3": (2, 13, 12, 20, 512, 3, 0.5, 5.0, None),
    "n24": (2, 13, 12, 20, 512, 24, 0.5, 5.0, None),                          # exactly one pass
    "n25": (2, 13, 12, 20, 512, 25, 0.5, 5.0, None),                          # a second pass with one class (wave 0, j = 0)
    "n920": (2, 13, 12, 20, 512, 920, 0.5, 5.0, None),                        # 39 passes, the last one partial
}


@pytest.mark.parametrize("case", list(CASES))
def test_instance_scoring_kernels_vs_float64(dev, case):
    B, Q, h, w, E, n, thr, T, L = CASES[case]
    mp, pt = _inputs(B, Q, h, w, E, thr, seed=len(case) * 131 + E + n, L=L)
    text = torch.from_numpy(detgen.text_embeddings(n, E))
    ref = _f64(mp, pt, text, thr, T)
    q0 = int(torch.nonzero(ref["sizes"][0] > 0)[0])
    text[n - 1] = _direction(ref, 0, q0)               # the last class (in the last, clamped pass) wins for query q0
    ref = _f64(mp, pt, text, thr, T)
    assert int(ref["cat"][0, q0]) == n - 1
    got = _run(dev, mp, pt, text, thr, T)
    e_conf, e_score = _check(got, ref, case)
    print(f"{case}: conf {e_conf:.2e} abs, score {e_score:.2e} rel")
    if Q >= 3:
        full = got["sizes"][:, Q - 2]
        assert bool((full == h * w).all() and (got["conf"][:, Q - 2] == 1.0).all())


def test_instance_scoring_unaligned_4_wide_rows(dev):
    """M % 4 == 0 but the proposals start one float past a 16-byte boundary: the statistics must take the scalar path."""
    B, Q, h, w, E, n, thr, T = 2, 13, 60, 80, 512, 81, 0.5, 5.0
    mp, pt = _inputs(B, Q, h, w, E, thr, seed=5)
    text = torch.from_numpy(detgen.text_embeddings(n, E))
    ref = _f64(mp, pt, text, thr, T)
    from zutis_amd import ops
    buf = torch.empty((mp.numel() + 1,), device=dev)
    buf[1:] = mp.flatten().to(dev)
    M = h * w
    sizes, conf = torch.empty((B * Q,), device=dev), torch.empty((B * Q,), device=dev)
    binary = torch.empty((B, Q, h, w), dtype=torch.uint8, device=dev)
    ops.instance_mask_stats(buf[1:], Q * M, thr, B, Q, M, sizes, conf, binary)
    assert torch.equal(binary.cpu(), ref["binary"].to(torch.uint8))
    assert torch.equal(sizes.cpu().double().view(B, Q), ref["sizes"])
    assert float((conf.cpu().double().view(B, Q) - ref["conf"]).abs().max()) <= 2e-6


def _scoring_case(seed=21, B=2, Q=13, h=12, w=20, E=512, n=81, thr=0.5):
    mp, pt = _inputs(B, Q, h, w, E, thr, seed=seed)
    text = torch.from_numpy(detgen.text_embeddings(n, E))
    return mp, pt, text, thr


def test_instance_classify_exact_ties_resolve_to_the_lowest_index(dev):
    """Duplicate text rows give bit-equal probabilities; torch.argmax keeps the first.  Pairs: same wave and pass (2, 6), same
    wave in different passes (5, 29), different waves (3 in wave 3, 77 in wave 1: the cross-wave merge meets 77 first)."""
    mp, pt, text, thr = _scoring_case()
    ref = _f64(mp, pt, text, thr, 5.0)
    for q, (lo, hi) in enumerate(((2, 6), (5, 29), (3, 77))):
        text[lo] = text[hi] = _direction(ref, 0, q)
    ref = _f64(mp, pt, text, thr, 5.0)
    got = _run(dev, mp, pt, text, thr, 5.0)
    assert [int(c) for c in got["cat"][0, :3]] == [2, 5, 3]
    assert [int(c) for c in ref["cat"][0, :3]] == [2, 5, 3]
    _check(got, ref)


def test_instance_classify_saturated_sigmoid_keeps_the_first_class(dev):
    """T = 100 and three classes at d = 0.30 / 0.34 / 0.32: their fp32 probabilities are all exactly 1.0 (1 - e^-30 rounds up), so the
    reference's fp32 argmax is the first of them (7, wave 3), ahead of 30 (wave 2, pass 1) and 56 (wave 0, pass 2).  In float64
    they still differ, and the argmax is the largest d (30)."""
    mp, pt, text, thr = _scoring_case(seed=22)
    T, q = 100.0, 4
    ref = _f64(mp, pt, text, thr, 5.0)
    u = _direction(ref, 0, q)
    g = torch.Generator().manual_seed(9)
    for k, d in ((7, 0.30), (30, 0.34), (56, 0.32)):
        r = torch.randn(u.shape, generator=g)
        r = r - (r @ u) * u
        text[k] = d * u + (1 - d * d) ** 0.5 * r / r.norm()
    ref64 = _f64(mp, pt, text, thr, T)
    _, cat32, score32 = O.instance_scores(mp, pt, text, threshold=thr, temperature=T)
    assert cat32[0, q] == 7 and int(ref64["cat"][0, q]) == 30
    got = _run(dev, mp, pt, text, thr, T)
    assert int(got["cat"][0, q]) == 7
    assert abs(float(got["score"][0, q]) - float(score32[0, q])) <= 4e-6 * abs(float(score32[0, q]))


@pytest.mark.parametrize("nan_rows,first", [((13, 29, 50), 13), ((50, 77), 50)])
def test_instance_classify_nan_text_rows_pick_the_first_nan(dev, nan_rows, first):
    """A NaN probability is the maximum for torch.argmax / torch.max and the first NaN wins: 13 beats a finite best class, 29 (the
    same wave, a later pass) and 50 (another wave); 50 (wave 2) beats 77 (wave 1, merged first).  The score is NaN."""
    mp, pt, text, thr = _scoring_case(seed=23)
    for k in nan_rows:
        text[k, 17] = float("nan")
    _, cat32, score32 = O.instance_scores(mp, pt, text, threshold=thr)
    assert (cat32 == first).all() and np.isnan(score32).all()
    got = _run(dev, mp, pt, text, thr, 5.0)
    assert bool((got["cat"] == first).all()), got["cat"].tolist()
    assert bool(torch.isnan(got["score"]).all())


def test_instance_scoring_nan_token_gives_the_references_first_nan(dev):
    """A NaN patch token makes every masked mean of its image NaN (0 * NaN in the reference's masked sum and here): category 0 (the
    first NaN) and a NaN score, as torch.argmax / torch.max on the fp32 oracle.  The other image is untouched."""
    mp, pt, text, thr = _scoring_case(seed=24)
    pt[1, 3, 5, 100] = float("nan")
    _, cat32, score32 = O.instance_scores(mp, pt, text, threshold=thr)
    got = _run(dev, mp, pt, text, thr, 5.0)
    assert (cat32[1] == 0).all() and np.isnan(score32[1]).all()
    assert torch.equal(got["cat"][1], torch.from_numpy(cat32[1])) and bool(torch.isnan(got["score"][1]).all())
    ref = _f64(mp[:1], pt[:1], text, thr, 5.0)
    _check({k: (v[:1] if torch.is_tensor(v) else v) for k, v in got.items()}, ref)


# ---- zh_mask_iou_counts: exact intersection / union counts at arbitrary pixel counts

def _masks(n, P, seed):
    """u8 masks of varied density: 0 empty, 1 full, 3 a copy of 2, 4 set with 255, 5 with arbitrary non-zero bytes."""
    g = torch.Generator().manual_seed(seed)
    dens = torch.rand((n, 1), generator=g)
    m = (torch.rand((n, P), generator=g) < dens).to(torch.uint8)
    if n >= 6:
        m[0] = 0
        m[1] = 1
        m[3] = m[2]
        m[4] *= 255
        m[5] *= torch.randint(1, 256, (P,), generator=g, dtype=torch.int32).to(torch.uint8)
    elif n == 1:
        m[0] = 255
    return m


@pytest.mark.parametrize("n,H,W", [(100, 480, 640), (100, 375, 500), (7, 61, 83), (150, 33, 47), (1, 1, 1)])
def test_mask_iou_counts_exact(dev, n, H, W):
    """Integer counts against a float32 matmul of the {0,1} matrices (exact below 2^24).  375 x 500 leaves a 44-pixel last word;
    the odd byte offset (instance_nms passes m[b]) sends every word down the byte-wise packer."""
    from zutis_amd import ops
    P = H * W
    m = _masks(n, P, seed=n + P)
    A = (m != 0).float()
    inter = A @ A.t()
    area = A.sum(1)
    uni = area[:, None] + area[None, :] - inter
    for off in (0, 1):
        buf = torch.zeros((n * P + 16,), dtype=torch.uint8, device=dev)
        buf[off:off + n * P] = m.flatten().to(dev)
        gi, gu = torch.empty((n, n), dtype=torch.int32, device=dev), torch.empty((n, n), dtype=torch.int32, device=dev)
        ops.mask_iou_counts(buf[off:off + n * P], n, P, gi, gu)
        gi, gu = gi.cpu(), gu.cpu()
        assert torch.equal(gi, inter.to(torch.int32)), off
        assert torch.equal(gu, uni.to(torch.int32)), off
        assert torch.equal(torch.diagonal(gi), area.to(torch.int32))


def test_mask_iou_counts_rejects_a_short_workspace(dev):
    """375 x 500 needs 2930 words per mask: a workspace one byte short is an error before anything is launched."""
    from zutis_amd import ops, _lib
    n, P = 3, 375 * 500
    m = torch.zeros((n, P), dtype=torch.uint8, device=dev)
    gi, gu = torch.empty((n, n), dtype=torch.int32, device=dev), torch.empty((n, n), dtype=torch.int32, device=dev)
    with pytest.raises(_lib.ZutisHipError):
        ops.mask_iou_counts(m, n, P, gi, gu, workspace=torch.empty((n * 2930 * 8 - 1,), dtype=torch.uint8, device=dev))


def test_engine_mask_iou_matrix_equals_compute_iou_pairwise(dev):
    from zutis_amd.engine import ZutisEngine
    cfg = detgen.TINY
    eng = ZutisEngine({k: torch.from_numpy(v).to(dev) for k, v in detgen.zutis_state_dict(cfg).items()}, cfg.patch, cfg.dec_heads)
    n, H, W = 7, 61, 83
    m = _masks(n, H * W, seed=3).view(n, H, W)
    iou, areas = eng.mask_iou_matrix(m.to(dev), return_areas=True)
    mb = (m != 0).numpy()
    assert np.array_equal(areas, mb.reshape(n, -1).sum(1))
    for i in range(n):
        for j in range(n):
            assert iou[i, j] == O.compute_iou(mb[i], mb[j]), (i, j)


# ---- text-tower glue

def test_embed_tokens_bit_exact(dev):
    from zutis_amd import ops
    n, ctx, D, vocab = 3, 77, 512, 49408
    g = torch.Generator().manual_seed(31)
    tokens = torch.randint(0, vocab, (n, ctx), generator=g)
    tokens[0, 0], tokens[0, 76], tokens[1, 5], tokens[2, 64] = 0, vocab - 1, vocab - 1, 0
    table, pos = torch.randn((vocab, D), generator=g), torch.randn((ctx, D), generator=g)
    out = torch.empty((n * ctx, D), device=dev)
    ops.embed_tokens(tokens.to(dev), table.to(dev), pos.to(dev), out)
    assert torch.equal(out.cpu(), (table[tokens] + pos).reshape(n * ctx, D))


def test_eot_rows_take_the_first_maximum(dev):
    """One wave per row, lane t % 64 scans t, t + 64: the first maximum must win within a lane and across lanes."""
    from zutis_amd import ops
    ctx, D = 77, 512
    rows = [({70: 49407}, 70),                        # EOT past the first 64 positions
            ({5: 9, 69: 9}, 5),                       # equal maxima in one lane (5 and 5 + 64)
            ({3: 9, 10: 9}, 3),                       # equal maxima in two lanes
            ({10: 9, 66: 9}, 10),                     # the later one in another lane's second step
            ({64: 9, 76: 9}, 64),                     # both past 64
            ({}, 0)]                                  # all zero: index 0
    g = torch.Generator().manual_seed(32)
    tokens = torch.zeros((len(rows), ctx), dtype=torch.int64)
    for i, (vals, _) in enumerate(rows):
        if vals:
            tokens[i] = torch.randint(0, 8, (ctx,), generator=g)
        for t, v in vals.items():
            tokens[i, t] = v
    want = [e for _, e in rows]
    assert torch.argmax(tokens, dim=-1).tolist() == want
    x = torch.randn((len(rows) * ctx, D), generator=g)
    out = torch.empty((len(rows), D), device=dev)
    ops.eot_rows(tokens.to(dev), x.to(dev), out)
    assert torch.equal(out.cpu(), x.view(len(rows), ctx, D)[torch.arange(len(rows)), torch.tensor(want)])


@pytest.mark.parametrize("T", [2, 85])
@pytest.mark.parametrize("E", [64, 512, 1000])
def test_group_mean_l2norm_vs_float64(dev, T, E):
    from zutis_amd import ops
    G = 5
    x = torch.randn((G, T, E), generator=torch.Generator().manual_seed(T * E))
    x = x / x.norm(dim=-1, keepdim=True)
    m = x.double().mean(1)
    ref = m / m.norm(dim=-1, keepdim=True)
    out = torch.empty((G, E), device=dev)
    ops.group_mean_l2norm(x.to(dev), out, G, T, E)
    assert float((out.cpu().double() - ref).abs().max()) <= 1e-6
