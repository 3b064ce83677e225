"""Developer tool: the GEMMs of the headline step (`exact`, B = 32, 336 px) under candidate tile codes, with 1, 2 and 3 copies of the same call
meeting on the chip.  Which model of the chip the tile chooser should use for launches that arrive together — whole rounds of
`c x tiles` workgroups, or CU-time — is decided by this table.

Each measurement replays `c` recorded plans round-robin on `c` streams from the C loop the engine's replay uses (zh_plan_run_multi):
group g of a plan is the same call on the same weights in every stream (the weights rotate through NW buffers from group to group, as
the layers of the model do), each stream with its own A and its own C.  Epilogues are the model's: fp32 + bias + in-place residual
(out_proj, c_proj, the decoder's output projections and linear2), split pair out + bias (QKV, the K / V projections), + QuickGELU
(c_fc), + ReLU (linear1), split pair out + a row-periodic table of 100 rows (the decoder's query projections).  The tile is forced through
the developer override, the candidates of a shape alternate within a round, and a figure is us per group of c launches: median and
min .. max over the rounds.

    python tools/gemm_inflight_ab.py [--rounds 7] [--fast] [--only NAME,...] [--out profiles/gemm_inflight_ab.json]
    python tools/gemm_inflight_ab.py --flips          # no timing: the GEMMs of the c2 / c4 steps whose plan changes at 2 or 3 in flight
"""
import argparse, ctypes, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from zutis_amd import ops, _lib
from zutis_amd import plan as zplan
from zutis_amd.ops import Act

dev = torch.device("cuda:0")
L = _lib.load(raw=True)
NW = 12                     # weight buffers a plan rotates through (the encoder's depth)
STREAMS = 3

# (name, mode, M, N, K, epilogue, candidate tile codes (first: what one launch on an empty chip gets), groups per plan)
X3_SHAPES = [
    ("proj", "x3", 14144, 768, 3072, "res32", (448, 512), 36),
    ("out", "x3", 14144, 768, 768, "res32", (448, 512), 72),
    ("qkv", "x3", 14144, 2304, 768, "pair", (512, 448), 48),
    ("fc", "x3", 14144, 3072, 768, "pair_gelu", (512, 448), 36),
    ("dec_kv", "x3", 56448, 4608, 256, "pair", (512, 448), 12),
    ("dec o", "x3", 3200, 768, 768, "res32", (7096, 256, 1288, 192), 192),
    ("dec q", "x3", 3200, 768, 768, "pair_tab", (7096, 256, 1288, 192), 192),
    ("dec l2", "x3", 3200, 768, 2048, "res32", (7096, 256, 1288, 192), 120),
    ("dec l1", "x3", 3200, 2048, 768, "pair_relu", (256, 192, 1288), 120),
    ("dec qkv", "x3", 3200, 2304, 768, "pair_tab", (256, 192, 1288), 120),
    # config 4 (8 images of 518 px: 8200 token rows; its decoder's 800 rows stay in the few-tile regime)
    ("c4 proj", "x3", 8200, 768, 3072, "res32", (256, 448, 512), 48),
    ("c4 out", "x3", 8200, 768, 768, "res32", (256, 448, 512), 96),
    ("c4 qkv", "x3", 8200, 2304, 768, "pair", (448, 512, 256), 60),
    ("c4 fc", "x3", 8200, 3072, 768, "pair_gelu", (512, 448), 48),
    # one-plane weights (fp16-valued: the released CLIP towers) at the sites that flip with two planes
    ("proj", "x2", 14144, 768, 3072, "res32", (448, 512), 36),
    ("out", "x2", 14144, 768, 768, "res32", (448, 512), 72),
]
# --fast: the plain-fp16 dispatcher's picks for the same N = 768 sites beside the tiles that `3 x tiles` would give them
F16_SHAPES = [
    ("proj", "f16", 14144, 768, 3072, "res32", (192, 256), 48),
    ("out", "f16", 14144, 768, 768, "res32", (192, 256), 96),
    ("dec o", "f16", 3200, 768, 768, "res32", (7096, 128, 192), 192),
    ("dec q", "f16", 3200, 768, 768, "half", (7096, 128, 192), 192),
    ("dec l2", "f16", 3200, 768, 2048, "res32", (7096, 128, 192), 120),
    ("dec l1", "f16", 3200, 2048, 768, "half_relu", (128, 192, 256), 120),
    ("dec qkv", "f16", 3200, 2304, 768, "half", (128, 192, 256), 120),
    ("qkv", "f16", 14144, 2304, 768, "half", (256, 192), 48),
    ("fc", "f16", 14144, 3072, 768, "half_gelu", (256, 192), 36),
    ("c4 proj", "f16", 8200, 768, 3072, "res32", (128, 192, 256), 48),
    ("c4 out", "f16", 8200, 768, 768, "res32", (128, 192, 256), 96),
]


def operands(mode, M, N, K, epi):
    """Per stream its own A and C, the NW weights and the bias shared; call(j, g) launches group g of stream j."""
    gen = torch.Generator(device=dev).manual_seed(1000)
    x3 = mode in ("x3", "x2")
    Ws = []
    for _ in range(NW):
        w = torch.randn(N, K, device=dev, generator=gen) * 0.03
        if mode == "x2":
            w = w.half().float()                           # fp16 values: split_weight() packs one plane
        Ws.append(ops.split_weight(w) if x3 else w.half())
    assert mode != "x2" or all(W.x2 for W in Ws)
    bias = torch.randn(N, device=dev, generator=gen)
    tab = torch.randn(100, N, device=dev, generator=gen)
    As, Cs = [], []
    for _ in range(STREAMS):
        a32 = torch.randn(M, K, device=dev, generator=gen)
        if x3:
            A = Act.empty((M, K), True, dev)
            ops.cast_f16(a32, A, M, K)
        else:
            A = a32.half()
        As.append(A)
        if epi == "res32":
            Cs.append(torch.zeros(M, N, device=dev))
        elif epi.startswith("half"):
            Cs.append(torch.empty(M, N, device=dev, dtype=torch.float16))
        else:
            Cs.append(Act.empty((M, N), True, dev))
    g = ops.gemm_x3 if x3 else ops.gemm

    def call(j, i):
        W = Ws[i % NW]
        if epi == "res32":
            g(As[j], W, Cs[j], bias=bias, residual=Cs[j])
        elif epi == "pair_tab":
            g(As[j], W, Cs[j], residual=tab, res_rows=100)
        else:
            g(As[j], W, Cs[j], bias=bias, act={"gelu": ops.ACT_QUICKGELU, "relu": ops.ACT_RELU}.get(epi.partition("_")[2], ops.ACT_NONE))
    return call


def unforced(mode, M, N, K, epi, inflight):
    """The chooser's own code for the call (aligned operands), at `inflight` where the library can be asked for it."""
    kind = 0 if epi == "res32" else (1 if epi.startswith("half") else 2)
    planeC = M * N if kind == 2 else 0
    res = 0x7F2000000000 if epi in ("res32", "pair_tab") else 0
    out = (ctypes.c_int * 6)()
    args = ({"f16": 0, "x3": 2, "x2": 3}[mode], M, N, K, 1, K, K, N, 0, planeC, N if res else 0, 0, (100 if "tab" in epi else M) if res else 0, kind, 0, 0,
            0x7F0000000000, 0 if "tab" in epi else 0x7F1000000000, res, 0)
    if hasattr(L, "zh_dev_gemm_plan_inflight"):
        rc = L.zh_dev_gemm_plan_inflight(*args, inflight, out)
    elif inflight == 1:
        rc = L.zh_dev_gemm_plan(*args, out)
    else:
        return None
    return out[1] if rc == 0 else None


def measure(shape, rounds):
    name, mode, M, N, K, epi, tiles, G = shape
    call = operands(mode, M, N, K, epi)
    streams = [torch.cuda.Stream(device=dev) for _ in range(STREAMS)]
    hs = [s.cuda_stream for s in streams]
    plans = []
    for j in range(STREAMS):
        with zplan.Recorder() as rec:
            for i in range(G):
                call(j, i)
        plans.append(rec.build())
    samples = {(t, c): [] for t in tiles for c in (1, 2, 3)}
    try:
        for r in range(rounds + 1):                       # round 0 warms every (tile, c) up and is not kept
            for t in (tiles if r % 2 == 0 else tiles[::-1]):
                _lib.check(L.zh_dev_set_gemm_overrides(0, t, 0), "zh_dev_set_gemm_overrides")
                for c in (1, 2, 3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    zplan.run_many(plans[:c], hs[:c])
                    torch.cuda.synchronize()
                    if r:
                        samples[(t, c)].append((time.perf_counter() - t0) / G * 1e6)
    finally:
        L.zh_dev_set_gemm_overrides(0, 0, 0)
    row = {"site": name, "mode": mode, "M": M, "N": N, "K": K, "epilogue": epi, "groups": G, "rounds": rounds,
           "pick_inflight1": unforced(mode, M, N, K, epi, 1), "pick_inflight3": unforced(mode, M, N, K, epi, 3), "tiles": {}}
    for t in tiles:
        row["tiles"][str(t)] = {f"c{c}": {"median_us": round(statistics.median(samples[(t, c)]), 2), "min_us": round(min(samples[(t, c)]), 2),
                                          "max_us": round(max(samples[(t, c)]), 2)} for c in (1, 2, 3)}
    line = f"{mode} {name:8s} {M} x {N} x {K} {epi:9s} picks {row['pick_inflight1']} / {row['pick_inflight3']}"
    for t in tiles:
        line += f" | t{t}:" + " ".join(" c%d %.1f (%.1f .. %.1f)" % (c, *[row["tiles"][str(t)][f"c{c}"][k] for k in ("median_us", "min_us", "max_us")])
                                       for c in (1, 2, 3))
    print(line, flush=True)
    return row


def step_flips():
    """The recorded steps of the headline (c2) and of config 4, both precisions: every GEMM shape whose plan at 2 or 3 launches in
    flight is not the plan of one launch, with its number of calls per step."""
    from tests import _gemm_inflight as GI
    from zutis_amd import detgen
    from zutis_amd.engine import ZutisEngine
    cfg = detgen.VIT_B16
    P = {k: torch.from_numpy(v).to(dev) for k, v in detgen.zutis_state_dict(cfg).items()}
    for wl, B, S, n in (("c2", 32, 336, 81), ("c4", 8, 518, 920)):
        text = torch.from_numpy(detgen.text_embeddings(n, cfg.embed_dim)).to(dev)
        x = torch.randn((B, 3, S, S), generator=torch.Generator().manual_seed(1000)).to(dev)
        for precision in ("exact", "fast"):
            eng = ZutisEngine(P, cfg.patch, cfg.dec_heads, precision=precision)
            eng.forward(x)
            with zplan.Recorder() as rec:
                out = eng.forward(x)
                lo = eng.semantic_logits_lowres(out["patch_tokens"], text)
                labels = torch.empty((B, S, S), dtype=torch.int64, device=dev)
                ops.upsample_argmax(lo, labels, B, n, lo.shape[2], lo.shape[3], S, S)
            seen = {}
            for name, args in rec.calls:
                c = GI.case_of(name, args)
                if c is None:
                    continue
                key = (c.mode, c.M, c.N, c.K, c.batch, c.out_kind, bool(c.has_pos), c.res_rows if c.residual else 0)
                plans = tuple(GI.plan_at(L, c, i) for i in (1, 2, 3))
                e = seen.setdefault(key, [0, plans])
                e[0] += 1
                assert e[1] == plans, (key, e[1], plans)
            print(f"{wl} {precision}: {sum(e[0] for e in seen.values())} GEMM calls, {len(seen)} shapes")
            for key, (cnt, plans) in sorted(seen.items(), key=lambda kv: -kv[1][0]):
                mark = "FLIPS" if len(set(plans)) > 1 else "     "
                print(f"  {mark} x{cnt:3d} mode {key[0]} {key[1]} x {key[2]} x {key[3]} batch {key[4]} out {key[5]} pos {int(key[6])} res {key[7]}: " +
                      " | ".join(f"{i + 1}: {p.code} {p.tile_m}x{p.tile_n}" + (f" peel {p.peel}" if p.peel else "") for i, p in enumerate(plans)), flush=True)
            del eng
            torch.cuda.empty_cache()


if __name__ == "__main__":
    if "--flips" in sys.argv:
        step_flips()
        sys.exit(0)
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--fast", action="store_true", help="also the plain-fp16 (`fast`) forms of the N = 768 sites")
    ap.add_argument("--only", default="", help="comma-separated site names")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gemm_inflight_ab.json"))
    a = ap.parse_args()
    only = {s for s in a.only.split(",") if s}
    rows = []
    for shape in X3_SHAPES + (F16_SHAPES if a.fast else []):
        if only and shape[0] not in only:
            continue
        rows.append(measure(shape, a.rounds))
        torch.cuda.empty_cache()
    doc = {"tool": "tools/gemm_inflight_ab.py", "device": torch.cuda.get_device_name(0),
           "unit": "us per group of c launches (one per stream, the same call on the same weights), replayed by zh_plan_run_multi; median, min, max over alternated rounds",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
