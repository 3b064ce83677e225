"""Which kernel form a shape gets: every rule of the engines' determinism contract, as pure functions.

A rule reads shapes and engine settings only — never data — so a result is bitwise reproducible for a given (shape, setting).
Some rules read the BATCH: across the batch sizes they tell apart, sums are re-associated (fp32-class differences, ~1e-7 on
tokens); each function says whether it does.  Nothing here imports torch or the library: tests/test_shape_rules_cpu.py pins the
decisions on a CPU and tests/test_launch_trace_gpu.py pins what the engines launch with them."""
import os

CUS = 256               # compute units of the MI355X
QUERY_BLOCK = 128       # queries per attention workgroup (ZH_ATTN_QUERY_BLOCK of include/zutis_hip.h)
FEW_ITEMS = 128         # (image, head, query block) workgroups up to which a self-attention splits its keys
# Head dims zh_attention_f16 has kernels for (csrc/attention_dispatch.h ATTN_HEAD_DIMS): 64 the encoders, 96 / 128 the ZUTIS decoder's 8
# heads over the ViT-B / ViT-L towers' width.  The engines' checks and error texts read this tuple; tests/test_attention_dh128_cpu.py
# holds it to what the library's plan accepts.
HEAD_DIMS = (64, 96, 128)
PIPELINED_HEAD_DIMS = (64, 96)     # ... of which these have the software-pipelined split-pair loop (ATTN_PIPE_HEAD_DIMS)


def key_tile(x3: bool) -> int:
    """Keys per tile of the attention kernels: 32 for split pairs, 64 for fp16 (ZH_ATTN_KEY_TILE_X3 / _F16)."""
    return 32 if x3 else 64


def key_tiles(Tk: int, x3: bool) -> int:
    return -(-Tk // key_tile(x3))


def fit_key_split(S: int, ktiles: int) -> int:
    """The largest split s <= S that leaves no workgroup without keys: (s - 1) * ceil(ktiles / s) < ktiles.  Never below 1: a
    setting of 0 or less, which the engines used to hand to the attention launcher (where anything <= 1 is the unsplit kernel), reads as 1."""
    while S > 1 and (S - 1) * -(-ktiles // S) >= ktiles:
        S -= 1
    return max(1, S)


def pipelined_loop(n: int, head_dim: int, x3: bool) -> bool:
    """Whether `n` attention workgroups (items x key split) run the software-pipelined split-pair loop: the launcher's rule
    (csrc/attention_dispatch.h attn_pipelined; tests/test_attention_plan_cpu.py holds this copy to it).  dh = 96 always, dh = 64 when
    the grid needs no more rounds of the chip at two workgroups per CU than at three, dh = 128 never (it has no pipelined kernel).  The launcher asks it of n rounded up to 8,
    which gives the same rounds: 2 * CUS and 3 * CUS are multiples of 8.  It reads the grid, and so the BATCH; the results are
    bit-identical either way."""
    return x3 and head_dim in PIPELINED_HEAD_DIMS and (head_dim == 96 or -(-n // (2 * CUS)) <= -(-n // (3 * CUS)))


def long_sequence_key_split(items: int, ktiles: int, head_dim: int, x3: bool, out_elems: int) -> int:
    """Key split (1 .. 8) of a LONG self-attention (SelfMask's DINO ViT-S/8 at 512x683: T = 5505, networks/selfmask/vision_transformer.py:110-133)
    from a round-quantisation model of zh_attention_f16's grid: `items` = (image, head, 128-query block) workgroups, each walking `ktiles`
    key tiles.  A CU holds 3 such workgroups (2 for the pipelined split-pair loop and at dh = 96 / 128), so 4 images x 6 heads x 44 blocks = 1056
    workgroups are 1.375 rounds of the chip's 768 slots — two rounds, the second a third full — and ONE image (264 workgroups) leaves
    every SIMD a single wave with nothing to overlap its softmax with.  Splitting the keys over S workgroups per item (partials merged by
    attn_combine_kernel) buys finer rounds for one pass over the fp32 partials.  Cost in key-tile times of a full CU:
    rounds x (chunk + fixed) + a last partial round at the (faster) per-tile time of its occupancy + the merge traffic.
    `items` counts every image, so the split DEPENDS ON THE BATCH: 5 / 4 / 2 / 1 for 1 / 2 / 4 / 8 images at T = 5505 (split pairs)."""
    def wpc_of(n):
        return 2 if pipelined_loop(n, head_dim, x3) or head_dim in (96, 128) else 3
    tile_time = {1: 0.78, 2: 0.89, 3: 1.0}                 # per-tile time of a workgroup with 1 / 2 / 3 resident per CU (stamps, profiles/NOTES.md)
    tile_us = 1.85 if x3 else 0.95                         # one key tile of a workgroup at full occupancy
    best, best_cost = 1, None
    for S in range(1, 9):
        chunk = -(-ktiles // S)
        if S > 1 and (S - 1) * chunk >= ktiles:
            continue
        n = items * S
        wpc = wpc_of(n)
        full, rem = divmod(n, CUS * wpc)
        cost = full * (chunk + 2) * tile_time[wpc]
        if rem:
            cost += (chunk + 2) * tile_time[min(wpc, -(-rem // CUS))]
        if S > 1:
            cost += S * out_elems * 4 * 2 / 3.0e12 * 1e6 / tile_us      # partials written and read once, ~3 TB/s
        if best_cost is None or cost < best_cost * 0.97:               # a larger split must win by 3 %
            best, best_cost = S, cost
    return best


def self_attention_key_split(B: int, T: int, heads: int, head_dim: int, x3: bool, causal: bool = False) -> int:
    """Key split of the encoders' self-attention (zh_attention_f16_splitk + merge, as the decoder's cross-attention).  Few
    (image, head, 128-query block) items — one image at 480x640: 12 heads x 10 blocks on 256 CUs — split the keys so that about every CU
    gets a workgroup.  The gate reads the batch (B * per_image <= FEW_ITEMS) and the long-sequence model reads it throughout; inside the gate
    the split is a function of heads and T alone.  The causal kernel has no split form."""
    if causal:
        return 1
    per_image = heads * -(-T // QUERY_BLOCK)
    S = max(1, min(8, CUS // per_image)) if B * per_image <= FEW_ITEMS else 1
    ktiles = key_tiles(T, x3)
    if S == 1 and T >= 2048:
        S = long_sequence_key_split(B * per_image, ktiles, head_dim, x3, out_elems=B * T * heads * head_dim)
    return fit_key_split(S, ktiles)


# The engines' default cross-attention setting (ZH_CROSS_KSPLIT = developer override).  Throughput: 1, what bench.py's batch-32 runs
# use; the drop-in modules, which serve batch-1 evaluation loops, set their own: 12 for ZUTIS, 8 for SelfMask (SelfMaskEngine's default too).
CROSS_KSPLIT_DEFAULT = int(os.environ.get("ZH_CROSS_KSPLIT", "1"))


def cross_attention_key_split(setting, B: int, heads: int, Q: int, M: int, x3: bool) -> int:
    """Key split of the decoder's cross-attention.  Q <= 128 queries against M keys is ONE workgroup per (image, head): 8 workgroups at
    batch 1 (the COCO-20K evaluation's regime), 256 at batch 32 (one per CU, each streaming its K / V with a single tile of prefetch).
    The keys can be split over `setting` workgroups + a merge launch.  Measured (round 3): batch-1 forward + predict 2.99 / 2.73 / 2.60 /
    2.54 ms for splits 1 / 2 / 4 / 8 (at the COCO-20K shape, 480x640 = 4800 keys, the forward is 4.25 / 3.56 / 3.04 ms for splits
    1 / 2 / 8); the batch-32 step with three batches in flight loses 0.3 - 1 % with a split of 2 (2825 / 2842 against 2852 / 2851
    images/s, same box: the partials' round trip costs more than the extra occupancy gives there).
    An integer `setting` is a property of the ENGINE INSTANCE and never of the batch: the result is then a function of Q and M only.
    "auto" (opt-in, round 6; bench.py's config-4 runs: 8 images x 8 heads = 64 workgroups of 171 key tiles on 256 CUs) is the split
    that puts about one workgroup on every CU.  It DEPENDS ON THE BATCH, so results are re-associated between batch sizes (~1e-7) —
    which is why it is not the default: equal rank shards must reproduce the single-GPU batch bit for bit."""
    if setting == "auto":
        setting = max(1, min(8, CUS // max(1, B * heads)))
    if not (Q <= QUERY_BLOCK and M >= 1024):
        return 1
    return fit_key_split(setting, key_tiles(M, x3))


# Few-row regime (batch-1 evaluation: configs/*.yaml val batch_size 1, trainer.py:328-345): the two N = D GEMMs of a transformer block
# (out_proj, c_proj) are 60 tiles of 128 x 128 for 256 CUs, so their K is split over S workgroups per tile — a batched GEMM over K
# slabs writing fp32 partial planes — and the planes are summed by the LayerNorm that follows (zh_sum_layernorm_f32).
SPLITK_MAX_ROWS = int(os.environ.get("ZH_SPLITK_MAX_ROWS", "2048"))     # rows (B * T) up to which those GEMMs run split-K
SPLITK_MAX = int(os.environ.get("ZH_SPLITK_MAX", "4"))
# shortest K slab: c_proj (K = 3072) splits four ways (38.4 -> 25.0 us for the GEMM, + 5 us in the LayerNorm that adds the planes);
# out_proj (K = 768) does not — its 228 tiles of 64 x 64 already fill the chip (11.8 us; planes + a longer LayerNorm cost more)
SPLITK_MIN_K = int(os.environ.get("ZH_SPLITK_MIN_K", "512"))


def gemm_k_split(rows: int, K: int) -> int:
    """K split of a [rows, N] = [rows, K] x [N, K]^T GEMM whose partial planes a zh_sum_layernorm_f32 launch adds up.  The row gate
    reads the batch (rows = B * T); inside the few-row regime the split is a function of K alone, so image i's result does not
    depend on how many images share its batch there."""
    if rows > SPLITK_MAX_ROWS or K % 64:
        return 1
    s = 1
    while 2 * s <= SPLITK_MAX and (K // (2 * s)) % 64 == 0 and K // (2 * s) >= SPLITK_MIN_K:
        s *= 2
    return s
