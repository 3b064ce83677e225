// Flash attention forward, fp16 operands / fp32 softmax+accumulate, head_dim 64, 96 or 128 (gfx950).
//
// Replaces nn.MultiheadAttention's softmax(QK^T/sqrt(dh))V at networks/clip_arch.py:314-316 (12 heads,
// dh=64, T=1+hw), networks/transformer.py:272-286 (decoder self/cross attention, 8 heads: dh=96 over the ViT-B towers' width 768,
// dh=128 over the ViT-L towers' 1024) and
// networks/selfmask/vision_transformer.py:110-133 (dh=64, T up to ~6k; the reference materialises
// [B,6,T,T]).  Nothing T x T ever reaches HBM here.
//
// Design: one workgroup = 4 waves = 128 queries of one (image, head); each wave owns 32 queries.
// K/V tiles of 64 keys are register-staged HBM -> LDS (issue loads for tile t+1 before computing tile t).
// "Query on the lane" throughout: S^T = K Q^T via v_mfma_f32_32x32x16_f16 puts query = lane&31 in every
// accumulator register, so the online-softmax max/sum are in-register (one cross-half shuffle) and the
// O^T = V^T P^T accumulator rescale is a per-lane scalar.  K rows are fed to the MFMA in an order that swaps
// key-index bits 2 and 3, which makes the S^T accumulator registers 8s..8s+7 exactly the natural-k fp16
// B-operand of k-step s of the PV product (no lane movement, no LDS round trip for P).  V stays row-major
// [key][d] in LDS and is consumed column-wise through ds_read_b64_tr_b16.
// LDS strides: K rows dh+8 halves (conflict-free ds_read_b128), V rows 96 halves, 160 at dh = 128 (4 consecutive rows cover
// disjoint 16-dword bank ranges for the transposed read: the stride in dwords is 16 or 48 mod 64 — 96 halves = 48, 160 halves =
// 80 = 16; dh + 8 = 136 halves = 68 = 4 would put the four rows on overlapping banks.  Derived from the bank layout, not measured).
// dh = 128 has the fp16 kernel and the plain split-pair loop, both at two workgroups per CU (75 776 bytes of LDS each); the pipelined
// split-pair loop does not fit its registers there (attention_dispatch.h ATTN_PIPE_HEAD_DIMS) and is not instantiated.
#include "attention_dispatch.h"
#include <type_traits>

struct AttnArgs {
  const half_t* Q; long ldq, sQ;
  const half_t* K; long ldk, sK;
  const half_t* V; long ldv, sV;
  half_t* O; long ldo, sO;
  int Tq, Tk, H, nqb, groups;
  float scale_log2;
  int causal;       // keys > query masked (CLIP text tower, clip_arch.py:525-531)
  long planeQ, planeK, planeV, planeO;   // X3 kernels: lo planes of the split-pair Q / K / V inputs; planeO != 0: O is written as a split pair
  // key split (zh_attention_f16_splitk): workgroup (group, qb, ks) covers keys [ks * kchunk, (ks + 1) * kchunk) and leaves its
  // UNNORMALISED fp32 accumulators + running max (log2 units) + row sum in the workspace; attn_combine_kernel merges them
  int ksplit, kchunk;
  float* part_o; float* part_m; float* part_l;   // [ksplit][B*Tq][H*dh], [ksplit][B*H][Tq] x 2
};

typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef __attribute__((address_space(3))) fp16x4* lds_fp16x4_ptr;

#define KT 64         // keys per tile of the fp16 kernels: the ABI's ZH_ATTN_KEY_TILE_F16 (asserted where KTT is formed)

// VALU diet of the key-tile loop (round 3; every vector instruction costs the SIMD's issue port 4 cycles, v_exp_f32 8, an MFMA 8 of
// its 32 — MI355X_MICROARCH.md "vector-instruction ISSUE cost" — and the softmax of a split-pair tile was ~145 of them beside 24
// MFMAs: issue-bound, not MFMA-bound).  Three pieces: the two key halves of a query meet through v_permlane32_swap instead of
// ds_bpermute (+ 6 address instructions + an LDS round trip per tile); tile loads are SGPR base + 32-bit lane offset with the
// row clamped to the last key (no zero fill, no 64-bit address arithmetic per tile); the running max only moves when it grows
// by more than 2^8 (the accumulator rescale — 32 multiplies per lane — then runs on the first tile and almost never again;
// P <= 256 stays far inside fp16 / the split pair).
// Measured (same box, us; split-pair / fp16 kernels): encoder 79.1 -> 73.3 / 41.8 -> 37.4, cross-attention 123.0 -> 118.0 / 43.7 ->
// 38.2, 518-px encoder 111.8 -> 101.6 / 56.9 -> 50.6, ViT-L/14 1335 -> 1246 / 681 -> 625, SelfMask T = 5505 251 -> 231 / 128 -> 113;
// each piece alone 1 - 3 %.  Not kept: s_setprio 1 around the K.Q^T MFMAs, the P.V MFMAs or the softmax (all within noise),
// -fno-slp-vectorize (the packed multiplies left are the now rare rescale).
#define ZH_ATTN_LAZY_LOG2 8.0f

// max over the two lanes l, l ^ 32 (both get it)
__device__ __forceinline__ float zh_xor32_max(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));   // a: lanes 32.. <- x[0..31]; b: lanes 0..31 <- x[32..]
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float zh_xor32_sum(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return a + b;
}

// X3 = 1 (the reference-equivalent mode): Q, K and V arrive as split pairs (hi = f16(x), lo = f16(x - hi)):
// S = Kh.Qh + Kl.Qh + Kh.Ql in fp32 — the softmax exponent sees fp32-class scores, which is where fp16 operand rounding is
// amplified (|s| * 2^-11 absolute) — and the probabilities are split in registers, O += Vh.Ph + Vl.Ph + Vh.Pl, so short
// key sets (decoder self-attention over 100 queries, small images) are not left with the 2^-11 rounding of single P / V
// values.  32-key tiles (the lo planes of K and V double the LDS tiles and the three-product accumulators the registers):
// three workgroups per CU at dh = 64, two at dh = 96.  The occupancy is checked at build time (build.py MIN_OCCUPANCY reads the
// compiler's resource remarks): asking for 3 through __launch_bounds__ makes hipcc pick a 168-VGPR allocation WITH 16 bytes of
// scratch, while the looser bound compiles to 165 VGPRs and none — so the bound stays loose and the build fails on a regression.
template <int DH, int NWAVE, int X3, int PIPE>
__global__ __launch_bounds__(64 * NWAVE, X3 ? 2 : (DH == 64 ? 3 : 2)) void attn_f16_kernel(AttnArgs p) {
  static_assert(!PIPE || X3, "the pipelined loop exists for the split-pair kernels");
  static_assert(32 * NWAVE == ZH_ATTN_QUERY_BLOCK, "a workgroup's queries (32 per wave) are the ABI's query block");
  constexpr int NT = 64 * NWAVE;
  static_assert(!PIPE || attn_has_pipelined(DH), "no pipelined loop at this head dim (it spills): attn_plan never asks for one");
  constexpr int KS = DH + 8;          // K row stride (halves)
  constexpr int VS = DH == 128 ? 160 : 96;   // V row stride (halves): >= DH, and 16 or 48 dwords mod 64 (header comment)
  static_assert(VS >= DH && (VS / 2) % 32 == 16, "V rows: four consecutive rows on disjoint 16-dword bank ranges");
  constexpr int NKS = DH / 16;        // k-steps of QK^T
  constexpr int NDT = DH / 32;        // 32-row d tiles of O^T
  constexpr int CPR = DH / 8;         // 16-byte chunks per K/V row
  // keys per tile: 64, except the split-pair kernels — their lo planes double the LDS tiles and their three-product
  // accumulators the registers, so at 64 keys only one workgroup fits a CU (one wave per SIMD, nothing to overlap with);
  // 32-key tiles halve both and two or three workgroups fit
  constexpr int KTT = X3 ? 32 : KT;        // (fp16 dh = 96 with 32 keys: cross-attention 44 -> 63 us — 256 workgroups, occupancy is not its limit)
  static_assert(KTT == attn_key_tile(X3), "the tile heights are the ABI's ZH_ATTN_KEY_TILE_F16 / ZH_ATTN_KEY_TILE_X3 (the launch plan chunks keys by them)");
  constexpr int NU = KTT / 32;        // 32-key slot tiles per key tile
  constexpr int NLD = (KTT * CPR + NT - 1) / NT;              // chunk passes per thread (the last may be partial: dh = 96 x 32 keys)
  constexpr bool LDFULL = (KTT * CPR) % NT == 0;
  __shared__ __attribute__((aligned(16))) half_t sKb[2][KTT * KS];   // double-buffered: one barrier per key tile
  __shared__ __attribute__((aligned(16))) half_t sKl[X3 ? 2 : 1][X3 ? KTT * KS : 8];   // lo plane of K (X3)
  __shared__ __attribute__((aligned(16))) half_t sVb[2][KTT * VS];
  __shared__ __attribute__((aligned(16))) half_t sVl[X3 ? 2 : 1][X3 ? KTT * VS : 8];   // lo plane of V (X3)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // XCD-aware block order: workgroups are dealt round-robin to the 8 XCDs (linear id % 8), each with its own L2.  The work items
  // (group = image * heads + head, query block, key split) are numbered group-major and every XCD takes a CONTIGUOUS eighth of
  // that list: the query blocks / key splits of one (image, head) — which stream the same K / V — meet in one L2 (two at a range
  // boundary), and the XCDs' shares differ by at most one workgroup.  (Round 3 dealt whole groups, group % 8 -> XCD: with the 12
  // heads of one image four XCDs got two heads and four got one — the batch-1 encoder ran at the pace of the loaded half.)
  const int id = blockIdx.y * gridDim.x + blockIdx.x;
  const int per_group = p.nqb * p.ksplit;
  const int item = (id & 7) * (int)(gridDim.x >> 3) + (id >> 3);   // the grid is 8 x (items per XCD)
  if (item >= p.groups * per_group) return;             // surplus workgroups of the last XCD share (whole workgroup, before any barrier)
  const int group = item / per_group;
  const int qbs = item - group * per_group;
  const int qb = qbs / p.ksplit, ks = qbs - qb * p.ksplit;
  const int head = group % p.H, img = group / p.H;
  const int q0 = qb * (32 * NWAVE) + wave * 32;     // first query of this wave
  const int ql = lane & 31, hh = lane >> 5;
  const long hoff = (long)head * DH;

  // this workgroup's keys: all of them, or chunk ks of the key split (kchunk is a multiple of the tile height)
  const int key0 = ks * p.kchunk;
  const int key_end = p.ksplit > 1 ? min(p.Tk, key0 + p.kchunk) : p.Tk;
  const half_t* Q = p.Q + (long)img * p.sQ + hoff;
  const half_t* K = p.K + (long)img * p.sK + hoff;
  const half_t* V = p.V + (long)img * p.sV + hoff;

  // Q fragments (B operand: col = query, k = d)
  half8_t qf[NKS], qfl[X3 ? NKS : 1];
  const half_t* qp = Q + (long)min(q0 + ql, p.Tq - 1) * p.ldq + 8 * hh;     // (a wave beyond Tq reads the last query row)
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) qf[ks] = *(const half8_t*)(qp + 16 * ks);
  if (X3) {
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qfl[ks] = *(const half8_t*)(qp + p.planeQ + 16 * ks);
  }

  f32x16 oacc[NDT];
#pragma unroll
  for (int d = 0; d < NDT; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;
  float m_run = -INFINITY;
  // Row sums of P ride the MFMA pipe: one extra "d tile" whose V^T operand is all ones accumulates sum_k P[k][q] in every row
  // of lacc (32 v_add_f32 per key tile leave the VALU, which is the bound; the sum is of the SAME rounded P the numerator uses).
  // Split-pair kernels (X3) keep the row sum on the VALU instead: they are MFMA-bound (three products per score and per P.V
  // element), the ones-operand tile is 4 of their 28 MFMAs per key tile, and P = hi + lo carries 22 bits, so the fp32 sum of the
  // un-rounded exponentials is the same number to 2^-22 — l_run accumulates this lane's 16 keys per tile (v_pk_add_f32), the
  // two key halves (lanes l, l ^ 32) meet once at the end.
  f32x16 lacc;
#pragma unroll
  for (int r = 0; r < 16; ++r) lacc[r] = 0.f;
  float l_run = 0.f;
  half8_t ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = (half_t)1.0f;

  // cooperative tile loads: chunk c -> (row = c / CPR, col chunk = c % CPR).  Tile t+1 is requested before tile t is computed
  // and stored into the other LDS buffer after it (a second register set, i.e. two tiles of load latency cover, measured no
  // gain — the kernel is VALU-bound — and its 16 registers are what keeps dh = 64 at three waves per SIMD).
  struct TileRegs { half8_t k[NLD], v[NLD], kl[X3 ? NLD : 1], vl[X3 ? NLD : 1]; };
  TileRegs ra;
  // per-lane byte offsets of this thread's chunk(s) inside a tile: SGPR base + 32-bit offset; a tile's rows are clamped to the last
  // key of the chunk (a duplicate of a real row: its scores are masked to -inf below, its V rows meet P = 0) — host check:
  // Tk * ld * 2 < 2^32.  K and V are fetched separately: the pipelined loop keeps K one tile ahead of V.
  // (Measured and not kept: a steady-state form with NO vector instruction per tile — constant per-lane offsets, the tile base
  //  advanced in SGPRs — on the theory that the 750-cycle tile-load segment of the stamps was the address instructions queueing
  //  for the vector issue port: encoder 79.8 vs 79.7 us, ViT-L/14 1331 vs 1300, fp16 kernels the same.  The segment is the
  //  loads' own issue into the CU's shared memory pipeline.  Nor did 8-wave workgroups help — 256 queries sharing every tile, one
  //  workgroup per CU with the pipelined loop, a third of the tile bytes per wave: encoder 85.2 vs 75.7 us, ViT-L/14 1438 vs 1255,
  //  518 px 99.1 vs 98.4, only SelfMask's T = 5505 gained (208 vs 219.5).  Dealing the partly filled last query block of every
  //  group after all the full ones (longest first): encoder 77.8 -> 75.7, 518 px 97.3 -> 94.9, but ViT-L/14 1248 -> 1325 (its
  //  light blocks then re-read K / V long after the group's other blocks left the L2).)
  const unsigned ldk2 = (unsigned)p.ldk * 2u, ldv2 = (unsigned)p.ldv * 2u;
  const char* const Kl = (const char*)(K + p.planeK);
  const char* const Vl = (const char*)(V + p.planeV);
  auto load_k = [&](int kbase, TileRegs& r) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int c = tid + i * NT;
      const int row = c / CPR, cc = c - row * CPR;
      if (LDFULL || c < KTT * CPR) {
        const unsigned ok = (unsigned)min(kbase + row, key_end - 1) * ldk2 + (unsigned)cc * 16u;
        r.k[i] = *(const half8_t*)((const char*)K + ok);
        if (X3) r.kl[i] = *(const half8_t*)(Kl + ok);
      }
    }
  };
  auto load_v = [&](int kbase, TileRegs& r) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int c = tid + i * NT;
      const int row = c / CPR, cc = c - row * CPR;
      if (LDFULL || c < KTT * CPR) {
        const unsigned ov = (unsigned)min(kbase + row, key_end - 1) * ldv2 + (unsigned)cc * 16u;
        r.v[i] = *(const half8_t*)((const char*)V + ov);
        if (X3) r.vl[i] = *(const half8_t*)(Vl + ov);
      }
    }
  };
  auto store_k = [&](int buf, const TileRegs& r) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int c = tid + i * NT;
      const int row = c / CPR, cc = c - row * CPR;
      if (LDFULL || c < KTT * CPR) {
        *(half8_t*)(sKb[buf] + row * KS + cc * 8) = r.k[i];
        if (X3) *(half8_t*)(sKl[buf] + row * KS + cc * 8) = r.kl[i];
      }
    }
  };
  auto store_v = [&](int buf, const TileRegs& r) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int c = tid + i * NT;
      const int row = c / CPR, cc = c - row * CPR;
      if (LDFULL || c < KTT * CPR) {
        *(half8_t*)(sVb[buf] + row * VS + cc * 8) = r.v[i];
        if (X3) *(half8_t*)(sVl[buf] + row * VS + cc * 8) = r.vl[i];
      }
    }
  };

  // K row fed at MFMA row i = lane&31: swap bits 2 and 3 of i
  const int krow = (ql & 0x13) | ((ql & 4) << 1) | ((ql & 8) >> 1);
  // transposed-read lane address pieces: group g = lane>>4, i = lane&15 -> row +(i>>2), col 16*(g&1)+4*(i&3)
  const int tr_row = 8 * hh + ((lane & 15) >> 2);
  const int tr_col = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);

  int ntiles = (max(key_end - key0, 0) + KTT - 1) / KTT;
  if (p.causal) {                                           // key tiles entirely above this block's last query are skipped
    const int qlast = min(p.Tq, (qb + 1) * (32 * NWAVE)) - 1;
    ntiles = min(ntiles, qlast / KTT + 1);
  }
  const int qidx = q0 + ql;
  // a wave whose 32 queries all lie beyond Tq (T = 442: two of the last block's four) only helps with the tile loads
  const bool active = q0 < p.Tq;

  // ---- S^T(t) = K(t) Q^T from K buffer t & 1 (NU 32-key slot tiles)
  auto qk = [&](int t, f32x16 (&s)[NU]) {
    const half_t* sK = sKb[t & 1];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[u][r] = 0.f;
      const half_t* kp = sK + (32 * u + krow) * KS + 8 * hh;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        half8_t kf = *(const half8_t*)(kp + 16 * ks);
        half8_t kl;
        if (X3) kl = *(const half8_t*)(sKl[t & 1] + (32 * u + krow) * KS + 8 * hh + 16 * ks);
        s[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], s[u], 0, 0, 0);
        if (X3) {
          s[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qf[ks], s[u], 0, 0, 0);
          s[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qfl[ks], s[u], 0, 0, 0);
        }
      }
    }
  };
  // P as packed fp16 pairs: register (r >> 1) & 3 of fragment r >> 3 holds scores r, r + 1 — the MFMA B operand as is
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  struct PFrag { u32x4 hi[NU][2], lo[X3 ? NU : 1][2]; };
  // ---- online softmax of tile t: scores -> P (fp16, or a split pair), accumulators rescaled when the reference point moves
  // (MASKED = false: the caller knows the tile is full and the attention not causal — no branch splits the block, so the
  //  pipelined loop's K.Q^T MFMAs of the next tile can be scheduled in among these instructions)
  auto softmax = [&](int t, f32x16 (&s)[NU], PFrag& P, auto masked) {
    constexpr bool MASKED = decltype(masked)::value;
    const int kbase = key0 + t * KTT;
    // register r of slot tile u holds key kbase + 32u + 16(r>>3) + 8*hh + (r&7)
    float mx = -INFINITY;
    if (MASKED && (kbase + KTT > key_end || (p.causal && kbase + KTT - 1 > q0))) {   // ragged last tile / tiles crossing the diagonal
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kbase + 32 * u + 16 * (r >> 3) + 8 * hh + (r & 7);
          if (key >= key_end || (p.causal && key > qidx)) s[u][r] = -INFINITY;
        }
    }
    {   // 32 scores per lane: four independent v_max3 chains instead of one 32-deep dependent chain
      float m4[4] = {mx, mx, mx, mx};
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int r = 0; r < 16; r += 8) {
          m4[0] = fmaxf(fmaxf(m4[0], s[u][r + 0]), s[u][r + 1]);
          m4[1] = fmaxf(fmaxf(m4[1], s[u][r + 2]), s[u][r + 3]);
          m4[2] = fmaxf(fmaxf(m4[2], s[u][r + 4]), s[u][r + 5]);
          m4[3] = fmaxf(fmaxf(m4[3], s[u][r + 6]), s[u][r + 7]);
        }
      mx = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
    }
    mx = zh_xor32_max(mx);
    // running max kept in log2 units (scale_log2 > 0 commutes with max): p = 2^(s*c - m) is ONE fma + v_exp_f32.
    // Lazy: the reference point only moves when the tile's max exceeds it by more than 2^8 (any fixed reference gives the same
    // softmax; both key halves of a query see the same mx and m_run, so they decide alike)
    const float m_cand = mx * p.scale_log2;
    const float m_new = m_cand > m_run + ZH_ATTN_LAZY_LOG2 ? m_cand : m_run;
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;
    float lsum2[2] = {0.f, 0.f};                             // scalar adds: packed fp32 VALU is an anti-lever beside MFMAs (v_pk_add_f32 ~ +13 issue cycles)
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const float e0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[u][r], p.scale_log2, -m_new));
        const float e1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[u][r + 1], p.scale_log2, -m_new));
        if (X3) { lsum2[0] += e0; lsum2[1] += e1; }
        const half2_t eh2 = {(half_t)e0, (half_t)e1};      // one v_cvt_pk_f16_f32
        unsigned eh = __builtin_bit_cast(unsigned, eh2);
        if (X3) {
          // lo = f16(e - hi) from the very bits that are used as hi (cf. zh_store_h4, common.h), ONE instruction per value:
          // v_fma_mix{lo,hi}_f16 reads hi as fp16, forms e - hi exactly in fp32 and rounds once (the plain expression costs
          // v_cvt_f32_f16 + v_sub_f32 + half a v_cvt_pk per value: of the softmax's ~26 VALU issue cycles per score, 6 go)
          unsigned el;
          asm("v_fma_mixlo_f16 %0, -%1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
              "v_fma_mixhi_f16 %0, -%1, 1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
              : "=&v"(el) : "v"(eh), "v"(e0), "v"(e1));
          P.lo[u][r >> 3][(r >> 1) & 3] = el;
        }
        P.hi[u][r >> 3][(r >> 1) & 3] = eh;
      }
    if (__any(alpha != 1.0f)) {
#pragma unroll
      for (int d = 0; d < NDT; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[d][r] *= alpha;
      if (!X3) {
#pragma unroll
        for (int r = 0; r < 16; ++r) lacc[r] *= alpha;
      }
    }
    if (X3) l_run = l_run * alpha + (lsum2[0] + lsum2[1]);
  };
  // ---- O^T += V(t)^T P^T from V buffer t & 1
  auto pv = [&](int t, const PFrag& P) {
    const half_t* sV = sVb[t & 1];
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        if (!X3) lacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ones, __builtin_bit_cast(half8_t, P.hi[u][ks]), lacc, 0, 0, 0);
        const half_t* vp = sV + (32 * u + 16 * ks + tr_row) * VS + tr_col;
#pragma unroll
        for (int d = 0; d < NDT; ++d) {
          fp16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4_ptr)(vp + 32 * d));
          fp16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4_ptr)(vp + 32 * d + 4 * VS));
          half8_t vf;
          __builtin_memcpy(&vf, &lo, 8);
          __builtin_memcpy(((char*)&vf) + 8, &hi, 8);
          half8_t vl;
          if (X3) {
            const half_t* vq = sVl[t & 1] + (32 * u + 16 * ks + tr_row) * VS + tr_col;
            fp16x4 llo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4_ptr)(vq + 32 * d));
            fp16x4 lhi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4_ptr)(vq + 32 * d + 4 * VS));
            __builtin_memcpy(&vl, &llo, 8);
            __builtin_memcpy(((char*)&vl) + 8, &lhi, 8);
          }
          const half8_t pf = __builtin_bit_cast(half8_t, P.hi[u][ks]);
          oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oacc[d], 0, 0, 0);
          if (X3) {
            oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, pf, oacc[d], 0, 0, 0);
            oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, __builtin_bit_cast(half8_t, P.lo[u][ks]), oacc[d], 0, 0, 0);
          }
        }
      }
  };

  if (PIPE && !p.causal) {
    // ---- software-pipelined loop (split-pair kernels): K runs ONE TILE AHEAD of V, and a wave issues the 12 K.Q^T MFMAs of tile
    // t+1 — which depend on nothing the softmax of tile t touches — in among that softmax's ~95 vector instructions, which
    // then issue in the shadow of the MFMAs instead of next to an idle matrix pipe (in-kernel stamps, profiles/r03_attn_stamp_x3.txt: with
    // three uncoordinated waves per SIMD the pipe was 62 % busy inside the loop; a wave spent 19 % of a tile in exp / split /
    // pack with no MFMA of its own in flight).  Step t: global loads of K(t+2), V(t+1) -> [S(t+1) || softmax(t)] -> P(t).V(t) ->
    // stores -> barrier.  K(t+2) overwrites the buffer of K(t), last read in step t-1; V(t+1) that of V(t-1), last read in step
    // t-1.  Steps are branch-free inside (full tiles, not causal); the last tile — the only one that can be ragged — is peeled.
    load_k(key0, ra);
    load_v(key0, ra);
    store_k(0, ra);
    store_v(0, ra);
    if (ntiles > 1) { load_k(key0 + KTT, ra); store_k(1, ra); }
    __syncthreads();
    f32x16 sA[NU], sB[NU];
    PFrag P;
    if (active) qk(0, sA);
    __syncthreads();                               // step 0 stores K(2) over K(0): every wave's reads of K(0) come first
    // one step: tile t has a successor; par = t & 1 as a compile-time constant
    auto step = [&](int t, auto par, f32x16 (&cur)[NU], f32x16 (&nxt)[NU]) {
      constexpr int PAR = decltype(par)::value;
      if (t + 2 < ntiles) load_k(key0 + (t + 2) * KTT, ra);
      load_v(key0 + (t + 1) * KTT, ra);
      if (active) {
        qk(PAR ^ 1, nxt);
        softmax(t, cur, P, std::false_type{});
        pv(PAR, P);
      }
      if (t + 2 < ntiles) store_k(PAR, ra);
      store_v(PAR ^ 1, ra);
      __syncthreads();
    };
    int t = 0;
    for (; t + 2 < ntiles; t += 2) {              // two tiles per trip: buffer indices and the S register sets are compile-time
      step(t, std::integral_constant<int, 0>{}, sA, sB);
      step(t + 1, std::integral_constant<int, 1>{}, sB, sA);
    }
    if (t + 1 < ntiles) {                         // two tiles left
      step(t, std::integral_constant<int, 0>{}, sA, sB);
      if (active) { softmax(t + 1, sB, P, std::true_type{}); pv(1, P); }
    } else if (active) {                          // one tile left
      softmax(t, sA, P, std::true_type{});
      pv(0, P);
    }
  } else {
  auto load_tile = [&](int kbase, TileRegs& r) { load_k(kbase, r); load_v(kbase, r); };
  auto store_tile = [&](int buf, const TileRegs& r) { store_k(buf, r); store_v(buf, r); };
  load_tile(key0, ra);
  store_tile(0, ra);
  __syncthreads();
  auto compute = [&](int t) {
    if (active) {
      f32x16 s[NU];
      PFrag P;
      qk(t, s);
      softmax(t, s, P, std::true_type{});
      pv(t, P);
    }
  };

  // buffer (t+1)&1 was last read in iteration t-1 and every wave passed the barrier that ended it => free to overwrite
  for (int t = 0; t < ntiles; t += 2) {           // two tiles per trip: the LDS buffer index is a compile-time constant
    if (t + 1 < ntiles) load_tile(key0 + (t + 1) * KTT, ra);
    compute(t);
    if (t + 1 < ntiles) store_tile(1, ra);
    __syncthreads();
    if (t + 1 >= ntiles) break;
    if (t + 2 < ntiles) load_tile(key0 + (t + 2) * KTT, ra);
    compute(t + 1);
    if (t + 2 < ntiles) store_tile(0, ra);
    __syncthreads();
  }
  }

  // f16: every row of lacc holds the full row sum of this lane's query (the MFMA already summed both key halves);
  // split pairs: this lane's half of the keys + the other half's (lane ^ 32).  (The one-trip loop is the form this epilogue had when a
  // wave could own two query tiles: written as straight-line code, hipcc rearranges the kernels' address arithmetic and register use.)
  for (int once = 0; once < 1; ++once) {
  const float l_row = X3 ? zh_xor32_sum(l_run) : lacc[0];
  const int qr = q0 + ql;
  if (p.ksplit > 1) {                                   // partial result of this key chunk: unnormalised O, running max, row sum
    if (qr < p.Tq) {
      float* po = p.part_o + (((long)ks * (p.groups / p.H) + img) * p.Tq + qr) * ((long)p.H * DH) + hoff + 4 * hh;
#pragma unroll
      for (int d = 0; d < NDT; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *(f32x4*)(po + 32 * d + 8 * g) = (f32x4){oacc[d][4 * g], oacc[d][4 * g + 1], oacc[d][4 * g + 2], oacc[d][4 * g + 3]};
      if (hh == 0) {
        const long mi = ((long)ks * p.groups + group) * p.Tq + qr;
        p.part_m[mi] = m_run;
        p.part_l[mi] = l_row;
      }
    }
    continue;
  }
  const float inv = 1.0f / l_row;
  if (qr < p.Tq) {
    half_t* op = p.O + (long)img * p.sO + (long)qr * p.ldo + hoff + 4 * hh;
#pragma unroll
    for (int d = 0; d < NDT; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 o = {oacc[d][4 * g] * inv, oacc[d][4 * g + 1] * inv, oacc[d][4 * g + 2] * inv, oacc[d][4 * g + 3] * inv};
        zh_store_h4(op + 32 * d + 8 * g, p.planeO, o);
      }
  }
  }
}

// Merge of the key-split partials: per (row = image * Tq + query, head), m = max_s m_s, w_s = 2^(m_s - m),
// O = sum_s w_s O_s / sum_s w_s l_s — the same arithmetic a single workgroup does when it meets a new running max.
__global__ __launch_bounds__(256) void attn_combine_kernel(const float* part_o, const float* part_m, const float* part_l, half_t* O, long ldo, long sO,
                                                           long planeO, int S, int B, int H, int Tq, int DH) {
  const int D = H * DH, c4 = D / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * Tq * c4) return;
  const int col = (int)(i % c4) * 4;
  const long row = i / c4;
  const int img = (int)(row / Tq), q = (int)(row - (long)img * Tq), head = col / DH;
  float m = -INFINITY;
  for (int s = 0; s < S; ++s) m = fmaxf(m, part_m[(((long)s * B + img) * H + head) * Tq + q]);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float l = 0.f;
  for (int s = 0; s < S; ++s) {
    const long mi = (((long)s * B + img) * H + head) * Tq + q;
    const float w = __builtin_amdgcn_exp2f(part_m[mi] - m);
    l += w * part_l[mi];
    acc += *(const f32x4*)(part_o + (((long)s * B + img) * Tq + q) * D + col) * w;
  }
  const float inv = 1.0f / l;
  zh_store_h4(O + (long)img * sO + (long)q * ldo + col, planeO, acc * inv);
}

// The eight instantiations, keyed as attn_plan (attention_dispatch.h) names them; workgroups of NW waves = ZH_ATTN_QUERY_BLOCK queries
constexpr int NW = ZH_ATTN_QUERY_BLOCK / 32;
struct AttnKernelRow { int head_dim, variant; void (*kernel)(AttnArgs); };
static constexpr AttnKernelRow ATTN_KERNELS[] = {
  {64, ATTN_X3_PIPE, attn_f16_kernel<64, NW, 1, 1>}, {64, ATTN_X3, attn_f16_kernel<64, NW, 1, 0>}, {64, ATTN_F16, attn_f16_kernel<64, NW, 0, 0>},
  {96, ATTN_X3_PIPE, attn_f16_kernel<96, NW, 1, 1>}, {96, ATTN_X3, attn_f16_kernel<96, NW, 1, 0>}, {96, ATTN_F16, attn_f16_kernel<96, NW, 0, 0>},
  {128, ATTN_X3, attn_f16_kernel<128, NW, 1, 0>}, {128, ATTN_F16, attn_f16_kernel<128, NW, 0, 0>},
};
static_assert(attn_table_complete(ATTN_KERNELS), "a (head_dim, variant) that attn_plan can return has no kernel");
static_assert(attn_table_no_unplanned_pipe(ATTN_KERNELS), "a pipelined kernel is listed for a head dim attn_plan never pipelines");

static int attention_launch(const void* Q, long ldq, long strideQ, const void* K, long ldk, long strideK,
                            const void* V, long ldv, long strideV, void* O, long ldo, long strideO,
                            int batch, int heads, int Tq, int Tk, int head_dim, float scale, int causal,
                            long planeQ, long planeK, long planeV, long planeO, hipStream_t stream, int ksplit = 1, void* workspace = nullptr,
                            size_t workspace_bytes = 0) {
  const AttnProblem q = attn_problem(Q, ldq, strideQ, K, ldk, strideK, V, ldv, strideV, O, ldo, strideO, batch, heads, Tq, Tk, head_dim, causal,
                                     planeQ, planeK, planeV, planeO, ksplit, workspace, workspace_bytes);
  AttnPlan plan;
  const int rc = attn_plan(q, &plan);
  if (rc != ZH_OK) return rc;
  AttnArgs p;
  p.Q = (const half_t*)Q; p.ldq = ldq; p.sQ = strideQ;
  p.K = (const half_t*)K; p.ldk = ldk; p.sK = strideK;
  p.V = (const half_t*)V; p.ldv = ldv; p.sV = strideV;
  p.O = (half_t*)O; p.ldo = ldo; p.sO = strideO;
  p.Tq = Tq; p.Tk = Tk; p.H = heads; p.nqb = plan.nqb; p.groups = plan.groups;
  p.scale_log2 = scale * 1.4426950408889634f;
  p.causal = causal;
  p.planeQ = planeQ; p.planeK = planeK; p.planeV = planeV; p.planeO = planeO;
  p.ksplit = plan.ksplit; p.kchunk = plan.kchunk;
  char* const ws = plan.ksplit > 1 ? (char*)workspace : nullptr;
  p.part_o = (float*)(ws + plan.off_o); p.part_m = (float*)(ws + plan.off_m); p.part_l = (float*)(ws + plan.off_l);
  hipLaunchKernelGGL(ATTN_KERNELS[attn_table_row(ATTN_KERNELS, head_dim, plan.variant)].kernel, dim3(plan.grid), dim3(64 * NW), 0, stream, p);
  ZH_CHECK_LAUNCH("zh_attention_f16");
  if (plan.ksplit > 1) {
    hipLaunchKernelGGL(attn_combine_kernel, dim3(plan.combine_grid), dim3(256), 0, stream, p.part_o, p.part_m, p.part_l, p.O, ldo, strideO,
                       planeO, plan.ksplit, batch, heads, Tq, head_dim);
    ZH_CHECK_LAUNCH("zh_attention_f16_splitk (combine)");
  }
  return ZH_OK;
}

// Keys split over `ksplit` workgroups per (image, head, query block) + one merge launch: for few queries against many keys (the
// decoder's cross-attention: 100 queries, 1764 keys -> 256 workgroups, ONE per CU, each streaming 1.35 MB of K / V with a single
// tile of prefetch: bytes in flight bound the kernel at half the HBM rate).  Two workgroups per CU double the bytes in flight.
extern "C" size_t zh_attention_splitk_workspace_size(int batch, int heads, int Tq, int head_dim, int ksplit) {
  return attn_splitk_workspace(batch, heads, Tq, head_dim, ksplit);
}
extern "C" int zh_attention_f16_splitk(const void* Q, long ldq, long strideQ, const void* K, long ldk, long strideK,
                                       const void* V, long ldv, long strideV, void* O, long ldo, long strideO,
                                       int batch, int heads, int Tq, int Tk, int head_dim, float scale,
                                       long planeQ, long planeK, long planeV, long planeO, int ksplit, void* workspace, size_t workspace_bytes,
                                       hipStream_t stream) {
  return attention_launch(Q, ldq, strideQ, K, ldk, strideK, V, ldv, strideV, O, ldo, strideO, batch, heads, Tq, Tk, head_dim,
                          scale, 0, planeQ, planeK, planeV, planeO, stream, ksplit, workspace, workspace_bytes);
}

extern "C" int zh_attention_f16(const void* Q, long ldq, long strideQ, const void* K, long ldk, long strideK,
                                const void* V, long ldv, long strideV, void* O, long ldo, long strideO,
                                int batch, int heads, int Tq, int Tk, int head_dim, float scale,
                                long planeQ, long planeK, long planeV, long planeO, hipStream_t stream) {
  return attention_launch(Q, ldq, strideQ, K, ldk, strideK, V, ldv, strideV, O, ldo, strideO, batch, heads, Tq, Tk, head_dim,
                          scale, 0, planeQ, planeK, planeV, planeO, stream);
}

extern "C" int zh_attention_causal_f16(const void* Q, long ldq, long strideQ, const void* K, long ldk, long strideK,
                                       const void* V, long ldv, long strideV, void* O, long ldo, long strideO,
                                       int batch, int heads, int T, int head_dim, float scale,
                                       long planeQ, long planeK, long planeV, long planeO, hipStream_t stream) {
  return attention_launch(Q, ldq, strideQ, K, ldk, strideK, V, ldv, strideV, O, ldo, strideO, batch, heads, T, T, head_dim,
                          scale, 1, planeQ, planeK, planeV, planeO, stream);
}
