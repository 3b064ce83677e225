// Attention dispatch (host only): what a call of zh_attention_f16, zh_attention_causal_f16 or zh_attention_f16_splitk launches.  One
// problem description and one pure plan function (no launch, no HIP call, no global read) that holds every argument check, the
// choice of the kernel variant, the grid, the key chunking and the split-K workspace layout.  attention.hip fills AttnArgs from the
// plan and launches its table row; zh_dev_attention_plan (capi.hip) asks the same plan without launching.
// The tile constants are the header's (ZH_ATTN_QUERY_BLOCK, ZH_ATTN_KEY_TILE_F16 / _X3): static_asserts in attention.hip hold the kernels to them.
#pragma once
#include "common.h"

// The chip the pipelined-loop rule quantises the grid against: the 256 CUs of an MI355X, as a constant (not the device's count: the
// rule must give one answer per shape wherever it is asked, with or without a GPU).
constexpr int ATTN_CUS = 256;

enum { ATTN_F16 = 0, ATTN_X3 = 1, ATTN_X3_PIPE = 2, ATTN_VARIANTS = 3 };     // kernel variant = the template pair (X3, PIPE): (0, 0), (1, 0), (1, 1)
constexpr int ATTN_HEAD_DIMS[] = {64, 96, 128};
// head dims whose split-pair kernel has a software-pipelined form.  Not 128: K(t+2) in flight beside the S accumulators of two tiles
// and four O tiles is 256 VGPRs plus 120 bytes of scratch per lane, and a spill in this file is a build error.
constexpr int ATTN_PIPE_HEAD_DIMS[] = {64, 96};

constexpr bool attn_head_dim_ok(int head_dim) {
  for (int dh : ATTN_HEAD_DIMS) if (dh == head_dim) return true;
  return false;
}
constexpr bool attn_has_pipelined(int head_dim) {
  for (int dh : ATTN_PIPE_HEAD_DIMS) if (dh == head_dim) return true;
  return false;
}

// What the choice depends on.  Q / K / V / O / workspace are pointer VALUES (null and alignment checks only); ksplit <= 1: no key split.
struct AttnProblem {
  int batch, heads, Tq, Tk, head_dim, causal, ksplit;
  bool x3;                                                   // split-pair operands: planeQ != 0
  long ldq, strideQ, ldk, strideK, ldv, strideV, ldo, strideO, planeQ, planeK, planeV, planeO;
  uintptr_t Q, K, V, O, workspace;
  size_t workspace_bytes;
};
struct AttnPlan {
  int variant, pipe;                                         // ATTN_*; pipe = (variant == ATTN_X3_PIPE)
  int key_tile, query_block;
  int nqb, groups;                                           // query blocks per (image, head); (image, head) pairs
  long items;                                                // workgroups with work: groups * nqb * ksplit
  unsigned grid;                                             // items rounded up to the 8 XCDs (the kernel decodes the id XCD-aware)
  int ksplit, kchunk;                                        // 1, 0: no split; else keys per chunk (a multiple of key_tile)
  size_t off_o, off_m, off_l, workspace_bytes;               // byte offsets of the three partial arrays in the workspace; bytes needed (0: no split)
  unsigned combine_grid;                                     // 256-thread blocks of attn_combine_kernel (0: no split)
};

static inline AttnProblem attn_problem(const void* Q, long ldq, long strideQ, const void* K, long ldk, long strideK, const void* V, long ldv,
                                       long strideV, const void* O, long ldo, long strideO, int batch, int heads, int Tq, int Tk, int head_dim,
                                       int causal, long planeQ, long planeK, long planeV, long planeO, int ksplit, const void* workspace,
                                       size_t workspace_bytes) {
  return {batch, heads, Tq, Tk, head_dim, causal, ksplit, planeQ != 0, ldq, strideQ, ldk, strideK, ldv, strideV, ldo, strideO,
          planeQ, planeK, planeV, planeO, (uintptr_t)Q, (uintptr_t)K, (uintptr_t)V, (uintptr_t)O, (uintptr_t)workspace, workspace_bytes};
}

constexpr int attn_key_tile(bool x3) { return x3 ? ZH_ATTN_KEY_TILE_X3 : ZH_ATTN_KEY_TILE_F16; }

// Split-K workspace: [ksplit][B*Tq][H*dh] unnormalised fp32 O, then [ksplit][B*H][Tq] running max and row sum.  Returns the bytes;
// off (optional): the byte offsets of the three arrays.
static inline size_t attn_splitk_workspace(int batch, int heads, int Tq, int head_dim, int ksplit, size_t* off = nullptr) {
  const size_t no = (size_t)ksplit * batch * Tq * heads * head_dim, nm = (size_t)ksplit * batch * heads * Tq;
  if (off) { off[0] = 0; off[1] = no * 4; off[2] = (no + nm) * 4; }
  return (no + 2 * nm) * 4;
}

// Split-pair kernels: the software-pipelined loop (K.Q^T of tile t+1 issued in among the softmax of tile t; bit-identical
// results) needs 193 registers at dh = 64, two waves per SIMD instead of three.  Same box, us, plain -> pipelined: decoder
// cross-attention (dh = 96, two waves either way) 120.4 -> 103.7; SelfMask T = 5505 (264 workgroups) 240.1 -> 223.2; 518-px
// encoder (864) 102.3 -> 98.7; 336-px encoder (1536) 76.5 -> 77.4; ViT-L/14 (20480) 1249 -> 1306.  So, of the head dims that have the
// pipelined kernel (ATTN_PIPE_HEAD_DIMS): dh = 96 always takes it (its plain loop has no occupancy to lose), dh = 64 when the grid
// needs no more rounds of the chip at two workgroups per CU than at three.  dh = 128 has none and runs the plain loop.
// `grid` is the launch grid, items rounded up to 8; shape_rules.pipelined_loop asks the same of the items themselves, and the two
// agree because 2 * ATTN_CUS and 3 * ATTN_CUS are multiples of 8: ceil(n / m) = ceil(8 ceil(n / 8) / m) whenever 8 divides m.
constexpr bool attn_pipelined_always(int head_dim) { return head_dim == 96; }
static inline bool attn_pipelined(bool x3, int head_dim, long grid) {
  return x3 && attn_has_pipelined(head_dim) &&
         (attn_pipelined_always(head_dim) || zh_cdiv(grid, 2L * ATTN_CUS) <= zh_cdiv(grid, 3L * ATTN_CUS));
}
// Whether attn_plan can return `variant` for `head_dim` (over all grids): the pairs the launcher's table must hold.
constexpr bool attn_plan_returns(int head_dim, int variant) {
  return attn_head_dim_ok(head_dim) &&
         (variant == ATTN_F16 || (variant == ATTN_X3 && !(attn_has_pipelined(head_dim) && attn_pipelined_always(head_dim))) ||
          (variant == ATTN_X3_PIPE && attn_has_pipelined(head_dim)));
}

static inline int attn_plan(const AttnProblem& q, AttnPlan* plan) {
  ZH_CHECK_ARG(q.Q && q.K && q.V && q.O, "zh_attention_f16: null operand");
  ZH_CHECK_ARG(q.batch > 0 && q.heads > 0 && q.Tq > 0 && q.Tk > 0, "zh_attention_f16: bad shape");
  ZH_CHECK_ARG(attn_head_dim_ok(q.head_dim), "zh_attention_f16: head_dim %d not in {64, 96, 128}", q.head_dim);
  ZH_CHECK_ARG(q.ldq % 8 == 0 && q.ldk % 8 == 0 && q.ldv % 8 == 0 && q.ldo % 4 == 0 && q.strideQ % 8 == 0 && q.strideK % 8 == 0 &&
                   q.strideV % 8 == 0 && q.strideO % 4 == 0 && q.planeQ % 8 == 0 && q.planeK % 8 == 0 && q.planeV % 8 == 0 && q.planeO % 4 == 0,
               "zh_attention_f16: row/batch/plane strides must keep 16-byte (Q,K,V) / 8-byte (O) alignment");
  ZH_CHECK_ARG((q.Q & 15) == 0 && (q.K & 15) == 0 && (q.V & 15) == 0 && (q.O & 7) == 0, "zh_attention_f16: misaligned pointer");
  ZH_CHECK_ARG(q.heads < 65536 && q.batch < 65536, "zh_attention_f16: heads/batch exceed grid limits");
  // K / V rows are addressed as (per-image, per-head base) + 32-bit byte offset
  ZH_CHECK_ARG((long)q.Tk * q.ldk * 2 < (1L << 32) && (long)q.Tk * q.ldv * 2 < (1L << 32), "zh_attention_f16: Tk * ldk (ldv) exceeds 2^31 elements");
  ZH_CHECK_ARG((q.planeQ != 0) == (q.planeK != 0) && (q.planeQ != 0) == (q.planeV != 0),
               "zh_attention_f16: the split-pair mode needs the lo planes of Q, K and V (all three or none)");
  AttnPlan& p = *plan;
  p = AttnPlan{};
  p.key_tile = attn_key_tile(q.x3);
  // 128-query (4-wave) blocks: each K/V tile is shared four ways.  A 64-query (2-wave) variant was measured slower on
  // every shape of the model (encoder 301 vs 423 TF, cross-attention 230 vs 397 TF) and was dropped.
  p.query_block = ZH_ATTN_QUERY_BLOCK;
  p.nqb = zh_cdiv(q.Tq, p.query_block);
  p.groups = q.heads * q.batch;
  p.ksplit = 1;
  if (q.ksplit > 1) {
    ZH_CHECK_ARG(!q.causal && q.ksplit <= 64, "zh_attention_f16_splitk: ksplit %d not in 1..64 (and not for the causal form)", q.ksplit);
    p.ksplit = q.ksplit;
    p.kchunk = zh_cdiv(zh_cdiv(q.Tk, p.key_tile), q.ksplit) * p.key_tile;
    // No empty key chunk.  With ktiles = ceil(Tk / key_tile) and c = ceil(ktiles / S) this is shape_rules.fit_key_split's
    // (S - 1) * c < ktiles: that gives (S - 1) * c * key_tile <= (ktiles - 1) * key_tile < Tk, and (S - 1) * c * key_tile < Tk <=
    // ktiles * key_tile gives it back.
    ZH_CHECK_ARG((long)(q.ksplit - 1) * p.kchunk < q.Tk, "zh_attention_f16_splitk: ksplit %d leaves an empty key chunk for Tk = %d", q.ksplit, q.Tk);
    size_t off[3];
    p.workspace_bytes = attn_splitk_workspace(q.batch, q.heads, q.Tq, q.head_dim, q.ksplit, off);
    ZH_CHECK_ARG(q.workspace && q.workspace_bytes >= p.workspace_bytes && (q.workspace & 15) == 0,
                 "zh_attention_f16_splitk: workspace too small or misaligned (%zu < %zu)", q.workspace_bytes, p.workspace_bytes);
    p.off_o = off[0]; p.off_m = off[1]; p.off_l = off[2];
    p.combine_grid = (unsigned)zh_cdiv((long)q.batch * q.Tq * q.heads * q.head_dim / 4, 256);
  }
  p.items = (long)p.groups * p.nqb * p.ksplit;
  ZH_CHECK_ARG(p.items < (1L << 31) - 8, "zh_attention_f16: grid too large");
  const long nblk = (long)zh_cdiv(p.items, 8) * 8;        // decoded XCD-aware in the kernel: XCD x takes items [x * nblk / 8, (x + 1) * nblk / 8)
  ZH_CHECK_ARG(nblk < (1L << 31), "zh_attention_f16: grid too large");
  p.grid = (unsigned)nblk;
  p.pipe = attn_pipelined(q.x3, q.head_dim, nblk);
  p.variant = !q.x3 ? ATTN_F16 : (p.pipe ? ATTN_X3_PIPE : ATTN_X3);
  return ZH_OK;
}

// The launcher's kernel table: rows of {head_dim, variant, ...}.  Index of the row of (head_dim, variant), -1: none.
template <class Row, size_t R>
constexpr int attn_table_row(const Row (&rows)[R], int head_dim, int variant) {
  for (size_t i = 0; i < R; ++i) if (rows[i].head_dim == head_dim && rows[i].variant == variant) return (int)i;
  return -1;
}
// every (head_dim, variant) attn_plan can return has a row.  Only those are required: dh = 128 has no pipelined kernel to list, and the
// (96, ATTN_X3) row the table keeps is the plain loop the pipelined one is measured against, which the plan never picks.
template <class Row, size_t R>
constexpr bool attn_table_complete(const Row (&rows)[R]) {
  for (int dh : ATTN_HEAD_DIMS)
    for (int v = 0; v < ATTN_VARIANTS; ++v) if (attn_plan_returns(dh, v) && attn_table_row(rows, dh, v) < 0) return false;
  return true;
}
// and no row is one the plan could pick by mistake: a head dim without a pipelined kernel lists none
template <class Row, size_t R>
constexpr bool attn_table_no_unplanned_pipe(const Row (&rows)[R]) {
  for (size_t i = 0; i < R; ++i) if (rows[i].variant == ATTN_X3_PIPE && !attn_has_pipelined(rows[i].head_dim)) return false;
  return true;
}
