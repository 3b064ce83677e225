// GEMM dispatch (host only): which instantiation of gemm_kernel.h / gemm_skinny.h a call of zh_gemm_f16, zh_gemm_f16_res16 or
// zh_gemm_f16x3 gets.  One problem description, one tile table per operand mode, two pure plan functions (no launch, no HIP call,
// no global read: the developer overrides and the number of launches in flight are passed in) and the tail peel.  gemm.hip /
// gemm_x3.hip validate, fill GemmArgs, ask the plan and launch its row; zh_dev_gemm_plan / zh_dev_gemm_plan_inflight (capi.hip) ask
// the same plan without launching.
// What was measured around these rules and not kept: profiles/NOTES.md, "GEMM dispatch: measured and not kept".
#pragma once
#include "common.h"
#include <utility>
#ifndef RING64
#define RING64 6      // ring depth of the x3 64 x 64 tile on 32-k slices (code 3066; developer A/B: -DRING64=8)
#endif
#ifndef ZH_SKINNY_MAX_ROWS
#define ZH_SKINNY_MAX_ROWS 128
#endif
#ifndef ZH_SKINNY_MAX_BLOCKS
#define ZH_SKINNY_MAX_BLOCKS 512
#endif

// Developer overrides (defined once, in capi.hip): initialised ONCE per process from ZH_GEMM_GROUP_M (super-tile height),
// ZH_GEMM_TILE (forced tile code; unknown codes are an argument error) and ZH_GEMM_TILE_SMALL (applied to M <= 4096 only) —
// never read per launch — and settable at run time through zh_dev_set_gemm_overrides() (tests / tools).
struct GemmDevOverrides { int group_m; int tile; int tile_small; };
const GemmDevOverrides& gemm_dev_overrides();

// ---- launches in flight.  A plan replay on several streams (zh_plan_run_multi / zh_plan_run2, plan.hip) issues the SAME GEMM once per
// stream, back to back, so `inflight` copies of a launch meet on the chip and share its 256 CUs: the count that the round model below
// has to fit into whole rounds is inflight x tiles, not the tiles of one launch.  gemm_inflight() (capi.hip) is that number for the
// calling thread: 1 outside a replay loop, the loop's stream count inside one, or the developer's forced value
// (zh_dev_set_gemm_inflight).  The plan functions take it as an input (default 1: one launch on an empty chip) and stay pure.
// What it was measured against: tools/gemm_inflight_ab.py, profiles/gemm_inflight_ab.json (profiles/NOTES.md, "GEMM tiles for the
// launches in flight").  Every ring tile sums K in the same order (ZH_GEMM_FIXED_K_ORDER's contract), so the bits of a result do
// not depend on the number: a replay in flight stays bitwise equal to the eager step.
int gemm_inflight();
struct GemmInflightScope {            // the replay loops: set for the duration of the loop, restored afterwards (this thread only)
  int prev;
  explicit GemmInflightScope(int n);
  ~GemmInflightScope();
  GemmInflightScope(const GemmInflightScope&) = delete;
  GemmInflightScope& operator=(const GemmInflightScope&) = delete;
};
#ifndef ZH_GEMM_INFLIGHT_MIN_ROWS
#define ZH_GEMM_INFLIGHT_MIN_ROWS 2048
#endif
#define ZH_GEMM_INFLIGHT_MAX 64

enum { GEMM_F16 = 0, GEMM_RES16 = 1, GEMM_X3 = 2, GEMM_X2 = 3 };        // operand mode (x2: zh_gemm_f16x3 with planeW = 0)
enum { GEMM_RING = 0, GEMM_SKINNY = 1 };                                // kernel family
enum { GEMM_STORE_SCALAR = 0, GEMM_STORE_DIRECT = 1, GEMM_STORE_WIDE = 2 };   // epilogue (= the kernel's VEC); the few-row kernel: 0 scalar, 1 vec

// What the choice depends on.  C / bias / residual are pointer VALUES (alignment only); out_kind: 0 f32, 1 f16, 2 split pair.
struct GemmProblem {
  int mode, M, N, K, batch; long lda, ldw, ldc, strideC, planeC, ldr, strideR; int res_rows, out_kind, act, flags;
  uintptr_t C, bias, residual; bool has_pos, res_f16;
};
struct GemmPlan { int family, code, path; long peel_rows; };            // code 0: the base tile of the scalar / direct paths; peel_rows 0: none

// ---- tile tables: code, waves WM x WN, 16 x 16 fragments per wave TM x TN (tile = WM TM 16 rows x WN TN 16 columns), ring slots
struct GemmTile { int code, wm, wn, tm, tn, stages; };
constexpr GemmTile GEMM_TILES_F16[] = {
  {128, 2, 2, 4, 4, 4},    // 128 x 128: the base tile (scalar / direct stores take it whatever the code)
  {64, 2, 2, 4, 2, 4},     // 128 x 64
  {192, 2, 4, 8, 3, 4},    // 256 x 192
  {256, 2, 4, 8, 4, 4},    // 256 x 256
  {2128, 2, 2, 4, 4, 8},   // 128 x 128, 8-deep ring
  {2064, 2, 2, 4, 2, 8},   // 128 x 64, 8-deep ring
  {3064, 2, 2, 2, 2, 8},   // 64 x 64, 8-deep ring
  {7032, 2, 2, 2, 2, 7},   // 64-k slices (gemm_k64_plain): 64 x 64, seven slots
  {7096, 2, 2, 4, 3, 5},   // ... 128 x 96, five
  {7128, 2, 2, 4, 4, 5},   // ... 128 x 128, five
};
constexpr GemmTile GEMM_TILES_X3[] = {
  {64, 2, 2, 4, 2, 3},     // 128 x 64, 4 waves, two blocks per CU: the base tile
  {512, 2, 4, 8, 4, 2},    // 256 x 256 on two slots (waves of 128 x 64, 64 KiB per K slice)
  {448, 2, 4, 6, 4, 2},    // 192 x 256 on two slots (waves of 96 x 64, 56 KiB)
  {256, 4, 2, 4, 4, 3},    // 256 x 128, 8 waves, 144 KiB ring
  {192, 4, 2, 3, 4, 3},    // 192 x 128, 120 KiB ring
  {96, 4, 2, 2, 3, 3},     // 128 x 96: 8 waves of 32 x 48
  {3064, 2, 2, 2, 2, 4},   // 64 x 64 on 64-k slices, four slots (three slices in flight)
  {3066, 2, 2, 2, 2, RING64},   // developer A/B: 64 x 64 on 32-k slices, six slots (the form until round 5)
  {1288, 4, 2, 2, 4, 4},   // 128 x 128, 8 waves of 32 x 64, 4 slots
  {6496, 4, 2, 2, 3, 2},   // K64 (64-k slices, two slots): 128 x 96, 8 waves of 32 x 48
  {6464, 4, 2, 2, 2, 3},   // K64 on THREE slots: 128 x 64, 8 waves of 32 x 32
  {7096, 4, 2, 2, 3, 4},   // K64 on a circular ring of 160 pieces: 128 x 96
  {7128, 4, 2, 2, 4, 3},   // ... 128 x 128
};
// one-plane weights: the big tiles stage 48 KiB per slice without the W lo rows: three slots (two slices of prefetch) fit the LDS
constexpr GemmTile GEMM_TILES_X2[] = {
  {64, 2, 2, 4, 2, 3},     // the base tile
  // 256 x 256 as 4 x 2 waves of 64 x 128: an A fragment costs two LDS reads (hi, lo), a W fragment one — 16 reads per slice and wave
  // instead of the 20 of 128 x 64 waves (5124): L/14 qkv 1604 -> 1568 us, c_proj 2266 -> 2099, c_fc 2219 -> 2204 (same box)
  {512, 4, 2, 4, 8, 3},
  {5122, 2, 4, 8, 4, 2},   // developer A/B: 256 x 256 on TWO slots (2 x 4 waves of 128 x 64)
  {5124, 2, 4, 8, 4, 3},   // developer A/B: ... on three
  {4484, 4, 2, 3, 8, 3},   // developer A/B: 192 x 256 as 4 x 2 waves of 48 x 128
  {448, 2, 4, 6, 4, 3},
  {256, 4, 2, 4, 4, 3},
  {192, 4, 2, 3, 4, 4},    // 4 slots: the epilogue slabs need 102 KiB
  {96, 4, 2, 2, 3, 3},
  {3064, 2, 2, 2, 2, 4},
  {3066, 2, 2, 2, 2, RING64},
  {6464, 4, 2, 2, 2, 3},
  {1288, 4, 2, 2, 4, 4},
  {6496, 4, 2, 2, 3, 2},
};
constexpr int gemm_tile_m(const GemmTile& t) { return t.wm * t.tm * 16; }
constexpr int gemm_tile_n(const GemmTile& t) { return t.wn * t.tn * 16; }
template <size_t R>
constexpr const GemmTile* gemm_tile(const GemmTile (&rows)[R], int code) {      // nullptr: the table has no such row
  for (size_t i = 0; i < R; ++i) if (rows[i].code == code) return &rows[i];
  return nullptr;
}
// the table row of a plan's code (0 = the mode's base tile, row 0); nullptr: no such row, or the few-row kernel (32 x 32 blocks, no table)
static inline const GemmTile* gemm_plan_tile(int mode, int code) {
  if (mode <= GEMM_RES16) return code ? gemm_tile(GEMM_TILES_F16, code) : GEMM_TILES_F16;
  if (mode == GEMM_X3) return code ? gemm_tile(GEMM_TILES_X3, code) : GEMM_TILES_X3;
  return code ? gemm_tile(GEMM_TILES_X2, code) : GEMM_TILES_X2;
}
// The plan's launch.  launch(GemmRow) -> bool instantiates one row with one epilogue: the base tile (row 0) for scalar / direct stores,
// else the row of the plan's code.  1 launched, 0 the epilogue is not instantiated, -1 the table lacks the code.
template <const auto& ROWS, size_t I, int VEC> struct GemmRow { static constexpr GemmTile t = ROWS[I]; static constexpr int vec = VEC; };
template <const auto& ROWS, class L, size_t... I>
static inline int gemm_launch_plan(const GemmPlan& plan, L&& launch, std::index_sequence<I...>) {
  if (plan.path != GEMM_STORE_WIDE) return plan.path == GEMM_STORE_SCALAR ? launch(GemmRow<ROWS, 0, 0>{}) : launch(GemmRow<ROWS, 0, 1>{});
  int ok = -1;
  (void)((ROWS[I].code == plan.code && ((ok = launch(GemmRow<ROWS, I, 2>{})), true)) || ...);
  return ok;
}

// ---- store-path predicates
// 4-element stores: columns, row / batch strides and every pointer the epilogue reads or writes aligned to four elements
static inline bool gemm_vec_ok(const GemmProblem& q) {
  const int esz = q.out_kind == 0 ? 4 : 2;
  return q.N % 4 == 0 && q.ldc % 4 == 0 && q.strideC % 4 == 0 && (q.C & (4 * esz - 1)) == 0 && (!q.bias || (q.bias & 15) == 0) &&
         (!q.residual || (q.ldr % 4 == 0 && q.strideR % 4 == 0 && (q.residual & (q.res_f16 ? 7 : 15)) == 0));
}
// the LDS-staged epilogue moves 16-byte chunks: 16-B aligned rows of 16-B multiples
static inline bool gemm_wide_ok(const GemmProblem& q) {
  const int esz = q.out_kind == 0 ? 4 : 2;
  if (!(gemm_vec_ok(q) && (q.C & 15) == 0 && (q.ldc * esz) % 16 == 0 && (q.strideC * esz) % 16 == 0 && (q.N * esz) % 16 == 0)) return false;
  // plain fp16 operands: with an fp16 output the residual is fp16 too (16-byte chunks of 8 halves) or absent
  if (q.mode <= GEMM_RES16)
    return !q.residual || (q.res_f16 ? (q.ldr % 8 == 0 && q.strideR % 8 == 0 && (q.residual & 15) == 0) : q.out_kind == 0);
  // split operands: an fp16 slab's residual takes the direct-store path; a split output's two planes are both 16-B aligned
  return (q.out_kind != 1 || !q.residual) && (q.out_kind != 2 || q.planeC % 8 == 0);
}

// host-side check of the optional pos tables (both or neither)
static inline bool zh_pos_tables_ok(const void* pos_y, const void* pos_x, long ld_pos, int pos_h, int pos_w, int N) {
  if (!pos_y && !pos_x) return true;
  return pos_y && pos_x && pos_h > 0 && pos_w > 0 && ld_pos >= N && ld_pos % 8 == 0 && N % 4 == 0 &&
         (((uintptr_t)pos_y | (uintptr_t)pos_x) & 15) == 0;
}

// The argument checks, the kernel-argument fill and the problem description that zh_gemm_f16 / zh_gemm_f16_res16 and zh_gemm_f16x3
// share.  `fn`: the entry's name for the error text; plain fp16 operands: planes 0, out_scale 1.  Args = GemmArgs of gemm_kernel.h
// (a template parameter: this header stays free of the kernel's).
template <class Args>
static inline int gemm_prepare(const char* fn, int mode, const void* A, long lda, long strideA, long planeA, const void* W, long ldw, long strideW,
                               long planeW, void* C, long ldc, long strideC, long planeC, int out_kind, float out_scale, const float* bias,
                               const void* residual, long ldr, long strideR, int res_rows, const void* pos_y, const void* pos_x, long ld_pos,
                               int pos_h, int pos_w, int pos_f16, int act, int M, int N, int K, int batch, int flags, Args* pp, GemmProblem* q) {
  ZH_CHECK_ARG(A && W && C, "%s: null operand", fn);
  ZH_CHECK_ARG(M > 0 && N > 0 && K > 0 && batch > 0, "%s: bad shape M=%d N=%d K=%d batch=%d", fn, M, N, K, batch);
  ZH_CHECK_ARG(K % 64 == 0, "%s: K=%d must be a multiple of 64", fn, K);
  ZH_CHECK_ARG(lda % 8 == 0 && ldw % 8 == 0 && strideA % 8 == 0 && strideW % 8 == 0 && planeA % 8 == 0 && planeW % 8 == 0,
               "%s: lda/ldw/strides/planes must be multiples of 8 halves (16-byte rows)", fn);
  ZH_CHECK_ARG(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0, "%s: A/W must be 16-byte aligned", fn);
  ZH_CHECK_ARG(act >= 0 && act <= 4, "%s: bad activation %d", fn, act);
  // the kernel addresses an operand row as base + (32-bit element offset): keep one batch item's A / W below 2^32 elements
  ZH_CHECK_ARG((long)(M - 1) * lda + K <= 0xFFFFFFFFL && (long)(N - 1) * ldw + K <= 0xFFFFFFFFL,
               "%s: an operand exceeds 2^32 elements per batch item (M=%d lda=%ld N=%d ldw=%ld)", fn, M, lda, N, ldw);
  ZH_CHECK_ARG(!residual || res_rows > 0, "%s: residual needs res_rows > 0", fn);
  ZH_CHECK_ARG(zh_pos_tables_ok(pos_y, pos_x, ld_pos, pos_h, pos_w, N), "%s: pos tables need both pointers 16-byte aligned, "
               "pos_h, pos_w > 0, ld_pos %% 8 == 0 and N %% 4 == 0", fn);
  *q = {mode, M, N, K, batch, lda, ldw, ldc, strideC, planeC, ldr, strideR, res_rows, out_kind, act, flags,
        (uintptr_t)C, (uintptr_t)bias, (uintptr_t)residual, pos_y != nullptr, mode == GEMM_RES16};
  Args& p = *pp;
  p.A = (const half_t*)A; p.lda = lda; p.sA = strideA; p.planeA = planeA;
  p.W = (const half_t*)W; p.ldw = ldw; p.sW = strideW; p.planeW = planeW;
  p.C = C; p.ldc = ldc; p.sC = strideC; p.planeC = planeC; p.out_scale = out_scale;
  p.bias = bias; p.R = (const float*)residual; p.ldr = ldr; p.sR = strideR; p.res_rows = res_rows;
  p.pos_y = pos_y; p.pos_x = pos_x; p.ld_pos = ld_pos; p.pos_hw = pos_h * pos_w; p.pos_w = pos_w; p.pos_f16 = pos_f16;
  p.M = M; p.N = N; p.K = K; p.act = act; p.nbm = p.nbn = 0;
  // super-tile height: 3..8 measure within 1-3 % of each other on the model (4: least fabric traffic, 134 vs 141 MB per launch,
  // and the best step), 14: -1 %, 16 / 32 lose 13 / 36 % on 8192^3 (tools/gemm_vs_blaslt.py) — the order in which an XCD's 32
  // resident tiles share panels matters
  p.group_m = gemm_dev_overrides().group_m;
  p.vec_ok = gemm_vec_ok(*q);
  return ZH_OK;
}

// Relative time estimate of a tiling: rounds of the 256-CU chip x time of one round.  With `bpc` blocks resident
// per CU a round takes bpc x the tile's own time; `eff` is the measured relative speed of the tile shape at
// K=768 (256x256: 1.0, 256x192: 0.95, 128x128: 0.8 — tools/gemm_bench.py on MI355X).  `inflight` copies of the launch
// share the rounds (the estimate is then the time of the whole group).
static inline double tiling_cost(long M, long N, int batch, int BM, int BN, int bpc, double eff, int inflight = 1) {
  const long tiles = (long)zh_cdiv(M, BM) * zh_cdiv(N, BN) * batch * inflight;
  const long slots = 256L * bpc;
  const long rounds = (tiles + slots - 1) / slots;
  return (double)rounds * BM * BN * bpc / eff;
}
static inline long gemm_tiles(const GemmProblem& q, int BM, int BN) { return (long)zh_cdiv(q.M, BM) * zh_cdiv(q.N, BN) * q.batch; }
// The copies of a launch that the choosers count.  A launch keeps the pick of one launch on an empty chip (1) unless it fills the
// chip by itself — more than one 128 x 64 tile per CU — and has at least ZH_GEMM_INFLIGHT_MIN_ROWS rows.  Below either bound is the
// few-tile regime (one image: M = 442 / 1201 / 1601 tokens; the decoder at small batches): bound by the load latency of a ring, not by
// rounds of the chip, the copies in flight overlap that latency, and none of its tiles was measured in flight.  Measured: M = 3200
// (the headline's decoder), 8200 (config 4's encoder) and 14144 (the headline's encoder), tools/gemm_inflight_ab.py.
static inline int gemm_inflight_counted(const GemmProblem& q, int inflight) {
  if (inflight <= 1 || q.M < ZH_GEMM_INFLIGHT_MIN_ROWS || gemm_tiles(q, 128, 64) <= 256) return 1;
  return inflight < ZH_GEMM_INFLIGHT_MAX ? inflight : ZH_GEMM_INFLIGHT_MAX;
}

// ---- tail peel.  A big-tile GEMM whose tile count is a few tiles more than whole rounds of the 256-CU chip pays a full round for
// them (config 5's out_proj / c_proj, 147712 x 1024: 2308 tiles of 256 x 256 = 9 rounds + 4 tiles, i.e. 10 rounds: +10 %).  When
// the surplus is at most a quarter round, the last m-tile rows that hold it are peeled into a second call on the row range
// [M', M) — its own, small-tile choice; same stream, same arithmetic per output element (the K order of a tile does not depend
// on the tile shape: results are bitwise those of one launch) — and the main launch is left with whole rounds.
// Only where row offsets are plain pointer offsets: no batch, no pos tables, a residual with a row of its own per output row.
// With `inflight` copies of the launch on the chip the rounds are those of inflight x tiles: the surplus of the group is shared out
// among the copies (each peels the same rows), and the quarter round bounds what the group peels.  (Config 5's 147712-row GEMMs peel
// the same one m-tile row at 1 and at 3 in flight: 4 / 12 / 16 surplus tiles a launch, 12 / 36 / 48 a group of three.)
// Returns M' (rows that stay: whole tiles, whole rounds or just under), 0 for no peel.
static inline long gemm_peel_rows(const GemmProblem& q, const GemmTile& big, bool wide, int inflight = 1) {
  if (!wide || q.batch != 1 || q.has_pos || (q.residual && q.res_rows < q.M)) return 0;
  const long BM = gemm_tile_m(big), nbm = zh_cdiv(q.M, BM), nbn = zh_cdiv(q.N, gemm_tile_n(big)), tiles = nbm * nbn * inflight, rem = tiles % 256;
  if (tiles <= 4 * 256 || rem == 0 || rem > 64) return 0;
  const long per = (rem + inflight - 1) / inflight;           // surplus tiles of one copy
  const long r = (per + nbn - 1) / nbn;                       // m-tile rows to peel
  return (r * nbn * inflight <= 64 && r < nbm) ? (nbm - r) * BM : 0;   // (0 < M' < M: r >= 1, and nbm > r since tiles > 16 r nbn inflight)
}
// the two calls of a peeled GEMM: call(A, C, residual, res_rows, M) on rows [0, M1) and [M1, M); c_esz / r_esz: bytes per element
template <class Call>
static inline int gemm_tail_peel(long M1, int M, const void* A, long lda, void* C, long ldc, int c_esz, const void* residual, long ldr,
                                 int r_esz, int res_rows, Call&& call) {
  const int rc = call(A, C, residual, residual ? res_rows : 0, (int)M1);
  if (rc != ZH_OK) return rc;
  return call((const char*)A + M1 * lda * 2, (char*)C + M1 * ldc * c_esz, residual ? (const char*)residual + M1 * ldr * r_esz : nullptr,
              residual ? (int)(res_rows - M1) : 0, (int)(M - M1));
}

static inline GemmPlan gemm_ring_plan(const GemmProblem& q, int pick, bool wide, long peel_rows) {
  return {GEMM_RING, wide ? pick : 0, wide ? GEMM_STORE_WIDE : (gemm_vec_ok(q) ? GEMM_STORE_DIRECT : GEMM_STORE_SCALAR), peel_rows};
}

// ---- plain fp16 operands (zh_gemm_f16, zh_gemm_f16_res16)
// `fl`: the copies of the launch that are counted (gemm_plan_f16 below decides that number)
static inline int gemm_plan_f16_counted(const GemmProblem& q, const GemmDevOverrides& ov, GemmPlan* plan, int fl) {
  const int M = q.M, N = q.N, batch = q.batch;
  ZH_CHECK_ARG(gemm_tiles(q, 64, 64) < (1L << 31), "zh_gemm_f16: grid too large");
  // the developer override: tile_small applies to M <= 4096 only; an unknown code is an error
  const int forced = ov.tile ? ov.tile : (M <= 4096 ? ov.tile_small : 0);
  ZH_CHECK_ARG(!forced || gemm_tile(GEMM_TILES_F16, forced),
               "zh_gemm_f16: ZH_GEMM_TILE(_SMALL)=%d is not a tile code (64|128|192|256|2064|2128|3064|7032|7096|7128)", forced);
  const double c256 = tiling_cost(M, N, batch, 256, 256, 1, 1.0, fl);
  const double c192 = tiling_cost(M, N, batch, 256, 192, 1, 0.95, fl);
  const double c128 = tiling_cost(M, N, batch, 128, 128, 2, 0.8, fl);
  int pick = (c128 < c256 && c128 < c192) ? 128 : (c192 < c256 ? 192 : 256);
  // (the few-tile and one-round rules below count the fl copies together, as the cost model does: fl = 1 is the rules as they were)
  const long t128 = fl * gemm_tiles(q, 128, 128);
  // few-tile GEMMs (batch-1 inference: M = 442 tokens -> 24 tiles of 128x128 on 256 CUs): 64x64 tiles on an 8-deep
  // ring put 4x the CUs to work; measured 32 -> 16 us on the 442x768x3072 MLP projection (tools/gemm_small.py)
  if (t128 <= 96) pick = 3064;
  // narrow outputs that do not fill the chip with 128 x 128 tiles (decoder M = B*Q rows x N = 768): 128 x 64 tiles put twice the
  // blocks to work; measured 19.6 -> 16.5 us (K = 768) and 32.7 -> 28.8 us (K = 2048) with the residual epilogue, while
  // N = 1536 / 2048 keep 128 x 128 (tools/gemm_dec_tiles.py)
  else if (pick == 128 && t128 <= 256 && N <= 768) pick = 64;
  // Round 5: one-round tiles on 64-k slices (128-B row pieces) with several slices in flight (gemm_kernel.h K64 / gemm_k64_plain; the
  // finding of the split-pair tiles, tools/gemm_small_bench.py k64f): 64 x 64 on seven slots instead of eight 32-k ones (c_proj at one
  // image 18.6 -> 15.1 us, at 442 tokens 17.4 -> 13.7); 128 x 96 on five where it makes ONE round (the decoder's 3200 x 768 x 768
  // 14.7 -> 13.1 / 12.3 -> 10.4 us, linear2 (K = 2048) 26.7 -> 22.1, QKV at one image 11.7 -> 10.7); 128 x 128 on five where that is one
  // round (c_fc at one image 14.2 -> 13.7).
  if (pick == 3064) pick = 7032;
  else if ((pick == 64 || pick == 128) && N % 96 == 0 && fl * (long)zh_cdiv(M, 128) * (N / 96) * batch <= 256) pick = 7096;
  else if (pick == 128 && t128 <= 256) pick = 7128;
  if (forced) pick = forced;
  const bool wide = gemm_wide_ok(q);
  // tail peel: the 256-row tiles only, never under a forced code
  const long peel = ((pick == 256 || pick == 192) && !forced) ? gemm_peel_rows(q, *gemm_plan_tile(q.mode, pick), wide, fl) : 0;
  *plan = gemm_ring_plan(q, pick, wide, peel);
  return ZH_OK;
}

// ---- split-pair operands (zh_gemm_f16x3; GEMM_X2 = its one-plane weights)
// `fl`: the copies of the launch that are counted (gemm_plan_x3 below decides that number)
static inline int gemm_plan_x3_counted(const GemmProblem& q, const GemmDevOverrides& ov, GemmPlan* plan, int fl) {
  const int M = q.M, N = q.N, batch = q.batch;
  const bool x2 = q.mode == GEMM_X2;
  // fl copies of this launch meet on the chip: the cost model and every one-round rule below count fl x tiles.  Measured at 3 in flight (us per group of three, median; profiles/gemm_inflight_ab.json):
  //   c_proj 14144 x 768 x 3072: 192 x 256 530.0 -> 256 x 256 506.9, out_proj (K = 768) 144.9 -> 141.9 (666 tiles = 2.6 rounds against
  //   504 = 1.97; alone on the chip 192 x 256 wins, 183.7 / 57.0 against 203.8 / 63.8); one-plane weights 385.4 -> 373.4, 111.5 -> 109.8;
  //   the decoder's 3200 x 768 x 768: 128 x 96 on the circular ring 46.8 (fp32 + residual) / 46.1 (split out + table) -> 256 x 128
  //   40.6 / 38.9, linear2 (K = 2048) 106.5 -> 87.2 (600 tiles = 2.3 rounds against 234 = one; alone 21.0 / 20.2 / 44.7 against
  //   31.3 / 30.4 / 64.7).  At 2 in flight the decoder takes 192 x 128 (204 tiles, one round): 32.1 / 30.9 / 70.1 -> 31.0 / 29.3 / 65.2.
  //   QKV, c_fc, the K / V projections (256 x 256) and the decoder's N = 2048 / 2304 GEMMs (256 x 128) keep their tiles, and the
  //   clock agrees: the runner-up of each is 3 - 6 % slower at 3 in flight.
  ZH_CHECK_ARG(gemm_tiles(q, 64, 64) < (1L << 31), "zh_gemm_f16x3: grid too large");
  // the developer override (tile_small never forces a tile here): a code of this mode's table is taken — the circular-ring tiles
  // not with pos tables — and any other code, such as one of zh_gemm_f16's, forces nothing.  ANY set code still marks the process
  // as a developer run: no few-row kernel (but code 32: that kernel for any M), no promotion of 96 to 7096, no tail peel.
  const int forced = ov.tile;
  const bool own = forced && (x2 ? gemm_tile(GEMM_TILES_X2, forced) != nullptr
                                 : gemm_tile(GEMM_TILES_X3, forced) && !((forced == 7096 || forced == 7128) && q.has_pos));
  // few-row GEMMs (the decoder at batch 1, ffn2, SelfMask's 20 queries): gemm_skinny.h — operands straight into fragments, K split
  // over the four waves of a block, no ring.  Shape only (never alignment): the K order of a row's sum — and with it the bits of
  // the result — must not depend on how many columns a caller asks for (sharded retrieval merges shards of any width).
  // ZH_GEMM_FIXED_K_ORDER: the caller compares results of calls with different M / N bit for bit (sharded retrieval): the LDS-ring
  // family only, whose K order is the same for every tile.  Otherwise: few rows AND a grid small enough that the kernel's re-reads of
  // the row block (once per 32 output columns) do not matter — the class-logit GEMM of a 32-image batch (81 x 1764 x 512 x 32 =
  // 5376 workgroups) took 113 us here against ~20 on the ring.
  const int max_rows = forced == 32 ? (1 << 30) : ((forced || (q.flags & ZH_GEMM_FIXED_K_ORDER)) ? 0 : ZH_SKINNY_MAX_ROWS);
  const long sk_blocks = gemm_tiles(q, 32, 32);
  if (!q.has_pos && M <= max_rows && sk_blocks <= 65535L * 8 && (forced == 32 || sk_blocks <= ZH_SKINNY_MAX_BLOCKS)) {
    *plan = {GEMM_SKINNY, 32, gemm_vec_ok(q) ? 1 : 0, 0};
    return ZH_OK;
  }
  // 256 x 128 or 192 x 128 (8 waves, 144 / 120 KiB ring, one block per CU; the 192-row tile quantises N = 768 GEMMs into
  // 1.73 rounds of the chip instead of 1.31) or 128 x 64 (4 waves, two blocks per CU) for small problems
  const double c256 = tiling_cost(M, N, batch, 256, 128, 1, 1.0, fl);
  const double c192 = tiling_cost(M, N, batch, 192, 128, 1, 0.95, fl);
  const double c64 = tiling_cost(M, N, batch, 128, 64, 2, 0.7, fl);
  int pick = (c64 < c256 && c64 < c192) ? 64 : (c192 < c256 ? 192 : 256);
  // ... or, for M >= 4096 rows, the two-slot big tiles (8 waves, 2 x 4): 256 x 256 (waves of 128 x 64, 64 KiB per K slice) and
  // 192 x 256 (waves of 96 x 64, 56 KiB) — a third fewer staged bytes per MFMA than 256 x 128, which is what bounds the 3-slot
  // loop (profiles/NOTES.md round 3).  256 x 256 serves the wide GEMMs (QKV, c_fc, the K / V projections); 192 x 256 turns the
  // N = 768 ones (out_proj, c_proj) into ONE round of 222 tiles where 192 x 128 needs two rounds of 444.
  if (M >= 4096) {
    const double cbig = tiling_cost(M, N, batch, 256, 256, 1, 1.25, fl);
    const double c448 = tiling_cost(M, N, batch, 192, 256, 1, 1.2, fl);
    const double cur = pick == 64 ? c64 : (pick == 192 ? c192 : c256);
    if (cbig < cur && cbig <= c448) pick = 512;
    else if (c448 < cur) pick = 448;
  }
  // The one-round rules below are stated for the fl copies together: a tile that is ONE round of the chip for a lone launch is fl
  // rounds of it in flight, and then is not what these rules measured — they hand the call back to the cost model's pick above
  // (the decoder's 3200 x 768 in flight: 256 x 128 / 192 x 128 instead of 128 x 96; fl = 1: exactly the rules as they were).
  const long t64 = fl * gemm_tiles(q, 128, 64);
  // few-row GEMMs whose 128 x 64 tiling is a bit more than one tile per CU (the decoder's 3200 x 768: 300 tiles — the CUs with two
  // tiles stream 1.2 MB of operands at the ~61 GB/s a CU's LDS-DMA sustains = 19 us, and that is the kernel): 128 x 96 tiles
  // (3-slot ring, one block per CU) make it 200 tiles of 0.69 MB, ONE per CU.  Eight waves of 32 x 48 (two per SIMD) rather than
  // four of 64 x 48: the fp32-residual epilogue has twice the waves to hide its loads behind (24.5 -> 21.8 us; split out 20.2 both)
  if (pick == 64 && M <= 4096 && N % 96 == 0 && t64 > 256 && fl * (long)zh_cdiv(M, 128) * (N / 96) * batch <= 256) pick = 96;
  // few-tile GEMMs (batch-1 inference, the COCO-20K evaluation's regime: M = 442 tokens -> 48 .. 192 tiles of 128 x 64 on 256 CUs):
  // they are bound by the load latency of a 3-slot ring, not by arithmetic — 64 x 64 tiles put more CUs to work, on 64-k slices
  // (128-B row pieces: 85 instead of 52 - 57 GB/s of request rate) in four slots, three slices in flight: out_proj at one image
  // 12.3 -> 11.1 us, QKV / c_fc at 442 tokens 13.6 -> 12.2 / 24.2 -> 21.2.  Only while the 64 x 64 tiles still fit ONE round of the
  // chip, one block per CU: c_fc at M = 442 is 336 such tiles and ran 18.3 -> 23.6 us with them
  if (pick == 64 && fl * gemm_tiles(q, 64, 64) <= 256) pick = 3064;
  // ... and a 128 x 64 tile on three 64-k slots of 48 KiB where ITS tiles are one round and the 64 x 64 ones are not
  // (1201 x 1536 x 768: 18.8 -> 15.1 us)
  if (pick == 64 && t64 <= 256) pick = 6464;
  if (own) pick = forced;
  // M ~ 1200 rows (one image at native resolution: c_fc 1201 x 3072, the split-K planes of c_proj / out_proj): 128 x 64 tiles are 480
  // workgroups, two per CU, each staging its own A panel; 128 x 128 tiles (8 waves of 32 x 64, 4 slots) are 240, ONE round with a third
  // fewer staged bytes: c_fc 29.4 -> 24.6 us, c_proj planes (S = 4) 28.8 -> 24.8, out_proj planes 12.2 -> 11.0 (round 4, same box).
  // (A forced 64 is still 64 here, so this rule applies to it.)
  if (pick == 64 && fl * gemm_tiles(q, 128, 128) <= 256 && t64 > 256) pick = 1288;
  // The 128 x 96 tile (56 KiB per 64-k slice) on a CIRCULAR ring of 160 one-KiB pieces (gemm_kernel.h FRAC): behind every barrier one
  // slice's worth of pieces — the tail of slice kt + 1, then the head of slice kt + 2 — refills what slice kt - 1 left, 48 .. 104 KiB
  // ahead of the reads instead of the 56 of two slots.  QKV at one image 23.5 -> 21.8 us, the decoder's 3200 x 768 x 768 21.1 -> 20.8
  // (r05_gemm_k64_deep.txt).  Two-plane weights only, not with pos tables.
  if (pick == 96 && !forced && !x2 && !q.has_pos) pick = 7096;
  // the two-slot tiles address operand rows as SGPR base + 32-bit per-lane BYTE offset
  if ((pick == 512 || pick == 448 || pick == 5122 || pick == 5124 || pick == 4484) &&
      ((long)(M - 1) * q.lda + q.K > 0x7FFFFFFFL || (long)(N - 1) * q.ldw + q.K > 0x7FFFFFFFL)) pick = 256;
  const bool wide = gemm_wide_ok(q);
  // tail peel: the 256-column two-slot tiles only, never in a developer run (tile_small only gates the peel here)
  const long peel = ((pick == 512 || pick == 448) && !forced && ov.tile_small == 0) ? gemm_peel_rows(q, *gemm_plan_tile(q.mode, pick), wide, fl) : 0;
  *plan = gemm_ring_plan(q, pick, wide, peel);
  return ZH_OK;
}

// ---- the plans of the entries: the copies in flight are counted where the launch fills the chip (gemm_inflight_counted), and they
// never SHRINK the tile of the lone launch.  More copies on the chip mean more, not fewer, tiles to fit into rounds, which favours the
// bigger tile; where fl x tiles nevertheless quantises in favour of a smaller one, the clock did not confirm it — c_fc
// (14144 x 3072 x 768) at 2 in flight: 1344 tiles of 256 x 256 are 5.25 rounds, 1776 of 192 x 256 are 6.94, the model takes the second
// and it measured 367.9 us per pair against 349.2 (profiles/gemm_inflight_ab.json) — so such a call keeps the lone launch's plan.
static inline long gemm_plan_area(int mode, const GemmPlan& p) {
  const GemmTile* t = p.family == GEMM_RING ? gemm_plan_tile(mode, p.code) : nullptr;
  return t ? (long)gemm_tile_m(*t) * gemm_tile_n(*t) : 32L * 32;
}
// A second exception, split pair only: a call whose lone launch runs a 3-slot tile moves to a two-slot tile (256 x 256 / 192 x 256) on
// account of the copies in flight only with K >= 1024 and three or more in flight.  The two-slot tiles pay a longer prologue and
// epilogue per tile, which the round model does not see: config 4's encoder (8200 rows, 256 x 128 alone), us per group, 256 x 128 /
// 192 x 256 / 256 x 256: c_proj (K = 3072) at three in flight 345.4 / 311.4 / 313.3 — taken — but at two 205.2 / 222.7 / 214.6, and
// out_proj (K = 768) at three 103.1 / 109.3 / 117.7, at two 63.9 / 65.3 / 63.8: the model's picks (256 x 256 at two, 192 x 256 at three)
// lose or tie there, so those calls keep the lone launch's plan.
static inline bool gemm_two_slot(int mode, const GemmPlan& p) {
  return mode >= GEMM_X3 && p.family == GEMM_RING && (p.code == 512 || p.code == 448);
}
template <class PlanFn>
static inline int gemm_plan_in_flight(const GemmProblem& q, const GemmDevOverrides& ov, GemmPlan* plan, int fl, PlanFn&& counted) {
  int rc = counted(q, ov, plan, fl);
  if (rc != ZH_OK || fl == 1) return rc;
  GemmPlan lone;
  if ((rc = counted(q, ov, &lone, 1)) != ZH_OK) return rc;
  if (gemm_plan_area(q.mode, *plan) < gemm_plan_area(q.mode, lone)) *plan = lone;
  else if (gemm_two_slot(q.mode, *plan) && !gemm_two_slot(q.mode, lone) && !(q.K >= 1024 && fl >= 3)) *plan = lone;
  return ZH_OK;
}
// Plain fp16 operands count the copies in flight for N <= 768 at three or more in flight: the flips that the table shows winning at
// `fast`, us per group of three — c_proj / out_proj (14144 rows) 256 x 192 -> 256 x 256: 241.0 -> 217.8 / 81.7 -> 77.4; the decoder's
// 3200 x 768 GEMMs 128 x 96 -> 128 x 128: 27.2 -> 22.9 (fp32 + residual), 21.5 -> 17.8 (fp16 out), linear2 49.5 -> 42.1; config 4's
// c_proj / out_proj (8200 rows) 128 x 128 -> 256 x 192: 157.3 -> 126.9 / 50.9 -> 49.0.  Everything else stays on its present pick: at
// two in flight the model's flips lose as often as they win (the decoder's QKV 3200 x 2304 to 256 x 256 38.6 -> 42.4, config 4's
// out_proj to 256 x 256 31.5 -> 35.3; its c_proj 102.0 -> 84.0), and of the wider outputs at three the decoder's linear1 (3200 x 2048
// to 256 x 192) gains, 41.2 -> 38.6, while its QKV does not, 49.4 -> 50.8.
static inline int gemm_plan_f16(const GemmProblem& q, const GemmDevOverrides& ov, GemmPlan* plan, int inflight = 1) {
  const int fl = (inflight >= 3 && q.N <= 768) ? gemm_inflight_counted(q, inflight) : 1;
  return gemm_plan_in_flight(q, ov, plan, fl, gemm_plan_f16_counted);
}
static inline int gemm_plan_x3(const GemmProblem& q, const GemmDevOverrides& ov, GemmPlan* plan, int inflight = 1) {
  return gemm_plan_in_flight(q, ov, plan, gemm_inflight_counted(q, inflight), gemm_plan_x3_counted);
}
