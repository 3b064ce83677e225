// C-ABI plumbing for libzutis_hip: version + thread-local error text, and the GEMM developer switches.
#include "common.h"
#include <stdarg.h>

static thread_local char g_err[512] = "";

void zh_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* zh_last_error(void) { return g_err; }
extern "C" int zh_version(void) { return ZH_ABI_VERSION; }   // include/zutis_hip.h
extern "C" const char* zh_arch(void) { return "gfx950"; }

// ---- developer overrides of the GEMM tile choice (gemm_dispatch.h): one process-wide instance, initialised from the environment
//      once, changed only through zh_dev_set_gemm_overrides (tests force every tile variant with it)
#include <stdlib.h>
#include "gemm_dispatch.h"
static GemmDevOverrides& gemm_dev_state() {
  static GemmDevOverrides o = [] {
    GemmDevOverrides v{4, 0, 0};
    if (const char* g = getenv("ZH_GEMM_GROUP_M")) { const int x = atoi(g); if (x >= 1) v.group_m = x; }
    if (const char* t = getenv("ZH_GEMM_TILE")) v.tile = atoi(t);
    if (const char* t = getenv("ZH_GEMM_TILE_SMALL")) v.tile_small = atoi(t);
    return v;
  }();
  return o;
}
const GemmDevOverrides& gemm_dev_overrides() { return gemm_dev_state(); }
extern "C" int zh_dev_set_gemm_overrides(int group_m, int tile, int tile_small) {
  ZH_CHECK_ARG(group_m >= 0 && tile >= 0 && tile_small >= 0, "zh_dev_set_gemm_overrides: negative argument");
  GemmDevOverrides& o = gemm_dev_state();
  o.group_m = group_m >= 1 ? group_m : 4;
  o.tile = tile;
  o.tile_small = tile_small;
  return ZH_OK;
}

// ---- launches in flight (gemm_dispatch.h): how many copies of a GEMM launch meet on the chip.  The replay loops of plan.hip set the
//      calling thread's number for the duration of their loop (GemmInflightScope); everywhere else it is 1.  The developer setter
//      forces one value for every launch of the process (tests and tools: eager calls at a forced value), 0 = not forced.
static thread_local int t_gemm_inflight = 1;
static int g_gemm_inflight_forced = 0;
int gemm_inflight() { return g_gemm_inflight_forced ? g_gemm_inflight_forced : t_gemm_inflight; }
GemmInflightScope::GemmInflightScope(int n) : prev(t_gemm_inflight) { t_gemm_inflight = n < 1 ? 1 : (n > ZH_GEMM_INFLIGHT_MAX ? ZH_GEMM_INFLIGHT_MAX : n); }
GemmInflightScope::~GemmInflightScope() { t_gemm_inflight = prev; }
extern "C" int zh_dev_set_gemm_inflight(int inflight) {
  ZH_CHECK_ARG(inflight >= 0 && inflight <= ZH_GEMM_INFLIGHT_MAX, "zh_dev_set_gemm_inflight: %d is not 0 (not forced) or 1 .. %d", inflight, ZH_GEMM_INFLIGHT_MAX);
  g_gemm_inflight_forced = inflight;
  return ZH_OK;
}

// What the dispatcher decides for a GEMM, asked without launching: the plan functions the three entries call, under the process's
// current overrides.  Pointer VALUES only (alignment); runs without a GPU.  zh_dev_gemm_plan: for the number of launches in flight the
// calling thread's next launch would see (gemm_inflight()); zh_dev_gemm_plan_inflight: for a given number.
extern "C" int zh_dev_gemm_plan(int mode, int M, int N, int K, int batch, long lda, long ldw, long ldc, long strideC, long planeC,
                                long ldr, long strideR, int res_rows, int out_kind, int act, int flags,
                                const void* C, const void* bias, const void* residual, int has_pos, int* plan) {
  return zh_dev_gemm_plan_inflight(mode, M, N, K, batch, lda, ldw, ldc, strideC, planeC, ldr, strideR, res_rows, out_kind, act, flags, C, bias, residual,
                                   has_pos, gemm_inflight(), plan);
}
extern "C" int zh_dev_gemm_plan_inflight(int mode, int M, int N, int K, int batch, long lda, long ldw, long ldc, long strideC, long planeC,
                                         long ldr, long strideR, int res_rows, int out_kind, int act, int flags,
                                         const void* C, const void* bias, const void* residual, int has_pos, int inflight, int* plan) {
  ZH_CHECK_ARG(plan && mode >= GEMM_F16 && mode <= GEMM_X2, "zh_dev_gemm_plan: null plan or mode %d not in {0 f16, 1 res16, 2 x3, 3 x2}", mode);
  ZH_CHECK_ARG(M > 0 && N > 0 && K > 0 && batch > 0, "zh_dev_gemm_plan: bad shape M=%d N=%d K=%d batch=%d", M, N, K, batch);
  ZH_CHECK_ARG(inflight >= 1 && inflight <= ZH_GEMM_INFLIGHT_MAX, "zh_dev_gemm_plan_inflight: inflight %d not in 1 .. %d", inflight, ZH_GEMM_INFLIGHT_MAX);
  const GemmProblem q = {mode, M, N, K, batch, lda, ldw, ldc, strideC, planeC, ldr, strideR, res_rows, out_kind, act, flags,
                         (uintptr_t)C, (uintptr_t)bias, (uintptr_t)residual, has_pos != 0, mode == GEMM_RES16};
  GemmPlan g;
  const int rc = mode <= GEMM_RES16 ? gemm_plan_f16(q, gemm_dev_overrides(), &g, inflight) : gemm_plan_x3(q, gemm_dev_overrides(), &g, inflight);
  if (rc != ZH_OK) return rc;
  const GemmTile* t = gemm_plan_tile(mode, g.code);
  ZH_CHECK_ARG(t || g.family == GEMM_SKINNY, "zh_dev_gemm_plan: the plan's tile code %d has no table row", g.code);
  plan[0] = g.family; plan[1] = g.code; plan[2] = t ? gemm_tile_m(*t) : 32; plan[3] = t ? gemm_tile_n(*t) : 32;   // few-row kernel: 32 x 32 blocks
  plan[4] = g.path; plan[5] = (int)g.peel_rows;
  return ZH_OK;
}

// What the attention launcher decides for a call, asked without launching: the plan function attention_launch calls (attention.hip).
#include "attention_dispatch.h"
extern "C" int zh_dev_attention_plan(const void* Q, long ldq, long strideQ, const void* K, long ldk, long strideK,
                                     const void* V, long ldv, long strideV, const void* O, long ldo, long strideO,
                                     int batch, int heads, int Tq, int Tk, int head_dim, int causal,
                                     long planeQ, long planeK, long planeV, long planeO, int ksplit, const void* workspace, size_t workspace_bytes,
                                     int* plan) {
  ZH_CHECK_ARG(plan, "zh_dev_attention_plan: null plan");
  AttnPlan a;
  const int rc = attn_plan(attn_problem(Q, ldq, strideQ, K, ldk, strideK, V, ldv, strideV, O, ldo, strideO, batch, heads, Tq, Tk, head_dim, causal,
                                        planeQ, planeK, planeV, planeO, ksplit, workspace, workspace_bytes), &a);
  if (rc != ZH_OK) return rc;
  ZH_CHECK_ARG(a.workspace_bytes <= 0x7FFFFFFF, "zh_dev_attention_plan: a workspace of %zu bytes does not fit the int row", a.workspace_bytes);
  plan[0] = a.variant; plan[1] = a.key_tile; plan[2] = a.nqb; plan[3] = (int)a.items; plan[4] = (int)a.grid; plan[5] = a.pipe;
  plan[6] = a.ksplit; plan[7] = a.kchunk; plan[8] = (int)a.workspace_bytes; plan[9] = (int)a.combine_grid;
  return ZH_OK;
}

// persistent big-tile GEMMs (gemm_kernel.h PERS): workgroups per launch = the CUs of the CURRENT device rounded down to a multiple
// of 8 (a persistent workgroup takes a CU's whole LDS; the tile walk deals ids modulo 8 to the XCDs) — 256 on an MI355X in SPX mode,
// fewer in a partitioned mode.  Resolved at the first launch (no HIP call at load time: build() loads the library without a GPU) and
// cached per process; ZH_GEMM_PERSIST / zh_dev_set_gemm_persist override it for tests and A/B runs (0 = off, else a multiple of 8).
// The one mutable word that steers product launches: written only by the developer setter, read once per launch.
static int gemm_persist_valid(int n) { return n >= 0 && n % 8 == 0; }
static int g_gemm_persist = [] {
  const char* e = getenv("ZH_GEMM_PERSIST");
  if (!e) return -1;                                    // auto
  char* end = nullptr;
  const long v = strtol(e, &end, 10);
  if (end == e || *end != 0 || v < 0 || v > (1 << 20) || !gemm_persist_valid((int)v)) {
    fprintf(stderr, "zutis_hip: ZH_GEMM_PERSIST=%s ignored (not 0 or a multiple of 8)\n", e);
    return -1;
  }
  return (int)v;
}();
int gemm_persist_cus() {
  if (g_gemm_persist >= 0) return g_gemm_persist;
  static const int auto_cus = [] {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 8) return 256;
    return cus / 8 * 8;
  }();
  return auto_cus;
}
extern "C" int zh_dev_set_gemm_persist(int workgroups) {
  ZH_CHECK_ARG(workgroups >= -1 && (workgroups == -1 || gemm_persist_valid(workgroups)), "zh_dev_set_gemm_persist: %d is not -1 (auto), 0 (off) or a multiple of 8", workgroups);
  g_gemm_persist = workgroups;
  return ZH_OK;
}
