// zh_gemm_f16: fp16-operand / fp32-accumulate instantiations of the MFMA GEMM (kernel + design notes: gemm_kernel.h; which
// instantiation a call gets: gemm_dispatch.h).
#include "gemm_kernel.h"
#include "gemm_dispatch.h"

// Instantiated (out type, activation) pairs = the ones the hot path uses; anything else is an argument error.
template <int WM, int WN, int TM, int TN, int STAGES, int VEC>
static bool launch_gemm(const GemmArgs& p, int batch, int out_f16, int res_f16, hipStream_t stream) {
  const int key = res_f16 * 16 + out_f16 * 8 + p.act;
  switch (key) {
    case 0 + ZH_ACT_NONE: launch_one<WM, WN, TM, TN, STAGES, 0, ZH_ACT_NONE, VEC, 0>(p, batch, stream); return true;
    case 0 + ZH_ACT_SIGMOID: launch_one<WM, WN, TM, TN, STAGES, 0, ZH_ACT_SIGMOID, VEC, 0>(p, batch, stream); return true;
    case 8 + ZH_ACT_NONE: launch_one<WM, WN, TM, TN, STAGES, 1, ZH_ACT_NONE, VEC, 0>(p, batch, stream); return true;
    case 8 + ZH_ACT_QUICKGELU: launch_one<WM, WN, TM, TN, STAGES, 1, ZH_ACT_QUICKGELU, VEC, 0>(p, batch, stream); return true;
    case 8 + ZH_ACT_RELU: launch_one<WM, WN, TM, TN, STAGES, 1, ZH_ACT_RELU, VEC, 0>(p, batch, stream); return true;
    case 8 + ZH_ACT_GELU_ERF: launch_one<WM, WN, TM, TN, STAGES, 1, ZH_ACT_GELU_ERF, VEC, 0>(p, batch, stream); return true;
    case 16 + 8 + ZH_ACT_NONE: launch_one<WM, WN, TM, TN, STAGES, 3, ZH_ACT_NONE, VEC, 0>(p, batch, stream); return true;   // f16 out, f16 residual
    default: return false;
  }
}

// zh_gemm_f16 (res_f16 = 0: residual fp32) and zh_gemm_f16_res16 (res_f16 = 1: residual fp16, output fp16)
static int gemm_f16_impl(const void* A, long lda, long strideA, const void* W, long ldw, long strideW,
                         void* C, long ldc, long strideC, int out_f16,
                         const float* bias, const void* residual, int res_f16, long ldr, long strideR, int res_rows,
                         const void* pos_y, const void* pos_x, long ld_pos, int pos_h, int pos_w, int pos_f16,
                         int act, int M, int N, int K, int batch, hipStream_t stream) {
  GemmArgs p;
  GemmProblem q;
  GemmPlan plan;
  int rc = gemm_prepare("zh_gemm_f16", res_f16 ? GEMM_RES16 : GEMM_F16, A, lda, strideA, 0, W, ldw, strideW, 0, C, ldc, strideC, 0, out_f16 ? 1 : 0, 1.0f,
                        bias, residual, ldr, strideR, res_rows, pos_y, pos_x, ld_pos, pos_h, pos_w, pos_f16, act, M, N, K, batch, 0, &p, &q);
  if (rc != ZH_OK) return rc;
  ZH_CHECK_ARG(!res_f16 || (out_f16 && act == ZH_ACT_NONE), "zh_gemm_f16_res16: an fp16 residual goes with an fp16 output and no activation");
  if ((rc = gemm_plan_f16(q, gemm_dev_overrides(), &plan, gemm_inflight())) != ZH_OK) return rc;
  if (plan.peel_rows)
    return gemm_tail_peel(plan.peel_rows, M, A, lda, C, ldc, out_f16 ? 2 : 4, residual, ldr, res_f16 ? 2 : 4, res_rows,
                          [&](const void* a, void* c, const void* r, int rows, int m) {
                            return gemm_f16_impl(a, lda, strideA, W, ldw, strideW, c, ldc, strideC, out_f16, bias, r, res_f16, ldr, strideR, rows,
                                                 pos_y, pos_x, ld_pos, pos_h, pos_w, pos_f16, act, m, N, K, 1, stream);
                          });
  const int ok = gemm_launch_plan<GEMM_TILES_F16>(plan, [&](auto row) {
    constexpr GemmTile t = decltype(row)::t;
    return launch_gemm<t.wm, t.wn, t.tm, t.tn, t.stages, decltype(row)::vec>(p, batch, out_f16, res_f16, stream);
  }, std::make_index_sequence<std::size(GEMM_TILES_F16)>{});
  ZH_CHECK_ARG(ok >= 0, "zh_gemm_f16: the plan's tile code %d has no table row", plan.code);
  ZH_CHECK_ARG(ok, "zh_gemm_f16: (out_f16=%d, act=%d) is not an instantiated epilogue (f32: none|sigmoid; f16: none|quickgelu|relu|gelu_erf)",
               out_f16, act);
  ZH_CHECK_LAUNCH("zh_gemm_f16");
  return ZH_OK;
}

extern "C" int zh_gemm_f16(const void* A, long lda, long strideA, const void* W, long ldw, long strideW,
                           void* C, long ldc, long strideC, int out_f16,
                           const float* bias, const float* residual, long ldr, long strideR, int res_rows,
                           const void* pos_y, const void* pos_x, long ld_pos, int pos_h, int pos_w, int pos_f16,
                           int act, int M, int N, int K, int batch, hipStream_t stream) {
  return gemm_f16_impl(A, lda, strideA, W, ldw, strideW, C, ldc, strideC, out_f16, bias, residual, 0, ldr, strideR, res_rows,
                       pos_y, pos_x, ld_pos, pos_h, pos_w, pos_f16, act, M, N, K, batch, stream);
}

// The fp16 residual stream (precision "half"): C f16 = f16(f16(A W^T + bias) + residual), residual f16 (may alias C).
extern "C" int zh_gemm_f16_res16(const void* A, long lda, long strideA, const void* W, long ldw, long strideW,
                                 void* C, long ldc, long strideC,
                                 const float* bias, const void* residual, long ldr, long strideR, int res_rows,
                                 int M, int N, int K, int batch, hipStream_t stream) {
  ZH_CHECK_ARG(residual, "zh_gemm_f16_res16: null residual (zh_gemm_f16 is the form without one)");
  return gemm_f16_impl(A, lda, strideA, W, ldw, strideW, C, ldc, strideC, 1, bias, residual, 1, ldr, strideR, res_rows,
                       nullptr, nullptr, 0, 0, 0, 0, ZH_ACT_NONE, M, N, K, batch, stream);
}
