// zh_gemm_f16x3: the reference-equivalent GEMM mode.  The reference computes every contraction in fp32
// (networks/clip_arch.py:286-292 keeps LayerNorm in fp32, networks/zutis.py:55 casts the CLIP weights back to fp32);
// gfx950 has no fast fp32 matrix path (v_mfma_f32_*_f32: 157 TFLOP/s dense against 2.5 PFLOP/s for fp16), so fp32-class
// products are built from fp16 MFMAs: each operand x is carried as the pair hi = f16(x), lo = f16(x - hi) — 22
// significand bits — and  A.W = Ah.Wh + Ah.Wl + Al.Wh  accumulates in fp32 (dropped Al.Wl term: 2^-22 relative).
// Weights are packed as W * 2^s (s chosen per matrix so that lo stays a normal fp16 number); `out_scale` = 2^-s is applied
// to the accumulator before the bias.  Kernel: gemm_kernel.h with SPLIT = 1; which instantiation a call gets: gemm_dispatch.h.
#include "gemm_kernel.h"
#include "gemm_skinny.h"
#include "gemm_dispatch.h"

template <int WM, int WN, int TM, int TN, int STAGES, int VEC, int SP = 1>
static bool launch_x3(const GemmArgs& p, int batch, int out_kind, hipStream_t stream) {
  const int key = out_kind * 8 + p.act;
  switch (key) {
    case 0 + ZH_ACT_NONE: launch_one<WM, WN, TM, TN, STAGES, 0, ZH_ACT_NONE, VEC, SP>(p, batch, stream); return true;
    case 0 + ZH_ACT_SIGMOID: launch_one<WM, WN, TM, TN, STAGES, 0, ZH_ACT_SIGMOID, VEC, SP>(p, batch, stream); return true;
    case 8 + ZH_ACT_NONE: launch_one<WM, WN, TM, TN, STAGES, 1, ZH_ACT_NONE, VEC, SP>(p, batch, stream); return true;
    case 16 + ZH_ACT_NONE: launch_one<WM, WN, TM, TN, STAGES, 2, ZH_ACT_NONE, VEC, SP>(p, batch, stream); return true;
    default: break;
  }
  if (VEC == 2) {   // activations feeding another GEMM only occur on 16-byte aligned rows
    switch (key) {
      case 8 + ZH_ACT_QUICKGELU: launch_one<WM, WN, TM, TN, STAGES, 1, ZH_ACT_QUICKGELU, 2, SP>(p, batch, stream); return true;
      case 8 + ZH_ACT_RELU: launch_one<WM, WN, TM, TN, STAGES, 1, ZH_ACT_RELU, 2, SP>(p, batch, stream); return true;
      case 8 + ZH_ACT_GELU_ERF: launch_one<WM, WN, TM, TN, STAGES, 1, ZH_ACT_GELU_ERF, 2, SP>(p, batch, stream); return true;
      case 16 + ZH_ACT_QUICKGELU: launch_one<WM, WN, TM, TN, STAGES, 2, ZH_ACT_QUICKGELU, 2, SP>(p, batch, stream); return true;
      case 16 + ZH_ACT_RELU: launch_one<WM, WN, TM, TN, STAGES, 2, ZH_ACT_RELU, 2, SP>(p, batch, stream); return true;
      case 16 + ZH_ACT_GELU_ERF: launch_one<WM, WN, TM, TN, STAGES, 2, ZH_ACT_GELU_ERF, 2, SP>(p, batch, stream); return true;
      default: break;
    }
  }
  return false;
}

// a ring plan's launch from one mode's table (SP: 1 = two-plane weights, 2 = one plane)
template <const auto& ROWS, int SP>
static int launch_x3_plan(const GemmPlan& plan, const GemmArgs& p, int batch, int out_kind, hipStream_t stream) {
  return gemm_launch_plan<ROWS>(plan, [&](auto row) {
    constexpr GemmTile t = decltype(row)::t;
    return launch_x3<t.wm, t.wn, t.tm, t.tn, t.stages, decltype(row)::vec, SP>(p, batch, out_kind, stream);
  }, std::make_index_sequence<std::size(ROWS)>{});
}

extern "C" int zh_gemm_f16x3(const void* A, long lda, long strideA, long planeA, const void* W, long ldw, long strideW, long planeW,
                             void* C, long ldc, long strideC, long planeC, int out_kind, float out_scale,
                             const float* bias, const float* residual, long ldr, long strideR, int res_rows,
                             const void* pos_y, const void* pos_x, long ld_pos, int pos_h, int pos_w, int pos_f16,
                             int act, int M, int N, int K, int batch, int flags, hipStream_t stream) {
  // planeW == 0: W has no lo plane — every packed value is an fp16 number (the released CLIP weights after the reference's
  // convert_weights) — and the kernel skips the zero product (SPLIT = 2 in gemm_kernel.h: bit-identical results, 2/3 of the MFMAs)
  const bool x2 = planeW == 0;
  GemmArgs p;
  GemmProblem q;
  GemmPlan plan;
  int rc = gemm_prepare("zh_gemm_f16x3", x2 ? GEMM_X2 : GEMM_X3, A, lda, strideA, planeA, W, ldw, strideW, planeW, C, ldc, strideC, planeC, out_kind, out_scale,
                        bias, residual, ldr, strideR, res_rows, pos_y, pos_x, ld_pos, pos_h, pos_w, pos_f16, act, M, N, K, batch, flags, &p, &q);
  if (rc != ZH_OK) return rc;
  ZH_CHECK_ARG(planeA != 0, "zh_gemm_f16x3: A must be a split pair (plane offset of the lo half)");
  ZH_CHECK_ARG(out_kind >= 0 && out_kind <= 2, "zh_gemm_f16x3: out_kind %d not in {0 f32, 1 f16, 2 split pair}", out_kind);
  ZH_CHECK_ARG(out_kind != 2 || (planeC != 0 && planeC % 4 == 0), "zh_gemm_f16x3: split output needs planeC (multiple of 4)");
  // residual[m % res_rows] is added in fp32 after the activation; for fp16 / split-pair outputs (a row-periodic additive table:
  // the decoder's query_pos terms) that is BEFORE the one rounding, and only without an activation
  ZH_CHECK_ARG(!residual || out_kind == 0 || act == ZH_ACT_NONE, "zh_gemm_f16x3: a residual of an fp16 / split output goes with no activation");
  ZH_CHECK_ARG(out_scale > 0.0f, "zh_gemm_f16x3: out_scale must be positive");
  if ((rc = gemm_plan_x3(q, gemm_dev_overrides(), &plan, gemm_inflight())) != ZH_OK) return rc;
  if (plan.peel_rows)
    return gemm_tail_peel(plan.peel_rows, M, A, lda, C, ldc, out_kind == 0 ? 4 : 2, residual, ldr, 4, res_rows,
                          [&](const void* a, void* c, const void* r, int rows, int m) {
                            return zh_gemm_f16x3(a, lda, strideA, planeA, W, ldw, strideW, planeW, c, ldc, strideC, planeC, out_kind, out_scale, bias,
                                                 (const float*)r, ldr, strideR, rows, pos_y, pos_x, ld_pos, pos_h, pos_w, pos_f16, act, m, N, K, 1, flags, stream);
                          });
  int ok = 1;
  if (plan.family == GEMM_SKINNY) {
    if (x2) launch_skinny<1>(p, batch, out_kind, stream);
    else launch_skinny<2>(p, batch, out_kind, stream);
  } else
    ok = x2 ? launch_x3_plan<GEMM_TILES_X2, 2>(plan, p, batch, out_kind, stream) : launch_x3_plan<GEMM_TILES_X3, 1>(plan, p, batch, out_kind, stream);
  ZH_CHECK_ARG(ok >= 0, "zh_gemm_f16x3: the plan's tile code %d has no table row", plan.code);
  ZH_CHECK_ARG(ok, "zh_gemm_f16x3: (out_kind=%d, act=%d) is not an instantiated epilogue", out_kind, act);
  ZH_CHECK_LAUNCH("zh_gemm_f16x3");
  return ZH_OK;
}
