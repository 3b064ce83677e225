// Training criterion (criterion.py::Criterion, the loss of every Trainer.fit step, trainer.py:105-160) without its full-resolution
// tensors.  The reference upsamples the proposals / patch tokens to the GT resolution and runs BCE on repeat()-ed [Q, n, H*W] copies
// (criterion.py:77-150).  Here every full-resolution value is interpolated from the low-res planes on the fly (lin_weights, the ATen
// index / weight rule of resample.hip) and reduced at once:
//   * cost:  per (image, layer) the [n, Q] dice + BCE matrix from four blocked sums (sum p, sum g.p, sum (g ? A : B), sum g),
//            A = max(log p, -100), B = max(log(1 - p), -100) (torch's clamp).  Each pixel's BCE term is taken whole: the split
//            B + g.(A - B) adds -100 and +100 per saturated pixel (p == 1, g == 1) and the fp32 sums do not cancel.
//   * CE:    upsample(te . tok) = te . upsample(tok): the logits are a low-res GEMM; one kernel interpolates them per pixel,
//            forms the log-sum-exp and the NLL and reduces per block; a one-block kernel reduces the partials in a fixed order.
//   * grads: the full-resolution gradient of a matched pair / of the softmax goes straight through the adjoint of the bilinear
//            upsample, rows first (a full-res row into its w low-res columns) then columns; every low-res output is owned by one
//            thread and summed in a fixed order, so the gradients are bitwise reproducible (no float atomics).
#include "common.h"

// ---- adjoint window: the full-resolution indices d whose bilinear weights touch low-res index i (a superset; the caller
//      weighs each d with adj_weight, which is 0 outside the true support)
__device__ __forceinline__ void adj_window(int i, int n_in, int n_out, float scale, int& lo, int& hi) {
  if (n_in == n_out) { lo = hi = i; return; }
  const float inv = 1.f / scale;
  lo = max(0, (int)floorf(((float)i - 0.5f) * inv - 0.5f) - 2);
  hi = i >= n_in - 1 ? n_out - 1 : min(n_out - 1, (int)ceilf(((float)i + 1.5f) * inv - 0.5f) + 2);
}
__device__ __forceinline__ float adj_weight(int d, int i, int n_in, int n_out, float scale) {
  const LinW L = lin_weights(d, n_in, n_out, scale);
  return (L.i0 == i ? L.l0 : 0.f) + (L.i1 == i ? L.l1 : 0.f);
}
// bilinear sample of a [h, w] plane, the arithmetic of bilinear_nchw_kernel (resample.hip)
__device__ __forceinline__ float interp(const float* p, int w, const LinW& wy, const LinW& wx) {
  const float r0 = __fmaf_rn(p[wy.i0 * w + wx.i0], wx.l0, __fmul_rn(p[wy.i0 * w + wx.i1], wx.l1));
  const float r1 = __fmaf_rn(p[wy.i1 * w + wx.i0], wx.l0, __fmul_rn(p[wy.i1 * w + wx.i1], wx.l1));
  return __fmaf_rn(r0, wy.l0, __fmul_rn(r1, wy.l1));
}

// ================================================================================================================================
// Matching costs
// ================================================================================================================================
#define MC_QG 2      // queries per workgroup (the GT bits of a pixel are read once for all of them)
#define MC_MAXI 16   // instances per workgroup (blockIdx.z also walks instance groups of 16)
#define MC_BAND 48   // full-resolution rows per workgroup
#define MC_RV(NGM) (1 + 2 * (NGM))   // partial record per (b, l, q, band): [sum p, sum g.p [NGM], sum (g ? A : B) [NGM]]
#define MC_QV (1 + 2 * MC_MAXI)      // values per query of a workgroup's reduction: sum p, sum g.p [MC_MAXI], sum (g ? A : B) [MC_MAXI]
#define MC_NV (MC_QG * MC_QV + MC_MAXI)   // ... and sum g [MC_MAXI]

__global__ __launch_bounds__(256) void mask_cost_partial_kernel(const float* prop, const unsigned char* gt, const int* inst_off,
                                                                float* part, float* part_g, int* status, int L, int Q, int h, int w,
                                                                int H, int W, int NB, int NG, float sh, float sw) {
  extern __shared__ float mc_lds[];                  // [MC_QG][h*w] planes, then [4 waves][values] reduction
  const int band = blockIdx.x, qg = blockIdx.y;
  int z = blockIdx.z;
  const int ig = z % NG; z /= NG;
  const int l = z % L, b = z / L;
  const int n_b = inst_off[b + 1] - inst_off[b];
  if (ig > 0 && ig * MC_MAXI >= n_b) return;          // uniform per workgroup, before any barrier
  const int ni = min(MC_MAXI, n_b - ig * MC_MAXI);    // may be <= 0 for ig == 0 (sum p is still produced)
  const int q0 = qg * MC_QG, nq = min(MC_QG, Q - q0);
  const int hw = h * w;
  const long HW = (long)H * W;
  int bad = 0;
  for (int k = threadIdx.x; k < MC_QG * hw; k += 256) {
    const int j = k / hw;
    float v = 0.f;
    if (j < nq) {
      v = prop[(((long)b * L + l) * Q + q0 + j) * hw + (k - j * hw)];
      bad |= !(v >= 0.f && v <= 1.f);
    }
    mc_lds[k] = v;
  }
  if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(status, ZH_STATUS_RANGE);
  __syncthreads();
  const bool do_g = (l == 0 && qg == 0);
  float sp[MC_QG], spg[MC_QG][MC_MAXI], sab[MC_QG][MC_MAXI], sg[MC_MAXI];
#pragma unroll
  for (int j = 0; j < MC_QG; ++j) {
    sp[j] = 0.f;
#pragma unroll
    for (int i = 0; i < MC_MAXI; ++i) spg[j][i] = sab[j][i] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < MC_MAXI; ++i) sg[i] = 0.f;
  const unsigned char* g0 = gt + (long)(inst_off[b] + ig * MC_MAXI) * HW;
  const int y0 = band * MC_BAND, y1 = min(H, y0 + MC_BAND);
  int y = y0, x = threadIdx.x;
  while (x >= W) { x -= W; ++y; }
  for (; y < y1;) {
    const LinW wy = lin_weights(y, h, H, sh), wx = lin_weights(x, w, W, sw);
    const long pix = (long)y * W + x;
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < MC_MAXI; ++i)
      if (i < ni) m |= (g0[(long)i * HW + pix] != 0 ? 1u : 0u) << i;
#pragma unroll
    for (int j = 0; j < MC_QG; ++j) {
      const float p = interp(mc_lds + j * hw, w, wy, wx);
      const float A = fmaxf(__logf(p), -100.f), Bv = fmaxf(__logf(1.f - p), -100.f);
      sp[j] += p;
#pragma unroll
      for (int i = 0; i < MC_MAXI; ++i) {
        const bool on = (m >> i) & 1u;
        spg[j][i] += on ? p : 0.f;
        sab[j][i] += on ? A : Bv;
      }
    }
    if (do_g) {
#pragma unroll
      for (int i = 0; i < MC_MAXI; ++i) sg[i] += (float)((m >> i) & 1u);
    }
    x += 256;
    while (x >= W) { x -= W; ++y; }
  }
  // fixed-order block reduction: wave tree, then the 4 waves in order
  float* red = mc_lds + MC_QG * hw;
  const int NV = MC_NV;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < MC_QG; ++j) {
    const float a = wave_sum(sp[j]);
    if (lane == 0) red[wave * NV + j * MC_QV] = a;
#pragma unroll
    for (int i = 0; i < MC_MAXI; ++i) {
      const float e = wave_sum(spg[j][i]), f = wave_sum(sab[j][i]);
      if (lane == 0) { red[wave * NV + j * MC_QV + 1 + i] = e; red[wave * NV + j * MC_QV + 1 + MC_MAXI + i] = f; }
    }
  }
  if (do_g) {
#pragma unroll
    for (int i = 0; i < MC_MAXI; ++i) {
      const float e = wave_sum(sg[i]);
      if (lane == 0) red[wave * NV + MC_QG * MC_QV + i] = e;
    }
  }
  __syncthreads();
  const int NGM = NG * MC_MAXI, RV = MC_RV(NGM);
  for (int v = threadIdx.x; v < NV; v += 256) {
    const float s = ((red[v] + red[NV + v]) + red[2 * NV + v]) + red[3 * NV + v];
    if (v < MC_QG * MC_QV) {
      const int j = v / MC_QV, r = v - j * MC_QV;
      if (j >= nq) continue;
      float* rec = part + ((((long)b * L + l) * Q + q0 + j) * NB + band) * RV;
      if (r < 1) {
        if (ig == 0) rec[0] = s;
      } else {
        const int i = (r - 1) % MC_MAXI, which = (r - 1) / MC_MAXI;
        if (i < ni) rec[1 + which * NGM + ig * MC_MAXI + i] = s;
      }
    } else if (do_g) {
      const int i = v - MC_QG * MC_QV;
      if (i < ni) part_g[((long)b * NB + band) * NGM + ig * MC_MAXI + i] = s;
    }
  }
}

// ---- band partials -> cost[b] [L, n_b, Q] (at L * inst_off[b] * Q), the sums the gradient needs, the per-image skip flags
__global__ __launch_bounds__(256) void mask_cost_final_kernel(const float* part, const float* part_g, const int* inst_off, float* costs,
                                                              float* stat_p, float* stat_pg, float* stat_g, int* skip, int B, int L, int Q,
                                                              int NB, int NG, long HW, float wd, float wb) {
  const int NGM = NG * MC_MAXI, RV = MC_RV(NGM);
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const int n_tot = inst_off[B];
  if (t < B) {
    const int b = (int)t;
    float tot = 0.f;
    for (int i = 0; i < inst_off[b + 1] - inst_off[b]; ++i)
      for (int k = 0; k < NB; ++k) tot += part_g[((long)b * NB + k) * NGM + i];
    skip[b] = tot == 0.f ? 1 : 0;
  }
  if (t < n_tot) {                                     // sum g per instance
    int b = 0;
    while (inst_off[b + 1] <= t) ++b;
    const int i = (int)t - inst_off[b];
    float s = 0.f;
    for (int k = 0; k < NB; ++k) s += part_g[((long)b * NB + k) * NGM + i];
    stat_g[t] = s;
  }
  if (t < (long)B * L * Q) {                           // sum p per (b, l, q)
    float s = 0.f;
    for (int k = 0; k < NB; ++k) s += part[(t * NB + k) * RV];
    stat_p[t] = s;
  }
  if (t >= (long)L * n_tot * Q) return;
  // t = (L * inst_off[b] + l * n_b + i) * Q + q
  const int q = (int)(t % Q);
  const long r = t / Q;
  int b = 0;
  while ((long)L * inst_off[b + 1] <= r) ++b;
  const int n_b = inst_off[b + 1] - inst_off[b];
  const int rr = (int)(r - (long)L * inst_off[b]);
  const int l = rr / n_b, i = rr - l * n_b;
  float Sp = 0.f, Spg = 0.f, Sab = 0.f, Sg = 0.f;
  const float* rec = part + (((long)b * L + l) * Q + q) * NB * RV;
  for (int k = 0; k < NB; ++k) {
    Sp += rec[k * RV];
    Spg += rec[k * RV + 1 + i];
    Sab += rec[k * RV + 1 + NGM + i];
    Sg += part_g[((long)b * NB + k) * NGM + i];
  }
  const float dice = 1.f - (2.f * Spg + 1.f) / (Sp + Sg + 1.f);
  const float bce = -Sab / (float)HW;
  costs[t] = wd * dice + wb * bce;
  stat_pg[t] = Spg;
}

extern "C" size_t zh_mask_match_cost_workspace_size(int B, int L, int Q, int H, int n_max) {
  const long NB = zh_cdiv(H, MC_BAND), NGM = (long)zh_cdiv(n_max > 0 ? n_max : 1, MC_MAXI) * MC_MAXI;
  return (size_t)((long)B * L * Q * NB * MC_RV(NGM) + (long)B * NB * NGM) * sizeof(float);
}

extern "C" int zh_mask_match_cost(const float* proposals, const unsigned char* gt_u8, const int* inst_off, float* costs, float* stat_p,
                                  float* stat_pg, float* stat_g, int* skip, int* status, int B, int L, int Q, int h, int w, int H, int W,
                                  int n_max, float weight_dice, float weight_bce, float scale_h, float scale_w, void* workspace,
                                  size_t workspace_bytes, hipStream_t stream) {
  ZH_CHECK_ARG(proposals && inst_off && costs && stat_p && stat_pg && stat_g && skip && status && workspace, "zh_mask_match_cost: null pointer");
  ZH_CHECK_ARG(n_max == 0 || gt_u8, "zh_mask_match_cost: null gt_u8");
  ZH_CHECK_ARG(B > 0 && L > 0 && Q > 0 && h > 0 && w > 0 && H > 0 && W > 0 && n_max >= 0, "zh_mask_match_cost: bad shape");
  const size_t lds = (size_t)(MC_QG * h * w + 4 * MC_NV) * sizeof(float);
  ZH_CHECK_ARG(lds <= 65536, "zh_mask_match_cost: proposal plane %dx%d too large for LDS", h, w);
  ZH_CHECK_ARG(workspace_bytes >= zh_mask_match_cost_workspace_size(B, L, Q, H, n_max), "zh_mask_match_cost: workspace too small");
  const int NB = zh_cdiv(H, MC_BAND), NG = zh_cdiv(n_max > 0 ? n_max : 1, MC_MAXI);
  float* part = (float*)workspace;
  float* part_g = part + (long)B * L * Q * NB * MC_RV(NG * MC_MAXI);
  hipLaunchKernelGGL(mask_cost_partial_kernel, dim3(NB, zh_cdiv(Q, MC_QG), B * L * NG), dim3(256), lds, stream, proposals, gt_u8,
                     inst_off, part, part_g, status, L, Q, h, w, H, W, NB, NG, scale_h, scale_w);
  ZH_CHECK_LAUNCH("zh_mask_match_cost");
  // enough threads for L * n_tot * Q costs (n_tot <= B * n_max), B * L * Q sums and the instances
  const long work = (long)Q * L * ((long)B * n_max > B ? (long)B * n_max : B);
  hipLaunchKernelGGL(mask_cost_final_kernel, dim3(zh_cdiv(work, 256)), dim3(256), 0, stream, part, part_g, inst_off, costs, stat_p,
                     stat_pg, stat_g, skip, B, L, Q, NB, NG, (long)H * W, weight_dice, weight_bce);
  ZH_CHECK_LAUNCH("zh_mask_match_cost");
  return ZH_OK;
}

// ================================================================================================================================
// Adjoint-upsample gradients
// ================================================================================================================================
#define AD_ROWS 4    // full-resolution rows per step of the mask-gradient workgroup

// One workgroup per (matched pair, low-res row iy): the full-resolution rows y that touch iy are formed AD_ROWS at a time in LDS,
// reduced along x into the w low-res columns, then weighted along y into iy.
__global__ __launch_bounds__(256) void mask_grad_kernel(const float* prop, const unsigned char* gt, const int* inst_off, const int* pairs,
                                                        const float* stat_p, const float* stat_pg, const float* stat_g, const float* grad_out,
                                                        float* grad, int L, int Q, int h, int w, int H, int W, float wd, float wb,
                                                        float loss_scale, float sh, float sw) {
  extern __shared__ float ad_lds[];                  // plane [h*w] | G [AD_ROWS][W] | R [AD_ROWS][w] | acc [w]
  const int iy = blockIdx.x, k = blockIdx.y;
  const int b = pairs[4 * k], l = pairs[4 * k + 1], q = pairs[4 * k + 2], i = pairs[4 * k + 3];
  const int hw = h * w;
  const long HW = (long)H * W;
  float* plane = ad_lds;
  float* G = plane + hw;
  float* R = G + AD_ROWS * W;
  float* acc = R + AD_ROWS * w;
  const long pl = ((long)b * L + l) * Q + q;
  for (int t = threadIdx.x; t < hw; t += 256) plane[t] = prop[pl * hw + t];
  for (int t = threadIdx.x; t < w; t += 256) acc[t] = 0.f;
  const int n_b = inst_off[b + 1] - inst_off[b];
  const long ci = ((long)L * inst_off[b] + (long)l * n_b + i) * Q + q;
  const float D = stat_p[pl] + stat_g[inst_off[b] + i] + 1.f, N = 2.f * stat_pg[ci] + 1.f;
  const float s = grad_out[0] * loss_scale;
  const float cd = s * wd / (D * D), cb = s * wb / (float)HW;
  const unsigned char* g = gt + (long)(inst_off[b] + i) * HW;
  int ylo, yhi;
  adj_window(iy, h, H, sh, ylo, yhi);
  __syncthreads();
  for (int yb = ylo; yb <= yhi; yb += AD_ROWS) {
    const int nr = min(AD_ROWS, yhi - yb + 1);
    for (int t = threadIdx.x; t < nr * W; t += 256) {
      const int r = t / W, x = t - r * W, y = yb + r;
      const float p = interp(plane, w, lin_weights(y, h, H, sh), lin_weights(x, w, W, sw));
      const float gv = g[(long)y * W + x] != 0 ? 1.f : 0.f;
      G[r * W + x] = cd * (N - 2.f * gv * D) + cb * (p - gv) / fmaxf(p * (1.f - p), 1e-12f);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nr * w; t += 256) {
      const int r = t / w, ix = t - r * w;
      int xlo, xhi;
      adj_window(ix, w, W, sw, xlo, xhi);
      float a = 0.f;
      for (int x = xlo; x <= xhi; ++x) a += adj_weight(x, ix, w, W, sw) * G[r * W + x];
      R[r * w + ix] = a;
    }
    __syncthreads();
    for (int ix = threadIdx.x; ix < w; ix += 256) {
      float a = acc[ix];
      for (int r = 0; r < nr; ++r) a += adj_weight(yb + r, iy, h, H, sh) * R[r * w + ix];
      acc[ix] = a;
    }
    __syncthreads();
  }
  for (int ix = threadIdx.x; ix < w; ix += 256) grad[pl * hw + (long)iy * w + ix] = acc[ix];
}

extern "C" int zh_mask_match_grad(const float* proposals, const unsigned char* gt_u8, const int* inst_off, const int* pairs, int n_pairs,
                                  const float* stat_p, const float* stat_pg, const float* stat_g, const float* grad_out,
                                  float* grad_proposals, int B, int L, int Q, int h, int w, int H, int W, float weight_dice,
                                  float weight_bce, float loss_scale, float scale_h, float scale_w, hipStream_t stream) {
  ZH_CHECK_ARG(proposals && inst_off && stat_p && stat_pg && stat_g && grad_out && grad_proposals, "zh_mask_match_grad: null pointer");
  ZH_CHECK_ARG(n_pairs == 0 || (pairs && gt_u8), "zh_mask_match_grad: null pairs / gt_u8");
  ZH_CHECK_ARG(B > 0 && L > 0 && Q > 0 && h > 0 && w > 0 && H > 0 && W > 0 && n_pairs >= 0, "zh_mask_match_grad: bad shape");
  const size_t lds = (size_t)(h * w + AD_ROWS * W + AD_ROWS * w + w) * sizeof(float);
  ZH_CHECK_ARG(lds <= 65536, "zh_mask_match_grad: %dx%d -> %dx%d too large for LDS", h, w, H, W);
  if (hipMemsetAsync(grad_proposals, 0, (size_t)B * L * Q * h * w * sizeof(float), stream) != hipSuccess) {
    zh_set_error("zh_mask_match_grad: memset failed");
    return ZH_ERR_HIP;
  }
  if (n_pairs == 0) return ZH_OK;
  hipLaunchKernelGGL(mask_grad_kernel, dim3(h, n_pairs), dim3(256), lds, stream, proposals, gt_u8, inst_off, pairs, stat_p, stat_pg, stat_g,
                     grad_out, grad_proposals, L, Q, h, w, H, W, weight_dice, weight_bce, loss_scale, scale_h, scale_w);
  ZH_CHECK_LAUNCH("zh_mask_match_grad");
  return ZH_OK;
}

// ================================================================================================================================
// Cross-entropy on the upsampled low-res logits
// ================================================================================================================================
// One thread per full-resolution pixel: online log-sum-exp over the classes (one exp per class), NLL of the label; ignored and
// out-of-range labels contribute nothing (an out-of-range one sets ZH_STATUS_LABEL and is never used as an index).
__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* lo, const long long* labels, float* lse, float* part, int* status,
                                                     int n_cat, int h, int w, int H, int W, long long ignore, float sh, float sw) {
  __shared__ float red[2][4];
  const long HW = (long)H * W;
  const int b = blockIdx.y;
  const long pix = (long)blockIdx.x * 256 + threadIdx.x;
  float nll = 0.f, cnt = 0.f;
  int bad = 0;
  if (pix < HW) {
    const long long lab = labels[(long)b * HW + pix];
    const bool valid = lab != ignore && lab >= 0 && lab < n_cat;
    bad = lab != ignore && !valid;
    const int y = (int)(pix / W), x = (int)(pix - (long)y * W);
    const LinW wy = lin_weights(y, h, H, sh), wx = lin_weights(x, w, W, sw);
    const float* p = lo + (long)b * n_cat * h * w;
    float m = -INFINITY, s = 0.f, vl = 0.f;
    for (int c = 0; c < n_cat; ++c) {
      const float v = interp(p + (long)c * h * w, w, wy, wx);
      const float e = __expf(-fabsf(v - m));
      s = v > m ? __fmaf_rn(s, e, 1.f) : s + e;
      m = fmaxf(m, v);
      vl = (valid && c == (int)lab) ? v : vl;
    }
    const float ls = m + __logf(s);
    lse[(long)b * HW + pix] = ls;
    if (valid) { nll = ls - vl; cnt = 1.f; }
  }
  if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(status, ZH_STATUS_LABEL);
  nll = wave_sum(nll);
  cnt = wave_sum(cnt);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][wave] = nll; red[1][wave] = cnt; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const long blk = (long)b * gridDim.x + blockIdx.x;
    part[2 * blk + threadIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
  }
}

// partials -> out[0] = sum NLL / count (NaN when every pixel is ignored, as torch), out[1] = count.  Fixed order: per thread ascending
// partials in double, then a fixed tree.
__global__ __launch_bounds__(256) void ce_final_kernel(const float* part, long n_part, float* out) {
  __shared__ double red[2][256];
  double a = 0.0, c = 0.0;
  for (long k = threadIdx.x; k < n_part; k += 256) { a += (double)part[2 * k]; c += (double)part[2 * k + 1]; }
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)(red[0][0] / red[1][0]);
    out[1] = (float)red[1][0];
  }
}

extern "C" size_t zh_upsample_ce_workspace_size(int B, int H, int W) {
  return (size_t)B * zh_cdiv((long)H * W, 256) * 2 * sizeof(float);
}

extern "C" int zh_upsample_ce_fwd(const float* logits_lo, const long long* labels, float* lse, float* out, int* status, int B, int n_cat,
                                  int h, int w, int H, int W, int ignore_index, float scale_h, float scale_w, void* workspace,
                                  size_t workspace_bytes, hipStream_t stream) {
  ZH_CHECK_ARG(logits_lo && labels && lse && out && status && workspace, "zh_upsample_ce_fwd: null pointer");
  ZH_CHECK_ARG(B > 0 && n_cat > 0 && h > 0 && w > 0 && H > 0 && W > 0, "zh_upsample_ce_fwd: bad shape");
  ZH_CHECK_ARG(workspace_bytes >= zh_upsample_ce_workspace_size(B, H, W), "zh_upsample_ce_fwd: workspace too small");
  const int nx = zh_cdiv((long)H * W, 256);
  float* part = (float*)workspace;
  hipLaunchKernelGGL(ce_fwd_kernel, dim3(nx, B), dim3(256), 0, stream, logits_lo, labels, lse, part, status, n_cat, h, w, H, W,
                     (long long)ignore_index, scale_h, scale_w);
  ZH_CHECK_LAUNCH("zh_upsample_ce_fwd");
  hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(256), 0, stream, part, (long)B * nx, out);
  ZH_CHECK_LAUNCH("zh_upsample_ce_fwd");
  return ZH_OK;
}

#define CE_CC 16     // classes per workgroup of the CE backward

// One workgroup per (image, class chunk, low-res row iy): each full-resolution row y that touches iy is formed for CE_CC classes
// in LDS (softmax - onehot, scaled by grad / count; 0 on ignored pixels), reduced along x into the w columns and weighted into iy.
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* lo, const long long* labels, const float* lse, const float* ce_out,
                                                     const float* grad_out, float* grad, int n_cat, int h, int w, int H, int W,
                                                     long long ignore, float sh, float sw) {
  extern __shared__ float cb_lds[];                  // G [CE_CC][W] | acc [CE_CC][w]
  const int iy = blockIdx.x, c0 = blockIdx.y * CE_CC, b = blockIdx.z;
  const int nc = min(CE_CC, n_cat - c0);
  const long HW = (long)H * W;
  float* G = cb_lds;
  float* acc = G + CE_CC * W;
  for (int t = threadIdx.x; t < CE_CC * w; t += 256) acc[t] = 0.f;
  const float s = grad_out[0] / ce_out[1];
  const float* p = lo + ((long)b * n_cat + c0) * h * w;
  int ylo, yhi;
  adj_window(iy, h, H, sh, ylo, yhi);
  for (int y = ylo; y <= yhi; ++y) {
    const float wyv = adj_weight(y, iy, h, H, sh);
    if (wyv == 0.f) continue;                        // uniform
    __syncthreads();
    const LinW wy = lin_weights(y, h, H, sh);
    for (int x = threadIdx.x; x < W; x += 256) {
      const long long lab = labels[(long)b * HW + (long)y * W + x];
      const bool valid = lab != ignore && lab >= 0 && lab < n_cat;
      const float ls = lse[(long)b * HW + (long)y * W + x];
      const LinW wx = lin_weights(x, w, W, sw);
      for (int c = 0; c < nc; ++c) {
        const float v = interp(p + (long)c * h * w, w, wy, wx);
        const float e = __expf(v - ls) - ((long long)(c0 + c) == lab ? 1.f : 0.f);
        G[c * W + x] = valid ? e * s : 0.f;
      }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nc * w; t += 256) {
      const int c = t / w, ix = t - c * w;
      int xlo, xhi;
      adj_window(ix, w, W, sw, xlo, xhi);
      float a = 0.f;
      for (int x = xlo; x <= xhi; ++x) a += adj_weight(x, ix, w, W, sw) * G[c * W + x];
      acc[t] += wyv * a;
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < nc * w; t += 256) {
    const int c = t / w, ix = t - c * w;
    grad[(((long)b * n_cat + c0 + c) * h + iy) * w + ix] = acc[t];
  }
}

extern "C" int zh_upsample_ce_bwd(const float* logits_lo, const long long* labels, const float* lse, const float* ce_out,
                                  const float* grad_out, float* grad_logits_lo, int B, int n_cat, int h, int w, int H, int W,
                                  int ignore_index, float scale_h, float scale_w, hipStream_t stream) {
  ZH_CHECK_ARG(logits_lo && labels && lse && ce_out && grad_out && grad_logits_lo, "zh_upsample_ce_bwd: null pointer");
  ZH_CHECK_ARG(B > 0 && n_cat > 0 && h > 0 && w > 0 && H > 0 && W > 0, "zh_upsample_ce_bwd: bad shape");
  const size_t lds = (size_t)(CE_CC * W + CE_CC * w) * sizeof(float);
  ZH_CHECK_ARG(lds <= 65536, "zh_upsample_ce_bwd: W = %d too large for LDS", W);
  hipLaunchKernelGGL(ce_bwd_kernel, dim3(h, zh_cdiv(n_cat, CE_CC), B), dim3(256), lds, stream, logits_lo, labels, lse, ce_out, grad_out,
                     grad_logits_lo, n_cat, h, w, H, W, (long long)ignore_index, scale_h, scale_w);
  ZH_CHECK_LAUNCH("zh_upsample_ce_bwd");
  return ZH_OK;
}

// ================================================================================================================================
// Strided fp32 GEMM for the low-res text contraction and its transpose:  C[t](m, n) = sum_k A[t](m, k) * B[t](n, k)
// 64 x 64 tiles, 16-deep k slices, 4 x 4 outputs per thread; k ascends in one fp32 chain per output (fixed order).
// ================================================================================================================================
__global__ __launch_bounds__(256) void gemm_f32_strided_kernel(const float* A, long sAb, long sAm, long sAk, const float* Bm, long sBb,
                                                               long sBn, long sBk, float* C, long sCb, long sCm, long sCn, int M, int N,
                                                               int K) {
  __shared__ float As[16][64 + 4], Bs[16][64 + 4];
  const int t = blockIdx.z;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  A += t * sAb;
  Bm += t * sBb;
  C += t * sCb;
  const int tm = (threadIdx.x >> 4) * 4, tn = (threadIdx.x & 15) * 4;
  float acc[4][4] = {};
  for (int k0 = 0; k0 < K; k0 += 16) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = threadIdx.x + 256 * j;
      // k-contiguous operands: consecutive threads walk k; otherwise consecutive threads walk m / n
      const int am = sAk == 1 ? e >> 4 : e & 63, ak = sAk == 1 ? e & 15 : e >> 6;
      const int bn = sBk == 1 ? e >> 4 : e & 63, bk = sBk == 1 ? e & 15 : e >> 6;
      As[ak][am] = (m0 + am < M && k0 + ak < K) ? A[(long)(m0 + am) * sAm + (long)(k0 + ak) * sAk] : 0.f;
      Bs[bk][bn] = (n0 + bn < N && k0 + bk < K) ? Bm[(long)(n0 + bn) * sBn + (long)(k0 + bk) * sBk] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      float a[4], bv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) { a[r] = As[kk][tm + r]; bv[r] = Bs[kk][tn + r]; }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = __fmaf_rn(a[r], bv[c], acc[r][c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (m0 + tm + r < M && n0 + tn + c < N) C[(long)(m0 + tm + r) * sCm + (long)(n0 + tn + c) * sCn] = acc[r][c];
}

extern "C" int zh_gemm_f32_strided(const float* A, long sAb, long sAm, long sAk, const float* Bm, long sBb, long sBn, long sBk, float* C,
                                   long sCb, long sCm, long sCn, int batch, int M, int N, int K, hipStream_t stream) {
  ZH_CHECK_ARG(A && Bm && C, "zh_gemm_f32_strided: null pointer");
  ZH_CHECK_ARG(batch > 0 && M > 0 && N > 0 && K > 0 && batch <= 65535 && M <= 65535 * 64, "zh_gemm_f32_strided: bad shape");
  hipLaunchKernelGGL(gemm_f32_strided_kernel, dim3(zh_cdiv(N, 64), zh_cdiv(M, 64), batch), dim3(256), 0, stream, A, sAb, sAm, sAk, Bm, sBb,
                     sBn, sBk, C, sCb, sCm, sCn, M, N, K);
  ZH_CHECK_LAUNCH("zh_gemm_f32_strided");
  return ZH_OK;
}
