// Pillow's 8-bit resampler arithmetic (src/libImaging/Resample.c), shared by preprocess.hip and synth.hip: ONE statement of the
// coefficient maths.  Every file that includes this is compiled with -ffp-contract=off (zutis_amd/build.py EXTRA_FLAGS).
#pragma once
#include "common.h"

// taps per output pixel are capped at ZH_RCN_KMAX: 96 * 152 * 4 + 768 bytes of LDS < 64 KiB; FILTER is ZH_FILTER_BILINEAR / ZH_FILTER_BICUBIC
#define RCN_PRECISION_BITS 22

// Pillow's filter functions (Resample.c: bilinear_filter, bicubic_filter) and their supports
template <int FILTER>
__device__ __forceinline__ double rcn_filter(double x) {
  if (x < 0.0) x = -x;
  if (FILTER == ZH_FILTER_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
  const double a = -0.5;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

template <int FILTER>
__host__ __device__ __forceinline__ int rcn_ksize(int in_size, int out_size) {
  double fs = (double)in_size / (double)out_size;
  if (fs < 1.0) fs = 1.0;
  return (int)ceil((FILTER == ZH_FILTER_BILINEAR ? 1.0 : 2.0) * fs) * 2 + 1;
}

// precompute_coeffs + normalize_coeffs_8bpc for ONE output index xx: taps K[0 .. count) (stride `stride` ints), first source index xmin
template <int FILTER>
__device__ void rcn_coeffs(int in_size, int out_size, int xx, int* K, int stride, int& xmin_out, int& count_out) {
  const double scale = (double)in_size / (double)out_size;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = (FILTER == ZH_FILTER_BILINEAR ? 1.0 : 2.0) * fs, ss = 1.0 / fs;
  const double center = (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += rcn_filter<FILTER>((x + xmin - center + 0.5) * ss);
  for (int x = 0; x < xmax; ++x) {
    double k = rcn_filter<FILTER>((x + xmin - center + 0.5) * ss);
    if (ww != 0.0) k /= ww;
    K[x * stride] = k < 0.0 ? (int)(-0.5 + k * (double)(1 << RCN_PRECISION_BITS)) : (int)(0.5 + k * (double)(1 << RCN_PRECISION_BITS));
  }
  xmin_out = xmin;
  count_out = xmax;
}

__device__ __forceinline__ int rcn_clip8(int s) {
  s >>= RCN_PRECISION_BITS;                         // arithmetic shift, as Pillow's clip8
  return s < 0 ? 0 : (s > 255 ? 255 : s);
}

// ---- the two-pass tile body, shared by every kernel that resamples ------------------------------------------------------------
#define RCN_TX 64       // output columns per workgroup (= lanes)
#define RCN_WAVES 4
#define RCN_RY 8        // output rows per wave
#define RCN_TY (RCN_WAVES * RCN_RY)

// One workgroup (RCN_TX * RCN_WAVES threads), one RCN_TY x RCN_TX tile of the nw x nh resize of src [h, w, 3] as BYTES: the lane's column
// sx and the wave's RCN_RY rows sy_base + wave * RCN_RY + r.  RCN_TX threads compute the columns' coefficient sets, RCN_TY the rows', into
// LDS as int32 ([tap][column] / [row][tap]); the wave then streams over the source rows its rows tap: per source row the lane forms the
// horizontal pass's u8 pixel from global memory and adds it, times the row's coefficient, to the accumulators of those of its rows whose
// window holds that source row — the u8 intermediate never leaves registers.  A column outside [0, nw), a row outside [0, nh) or at or
// beyond tile row n_rows has no taps: its result is not meaningful and nothing is read for it.  Contains a __syncthreads(): every thread
// of the workgroup calls it.  lds: (RCN_TX + RCN_TY) * kmax + 2 * (RCN_TX + RCN_TY) ints.
template <int FILTER>
__device__ __forceinline__ void rcn_tile_u8(const unsigned char* __restrict__ src, int w, int h, int nw, int nh, int sx, int sy_base,
                                            int n_rows, int kmax, int* lds, int out[RCN_RY][3]) {
  int* Kx = lds;                                   // [kmax][RCN_TX]
  int* Ky = Kx + kmax * RCN_TX;                     // [RCN_TY][kmax]
  int* x_min = Ky + RCN_TY * kmax;
  int* x_cnt = x_min + RCN_TX;
  int* y_min = x_cnt + RCN_TX;
  int* y_cnt = y_min + RCN_TY;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < RCN_TX) {
    int mn = 0, cnt = 0;
    if (sx >= 0 && sx < nw) rcn_coeffs<FILTER>(w, nw, sx, Kx + tid, RCN_TX, mn, cnt);
    x_min[tid] = mn;
    x_cnt[tid] = cnt;
  } else if (tid < RCN_TX + RCN_TY) {
    const int r = tid - RCN_TX, sy = sy_base + r;
    int mn = 0, cnt = 0;
    if (r < n_rows && sy >= 0 && sy < nh) rcn_coeffs<FILTER>(h, nh, sy, Ky + r * kmax, 1, mn, cnt);
    y_min[r] = mn;
    y_cnt[r] = cnt;
  }
  __syncthreads();
  const int xmin = x_min[lane], xcnt = x_cnt[lane];
  int ymin[RCN_RY], ycnt[RCN_RY];
  int ylo = 0x7fffffff, yhi = 0;
#pragma unroll
  for (int r = 0; r < RCN_RY; ++r) {
    ymin[r] = y_min[wave * RCN_RY + r];
    ycnt[r] = y_cnt[wave * RCN_RY + r];
    if (ycnt[r] > 0) {
      ylo = min(ylo, ymin[r]);
      yhi = max(yhi, ymin[r] + ycnt[r]);
    }
  }
  int acc[RCN_RY][3];
#pragma unroll
  for (int r = 0; r < RCN_RY; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 1 << (RCN_PRECISION_BITS - 1);
  const int* ky = Ky + wave * RCN_RY * kmax;
  for (int y = ylo; y < yhi; ++y) {                 // wave-uniform bounds; xmin + xcnt <= w and y < h by rcn_coeffs
    const unsigned char* p = src + ((size_t)y * w + xmin) * 3;
    int s0 = 1 << (RCN_PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < xcnt; ++t) {
      const int k = Kx[t * RCN_TX + lane];
      s0 += (int)p[3 * t] * k;
      s1 += (int)p[3 * t + 1] * k;
      s2 += (int)p[3 * t + 2] * k;
    }
    const int h0 = rcn_clip8(s0), h1 = rcn_clip8(s1), h2 = rcn_clip8(s2);
#pragma unroll
    for (int r = 0; r < RCN_RY; ++r) {
      const int t = y - ymin[r];
      if ((unsigned)t < (unsigned)ycnt[r]) {
        const int k = ky[r * kmax + t];
        acc[r][0] += h0 * k;
        acc[r][1] += h1 * k;
        acc[r][2] += h2 * k;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RCN_RY; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) out[r][c] = rcn_clip8(acc[r][c]);
}
