// CLIP's image pre-processing on the device — torchvision Resize(n_px, BICUBIC) + CenterCrop(n_px) + ToTensor + Normalize,
// utils/extract_image_embeddings.py:97-103 — for a ragged batch of decoded RGB images, bit-identical to Pillow + NumPy on the host.
//
// Pillow resamples 8-bit images in integers: per axis a set of 22-bit fixed-point coefficients (computed in double, normalised
// by their sequential sum, rounded half away from zero), a horizontal pass to a u8 intermediate, then a vertical pass
// (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc).
// This file restates exactly that and is compiled with -ffp-contract=off, so the coefficient arithmetic is the host's IEEE
// double sequence.  The normalisation is a function of (channel, byte): a 3 x 256 fp32 table filled by the host's own NumPy
// expression, looked up here — no floating-point pixel arithmetic on the device at all.
//
// MI355X design.  One launch per batch; one workgroup (4 waves) per (image, tile of 32 output rows x 64 output columns).
//   1. 64 threads compute the tile's column coefficient sets, 32 its row sets, into LDS as int32 ([tap][column] / [row][tap]).
//   2. A lane owns one output column (all three channels), a wave 8 output rows.  The wave streams over the source rows its
//      8 rows tap: per source row the lane forms the horizontal pass's u8 pixel from global memory (the source of a typical
//      photograph is ~0.5 MB and is read by the ~60 workgroups of its image out of L2) and adds it, times the row's
//      coefficient, to the accumulators of those of its 8 output rows whose window holds that source row.  The u8
//      intermediate never leaves registers; only the crop's columns and the rows its taps touch are ever computed.
//   3. Clamp, table lookup, one fp32 store per plane with lanes along x.
// LDS = 96 * kmax ints for the coefficient sets, sized per launch by the caller's `kmax` (the largest tap count of the batch:
// 7 for a 500 x 375 photograph at 336, 149 for an 8192-pixel shorter side at 224), so the common case keeps full occupancy.
// Bound: bytes — sum 3 w h read + 12 n_px^2 written per image.
//
// The same kernel, instantiated on the filter and with a rectangular out_h x out_w output, is MaskDataset's transform
// (datasets/index_dataset.py:405-411: TF.resize(image, 512, BILINEAR) + to_tensor + normalize) for a batch whose images all
// resize to ONE shape: Pillow's BILINEAR is the same two-pass code with the triangle filter of support 1 (3 taps per axis when
// up-scaling).  There a 375 x 500 photograph becomes 512 x 682: 0.56 MB read, 4.2 MB written — store-bound, every wave's store
// is 64 consecutive floats of one plane row, and the 32 x 64 tile gives 11 x 16 workgroups per image (1408 at eight images, 5.5 per
// CU) with 3 % of the lanes idle (the last tile column).
#include "common.h"

#define RCN_TX 64       // output columns per workgroup (= lanes)
#define RCN_WAVES 4
#define RCN_RY 8        // output rows per wave
#define RCN_TY (RCN_WAVES * RCN_RY)
#define RCN_KMAX 152    // include/zutis_hip.h ZH_RCN_KMAX: 96 * 152 * 4 + 768 bytes of LDS < 64 KiB
#define RCN_PRECISION_BITS 22

#define RCN_BILINEAR 2  // include/zutis_hip.h ZH_FILTER_BILINEAR / ZH_FILTER_BICUBIC
#define RCN_BICUBIC 3

// Pillow's filter functions (Resample.c: bilinear_filter, bicubic_filter) and their supports
template <int FILTER>
__device__ __forceinline__ double rcn_filter(double x) {
  if (x < 0.0) x = -x;
  if (FILTER == RCN_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
  const double a = -0.5;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

template <int FILTER>
__host__ __device__ __forceinline__ int rcn_ksize(int in_size, int out_size) {
  double fs = (double)in_size / (double)out_size;
  if (fs < 1.0) fs = 1.0;
  return (int)ceil((FILTER == RCN_BILINEAR ? 1.0 : 2.0) * fs) * 2 + 1;
}

// precompute_coeffs + normalize_coeffs_8bpc for ONE output index xx: taps K[0 .. count) (stride `stride` ints), first source index xmin
template <int FILTER>
__device__ void rcn_coeffs(int in_size, int out_size, int xx, int* K, int stride, int& xmin_out, int& count_out) {
  const double scale = (double)in_size / (double)out_size;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = (FILTER == RCN_BILINEAR ? 1.0 : 2.0) * fs, ss = 1.0 / fs;
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

// desc row (8 int32): offset / 16, w, h, nw, nh, left, top, 0; the output is the out_h x out_w window at (left, top) of the resized image
template <int FILTER>
__global__ __launch_bounds__(RCN_TX * RCN_WAVES) void resize_crop_normalize_kernel(
    const unsigned char* __restrict__ packed, long packed_bytes, const int* __restrict__ desc, int out_h, int out_w, int kmax,
    const float* __restrict__ lut, float* __restrict__ out, int tiles_x, int whole) {
  extern __shared__ int rcn_lds[];
  int* Kx = rcn_lds;                                // [kmax][RCN_TX]
  int* Ky = Kx + kmax * RCN_TX;                     // [RCN_TY][kmax]
  int* x_min = Ky + RCN_TY * kmax;                  // [RCN_TX]
  int* x_cnt = x_min + RCN_TX;                      // [RCN_TX]
  int* y_min = x_cnt + RCN_TX;                      // [RCN_TY]
  int* y_cnt = y_min + RCN_TY;                      // [RCN_TY]

  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int* d = desc + (size_t)b * 8;
  const size_t off = (size_t)(unsigned)d[0] * 16;
  const int w = d[1], h = d[2], nw = d[3], nh = d[4], left = d[5], top = d[6];
  const int ox = tx * RCN_TX + lane;                // this lane's output column
  const size_t plane = (size_t)out_h * out_w;
  float* o = out + (size_t)b * 3 * plane;

  // a descriptor this launch cannot serve (outside the packed buffer, crop outside the resized image, more taps than kmax; `whole`:
  // anything but the whole resized image):
  // the image's output is NaN — nothing is read through it
  bool ok = w > 0 && h > 0 && nw > 0 && nh > 0 && left >= 0 && top >= 0 && (long)left + out_w <= nw && (long)top + out_h <= nh;
  ok = ok && (!whole || (nw == out_w && nh == out_h && left == 0 && top == 0));
  ok = ok && (long)off + 3l * w * h <= packed_bytes;
  ok = ok && rcn_ksize<FILTER>(w, nw) <= kmax && rcn_ksize<FILTER>(h, nh) <= kmax;
  if (!ok) {
    if (ox < out_w)
      for (int r = 0; r < RCN_RY; ++r) {
        const int oy = ty * RCN_TY + wave * RCN_RY + r;
        if (oy < out_h)
          for (int c = 0; c < 3; ++c) o[c * plane + (size_t)oy * out_w + ox] = __builtin_nanf("");
      }
    return;
  }

  if (tid < RCN_TX) {
    int mn = 0, cnt = 0;
    if (ox < out_w) rcn_coeffs<FILTER>(w, nw, left + ox, Kx + tid, RCN_TX, mn, cnt);
    x_min[tid] = mn;
    x_cnt[tid] = cnt;
  } else if (tid < RCN_TX + RCN_TY) {
    const int r = tid - RCN_TX, oy = ty * RCN_TY + r;
    int mn = 0, cnt = 0;
    if (oy < out_h) rcn_coeffs<FILTER>(h, nh, top + oy, Ky + r * kmax, 1, mn, cnt);
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

  const unsigned char* src = packed + off;
  const int* ky = Ky + wave * RCN_RY * kmax;
  for (int y = ylo; y < yhi; ++y) {                 // wave-uniform bounds
    const unsigned char* p = src + ((size_t)y * w + xmin) * 3;
    int s0 = 1 << (RCN_PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < xcnt; ++t) {
      const int k = Kx[t * RCN_TX + lane];
      s0 += (int)p[3 * t] * k;
      s1 += (int)p[3 * t + 1] * k;
      s2 += (int)p[3 * t + 2] * k;
    }
    const int h0 = rcn_clip8(s0), h1 = rcn_clip8(s1), h2 = rcn_clip8(s2);      // the u8 intermediate of the horizontal pass
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

  if (ox < out_w) {
#pragma unroll
    for (int r = 0; r < RCN_RY; ++r) {
      const int oy = ty * RCN_TY + wave * RCN_RY + r;
      if (oy < out_h) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c * plane + (size_t)oy * out_w + ox] = lut[c * 256 + rcn_clip8(acc[r][c])];
      }
    }
  }
}

template <int FILTER>
static void rcn_launch(const unsigned char* packed, long packed_bytes, const int* desc, int B, int out_h, int out_w, int kmax,
                       const float* lut, float* out, int whole, hipStream_t stream) {
  const int tiles_x = zh_cdiv(out_w, RCN_TX), tiles_y = zh_cdiv(out_h, RCN_TY);
  const size_t lds = ((size_t)(RCN_TX + RCN_TY) * kmax + 2 * (RCN_TX + RCN_TY)) * sizeof(int);
  hipLaunchKernelGGL(resize_crop_normalize_kernel<FILTER>, dim3(tiles_x * tiles_y, B), dim3(RCN_TX * RCN_WAVES), lds, stream,
                     packed, packed_bytes, desc, out_h, out_w, kmax, lut, out, tiles_x, whole);
}

extern "C" int zh_resize_crop_normalize_u8(const unsigned char* packed, long packed_bytes, const int* desc, int B, int n_px, int kmax,
                                           const float* lut, float* out, hipStream_t stream) {
  ZH_CHECK_ARG(packed && desc && lut && out, "zh_resize_crop_normalize_u8: null pointer");
  ZH_CHECK_ARG(B > 0 && B <= 65535 && n_px > 0 && n_px <= 16384 && packed_bytes > 0,
               "zh_resize_crop_normalize_u8: bad sizes (B=%d n_px=%d packed_bytes=%ld)", B, n_px, packed_bytes);
  ZH_CHECK_ARG(((uintptr_t)packed & 15) == 0, "zh_resize_crop_normalize_u8: packed must be 16-byte aligned");
  ZH_CHECK_ARG(kmax >= 5 && kmax <= RCN_KMAX, "zh_resize_crop_normalize_u8: kmax %d outside [5, %d] (taps per output pixel: resize such an image on the host)",
               kmax, RCN_KMAX);
  rcn_launch<RCN_BICUBIC>(packed, packed_bytes, desc, B, n_px, n_px, kmax, lut, out, 0, stream);
  ZH_CHECK_LAUNCH("zh_resize_crop_normalize_u8");
  return ZH_OK;
}

// every image of the launch resized to out_w x out_h, no crop: a descriptor whose (nw, nh, left, top) is not (out_w, out_h, 0, 0) gives NaN
extern "C" int zh_resize_normalize_u8(const unsigned char* packed, long packed_bytes, const int* desc, int B, int out_h, int out_w,
                                      int filter, int kmax, const float* lut, float* out, hipStream_t stream) {
  ZH_CHECK_ARG(packed && desc && lut && out, "zh_resize_normalize_u8: null pointer");
  ZH_CHECK_ARG(B > 0 && B <= 65535 && out_h > 0 && out_h <= 16384 && out_w > 0 && out_w <= 16384 && packed_bytes > 0,
               "zh_resize_normalize_u8: bad sizes (B=%d out_h=%d out_w=%d packed_bytes=%ld)", B, out_h, out_w, packed_bytes);
  ZH_CHECK_ARG(((uintptr_t)packed & 15) == 0, "zh_resize_normalize_u8: packed must be 16-byte aligned");
  ZH_CHECK_ARG(filter == RCN_BILINEAR || filter == RCN_BICUBIC, "zh_resize_normalize_u8: filter %d is neither ZH_FILTER_BILINEAR nor ZH_FILTER_BICUBIC", filter);
  const int kmin = filter == RCN_BILINEAR ? 3 : 5;
  ZH_CHECK_ARG(kmax >= kmin && kmax <= RCN_KMAX, "zh_resize_normalize_u8: kmax %d outside [%d, %d] (taps per output pixel: resize such an image on the host)",
               kmax, kmin, RCN_KMAX);
  if (filter == RCN_BILINEAR) rcn_launch<RCN_BILINEAR>(packed, packed_bytes, desc, B, out_h, out_w, kmax, lut, out, 1, stream);
  else rcn_launch<RCN_BICUBIC>(packed, packed_bytes, desc, B, out_h, out_w, kmax, lut, out, 1, stream);
  ZH_CHECK_LAUNCH("zh_resize_normalize_u8");
  return ZH_OK;
}
