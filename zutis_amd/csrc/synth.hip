// One training sample of IndexDataset.__getitem__ (datasets/index_dataset.py:301-385) on the device, from the decoded bytes of its 1 - 10
// files and a recipe that holds every random draw (zutis_amd/synth.py): random_scale, random_crop, random_hflip
// (datasets/augmentations/geometric_transforms.py), ColorJitter / RandomGrayscale / GaussianBlur (datasets/base_dataset.py:62-78),
// to_tensor + normalize, copy_paste (datasets/augmentations/copy_paste.py).  Everything but the blur is bit-identical to
// Pillow / torch on the host; compiled with -ffp-contract=off (the blend and the HSV round trip are sequences of single IEEE operations).
//
// A batch of B samples is N = sum n_i sub-images (N <= 80 at the reference's batch of 8).  Between the stages a sub-image is a C x C
// array of 4-byte pixels (R, G, B, mask byte in {0, 1, ignore_index}): one 4-byte load / store per lane, the mask travels with its pixel.
//
//   zh_synth_geometry_u8     (1) only for sub-images that are padded: the channel sums of the WHOLE scaled image (the fill colour is its
//                            mean), one workgroup per 32 x 64 tile, 64-bit vector atomics;  (2) one workgroup per (sub-image, 32 x 64
//                            tile of the crop): Pillow's BILINEAR at the recipe's size — rcn.h's tile body, the one preprocess.hip runs,,
//                            only the crop's pixels are ever resampled — the ATen nearest index for the mask, pad corner, crop, flip,
//                            and the object's bounding box by int atomics.
//   zh_synth_photometric_u8  ColorJitter's four ops in the recipe's order + RandomGrayscale, per pixel in place.  Contrast blends with the
//                            grey mean of the image AS IT STANDS when contrast is reached, so launch (1) applies the ops before contrast
//                            and reduces the grey sum, launch (2) repeats them (a few flops per pixel, cheaper than a round trip) and goes on.
//   zh_synth_blur_u8         the separable Gaussian (BORDER_REFLECT_101) of the sub-images whose recipe blurs, into a second buffer:
//                            the horizontal pass of a 32 x 32 tile and its halo rows goes to LDS as fp32, the vertical pass reads LDS.
//   zh_synth_compose         copy_paste per OUTPUT pixel: the value comes from the last sub-image j >= 1 whose shifted object region
//                            covers the pixel, else from sub-image 0 — one pass instead of n - 1; writes the normalised image, the
//                            semantic mask (int64) and the one-hot instance rows.
// Bounds: bytes.  At C = 384 a sub-image is 0.59 MB per stage buffer; the stages re-read it out of L2 (80 sub-images: 47 MB).
// Sums and boxes use VECTOR atomics (global_atomic_add_x2 / smin / smax) only.
#include "common.h"
#include "rcn.h"

#define SY_TX RCN_TX        // the resampling launches use rcn.h's tile: 64 columns (= lanes) x 4 waves x 8 rows
#define SY_WAVES RCN_WAVES
#define SY_RY RCN_RY
#define SY_TY RCN_TY
#define SY_DESC 32          // int32 per sub-image descriptor row (zutis_amd/synth.py DESC_*)
#define SY_WORK 12          // int32 per sub-image work row: 4 x u64 (fill sums R G B, grey sum), ymin, ymax, xmin, xmax
#define SY_MAX_SUB 64       // sub-images per sample the compose kernel serves
#define SY_BLUR_T 32        // blur tile edge
#define SY_BLUR_RMAX 48     // blur radius served: 3 * (32 + 96) * 32 * 4 = 48 KiB of LDS

#define SYF_JITTER 1
#define SYF_GREY 2
#define SYF_BLUR 4
#define SYF_PADDED 8

// descriptor slots
#define SD_IMG 0
#define SD_W 1
#define SD_H 2
#define SD_NW 3
#define SD_NH 4
#define SD_MASK 5
#define SD_PAD_L 6
#define SD_PAD_T 7
#define SD_CROP_L 8
#define SD_CROP_T 9
#define SD_FLIP 10
#define SD_LABEL 11
#define SD_FLAGS 12
#define SD_ORDER 13     // four 2-bit op codes, first op in the low bits: 0 brightness, 1 contrast, 2 saturation, 3 hue
#define SD_HUE 14
#define SD_BRIGHT 15    // fp32 bits
#define SD_CONTRAST 16
#define SD_SATUR 17
#define SD_SCALE_H 18   // fp32 bits: float(h) / float(nh), the ATen nearest scale
#define SD_SCALE_W 19
#define SD_U_TOP 20     // double bits (2 slots): the paste draws
#define SD_U_LEFT 22

typedef unsigned long long u64_t;

__device__ __forceinline__ float sy_f32(int bits) { return __builtin_bit_cast(float, bits); }

// whether this launch can serve the descriptor: sizes positive, bytes inside the packed buffer, taps within kmax
__device__ __forceinline__ bool sy_desc_ok(const int* d, long packed_bytes, int kmax) {
  const int w = d[SD_W], h = d[SD_H], nw = d[SD_NW], nh = d[SD_NH];
  bool ok = w > 0 && h > 0 && nw > 0 && nh > 0 && d[SD_PAD_L] >= 0 && d[SD_PAD_T] >= 0 && d[SD_CROP_L] >= 0 && d[SD_CROP_T] >= 0;
  ok = ok && (long)(unsigned)d[SD_IMG] * 16 + 3l * w * h <= packed_bytes && (long)(unsigned)d[SD_MASK] * 16 + (long)w * h <= packed_bytes;
  ok = ok && rcn_ksize<ZH_FILTER_BILINEAR>(w, nw) <= kmax && rcn_ksize<ZH_FILTER_BILINEAR>(h, nh) <= kmax;
  return ok;
}

__device__ __forceinline__ u64_t sy_wave_sum_u64(u64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// (1) channel sums of the whole scaled image of every PADDED sub-image -> work[n][0..2] (u64)
__global__ __launch_bounds__(SY_TX * SY_WAVES) void synth_fill_sums_kernel(const unsigned char* __restrict__ packed, long packed_bytes,
                                                                           const int* __restrict__ desc, int kmax, int tiles_x,
                                                                           int* __restrict__ work) {
  extern __shared__ int sy_lds[];
  const int n = blockIdx.y, tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int* d = desc + (size_t)n * SY_DESC;
  if (!(d[SD_FLAGS] & SYF_PADDED) || !sy_desc_ok(d, packed_bytes, kmax)) return;
  const int nw = d[SD_NW], nh = d[SD_NH];
  if (tx * SY_TX >= nw || ty * SY_TY >= nh) return;                     // block-uniform
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sx = tx * SY_TX + lane;
  int px[SY_RY][3];
  rcn_tile_u8<ZH_FILTER_BILINEAR>(packed + (size_t)(unsigned)d[SD_IMG] * 16, d[SD_W], d[SD_H], nw, nh, sx, ty * SY_TY, SY_TY, kmax, sy_lds, px);
  u64_t s[3] = {0, 0, 0};
  if (sx < nw) {
#pragma unroll
    for (int r = 0; r < SY_RY; ++r)
      if (ty * SY_TY + wave * SY_RY + r < nh) {
        s[0] += px[r][0];
        s[1] += px[r][1];
        s[2] += px[r][2];
      }
  }
  u64_t* sums = (u64_t*)(work + (size_t)n * SY_WORK);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const u64_t t = sy_wave_sum_u64(s[c]);
    if (lane == 0 && t) atomicAdd(sums + c, t);
  }
}

// (2) the C x C crop of every sub-image -> out [N, C, C] of (R, G, B, mask); work[n][8..11] = ymin, ymax, xmin, xmax of the object
__global__ __launch_bounds__(SY_TX * SY_WAVES) void synth_geometry_kernel(const unsigned char* __restrict__ packed, long packed_bytes,
                                                                          const int* __restrict__ desc, int C, int ignore_index, int kmax,
                                                                          int tiles_x, int* __restrict__ work, uchar4* __restrict__ out) {
  extern __shared__ int sy_lds[];
  const int n = blockIdx.y, tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int* d = desc + (size_t)n * SY_DESC;
  const int ox = tx * SY_TX + lane;
  uchar4* o = out + (size_t)n * C * C;
  if (!sy_desc_ok(d, packed_bytes, kmax)) {         // not served: the whole crop is ignore_index on black — nothing is read through the descriptor
    if (ox < C)
      for (int r = 0; r < SY_RY; ++r) {
        const int oy = ty * SY_TY + wave * SY_RY + r;
        if (oy < C) o[(size_t)oy * C + ox] = make_uchar4(0, 0, 0, (unsigned char)ignore_index);
      }
    return;
  }
  const int w = d[SD_W], h = d[SD_H], nw = d[SD_NW], nh = d[SD_NH];
  // crop pixel (ox, oy) <- flip -> padded image (crop_left + x, crop_top + oy) -> scaled image (.. - pad_left, .. - pad_top)
  const int x = d[SD_FLIP] ? C - 1 - ox : ox;
  const int sx = ox < C ? d[SD_CROP_L] + x - d[SD_PAD_L] : -1;
  const int sy_base = d[SD_CROP_T] + ty * SY_TY - d[SD_PAD_T];
  int px[SY_RY][3];
  rcn_tile_u8<ZH_FILTER_BILINEAR>(packed + (size_t)(unsigned)d[SD_IMG] * 16, w, h, nw, nh, sx, sy_base, SY_TY, kmax, sy_lds, px);

  // the fill: np.array(image).mean(axis=(0, 1)).astype(np.uint8).  NumPy sums the bytes in float64 (exact: the sum is an integer below
  // 2^53) and divides once, correctly rounded.  If count divides the sum the quotient is exact; otherwise the true quotient lies at least
  // 1 / count >= 2^-31 below the next integer while the rounding error is below 2^-44 (the quotient is below 256), so the rounded
  // quotient has the same integer part: the truncated float64 mean IS the integer division.
  int fill[3] = {0, 0, 0};
  if (d[SD_FLAGS] & SYF_PADDED) {
    const u64_t* sums = (const u64_t*)(work + (size_t)n * SY_WORK);
    const u64_t count = (u64_t)nw * (u64_t)nh;
#pragma unroll
    for (int c = 0; c < 3; ++c) fill[c] = (int)(sums[c] / count);
  }
  const unsigned char* mask = packed + (size_t)(unsigned)d[SD_MASK] * 16;
  const float scale_h = sy_f32(d[SD_SCALE_H]), scale_w = sy_f32(d[SD_SCALE_W]);
  const bool col_in = sx >= 0 && sx < nw;
  const int mx = col_in ? min((int)floorf(__fmul_rn((float)sx, scale_w)), w - 1) : 0;      // ATen nearest_neighbor_compute_source_index
  const int label = d[SD_LABEL];
  const bool label_obj = 0 < label && label < ignore_index;
  int ymin = 0x7fffffff, ymax = -1, xmin = 0x7fffffff, xmax = -1;
#pragma unroll
  for (int r = 0; r < SY_RY; ++r) {
    const int oy = ty * SY_TY + wave * SY_RY + r, sy = sy_base + wave * SY_RY + r;
    if (ox >= C || oy >= C) continue;
    uchar4 v;
    if (col_in && sy >= 0 && sy < nh) {
      const int my = min((int)floorf(__fmul_rn((float)sy, scale_h)), h - 1);
      v = make_uchar4(px[r][0], px[r][1], px[r][2], mask[(size_t)my * w + mx]);
    } else {
      v = make_uchar4(fill[0], fill[1], fill[2], (unsigned char)ignore_index);
    }
    o[(size_t)oy * C + ox] = v;
    if (v.w == 1 && label_obj) {
      ymin = min(ymin, oy); ymax = max(ymax, oy);
      xmin = min(xmin, ox); xmax = max(xmax, ox);
    }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    ymin = min(ymin, __shfl_xor(ymin, s, 64)); ymax = max(ymax, __shfl_xor(ymax, s, 64));
    xmin = min(xmin, __shfl_xor(xmin, s, 64)); xmax = max(xmax, __shfl_xor(xmax, s, 64));
  }
  if (lane == 0 && ymax >= 0) {
    int* box = work + (size_t)n * SY_WORK + 8;
    atomicMin(box + 0, ymin); atomicMax(box + 1, ymax);
    atomicMin(box + 2, xmin); atomicMax(box + 3, xmax);
  }
}

// ---- photometric ops on bytes -------------------------------------------------------------------------------------------------
// Image.blend(degenerate, image, f) of ImageEnhance (Pillow src/libImaging/Blend.c): fp32 a + f * (b - a), truncated; outside [0, 1] clipped first
__device__ __forceinline__ int sy_blend(int a, int b, float f) {
  const float v = (float)a + f * (float)(b - a);
  if (f >= 0.f && f <= 1.f) return (int)v & 255;
  return v <= 0.f ? 0 : (v >= 255.f ? 255 : (int)v);
}
// Image.convert("L"): ITU-R 601-2 in 16-bit fixed point (Pillow Convert.c L24)
__device__ __forceinline__ int sy_grey(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Pillow Convert.c rgb2hsv_row / hsv2rgb with H += shift (mod 256) in between (torchvision adjust_hue on a PIL image).  The mixed
// float / double steps are Pillow's own: each line below is one of its C expressions.
__device__ __forceinline__ void sy_hue(int& r, int& g, int& b, int shift) {
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  int uh = 0, us = 0;
  const int uv = maxc;
  if (minc != maxc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
    uh = min(max((int)((double)h * 255.0), 0), 255);
    us = min(max((int)((double)s * 255.0), 0), 255);
  }
  uh = (uh + shift) & 255;
  if (us == 0) {
    r = g = b = uv;
    return;
  }
  const double hf = (double)(float)uh * 6.0 / 255.0;
  const int i = (int)floor(hf);
  const float f = (float)(hf - (double)(float)i);
  const float fs = (float)((double)(float)us / 255.0);
  const double vf = (double)(float)uv;
  const int p = min(max((int)round(vf * (1.0 - (double)fs)), 0), 255);
  const int q = min(max((int)round(vf * (1.0 - (double)(fs * f))), 0), 255);
  const int t = min(max((int)round(vf * (1.0 - (double)fs * (1.0 - (double)f))), 0), 255);
  switch (i % 6) {
    case 0: r = uv; g = t; b = p; break;
    case 1: r = q; g = uv; b = p; break;
    case 2: r = p; g = uv; b = t; break;
    case 3: r = p; g = q; b = uv; break;
    case 4: r = t; g = p; b = uv; break;
    default: r = uv; g = p; b = q; break;
  }
}

// ColorJitter's ops in the recipe's order.  mean < 0: stop when contrast is reached (returns false when there is no contrast to reach)
__device__ __forceinline__ void sy_jitter(int& r, int& g, int& b, const int* d, int mean) {
  const int order = d[SD_ORDER];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int op = (order >> (2 * k)) & 3;
    if (op == 0) {
      const float f = sy_f32(d[SD_BRIGHT]);
      r = sy_blend(0, r, f); g = sy_blend(0, g, f); b = sy_blend(0, b, f);
    } else if (op == 1) {
      if (mean < 0) return;
      const float f = sy_f32(d[SD_CONTRAST]);
      r = sy_blend(mean, r, f); g = sy_blend(mean, g, f); b = sy_blend(mean, b, f);
    } else if (op == 2) {
      const float f = sy_f32(d[SD_SATUR]);
      const int y = sy_grey(r, g, b);
      r = sy_blend(y, r, f); g = sy_blend(y, g, f); b = sy_blend(y, b, f);
    } else {
      sy_hue(r, g, b, d[SD_HUE]);
    }
  }
}

// (1) grey sum of the image as it stands when contrast is reached -> work[n][3] (u64); 256 threads x 4 pixels
__global__ __launch_bounds__(256) void synth_grey_sum_kernel(const uchar4* __restrict__ pix, const int* __restrict__ desc, int C,
                                                             int* __restrict__ work) {
  const int n = blockIdx.y;
  const int* d = desc + (size_t)n * SY_DESC;
  if (!(d[SD_FLAGS] & SYF_JITTER)) return;
  const uchar4* p = pix + (size_t)n * C * C;
  u64_t s = 0;
  for (int k = 0; k < 4; ++k) {
    const int i = (blockIdx.x * 4 + k) * 256 + threadIdx.x;
    if (i < C * C) {
      const uchar4 v = p[i];
      int r = v.x, g = v.y, b = v.z;
      sy_jitter(r, g, b, d, -1);
      s += sy_grey(r, g, b);
    }
  }
  s = sy_wave_sum_u64(s);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd((u64_t*)(work + (size_t)n * SY_WORK) + 3, s);
}

// (2) all ops, in place
__global__ __launch_bounds__(256) void synth_photometric_kernel(uchar4* __restrict__ pix, const int* __restrict__ desc, int C,
                                                                const int* __restrict__ work) {
  const int n = blockIdx.y;
  const int* d = desc + (size_t)n * SY_DESC;
  const int flags = d[SD_FLAGS];
  if (!(flags & (SYF_JITTER | SYF_GREY))) return;
  // ImageEnhance.Contrast: int(ImageStat.Stat(grey).mean[0] + 0.5) = floor(sum / count + 1 / 2) = (2 sum + count) / (2 count) in integers:
  // the float64 value sum / count + 0.5 is exact when it is an integer and otherwise at least 1 / (2 count) away from one
  const u64_t sum = ((const u64_t*)(work + (size_t)n * SY_WORK))[3], count = (u64_t)C * C;
  const int mean = (int)((2 * sum + count) / (2 * count));
  uchar4* p = pix + (size_t)n * C * C;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C * C) return;
  const uchar4 v = p[i];
  int r = v.x, g = v.y, b = v.z;
  if (flags & SYF_JITTER) sy_jitter(r, g, b, d, mean);
  if (flags & SYF_GREY) r = g = b = sy_grey(r, g, b);
  p[i] = make_uchar4(r, g, b, v.w);
}

// ---- blur ---------------------------------------------------------------------------------------------------------------------
// BORDER_REFLECT_101; an index further out than one reflection reaches (rows of a tile that hangs over the image, never used) is clamped
__device__ __forceinline__ int sy_reflect101(int i, int n) {
  i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
  return min(max(i, 0), n - 1);
}

// weights f32 [N, ks] (normalised on the host in float64); in -> out for the sub-images whose recipe blurs; the mask byte is carried over
__global__ __launch_bounds__(256) void synth_blur_kernel(const uchar4* __restrict__ in, const int* __restrict__ desc,
                                                         const float* __restrict__ weights, int C, int ks, int tiles_x,
                                                         uchar4* __restrict__ out) {
  extern __shared__ float sb_lds[];
  const int n = blockIdx.y;
  if (!(desc[(size_t)n * SY_DESC + SD_FLAGS] & SYF_BLUR)) return;
  const int R = ks >> 1, rows = SY_BLUR_T + 2 * R;
  float* wk = sb_lds;                               // [ks]
  float* hp = sb_lds + ((ks + 31) & ~31);           // [3][rows][32]: the horizontal pass
  const int tx0 = (blockIdx.x % tiles_x) * SY_BLUR_T, ty0 = (blockIdx.x / tiles_x) * SY_BLUR_T;
  const uchar4* src = in + (size_t)n * C * C;
  for (int t = threadIdx.x; t < ks; t += 256) wk[t] = weights[(size_t)n * ks + t];
  __syncthreads();
  for (int idx = threadIdx.x; idx < rows * SY_BLUR_T; idx += 256) {
    const int row = idx >> 5, col = idx & 31;
    const int gy = sy_reflect101(ty0 - R + row, C), x0 = tx0 + col - R;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    if (tx0 + col < C) {
      const uchar4* line = src + (size_t)gy * C;
      for (int t = 0; t < ks; ++t) {
        const uchar4 v = line[sy_reflect101(x0 + t, C)];
        const float k = wk[t];
        a0 = __fmaf_rn(k, (float)v.x, a0); a1 = __fmaf_rn(k, (float)v.y, a1); a2 = __fmaf_rn(k, (float)v.z, a2);
      }
    }
    hp[idx] = a0; hp[rows * SY_BLUR_T + idx] = a1; hp[2 * rows * SY_BLUR_T + idx] = a2;
  }
  __syncthreads();
  const int col = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int ox = tx0 + col;
  if (ox >= C) return;
  for (int r = 0; r < SY_BLUR_T / 8; ++r) {
    const int ly = rg * (SY_BLUR_T / 8) + r, oy = ty0 + ly;
    if (oy >= C) break;
    float a[3] = {0.f, 0.f, 0.f};
    for (int t = 0; t < ks; ++t) {
      const float k = wk[t];
#pragma unroll
      for (int c = 0; c < 3; ++c) a[c] = __fmaf_rn(k, hp[c * rows * SY_BLUR_T + (ly + t) * SY_BLUR_T + col], a[c]);
    }
    int q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = min(max((int)rintf(a[c]), 0), 255);
    const size_t o = (size_t)n * C * C + (size_t)oy * C + ox;
    out[o] = make_uchar4(q[0], q[1], q[2], in[o].w);
  }
}

// ---- compose ------------------------------------------------------------------------------------------------------------------
// samples int32 [B, 4]: first sub-image, n, first one-hot row, 0.  Per sample: image f32 [3, C, C], semantic int64 [C, C], one-hot bool rows.
__global__ __launch_bounds__(256) void synth_compose_kernel(const uchar4* __restrict__ plain, const uchar4* __restrict__ blurred,
                                                            const int* __restrict__ desc, const int* __restrict__ samples,
                                                            const int* __restrict__ work, const float* __restrict__ lut, int N, int C,
                                                            int ignore_index, float* __restrict__ image, long long* __restrict__ semantic,
                                                            unsigned char* __restrict__ onehot) {
  __shared__ int box[SY_MAX_SUB][6];                // ymin, ymax, xmin, xmax (maxima EXCLUSIVE, as the reference slices), dy, dx
  __shared__ const uchar4* srcs[SY_MAX_SUB];
  __shared__ int labels[SY_MAX_SUB];
  const int b = blockIdx.y, first = samples[b * 4], n = samples[b * 4 + 1], row0 = samples[b * 4 + 2];
  if (first < 0 || n < 1 || n > SY_MAX_SUB || first + n > N || row0 < 0) return;      // block-uniform: a sample row this launch cannot serve
  if (threadIdx.x < n) {
    const int j = threadIdx.x, s = first + j;
    const int* d = desc + (size_t)s * SY_DESC;
    const int* w = work + (size_t)s * SY_WORK + 8;
    const int ymin = w[0], ymax = w[1], xmin = w[2], xmax = w[3];
    int dy = 0, dx = 0;
    if (ymax >= 0) {
      // offset = randint(0, C - bbox) resolved from the recipe's unit-interval draw: floor(u * (range + 1))
      double ut, ul;
      __builtin_memcpy(&ut, d + SD_U_TOP, 8);
      __builtin_memcpy(&ul, d + SD_U_LEFT, 8);
      const int top = (int)floor(ut * (double)(C - (ymax - ymin) + 1)), left = (int)floor(ul * (double)(C - (xmax - xmin) + 1));
      dy = ymin - top;                              // source row = output row + dy
      dx = xmin - left;
    }
    box[j][0] = ymin; box[j][1] = ymax >= 0 ? ymax : -0x7fffffff; box[j][2] = xmin; box[j][3] = xmax;
    box[j][4] = dy; box[j][5] = dx;
    srcs[j] = ((d[SD_FLAGS] & SYF_BLUR) ? blurred : plain) + (size_t)s * C * C;
    labels[j] = d[SD_LABEL];
  }
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C * C) return;
  const int y = i / C, x = i - y * C;
  int win = 0;
  uchar4 v;
  for (int j = n - 1; j >= 1; --j) {
    const int sy = y + box[j][4], sx = x + box[j][5];
    if (sy >= box[j][0] && sy < box[j][1] && sx >= box[j][2] && sx < box[j][3] && 0 < labels[j] && labels[j] < ignore_index) {
      v = srcs[j][(size_t)sy * C + sx];
      if (v.w == 1) { win = j; break; }
    }
  }
  if (win == 0) v = srcs[0][i];
  const size_t plane = (size_t)C * C;
  float* im = image + (size_t)b * 3 * plane;
  im[i] = lut[v.x];
  im[plane + i] = lut[256 + v.y];
  im[2 * plane + i] = lut[512 + v.z];
  semantic[(size_t)b * plane + i] = v.w == 1 ? labels[win] : v.w;
  const int inst = v.w == 1 ? win + 1 : v.w;        // binary_mask[binary_mask == 1] = instance_id: the ignore value stays in the instance map
  for (int k = 0; k < n; ++k) onehot[(size_t)(row0 + k) * plane + i] = inst == k + 1;
}

// ---- entry points -------------------------------------------------------------------------------------------------------------
static size_t sy_tile_lds(int kmax) { return ((size_t)(SY_TX + SY_TY) * kmax + 2 * (SY_TX + SY_TY)) * sizeof(int); }

extern "C" int zh_synth_geometry_u8(const unsigned char* packed, long packed_bytes, const int* desc, int N, int C, int ignore_index,
                                    int kmax, int fill_w, int fill_h, int* work, unsigned char* out_rgbm, hipStream_t stream) {
  ZH_CHECK_ARG(packed && desc && work && out_rgbm, "zh_synth_geometry_u8: null pointer");
  ZH_CHECK_ARG(N > 0 && N <= 65535 && C > 0 && C <= 16384 && packed_bytes > 0, "zh_synth_geometry_u8: bad sizes (N=%d C=%d packed_bytes=%ld)", N, C, packed_bytes);
  ZH_CHECK_ARG(ignore_index > 1 && ignore_index <= 255, "zh_synth_geometry_u8: ignore_index %d outside (1, 255] (the mask travels as a byte)", ignore_index);
  ZH_CHECK_ARG(((uintptr_t)packed & 15) == 0 && ((uintptr_t)work & 7) == 0 && ((uintptr_t)out_rgbm & 3) == 0, "zh_synth_geometry_u8: packed must be 16-byte, work 8-byte, out 4-byte aligned");
  ZH_CHECK_ARG(kmax >= 3 && kmax <= ZH_RCN_KMAX, "zh_synth_geometry_u8: kmax %d outside [3, %d] (taps per output pixel: scale such an image on the host)", kmax, ZH_RCN_KMAX);
  ZH_CHECK_ARG(fill_w >= 0 && fill_h >= 0 && fill_w <= 65536 && fill_h <= 65536, "zh_synth_geometry_u8: bad fill extent %d x %d", fill_w, fill_h);
  if (fill_w > 0 && fill_h > 0) {
    const int tx = zh_cdiv(fill_w, SY_TX), ty = zh_cdiv(fill_h, SY_TY);
    hipLaunchKernelGGL(synth_fill_sums_kernel, dim3(tx * ty, N), dim3(SY_TX * SY_WAVES), sy_tile_lds(kmax), stream, packed, packed_bytes,
                       desc, kmax, tx, work);
    ZH_CHECK_LAUNCH("zh_synth_geometry_u8 (fill sums)");
  }
  const int tx = zh_cdiv(C, SY_TX), ty = zh_cdiv(C, SY_TY);
  hipLaunchKernelGGL(synth_geometry_kernel, dim3(tx * ty, N), dim3(SY_TX * SY_WAVES), sy_tile_lds(kmax), stream, packed, packed_bytes, desc,
                     C, ignore_index, kmax, tx, work, (uchar4*)out_rgbm);
  ZH_CHECK_LAUNCH("zh_synth_geometry_u8");
  return ZH_OK;
}

extern "C" int zh_synth_photometric_u8(unsigned char* rgbm, const int* desc, int N, int C, int* work, hipStream_t stream) {
  ZH_CHECK_ARG(rgbm && desc && work, "zh_synth_photometric_u8: null pointer");
  ZH_CHECK_ARG(N > 0 && N <= 65535 && C > 0 && C <= 16384, "zh_synth_photometric_u8: bad sizes (N=%d C=%d)", N, C);
  ZH_CHECK_ARG(((uintptr_t)rgbm & 3) == 0 && ((uintptr_t)work & 7) == 0, "zh_synth_photometric_u8: rgbm must be 4-byte, work 8-byte aligned");
  hipLaunchKernelGGL(synth_grey_sum_kernel, dim3(zh_cdiv((long)C * C, 1024), N), dim3(256), 0, stream, (const uchar4*)rgbm, desc, C, work);
  ZH_CHECK_LAUNCH("zh_synth_photometric_u8 (grey sum)");
  hipLaunchKernelGGL(synth_photometric_kernel, dim3(zh_cdiv((long)C * C, 256), N), dim3(256), 0, stream, (uchar4*)rgbm, desc, C, work);
  ZH_CHECK_LAUNCH("zh_synth_photometric_u8");
  return ZH_OK;
}

extern "C" int zh_synth_blur_u8(const unsigned char* rgbm, const int* desc, const float* weights, int N, int C, int ksize,
                                unsigned char* out_rgbm, hipStream_t stream) {
  ZH_CHECK_ARG(rgbm && desc && weights && out_rgbm && rgbm != out_rgbm, "zh_synth_blur_u8: null pointer or in-place call");
  ZH_CHECK_ARG(N > 0 && N <= 65535 && C > 0 && C <= 16384, "zh_synth_blur_u8: bad sizes (N=%d C=%d)", N, C);
  ZH_CHECK_ARG(ksize >= 1 && (ksize & 1) && ksize / 2 <= SY_BLUR_RMAX && ksize / 2 < C, "zh_synth_blur_u8: kernel size %d must be odd, at most %d and its radius below C=%d",
               ksize, 2 * SY_BLUR_RMAX + 1, C);
  ZH_CHECK_ARG((((uintptr_t)rgbm | (uintptr_t)out_rgbm) & 3) == 0, "zh_synth_blur_u8: buffers must be 4-byte aligned");
  const int t = zh_cdiv(C, SY_BLUR_T);
  const size_t lds = (((size_t)ksize + 31) & ~(size_t)31) * 4 + 3 * (size_t)(SY_BLUR_T + 2 * (ksize / 2)) * SY_BLUR_T * 4;
  hipLaunchKernelGGL(synth_blur_kernel, dim3(t * t, N), dim3(256), lds, stream, (const uchar4*)rgbm, desc, weights, C, ksize, t, (uchar4*)out_rgbm);
  ZH_CHECK_LAUNCH("zh_synth_blur_u8");
  return ZH_OK;
}

extern "C" int zh_synth_compose(const unsigned char* rgbm, const unsigned char* rgbm_blurred, const int* desc, const int* samples,
                                const int* work, const float* lut, int N, int B, int C, int ignore_index, float* image,
                                long long* semantic, unsigned char* onehot, hipStream_t stream) {
  ZH_CHECK_ARG(rgbm && rgbm_blurred && desc && samples && work && lut && image && semantic && onehot, "zh_synth_compose: null pointer");
  ZH_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && C <= 16384, "zh_synth_compose: bad sizes (B=%d C=%d)", B, C);
  ZH_CHECK_ARG(N >= B && N <= 65535, "zh_synth_compose: %d sub-images for %d samples", N, B);
  ZH_CHECK_ARG(ignore_index > 1 && ignore_index <= 255, "zh_synth_compose: ignore_index %d outside (1, 255]", ignore_index);
  hipLaunchKernelGGL(synth_compose_kernel, dim3(zh_cdiv((long)C * C, 256), B), dim3(256), 0, stream, (const uchar4*)rgbm,
                     (const uchar4*)rgbm_blurred, desc, samples, work, lut, N, C, ignore_index, image, semantic, onehot);
  ZH_CHECK_LAUNCH("zh_synth_compose");
  return ZH_OK;
}
