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
// (steps 1 and 2 are rcn_tile_u8 of rcn.h, which csrc/synth.hip runs as well)
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
#include "rcn.h"

// desc row (8 int32): offset / 16, w, h, nw, nh, left, top, 0; the output is the out_h x out_w window at (left, top) of the resized image
template <int FILTER>
__global__ __launch_bounds__(RCN_TX * RCN_WAVES) void resize_crop_normalize_kernel(
    const unsigned char* __restrict__ packed, long packed_bytes, const int* __restrict__ desc, int out_h, int out_w, int kmax,
    const float* __restrict__ lut, float* __restrict__ out, int tiles_x, int whole) {
  extern __shared__ int rcn_lds[];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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

  int px[RCN_RY][3];       // the tile's bytes: rcn.h
  rcn_tile_u8<FILTER>(packed + off, w, h, nw, nh, ox < out_w ? left + ox : -1, top + ty * RCN_TY, out_h - ty * RCN_TY, kmax, rcn_lds, px);

  if (ox < out_w) {
#pragma unroll
    for (int r = 0; r < RCN_RY; ++r) {
      const int oy = ty * RCN_TY + wave * RCN_RY + r;
      if (oy < out_h) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c * plane + (size_t)oy * out_w + ox] = lut[c * 256 + px[r][c]];
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
  ZH_CHECK_ARG(kmax >= 5 && kmax <= ZH_RCN_KMAX, "zh_resize_crop_normalize_u8: kmax %d outside [5, %d] (taps per output pixel: resize such an image on the host)",
               kmax, ZH_RCN_KMAX);
  rcn_launch<ZH_FILTER_BICUBIC>(packed, packed_bytes, desc, B, n_px, n_px, kmax, lut, out, 0, stream);
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
  ZH_CHECK_ARG(filter == ZH_FILTER_BILINEAR || filter == ZH_FILTER_BICUBIC, "zh_resize_normalize_u8: filter %d is neither ZH_FILTER_BILINEAR nor ZH_FILTER_BICUBIC", filter);
  const int kmin = filter == ZH_FILTER_BILINEAR ? 3 : 5;
  ZH_CHECK_ARG(kmax >= kmin && kmax <= ZH_RCN_KMAX, "zh_resize_normalize_u8: kmax %d outside [%d, %d] (taps per output pixel: resize such an image on the host)",
               kmax, kmin, ZH_RCN_KMAX);
  if (filter == ZH_FILTER_BILINEAR) rcn_launch<ZH_FILTER_BILINEAR>(packed, packed_bytes, desc, B, out_h, out_w, kmax, lut, out, 1, stream);
  else rcn_launch<ZH_FILTER_BICUBIC>(packed, packed_bytes, desc, B, out_h, out_w, kmax, lut, out, 1, stream);
  ZH_CHECK_LAUNCH("zh_resize_normalize_u8");
  return ZH_OK;
}
