// Instance predictions as pictures (zh_instance_paint): an id map and / or a colour overlay of the masks zh_mask_nms kept, painted on
// the device where the masks, the kept list and the decoded image already lie.  What utils/visualiser.py:154-187 asks detectron2 for,
// stated in integers: per pixel the kept mask of highest score that covers it (ties: the lower slot), its slot + 1 as the id, its colour
// blended over the image with the arithmetic of zh_upsample_argmax_bytes, an outline where a 4-neighbour belongs to somebody else.
//
// Three launches on the caller's stream, no atomics on global memory, integer arithmetic only:
//   paint_rank_kernel    one workgroup per image: the painted slots (j < count, score > min_score in float64, index inside [0, Q))
//                        ordered by score descending, ties by slot, by counting -> (slot, query) pairs in rank order
//   paint_ids_kernel     one lane per pixel, a wave = 64 consecutive pixels = ONE word of every bit-packed mask (a wave-uniform 8-byte
//                        load per mask) or 64 consecutive bytes of the u8 masks; the walk over the ranks ends once every lane has its
//                        top.  Writes the id map, the u16 ids the outline pass reads, and (no outline) the blend itself.
//   paint_overlay_kernel one lane per pixel: the four neighbours' ids from the u16 map (words straddle rows when W % 64 != 0, so the
//                        neighbours cannot come from the wave's own word), outline or blend.
#include "common.h"

struct PaintArgs {
  const unsigned char* masks;           // u8 [B,Q,H,W] (read when bits is NULL)
  const unsigned long long* bits;       // u64 [B*Q][W64] or NULL
  const int2* order;                    // [B,Q]: (slot, query) of paint rank r
  const int* npaint;                    // [B]
  const unsigned char* colours;         // u8 [B,Q,3]
  const unsigned char* packed;
  const int* desc;
  unsigned char* ids_out;               // may be NULL
  unsigned char* overlay;               // may be NULL
  unsigned short* ids16;                // workspace [B,H*W]; written when the overlay pass follows
  long HW, W64;
  int Q, H, W, alpha, rg16, outline;
};

__global__ __launch_bounds__(256) void paint_rank_kernel(const int* index, const double* score, const int* count, double min_score, int Q,
                                                         int2* order, int* npaint) {
  __shared__ double sc[ZH_PAINT_MAX_Q];
  __shared__ unsigned char on[ZH_PAINT_MAX_Q];
  __shared__ int n_on;
  const int b = blockIdx.x;
  const int c = min(max(count[b], 0), Q);                    // entries past the count are uninitialised: never read
  if (threadIdx.x == 0) n_on = 0;
  for (int j = threadIdx.x; j < c; j += 256) {
    const double s = score[(long)b * Q + j];
    const int q = index[(long)b * Q + j];
    sc[j] = s;
    on[j] = (s > min_score) && q >= 0 && q < Q;              // strict, float64 (visualiser.py:139); a NaN score is not painted
  }
  __syncthreads();
  for (int j = threadIdx.x; j < c; j += 256) {
    if (!on[j]) continue;
    const double s = sc[j];
    int rank = 0;
    for (int k = 0; k < c; ++k) rank += on[k] && (sc[k] > s || (sc[k] == s && k < j));
    order[(long)b * Q + rank] = make_int2(j, index[(long)b * Q + j]);
    atomicAdd(&n_on, 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) npaint[b] = n_on;
}

__device__ __forceinline__ void paint_blend(const PaintArgs& a, int b, long p, int id) {
  const unsigned char* img = a.packed + (long)a.desc[8 * b] * 16 + 3 * p;
  unsigned char* o = a.overlay + 3 * ((long)b * a.HW + p);
  if (id == 0) {
    o[0] = img[0]; o[1] = img[1]; o[2] = img[2];
    return;
  }
  const unsigned char* col = a.colours + 3 * ((long)b * a.Q + (id - 1));
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = (unsigned char)(((int)img[c] * (256 - a.alpha) + (int)col[c] * a.alpha + 128) >> 8);
}

template <bool BITS>
__global__ __launch_bounds__(256) void paint_ids_kernel(PaintArgs a) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const long word = __builtin_amdgcn_readfirstlane((int)(((long)blockIdx.x * 256 + threadIdx.x) >> 6));   // wave-uniform: 64 pixels = one word
  if (word >= a.W64) return;                                 // the last workgroup's waves past the image (wave-uniform)
  const long p = word * 64 + lane;
  const bool inside = p < a.HW;
  const int np = a.npaint[b];
  const int2* ord = a.order + (long)b * a.Q;
  int id = 0;
  for (int r0 = 0; r0 < np; r0 += 4) {
    if (__ballot(inside && id == 0) == 0) break;             // every lane has its top
    int2 sq[4];
    unsigned long long m[4];                                 // bit `lane` = this lane's pixel (BITS), or bit 0 (bytes)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sq[k] = ord[min(r0 + k, np - 1)];
      if (BITS) {
        m[k] = a.bits[((long)b * a.Q + sq[k].y) * a.W64 + word] >> lane;          // the tail word's bits past H*W are zero
      } else {
        m[k] = inside ? (a.masks[((long)b * a.Q + sq[k].y) * a.HW + p] != 0) : 0;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (r0 + k < np && id == 0 && (m[k] & 1)) id = sq[k].x + 1;
  }
  if (!inside) return;
  const long pix = (long)b * a.HW + p;
  if (a.ids_out) {
    if (a.rg16) {
      unsigned char* o = a.ids_out + 3 * pix;
      o[0] = (unsigned char)(id & 255); o[1] = (unsigned char)(id >> 8); o[2] = 0;
    } else {
      a.ids_out[pix] = (unsigned char)id;
    }
  }
  if (a.overlay) {
    if (a.outline) a.ids16[pix] = (unsigned short)id;
    else paint_blend(a, b, p, id);
  }
}

__global__ __launch_bounds__(256) void paint_overlay_kernel(PaintArgs a) {
  const int b = blockIdx.y;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.HW) return;
  const unsigned short* ids = a.ids16 + (long)b * a.HW;
  const int id = ids[p];
  if (id != 0) {
    const int y = (int)(p / a.W), x = (int)(p - (long)y * a.W);
    // a neighbour outside the image does not count; one inside with another top (or none) makes this an outline pixel
    const bool edge = (x > 0 && ids[p - 1] != id) || (x < a.W - 1 && ids[p + 1] != id) || (y > 0 && ids[p - a.W] != id) ||
                      (y < a.H - 1 && ids[p + a.W] != id);
    if (edge) {
      const unsigned char* col = a.colours + 3 * ((long)b * a.Q + (id - 1));
      unsigned char* o = a.overlay + 3 * ((long)b * a.HW + p);
      o[0] = col[0]; o[1] = col[1]; o[2] = col[2];
      return;
    }
  }
  paint_blend(a, b, p, id);
}

static size_t paint_tables_bytes(int B, int Q) { return (((size_t)B * Q * 8 + (size_t)B * 4) + 15) & ~(size_t)15; }

extern "C" size_t zh_instance_paint_workspace_size(int B, int Q, int H, int W) {
  if (B <= 0 || Q <= 0 || H <= 0 || W <= 0) return 0;
  return paint_tables_bytes(B, Q) + (size_t)B * H * W * 2;
}

extern "C" int zh_instance_paint(const unsigned char* masks, const unsigned long long* bits, const int* index, const double* score,
                                 const int* count, const unsigned char* colours, int alpha, int outline, double min_score,
                                 const unsigned char* packed, const int* desc, unsigned char* ids_out, int id_format,
                                 unsigned char* overlay_out, int B, int Q, int H, int W, void* workspace, size_t workspace_bytes,
                                 hipStream_t stream) {
  ZH_CHECK_ARG((masks || bits) && index && score && count && (ids_out || overlay_out) && B > 0 && B <= 65535 && Q > 0 && H > 0 && W > 0 &&
               (long)H * W < (1L << 31) && (id_format == ZH_GT_U8 || id_format == ZH_GT_RG16) && (outline == 0 || outline == 1),
               "zh_instance_paint: bad arguments");
  ZH_CHECK_ARG(Q <= ZH_PAINT_MAX_Q, "zh_instance_paint: at most %d slots per image (the rank table lives in LDS)", ZH_PAINT_MAX_Q);
  ZH_CHECK_ARG(!ids_out || id_format == ZH_GT_RG16 || Q <= 255, "zh_instance_paint: ids up to %d do not fit one byte: use the rg16 format", Q);
  ZH_CHECK_ARG(!overlay_out || (colours && packed && desc && alpha >= 0 && alpha <= 256),
               "zh_instance_paint: an overlay needs colours, packed, desc and alpha in 0..256");
  if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < zh_instance_paint_workspace_size(B, Q, H, W)) {
    zh_set_error("zh_instance_paint: workspace too small or not 16-byte aligned");
    return ZH_ERR_WORKSPACE;
  }
  const long HW = (long)H * W;
  int2* order = (int2*)workspace;
  int* npaint = (int*)((char*)workspace + (size_t)B * Q * 8);
  unsigned short* ids16 = (unsigned short*)((char*)workspace + paint_tables_bytes(B, Q));
  hipLaunchKernelGGL(paint_rank_kernel, dim3(B), dim3(256), 0, stream, index, score, count, min_score, Q, order, npaint);
  const PaintArgs a{masks, bits, order, npaint, colours, packed, desc, ids_out, overlay_out, ids16, HW, (HW + 63) / 64,
                    Q, H, W, alpha, id_format == ZH_GT_RG16, outline};
  const dim3 grid(zh_cdiv(HW, 256), B);
  if (bits) hipLaunchKernelGGL(paint_ids_kernel<true>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(paint_ids_kernel<false>, grid, dim3(256), 0, stream, a);
  if (overlay_out && outline) hipLaunchKernelGGL(paint_overlay_kernel, grid, dim3(256), 0, stream, a);
  ZH_CHECK_LAUNCH("zh_instance_paint");
  return ZH_OK;
}
