// Device JPEG encoder (zutis_amd/jpeg_device.py encode_np / scan_np is the definition; the arithmetic is jpeg_codec.h's, which
// jpeg_host.hip's zh_jpeg_encode_host compiles for the CPU): the photographic pictures the file drivers write — the overlays — leave the
// GPU as the entropy-coded scan of a baseline JPEG, so that a writer thread only puts the header in front and FF D9 behind.
//
//   zh_jpeg_encode   launch A, one lane per 8 x 8 block of the scan: colour conversion, edge replication, h2v2 downsampling, forward DCT,
//                      quantisation and the dummy-block rule (jpeg_enc_block) -> 64 zig-zag int16 in the workspace, blocks in scan order.
//                    launch B, one workgroup per restart interval (ZH_JPEG_ENC_INTERVAL_MCUS MCUs), a wave per block, a lane per zig-zag
//                    position:
//                      1. the ballot of the nonzero AC positions gives every lane its run, hence its ZRLs, symbol and bit count
//                         (jpeg_enc_token); the DC lane takes the previous block of its component inside the interval;
//                      2. a wave scan gives the lane's bit offset inside the block, a scan over the blocks' sums the block's offset;
//                      3. the same tokens again, ORed into zeroed LDS words at their offsets (LDS atomics: order-independent);
//                      4. the last byte filled with 1-bits; each lane counts the FF of its share of the bytes, a scan of the counts gives
//                         the stuffed position; the bytes go to the interval's worst-case slot in the workspace with their count.
//                    launch C, one workgroup per interval again: the lengths of the intervals in front of it (and their markers), the
//                    slot copied to its place in the picture's scan, RSTn behind it; the last one stores the length.  Only bytes below
//                    slot_bytes are written; the length is the true one.
//
// An image that does not fit (jpeg_enc_image) is not read and nothing of its scan is written; its length is -1.  Every index is derived
// from checked sizes; every loop is bounded by them and by the header's constants.
#include "common.h"
#include "jpeg_codec.h"

#define JENC_THREADS 256
#define JENC_WAVES (JENC_THREADS / 64)
#define JENC_MAX_BLOCKS (ZH_JPEG_ENC_INTERVAL_MCUS * 6)                       // an interval of 4:2:0 MCUs
#define JENC_MAX_BYTES (JENC_MAX_BLOCKS * ZH_JPEG_ENC_BLOCK_BYTES)            // its bits before stuffing: 19968 bytes of LDS

static_assert(JENC_MAX_BLOCKS <= JENC_THREADS, "the scan over an interval's blocks has one lane per block");
static_assert(8 * ZH_JPEG_ENC_BLOCK_BYTES >= JPEG_ENC_BLOCK_BITS && ZH_JPEG_ENC_BLOCK_BYTES % 16 == 0, "a block's worst case fits its bytes; slots stay 16-byte aligned");

struct JencLayout { long coef_stride, slot_stride; int max_int, iv_slot; };     // per image: int16 coefficients, bytes of interval slots

__host__ __device__ inline JencLayout jenc_layout(long max_mcus, int sub) {
  JencLayout L;
  const int bpm = sub == 2 ? 6 : 3;
  L.max_int = (int)jpeg_enc_intervals(max_mcus);
  L.iv_slot = 2 * ZH_JPEG_ENC_INTERVAL_MCUS * bpm * ZH_JPEG_ENC_BLOCK_BYTES;
  L.coef_stride = max_mcus * bpm * 64;
  L.slot_stride = (long)L.max_int * L.iv_slot;
  return L;
}

__global__ __launch_bounds__(JENC_THREADS) void jenc_coef_kernel(const unsigned char* images, long image_bytes, const long long* img_off, const int* hw,
                                                                 int sub, long max_mcus, const unsigned short* quant, const long long* out_off,
                                                                 long out_bytes, long slot_bytes, short* coef) {
  __shared__ unsigned short s_q[128];
  const int b = blockIdx.y;
  if (threadIdx.x < 128) s_q[threadIdx.x] = quant[threadIdx.x];
  __syncthreads();
  const JpegEncImage im = jpeg_enc_image(img_off, hw, out_off, b, sub, image_bytes, out_bytes, slot_bytes, max_mcus);
  const long i = (long)blockIdx.x * JENC_THREADS + threadIdx.x;
  if (!im.ok || i >= im.mcus * im.bpm) return;
  short zz[64];
  jpeg_enc_block(im, images + im.off, s_q, i / im.bpm, (int)(i % im.bpm), zz);
  uint4* dst = (uint4*)(coef + (long)b * jenc_layout(max_mcus, sub).coef_stride + i * 64);      // 128 bytes a block, 16-byte aligned
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    uint4 o;
    o.x = (unsigned short)zz[8 * v] | (unsigned)(unsigned short)zz[8 * v + 1] << 16;
    o.y = (unsigned short)zz[8 * v + 2] | (unsigned)(unsigned short)zz[8 * v + 3] << 16;
    o.z = (unsigned short)zz[8 * v + 4] | (unsigned)(unsigned short)zz[8 * v + 5] << 16;
    o.w = (unsigned short)zz[8 * v + 6] | (unsigned)(unsigned short)zz[8 * v + 7] << 16;
    dst[v] = o;
  }
}

// the token of this lane's zig-zag position of block i of the interval (c: the interval's first coefficient) and the wave's inclusive scan of the bit counts
__device__ __forceinline__ int jenc_lane_token(const unsigned* s_tab, const short* c, int i, int bpm, int lum, int lane, unsigned long long* val, int* incl) {
  int v = c[i * 64 + lane];
  const unsigned long long nz = __ballot(lane > 0 && v != 0);
  if (lane == 0) {
    const int from = jpeg_enc_dc_from(i, bpm, lum);
    v -= from < 0 ? 0 : (int)c[from * 64];
  }
  const int n = jpeg_enc_token(s_tab, i % bpm >= lum, lane, v, nz, val);
  int s = n;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(s, o, 64);
    if (lane >= o) s += t;
  }
  *incl = s;
  return n;
}

__global__ __launch_bounds__(JENC_THREADS) void jenc_entropy_kernel(long image_bytes, const long long* img_off, const int* hw, int sub, long max_mcus,
                                                                    const long long* out_off, long out_bytes, long slot_bytes, const short* coef,
                                                                    unsigned char* slots, int* lens) {
  __shared__ unsigned s_tab[4 * JPEG_ENC_TABLE_WORDS];
  __shared__ unsigned s_words[JENC_MAX_BYTES / 4];
  __shared__ int s_scan[JENC_THREADS];
  const int b = blockIdx.y, iv = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const JpegEncImage im = jpeg_enc_image(img_off, hw, out_off, b, sub, image_bytes, out_bytes, slot_bytes, max_mcus);
  if (!im.ok || iv >= im.nint) return;                                      // block-uniform, in front of every barrier
  const JencLayout L = jenc_layout(max_mcus, sub);
  const long mcu0 = (long)iv * ZH_JPEG_ENC_INTERVAL_MCUS, left = im.mcus - mcu0;
  const int nb = (int)(left < ZH_JPEG_ENC_INTERVAL_MCUS ? left : ZH_JPEG_ENC_INTERVAL_MCUS) * im.bpm;       // 1 .. JENC_MAX_BLOCKS
  const short* c = coef + (long)b * L.coef_stride + mcu0 * im.bpm * 64;
  if (tid < 4) jpeg_enc_tables(tid, s_tab + tid * JPEG_ENC_TABLE_WORDS);
  for (int w = tid; w < nb * (ZH_JPEG_ENC_BLOCK_BYTES / 4); w += JENC_THREADS) s_words[w] = 0u;
  s_scan[tid] = 0;
  __syncthreads();
  // 1, 2. every block's bit count, then the blocks' offsets
  for (int i = wave; i < nb; i += JENC_WAVES) {
    unsigned long long val;
    int incl;
    jenc_lane_token(s_tab, c, i, im.bpm, im.lum, lane, &val, &incl);
    if (lane == 63) s_scan[i] = incl;
  }
  __syncthreads();
  for (int o = 1; o < JENC_THREADS; o <<= 1) {
    const int a = tid >= o ? s_scan[tid - o] : 0;
    __syncthreads();
    s_scan[tid] += a;
    __syncthreads();
  }
  const unsigned bits = (unsigned)s_scan[JENC_THREADS - 1];                  // <= nb * JPEG_ENC_BLOCK_BITS
  // 3. the tokens into the words
  for (int i = wave; i < nb; i += JENC_WAVES) {
    unsigned long long val;
    int incl;
    const int n = jenc_lane_token(s_tab, c, i, im.bpm, im.lum, lane, &val, &incl);
    jpeg_enc_put(s_words, (unsigned)(i ? s_scan[i - 1] : 0) + (unsigned)(incl - n), val, n);
  }
  if (tid == 0 && (bits & 7u)) { const int pad = 8 - (int)(bits & 7u); jpeg_enc_put(s_words, bits, (1ull << pad) - 1ull, pad); }
  __syncthreads();
  // 4. stuffing: lane t owns bytes [t per, (t + 1) per)
  const int nbytes = (int)((bits + 7u) >> 3), per = (nbytes + JENC_THREADS - 1) / JENC_THREADS;
  const int lo = min(nbytes, tid * per), hi = min(nbytes, lo + per);
  int ff = 0;
  for (int i = lo; i < hi; ++i) ff += jpeg_enc_byte(s_words, i) == 0xFFu;
  __syncthreads();                                                          // every s_scan read above is done
  s_scan[tid] = ff;
  __syncthreads();
  for (int o = 1; o < JENC_THREADS; o <<= 1) {
    const int a = tid >= o ? s_scan[tid - o] : 0;
    __syncthreads();
    s_scan[tid] += a;
    __syncthreads();
  }
  unsigned char* dst = slots + (long)b * L.slot_stride + (long)iv * L.iv_slot;      // nbytes <= iv_slot / 2, so the stuffed bytes fit
  int at = lo + s_scan[tid] - ff;
  for (int i = lo; i < hi; ++i) {
    const unsigned v = jpeg_enc_byte(s_words, i);
    dst[at++] = (unsigned char)v;
    if (v == 0xFFu) dst[at++] = 0;
  }
  if (tid == 0) lens[(long)b * L.max_int + iv] = nbytes + s_scan[JENC_THREADS - 1];
}

__global__ __launch_bounds__(JENC_THREADS) void jenc_gather_kernel(long image_bytes, const long long* img_off, const int* hw, int sub, long max_mcus,
                                                                   const long long* out_off, long out_bytes, long slot_bytes, const unsigned char* slots,
                                                                   const int* lens, unsigned char* out, int* lengths) {
  __shared__ long long s_r[JENC_THREADS];
  const int b = blockIdx.y, iv = blockIdx.x, tid = threadIdx.x;
  const JpegEncImage im = jpeg_enc_image(img_off, hw, out_off, b, sub, image_bytes, out_bytes, slot_bytes, max_mcus);
  if (!im.ok) {
    if (iv == 0 && tid == 0) lengths[b] = -1;
    return;
  }
  if (iv >= im.nint) return;
  const JencLayout L = jenc_layout(max_mcus, sub);
  const int* ln = lens + (long)b * L.max_int;
  long long front = 0;
  for (int j = tid; j < iv; j += JENC_THREADS) front += ln[j] + 2;           // an interval and the marker behind it
  s_r[tid] = front;
  __syncthreads();
  for (int o = JENC_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) s_r[tid] += s_r[tid + o];
    __syncthreads();
  }
  front = s_r[0];
  const int n = ln[iv];
  if (n < 1 || n > L.iv_slot) return;                                       // (never: the entropy launch wrote it)
  const unsigned char* src = slots + (long)b * L.slot_stride + (long)iv * L.iv_slot;
  unsigned char* dst = out + im.out;
  for (int i = tid; i < n; i += JENC_THREADS)
    if (front + i < slot_bytes) dst[front + i] = src[i];
  const bool last = iv == im.nint - 1;
  if (!last && tid < 2 && front + n + tid < slot_bytes) dst[front + n + tid] = tid == 0 ? 0xFF : (unsigned char)(0xD0 + (iv & 7));
  if (last && tid == 0) lengths[b] = (int)(front + n);
}

extern "C" size_t zh_jpeg_encode_workspace_size(int B, long max_mcus, int subsampling) {
  if (B < 1 || max_mcus < 1 || max_mcus > (1L << 26) || (subsampling != 0 && subsampling != 2)) return 0;
  const JencLayout L = jenc_layout(max_mcus, subsampling);
  return (size_t)B * ((size_t)L.coef_stride * sizeof(short) + (size_t)L.slot_stride + (size_t)L.max_int * sizeof(int));
}

extern "C" int zh_jpeg_encode(const unsigned char* images, long image_bytes, const long long* img_off, const int* hw, int B, int subsampling,
                              long max_mcus, const unsigned short* quant, const long long* out_off, unsigned char* out, long out_bytes,
                              long slot_bytes, int* lengths, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  ZH_CHECK_ARG(B >= 0 && B <= 65535, "zh_jpeg_encode: B = %d outside 0 .. 65535", B);
  ZH_CHECK_ARG(subsampling == 0 || subsampling == 2, "zh_jpeg_encode: subsampling = %d is not 0 (4:4:4) or 2 (4:2:0)", subsampling);
  ZH_CHECK_ARG(image_bytes >= 0 && out_bytes >= 0 && slot_bytes >= 0 && max_mcus >= 0, "zh_jpeg_encode: negative count");
  if (B == 0) return ZH_OK;
  ZH_CHECK_ARG(max_mcus >= 1 && max_mcus <= (1L << 26), "zh_jpeg_encode: max_mcus = %ld outside 1 .. 2^26", max_mcus);
  ZH_CHECK_ARG(images && img_off && hw && quant && out_off && out && lengths && workspace, "zh_jpeg_encode: null pointer");
  ZH_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "zh_jpeg_encode: workspace must be 16-byte aligned");
  if (workspace_bytes < zh_jpeg_encode_workspace_size(B, max_mcus, subsampling)) {
    zh_set_error("zh_jpeg_encode: workspace holds %zu bytes, %zu needed", workspace_bytes, zh_jpeg_encode_workspace_size(B, max_mcus, subsampling));
    return ZH_ERR_WORKSPACE;
  }
  const JencLayout L = jenc_layout(max_mcus, subsampling);
  const long blocks = L.coef_stride / 64;
  ZH_CHECK_ARG((blocks + JENC_THREADS - 1) / JENC_THREADS <= 0x7fffffffL, "zh_jpeg_encode: max_mcus = %ld: too many blocks for one grid", max_mcus);
  // coefficients first (128 bytes a block), the interval slots behind them (multiples of 16 bytes), the interval lengths last
  short* coef = (short*)workspace;
  unsigned char* slots = (unsigned char*)(coef + (size_t)B * L.coef_stride);
  int* lens = (int*)(slots + (size_t)B * L.slot_stride);
  hipLaunchKernelGGL(jenc_coef_kernel, dim3((unsigned)((blocks + JENC_THREADS - 1) / JENC_THREADS), B), dim3(JENC_THREADS), 0, stream, images, image_bytes,
                     img_off, hw, subsampling, max_mcus, quant, out_off, out_bytes, slot_bytes, coef);
  ZH_CHECK_LAUNCH("zh_jpeg_encode (coefficients)");
  hipLaunchKernelGGL(jenc_entropy_kernel, dim3(L.max_int, B), dim3(JENC_THREADS), 0, stream, image_bytes, img_off, hw, subsampling, max_mcus, out_off,
                     out_bytes, slot_bytes, (const short*)coef, slots, lens);
  ZH_CHECK_LAUNCH("zh_jpeg_encode (entropy)");
  hipLaunchKernelGGL(jenc_gather_kernel, dim3(L.max_int, B), dim3(JENC_THREADS), 0, stream, image_bytes, img_off, hw, subsampling, max_mcus, out_off,
                     out_bytes, slot_bytes, (const unsigned char*)slots, (const int*)lens, out, lengths);
  ZH_CHECK_LAUNCH("zh_jpeg_encode (gather)");
  return ZH_OK;
}
