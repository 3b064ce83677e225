// Device JPEG decoder (zutis_amd/jpeg_device.py is the definition, jpeg_codec.h the codec): baseline JPEG files cross PCIe as their file
// bytes and become interleaved RGB on the device, byte for byte what Pillow decodes on the host.
//
//   zh_jpeg_decode   fill: status and the workspace's MCU counters and coefficients to zero;
//                    launch A, one LANE per entropy segment (64 to a workgroup, the segments sorted by length so that a wave's lanes
//                      finish together): the launch's table sets are copied to LDS, then every lane runs jpeg_step — one Huffman symbol
//                      per iteration, the table picked by arithmetic on the lane's (block, coefficient) state — at most 64 x its blocks
//                      times; coefficients go to the workspace in natural order, a lane that finished clean adds its MCUs to its
//                      image's counter, any other ORs its status bits into status[image];
//                    launch B, one lane per 8 x 8 block: dequantise + islow inverse DCT from registers into the image's sample planes;
//                    launch C, one lane per output pixel: fancy chroma upsampling of the cropped planes + YCbCr -> RGB at the output
//                      offset of the image's row; its first lane sets INCOMPLETE when the counter is not the image's MCU count.
//
// Every index comes from a checked row (jpeg_image, jpeg_segment); an image whose row fails gets DESCRIPTOR and none of its bytes is
// read or written.
#include "common.h"
#include "jpeg_codec.h"

#define JPEG_ENTROPY_THREADS 64
#define JPEG_THREADS 256
#define JPEG_SET_WORDS (JPEG_HUFF_SET_BYTES / 4)

static_assert(ZH_JPEG_TABLE_SET_BYTES == JPEG_HUFF_SET_BYTES + 2 * 64 * 2, "a table set: four Huffman tables, two u16 quantisation tables");
static_assert(ZH_JPEG_HUFF_TABLE_BYTES == JPEG_T_VALS + 256 && ZH_JPEG_HUFF_TABLE_BYTES % 4 == 0, "a Huffman table: look, maxcode, valoff, vals");
static_assert(ZH_JPEG_MAX_TABLE_SETS * JPEG_HUFF_SET_BYTES <= 64 * 1024, "the launch's table sets live in LDS");

// the image row with the launch's grid widths checked as well
__device__ __forceinline__ JpegImage jpeg_image_dev(const int* images, int b, int n_sets, long n_blocks, long out_bytes, long max_image_blocks,
                                                    long max_image_pixels) {
  JpegImage im = jpeg_image(images + (long)b * ZH_JPEG_IMAGE_WORDS, n_sets, n_blocks, out_bytes);
  if (im.ok && (im.nblocks > max_image_blocks || (long)im.w * im.h > max_image_pixels)) im.ok = false;
  return im;
}

__global__ __launch_bounds__(JPEG_ENTROPY_THREADS) void jpeg_entropy_kernel(const unsigned char* scan, long scan_bytes, const int* segments,
                                                                            int n_segments, const int* images, int B, const unsigned char* tables,
                                                                            int n_sets, long n_blocks, long out_bytes, long max_image_blocks,
                                                                            long max_image_pixels, short* coef, int* counters, int* status) {
  __shared__ unsigned s_tab[ZH_JPEG_MAX_TABLE_SETS * JPEG_SET_WORDS];
  const int tid = threadIdx.x;
  for (int i = tid; i < n_sets * JPEG_SET_WORDS; i += JPEG_ENTROPY_THREADS) {
    const int set = i / JPEG_SET_WORDS, w = i - set * JPEG_SET_WORDS;
    s_tab[i] = ((const unsigned*)(tables + (long)set * ZH_JPEG_TABLE_SET_BYTES))[w];
  }
  __syncthreads();
  const long sg = (long)blockIdx.x * JPEG_ENTROPY_THREADS + tid;
  if (sg >= n_segments) return;
  const int* row = segments + sg * ZH_JPEG_SEGMENT_WORDS;
  const int b = row[0];
  if (b < 0 || b >= B) return;                                              // no image to report to
  const JpegImage im = jpeg_image_dev(images, b, n_sets, n_blocks, out_bytes, max_image_blocks, max_image_pixels);
  if (!im.ok) return;                                                       // launch C reports it
  JpegSegment s;
  int st;
  if (!jpeg_segment(row, im, scan, scan_bytes, s, &st)) { atomicOr(&status[b], st); return; }
  const unsigned char* huff = (const unsigned char*)(s_tab + im.tset * JPEG_SET_WORDS);
  short* c0 = coef + im.block0 * 64;
  const int mcus = s.mcu_end - s.mcu;
  const long steps = jpeg_segment_steps(s, im);
  for (long it = 0; it < steps && !jpeg_segment_done(s); ++it) jpeg_step(s, im, huff, c0);
  if (s.bits.status) atomicOr(&status[b], s.bits.status);
  else if (s.mcu >= s.mcu_end) atomicAdd(&counters[b], mcus);
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_idct_kernel(const int* images, const unsigned char* tables, int n_sets, long n_blocks,
                                                                 long out_bytes, long max_image_blocks, long max_image_pixels, const short* coef,
                                                                 unsigned char* samples) {
  const int b = blockIdx.y;
  const long j = (long)blockIdx.x * JPEG_THREADS + threadIdx.x;
  const JpegImage im = jpeg_image_dev(images, b, n_sets, n_blocks, out_bytes, max_image_blocks, max_image_pixels);
  if (!im.ok || j >= im.nblocks) return;
  long ld;
  int cls;
  const long at = jpeg_block_place(im, j, &ld, &cls);
  const unsigned short* q = (const unsigned short*)(tables + (long)im.tset * ZH_JPEG_TABLE_SET_BYTES + JPEG_HUFF_SET_BYTES) + 64 * cls;
  jpeg_idct_block(coef + (im.block0 + j) * 64, q, samples + im.block0 * 64 + at, ld);
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_colour_kernel(const int* images, int n_sets, long n_blocks, long out_bytes, long max_image_blocks,
                                                                   long max_image_pixels, const unsigned char* samples, const int* counters,
                                                                   unsigned char* out, int* status) {
  const int b = blockIdx.y;
  const long p = (long)blockIdx.x * JPEG_THREADS + threadIdx.x;
  const JpegImage im = jpeg_image_dev(images, b, n_sets, n_blocks, out_bytes, max_image_blocks, max_image_pixels);
  if (!im.ok) {
    if (p == 0) atomicOr(&status[b], ZH_JPEG_STATUS_DESCRIPTOR);
    return;
  }
  if (p == 0 && counters[b] != im.mcux * im.mcuy) atomicOr(&status[b], ZH_JPEG_STATUS_INCOMPLETE);
  if (p >= (long)im.w * im.h) return;
  const int y = (int)(p / im.w), x = (int)(p - (long)y * im.w);
  unsigned char rgb[3];
  jpeg_pixel(im, samples + im.block0 * 64, x, y, rgb);
  unsigned char* dst = out + im.out + 3 * p;
  dst[0] = rgb[0]; dst[1] = rgb[1]; dst[2] = rgb[2];
}

static size_t jpeg_counter_bytes(int B) { return ((size_t)B * sizeof(int) + 15) / 16 * 16; }

extern "C" size_t zh_jpeg_decode_workspace_size(int B, long n_blocks) {
  if (B < 1 || n_blocks < 1) return 0;
  return jpeg_counter_bytes(B) + (size_t)n_blocks * 64 * (sizeof(short) + 1);
}

extern "C" int zh_jpeg_decode(const unsigned char* scan, long scan_bytes, const int* segments, int n_segments, const int* images, int B,
                              const unsigned char* tables, int n_sets, long n_blocks, long max_image_blocks, long max_image_pixels,
                              unsigned char* out, long out_bytes, int* status, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  ZH_CHECK_ARG(B >= 0 && B <= 65535, "zh_jpeg_decode: B = %d outside 0 .. 65535", B);
  if (B == 0) return ZH_OK;
  ZH_CHECK_ARG(scan_bytes >= 0 && scan_bytes <= 0x7fffffffL && out_bytes >= 0, "zh_jpeg_decode: scan_bytes / out_bytes outside 0 .. 2^31 - 1 / negative");
  ZH_CHECK_ARG(n_segments >= 0 && n_segments <= ZH_JPEG_MAX_SEGMENTS, "zh_jpeg_decode: n_segments = %d outside 0 .. %d", n_segments, ZH_JPEG_MAX_SEGMENTS);
  ZH_CHECK_ARG(n_sets >= 1 && n_sets <= ZH_JPEG_MAX_TABLE_SETS, "zh_jpeg_decode: n_sets = %d outside 1 .. %d", n_sets, ZH_JPEG_MAX_TABLE_SETS);
  ZH_CHECK_ARG(n_blocks >= 1 && n_blocks < (1L << 24), "zh_jpeg_decode: n_blocks = %ld outside 1 .. 2^24 - 1", n_blocks);
  ZH_CHECK_ARG(max_image_blocks >= 1 && max_image_blocks <= n_blocks && max_image_pixels >= 1 && max_image_pixels <= 64 * n_blocks,
               "zh_jpeg_decode: max_image_blocks = %ld / max_image_pixels = %ld do not go with n_blocks = %ld", max_image_blocks, max_image_pixels, n_blocks);
  ZH_CHECK_ARG(scan && segments && images && tables && out && status && workspace, "zh_jpeg_decode: null pointer");
  ZH_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)tables & 3) == 0, "zh_jpeg_decode: workspace must be 16-byte, tables 4-byte aligned");
  if (workspace_bytes < zh_jpeg_decode_workspace_size(B, n_blocks)) {
    zh_set_error("zh_jpeg_decode: workspace holds %zu bytes, %zu needed", workspace_bytes, zh_jpeg_decode_workspace_size(B, n_blocks));
    return ZH_ERR_WORKSPACE;
  }
  int* counters = (int*)workspace;
  short* coef = (short*)((unsigned char*)workspace + jpeg_counter_bytes(B));
  unsigned char* samples = (unsigned char*)(coef + n_blocks * 64);
  if (hipMemsetAsync(status, 0, (size_t)B * sizeof(int), stream) != hipSuccess ||
      hipMemsetAsync(workspace, 0, jpeg_counter_bytes(B) + (size_t)n_blocks * 64 * sizeof(short), stream) != hipSuccess) {
    zh_set_error("zh_jpeg_decode: fill failed: %s", hipGetErrorString(hipGetLastError()));
    return ZH_ERR_HIP;
  }
  if (n_segments > 0) {
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(zh_cdiv(n_segments, JPEG_ENTROPY_THREADS)), dim3(JPEG_ENTROPY_THREADS), 0, stream, scan, scan_bytes,
                       segments, n_segments, images, B, tables, n_sets, n_blocks, out_bytes, max_image_blocks, max_image_pixels, coef, counters, status);
    ZH_CHECK_LAUNCH("zh_jpeg_decode (entropy)");
  }
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3(zh_cdiv(max_image_blocks, JPEG_THREADS), B), dim3(JPEG_THREADS), 0, stream, images, tables, n_sets, n_blocks,
                     out_bytes, max_image_blocks, max_image_pixels, (const short*)coef, samples);
  ZH_CHECK_LAUNCH("zh_jpeg_decode (inverse DCT)");
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3(zh_cdiv(max_image_pixels, JPEG_THREADS), B), dim3(JPEG_THREADS), 0, stream, images, n_sets, n_blocks,
                     out_bytes, max_image_blocks, max_image_pixels, (const unsigned char*)samples, (const int*)counters, out, status);
  ZH_CHECK_LAUNCH("zh_jpeg_decode (colour)");
  return ZH_OK;
}

// ---- zh_jpeg_decode_split: the entropy stage of a segment split among lanes (include/zutis_hip.h has the method, jpeg_codec.h the
// functions, jpeg_host.hip the same passes on the CPU).  One workgroup of JPEG_SPLIT_THREADS lanes owns a SEQUENCE of that many chunk
// rows in every kernel; workgroups exchange nothing inside a launch.
//   jpeg_sync_kernel    x passes: lane i decodes its chunk leniently from the state lane i - 1 handed it, round after round until no
//                       state of the sequence changes (at most one round per lane: lane i is final after round i); states, block counts
//                       and the sequence's last state (two slots, written in turn: the next launch reads what this one does not write)
//   jpeg_count_kernel   segmented scan of the block counts inside a sequence; jpeg_carry_kernel: the same scan over the sequences' sums
//   jpeg_strict_kernel  one lane per chunk: the row's unstuffed count checked against the bytes, jpeg_step from the state the passes
//                       left, coefficients with DC differences, status bits, the hand-over check, the MCU counter
//   jpeg_dc_kernel      one workgroup per segment: every lane sums the DC differences of a run of MCUs per component, the sums are
//                       scanned in LDS, the lane walks its run again with its carry
#define JPEG_SPLIT_THREADS ZH_JPEG_SPLIT_LANES
static_assert(ZH_JPEG_MAX_TABLE_SETS * JPEG_HUFF_SET_BYTES + JPEG_SPLIT_THREADS * 2 * (int)sizeof(JpegState) <= 64 * 1024, "tables and states live in LDS");
static_assert(ZH_JPEG_CHUNK_WORDS == 4 && ZH_JPEG_CHUNK_BYTES % 16 == 0 && ZH_JPEG_CHUNK_BYTES >= ZH_JPEG_CHUNK_BYTES_MIN && ZH_JPEG_CHUNK_BYTES <= 4096,
              "a chunk row: segment, first byte, unstuffed bits, first flag; the shipped chunk size is one the entry accepts");

__device__ __forceinline__ void jpeg_tables_to_lds(unsigned* s_tab, const unsigned char* tables, int n_sets) {
  for (int i = threadIdx.x; i < n_sets * JPEG_SET_WORDS; i += JPEG_SPLIT_THREADS) {
    const int set = i / JPEG_SET_WORDS, w = i - set * JPEG_SET_WORDS;
    s_tab[i] = ((const unsigned*)(tables + (long)set * ZH_JPEG_TABLE_SET_BYTES))[w];
  }
  __syncthreads();
}

__global__ __launch_bounds__(JPEG_SPLIT_THREADS) void jpeg_sync_kernel(JpegLaunch L, const unsigned char* tables, int pass, long n_seq, JpegState* st_in,
                                                                       JpegState* st_out, int* cnt, JpegState* hand) {
  __shared__ unsigned s_tab[ZH_JPEG_MAX_TABLE_SETS * JPEG_SET_WORDS];
  __shared__ JpegState s_out[JPEG_SPLIT_THREADS];
  jpeg_tables_to_lds(s_tab, tables, L.n_sets);
  const int t = threadIdx.x;
  const long w = blockIdx.x, i = w * JPEG_SPLIT_THREADS + t;
  JpegChunk c; JpegImage im; JpegSegment s;
  int b, n = 0;
  const bool ok = i < L.n_chunks && jpeg_chunk(L, i, c, im, s, &b) == 0, chained = ok && !c.first;
  JpegState in = {ok ? c.ubits : 0, 0}, out = in;
  bool dirty = ok;
  if (pass > 0 && ok) {
    in = st_in[i]; out = st_out[i]; n = cnt[i];
    dirty = false;
    if (t == 0 && chained && w > 0) {
      const JpegState h = hand[((pass - 1) & 1) * n_seq + w - 1];
      dirty = !jpeg_state_equal(h, in);
      in = h;
    }
  }
  const unsigned char* huff = (const unsigned char*)(s_tab + (ok ? im.tset : 0) * JPEG_SET_WORDS);
  for (int round = 0; round < JPEG_SPLIT_THREADS; ++round) {
    if (dirty) out = jpeg_chunk_lenient(L.scan, s.bits.end, c, im, huff, in, &n);
    s_out[t] = out;
    __syncthreads();
    dirty = false;
    if (chained && t > 0) {
      const JpegState p = s_out[t - 1];
      dirty = !jpeg_state_equal(p, in);
      in = p;
    }
    if (!__syncthreads_or(dirty)) break;
  }
  if (i < L.n_chunks) { st_in[i] = in; st_out[i] = out; cnt[i] = n; }
  if (i == L.n_chunks - 1 || (t == JPEG_SPLIT_THREADS - 1 && i < L.n_chunks)) hand[(pass & 1) * n_seq + w] = out;
}

// inclusive segmented sum over the workgroup's 256 lanes: f marks a lane that starts a segment; afterwards v is the sum since the last
// start at or in front of the lane, f whether there is one
__device__ __forceinline__ void jpeg_segmented_scan(int* s_v, int* s_f, int& v, int& f) {
  const int t = threadIdx.x;
  for (int d = 1; d < JPEG_SPLIT_THREADS; d <<= 1) {
    s_v[t] = v; s_f[t] = f;
    __syncthreads();
    if (t >= d) {
      if (!f) v = jpeg_block_sum(v, s_v[t - d]);
      f |= s_f[t - d];
    }
    __syncthreads();
  }
}

#define JPEG_FIRST_OPEN (1 << 30)      // the chunk's segment starts in an earlier sequence: the sequence's carry is added

__global__ __launch_bounds__(JPEG_SPLIT_THREADS) void jpeg_count_kernel(const int* chunks, long n_chunks, const int* cnt, int* first, int* seq_sum,
                                                                        int* seq_start) {
  __shared__ int s_v[JPEG_SPLIT_THREADS], s_f[JPEG_SPLIT_THREADS];
  const int t = threadIdx.x;
  const long i = (long)blockIdx.x * JPEG_SPLIT_THREADS + t;
  const int own = i < n_chunks ? cnt[i] : 0, start = i < n_chunks && chunks[i * ZH_JPEG_CHUNK_WORDS + 3] == 1;
  int v = own, f = start;
  jpeg_segmented_scan(s_v, s_f, v, f);
  s_v[t] = v; s_f[t] = f;
  __syncthreads();
  if (i < n_chunks) first[i] = start ? 0 : t == 0 ? JPEG_FIRST_OPEN : s_v[t - 1] | (s_f[t - 1] ? 0 : JPEG_FIRST_OPEN);
  if (t == JPEG_SPLIT_THREADS - 1) { seq_sum[blockIdx.x] = v; seq_start[blockIdx.x] = f; }
}

// one workgroup: carry[w] = the blocks the sequences in front of w add to a segment that is still open where w begins
__global__ __launch_bounds__(JPEG_SPLIT_THREADS) void jpeg_carry_kernel(const int* seq_sum, const int* seq_start, long n_seq, int* carry) {
  __shared__ int s_v[JPEG_SPLIT_THREADS], s_f[JPEG_SPLIT_THREADS];
  const int t = threadIdx.x;
  int run = 0;                                                        // the open sum in front of this group of 256 sequences
  for (long w0 = 0; w0 < n_seq; w0 += JPEG_SPLIT_THREADS) {
    const long w = w0 + t;
    int v = w < n_seq ? seq_sum[w] : 0, f = w < n_seq ? seq_start[w] : 0;
    jpeg_segmented_scan(s_v, s_f, v, f);
    v = f ? v : jpeg_block_sum(v, run);
    s_v[t] = v;
    __syncthreads();
    if (w < n_seq) carry[w] = t == 0 ? run : s_v[t - 1];
    run = s_v[JPEG_SPLIT_THREADS - 1];
    __syncthreads();
  }
}

__global__ __launch_bounds__(JPEG_SPLIT_THREADS) void jpeg_strict_kernel(JpegLaunch L, const unsigned char* tables, const JpegState* st_in, const int* cnt,
                                                                         const int* first, const int* carry, short* coef, int* counters, int* status) {
  __shared__ unsigned s_tab[ZH_JPEG_MAX_TABLE_SETS * JPEG_SET_WORDS];
  jpeg_tables_to_lds(s_tab, tables, L.n_sets);
  const long i = (long)blockIdx.x * JPEG_SPLIT_THREADS + threadIdx.x;
  if (i >= L.n_chunks) return;
  JpegChunk c; JpegImage im; JpegSegment s;
  int b, mcus;
  const int rc = jpeg_chunk(L, i, c, im, s, &b);
  if (rc < 0) return;
  if (rc > 0 || (!c.last && c.ubits + 8 * (int)(c.end - c.start - jpeg_chunk_pairs(L.scan, c, s.bits.end)) != c.uend)) {
    atomicOr(&status[b], ZH_JPEG_STATUS_DESCRIPTOR);
    return;
  }
  const int f = first[i], first_block = f & JPEG_FIRST_OPEN ? jpeg_block_sum(f & ~JPEG_FIRST_OPEN, carry[blockIdx.x]) : f;
  const JpegState pinned = {0, 0}, in = c.first ? pinned : st_in[i];
  JpegState next = pinned;
  if (!c.last) next = st_in[i + 1];
  const int st = jpeg_chunk_strict(L.scan, c, im, s, (const unsigned char*)(s_tab + im.tset * JPEG_SET_WORDS), coef + im.block0 * 64, in, first_block, cnt[i],
                                   c.last ? nullptr : &next, &mcus);
  if (st) atomicOr(&status[b], st);
  if (mcus) atomicAdd(&counters[b], mcus);
}

__global__ __launch_bounds__(JPEG_SPLIT_THREADS) void jpeg_dc_kernel(JpegLaunch L, short* coef, int* status) {
  __shared__ unsigned s_sum[3][JPEG_SPLIT_THREADS];
  const int t = threadIdx.x;
  const int* row = L.segments + (long)blockIdx.x * ZH_JPEG_SEGMENT_WORDS;
  const int b = row[0];
  if (b < 0 || b >= L.B) return;                                            // (uniform over the workgroup, as every return here)
  const JpegImage im = jpeg_launch_image(L, b);
  if (!im.ok) return;
  JpegSegment s;
  int st;
  if (!jpeg_segment(row, im, L.scan, L.scan_bytes, s, &st)) {
    if (t == 0) atomicOr(&status[b], st);
    return;
  }
  const long per = (s.mcu_end - s.mcu + JPEG_SPLIT_THREADS - 1) / JPEG_SPLIT_THREADS;
  const long m0 = s.mcu + t * per < s.mcu_end ? s.mcu + t * per : s.mcu_end, m1 = m0 + per < s.mcu_end ? m0 + per : s.mcu_end;
  short* c0 = coef + im.block0 * 64;
  unsigned pred[3] = {0, 0, 0};
  for (long m = m0; m < m1; ++m)
    for (int j = 0; j < im.bpm; ++j) {
      const unsigned d = jpeg_dc_add(0, c0[(m * im.bpm + j) * 64]);
      if (j < im.lum) pred[0] += d; else if (j == im.lum) pred[1] += d; else pred[2] += d;
    }
  for (int k = 0; k < 3; ++k) s_sum[k][t] = pred[k];
  __syncthreads();
  for (int d = 1; d < JPEG_SPLIT_THREADS; d <<= 1) {
    unsigned add[3] = {0, 0, 0};
    if (t >= d)
      for (int k = 0; k < 3; ++k) add[k] = s_sum[k][t - d];
    __syncthreads();
    for (int k = 0; k < 3; ++k) s_sum[k][t] += add[k];
    __syncthreads();
  }
  for (int k = 0; k < 3; ++k) pred[k] = t ? s_sum[k][t - 1] : 0;
  for (long m = m0; m < m1; ++m)
    for (int j = 0; j < im.bpm; ++j) {
      short* blk = c0 + (m * im.bpm + j) * 64;
      unsigned& p = j < im.lum ? pred[0] : j == im.lum ? pred[1] : pred[2];
      p = jpeg_dc_add(p, blk[0]);
      blk[0] = (short)p;
    }
}

static size_t jpeg_round16(size_t n) { return (n + 15) / 16 * 16; }
static size_t jpeg_sequences(long n_chunks) { return ((size_t)n_chunks + JPEG_SPLIT_THREADS - 1) / JPEG_SPLIT_THREADS; }

extern "C" size_t zh_jpeg_decode_split_workspace_size(int B, long n_blocks, long n_chunks) {
  if (B < 1 || n_blocks < 1 || n_chunks < 0) return 0;
  const size_t nc = (size_t)n_chunks, ns = jpeg_sequences(n_chunks);
  return jpeg_round16(zh_jpeg_decode_workspace_size(B, n_blocks)) + 2 * jpeg_round16(nc * sizeof(JpegState)) + 2 * jpeg_round16(nc * sizeof(int)) +
         jpeg_round16(2 * ns * sizeof(JpegState)) + 3 * jpeg_round16(ns * sizeof(int));
}

extern "C" int zh_jpeg_decode_split(const unsigned char* scan, long scan_bytes, const int* segments, int n_segments, const int* chunks, long n_chunks,
                                    int chunk_bytes, int passes, const int* images, int B, const unsigned char* tables, int n_sets, long n_blocks,
                                    long max_image_blocks, long max_image_pixels, unsigned char* out, long out_bytes, int* status, void* workspace,
                                    size_t workspace_bytes, hipStream_t stream) {
  ZH_CHECK_ARG(B >= 0 && B <= 65535, "zh_jpeg_decode_split: B = %d outside 0 .. 65535", B);
  if (B == 0) return ZH_OK;
  ZH_CHECK_ARG(scan_bytes >= 0 && scan_bytes <= 0x7fffffffL && out_bytes >= 0, "zh_jpeg_decode_split: scan_bytes / out_bytes outside 0 .. 2^31 - 1 / negative");
  ZH_CHECK_ARG(n_segments >= 0 && n_segments <= ZH_JPEG_MAX_SEGMENTS, "zh_jpeg_decode_split: n_segments = %d outside 0 .. %d", n_segments, ZH_JPEG_MAX_SEGMENTS);
  ZH_CHECK_ARG(n_chunks >= 0 && n_chunks <= ZH_JPEG_MAX_CHUNKS, "zh_jpeg_decode_split: n_chunks = %ld outside 0 .. %d", n_chunks, ZH_JPEG_MAX_CHUNKS);
  ZH_CHECK_ARG(chunk_bytes >= ZH_JPEG_CHUNK_BYTES_MIN && chunk_bytes <= 4096 && chunk_bytes % 16 == 0 && passes >= 1 && passes <= 64,
               "zh_jpeg_decode_split: chunk_bytes = %d (a multiple of 16 in %d .. 4096) / passes = %d (1 .. 64)", chunk_bytes, ZH_JPEG_CHUNK_BYTES_MIN, passes);
  ZH_CHECK_ARG(n_sets >= 1 && n_sets <= ZH_JPEG_MAX_TABLE_SETS, "zh_jpeg_decode_split: n_sets = %d outside 1 .. %d", n_sets, ZH_JPEG_MAX_TABLE_SETS);
  ZH_CHECK_ARG(n_blocks >= 1 && n_blocks < (1L << 24), "zh_jpeg_decode_split: n_blocks = %ld outside 1 .. 2^24 - 1", n_blocks);
  ZH_CHECK_ARG(max_image_blocks >= 1 && max_image_blocks <= n_blocks && max_image_pixels >= 1 && max_image_pixels <= 64 * n_blocks,
               "zh_jpeg_decode_split: max_image_blocks = %ld / max_image_pixels = %ld do not go with n_blocks = %ld", max_image_blocks, max_image_pixels, n_blocks);
  ZH_CHECK_ARG(scan && segments && chunks && images && tables && out && status && workspace, "zh_jpeg_decode_split: null pointer");
  ZH_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)tables & 3) == 0, "zh_jpeg_decode_split: workspace must be 16-byte, tables 4-byte aligned");
  if (workspace_bytes < zh_jpeg_decode_split_workspace_size(B, n_blocks, n_chunks)) {
    zh_set_error("zh_jpeg_decode_split: workspace holds %zu bytes, %zu needed", workspace_bytes, zh_jpeg_decode_split_workspace_size(B, n_blocks, n_chunks));
    return ZH_ERR_WORKSPACE;
  }
  const size_t nc = (size_t)n_chunks, ns = jpeg_sequences(n_chunks);
  unsigned char* at = (unsigned char*)workspace;
  int* counters = (int*)at;
  short* coef = (short*)(at + jpeg_counter_bytes(B));
  unsigned char* samples = (unsigned char*)(coef + n_blocks * 64);
  at += jpeg_round16(zh_jpeg_decode_workspace_size(B, n_blocks));
  JpegState* st_in = (JpegState*)at; at += jpeg_round16(nc * sizeof(JpegState));
  JpegState* st_out = (JpegState*)at; at += jpeg_round16(nc * sizeof(JpegState));
  int* cnt = (int*)at; at += jpeg_round16(nc * sizeof(int));
  int* first = (int*)at; at += jpeg_round16(nc * sizeof(int));
  JpegState* hand = (JpegState*)at; at += jpeg_round16(2 * ns * sizeof(JpegState));
  int* seq_sum = (int*)at; at += jpeg_round16(ns * sizeof(int));
  int* seq_start = (int*)at; at += jpeg_round16(ns * sizeof(int));
  int* carry = (int*)at;
  if (hipMemsetAsync(status, 0, (size_t)B * sizeof(int), stream) != hipSuccess ||
      hipMemsetAsync(workspace, 0, jpeg_counter_bytes(B) + (size_t)n_blocks * 64 * sizeof(short), stream) != hipSuccess) {
    zh_set_error("zh_jpeg_decode_split: fill failed: %s", hipGetErrorString(hipGetLastError()));
    return ZH_ERR_HIP;
  }
  const JpegLaunch L = {scan, scan_bytes, segments, n_segments, chunks, n_chunks, chunk_bytes, images, B, n_sets, n_blocks, out_bytes, max_image_blocks, max_image_pixels};
  if (n_chunks > 0) {
    for (int pass = 0; pass < passes; ++pass) {
      hipLaunchKernelGGL(jpeg_sync_kernel, dim3((unsigned)ns), dim3(JPEG_SPLIT_THREADS), 0, stream, L, tables, pass, (long)ns, st_in, st_out, cnt, hand);
      ZH_CHECK_LAUNCH("zh_jpeg_decode_split (sync)");
    }
    hipLaunchKernelGGL(jpeg_count_kernel, dim3((unsigned)ns), dim3(JPEG_SPLIT_THREADS), 0, stream, chunks, n_chunks, (const int*)cnt, first, seq_sum, seq_start);
    ZH_CHECK_LAUNCH("zh_jpeg_decode_split (count)");
    hipLaunchKernelGGL(jpeg_carry_kernel, dim3(1), dim3(JPEG_SPLIT_THREADS), 0, stream, (const int*)seq_sum, (const int*)seq_start, (long)ns, carry);
    ZH_CHECK_LAUNCH("zh_jpeg_decode_split (carry)");
    hipLaunchKernelGGL(jpeg_strict_kernel, dim3((unsigned)ns), dim3(JPEG_SPLIT_THREADS), 0, stream, L, tables, (const JpegState*)st_in, (const int*)cnt,
                       (const int*)first, (const int*)carry, coef, counters, status);
    ZH_CHECK_LAUNCH("zh_jpeg_decode_split (strict)");
  }
  if (n_segments > 0) {
    hipLaunchKernelGGL(jpeg_dc_kernel, dim3((unsigned)n_segments), dim3(JPEG_SPLIT_THREADS), 0, stream, L, coef, status);
    ZH_CHECK_LAUNCH("zh_jpeg_decode_split (DC)");
  }
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3(zh_cdiv(max_image_blocks, JPEG_THREADS), B), dim3(JPEG_THREADS), 0, stream, images, tables, n_sets, n_blocks,
                     out_bytes, max_image_blocks, max_image_pixels, (const short*)coef, samples);
  ZH_CHECK_LAUNCH("zh_jpeg_decode_split (inverse DCT)");
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3(zh_cdiv(max_image_pixels, JPEG_THREADS), B), dim3(JPEG_THREADS), 0, stream, images, n_sets, n_blocks,
                     out_bytes, max_image_blocks, max_image_pixels, (const unsigned char*)samples, (const int*)counters, out, status);
  ZH_CHECK_LAUNCH("zh_jpeg_decode_split (colour)");
  return ZH_OK;
}
