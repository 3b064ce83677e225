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
