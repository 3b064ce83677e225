// Host twin of the device JPEG decoder: the codec of jpeg_codec.h and its pixel arithmetic in three loops on the CPU, in the order of
// zh_jpeg_decode's launches.  HOST pointers throughout; no kernel and no HIP call in this file — it is what the CPU tests compare with
// jpeg_device.decode_np and what tools/host/jpeg_host_check.cpp runs under the host sanitizers (tools/README.md).  The scratch
// (coefficients, sample planes, MCU counters) is allocated here at exactly the sizes the device workspace has.
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "jpeg_codec.h"

extern "C" int zh_jpeg_decode_host(const unsigned char* scan, long scan_bytes, const int* segments, int n_segments, const int* images, int B,
                                   const unsigned char* tables, int n_sets, long n_blocks, unsigned char* out, long out_bytes, int* status) {
  ZH_CHECK_ARG(B >= 0 && B <= 65535, "zh_jpeg_decode_host: B = %d outside 0 .. 65535", B);
  if (B == 0) return ZH_OK;
  ZH_CHECK_ARG(scan_bytes >= 0 && scan_bytes <= 0x7fffffffL && out_bytes >= 0, "zh_jpeg_decode_host: scan_bytes / out_bytes outside 0 .. 2^31 - 1 / negative");
  ZH_CHECK_ARG(n_segments >= 0 && n_segments <= ZH_JPEG_MAX_SEGMENTS, "zh_jpeg_decode_host: n_segments = %d outside 0 .. %d", n_segments, ZH_JPEG_MAX_SEGMENTS);
  ZH_CHECK_ARG(n_sets >= 1 && n_sets <= ZH_JPEG_MAX_TABLE_SETS, "zh_jpeg_decode_host: n_sets = %d outside 1 .. %d", n_sets, ZH_JPEG_MAX_TABLE_SETS);
  ZH_CHECK_ARG(n_blocks >= 1 && n_blocks < (1L << 24), "zh_jpeg_decode_host: n_blocks = %ld outside 1 .. 2^24 - 1", n_blocks);
  ZH_CHECK_ARG(scan && segments && images && tables && out && status, "zh_jpeg_decode_host: null pointer");
  ZH_CHECK_ARG(((uintptr_t)tables & 3) == 0, "zh_jpeg_decode_host: tables must be 4-byte aligned");
  short* coef = (short*)calloc((size_t)n_blocks * 64, sizeof(short));
  unsigned char* samples = (unsigned char*)malloc((size_t)n_blocks * 64);
  int* counters = (int*)calloc((size_t)B, sizeof(int));
  if (!coef || !samples || !counters) {
    free(coef); free(samples); free(counters);
    zh_set_error("zh_jpeg_decode_host: out of memory for %ld blocks", n_blocks);
    return ZH_ERR_WORKSPACE;
  }
  memset(status, 0, (size_t)B * sizeof(int));
  // A: the entropy segments
  for (long sg = 0; sg < n_segments; ++sg) {
    const int* row = segments + sg * ZH_JPEG_SEGMENT_WORDS;
    const int b = row[0];
    if (b < 0 || b >= B) continue;
    const JpegImage im = jpeg_image(images + (long)b * ZH_JPEG_IMAGE_WORDS, n_sets, n_blocks, out_bytes);
    if (!im.ok) continue;
    JpegSegment s;
    int st;
    if (!jpeg_segment(row, im, scan, scan_bytes, s, &st)) { status[b] |= st; continue; }
    const unsigned char* huff = tables + (long)im.tset * ZH_JPEG_TABLE_SET_BYTES;
    const int mcus = s.mcu_end - s.mcu;
    const long steps = jpeg_segment_steps(s, im);
    for (long it = 0; it < steps && !jpeg_segment_done(s); ++it) jpeg_step(s, im, huff, coef + im.block0 * 64);
    if (s.bits.status) status[b] |= s.bits.status;
    else if (s.mcu >= s.mcu_end) counters[b] += mcus;
  }
  for (int b = 0; b < B; ++b) {
    const JpegImage im = jpeg_image(images + (long)b * ZH_JPEG_IMAGE_WORDS, n_sets, n_blocks, out_bytes);
    if (!im.ok) { status[b] |= ZH_JPEG_STATUS_DESCRIPTOR; continue; }
    if (counters[b] != im.mcux * im.mcuy) status[b] |= ZH_JPEG_STATUS_INCOMPLETE;
    // B: dequantise + inverse DCT
    const unsigned short* q = (const unsigned short*)(tables + (long)im.tset * ZH_JPEG_TABLE_SET_BYTES + JPEG_HUFF_SET_BYTES);
    unsigned char* planes = samples + im.block0 * 64;
    for (long j = 0; j < im.nblocks; ++j) {
      long ld;
      int cls;
      const long at = jpeg_block_place(im, j, &ld, &cls);
      jpeg_idct_block(coef + (im.block0 + j) * 64, q + 64 * cls, planes + at, ld);
    }
    // C: upsample + colour
    for (int y = 0; y < im.h; ++y)
      for (int x = 0; x < im.w; ++x) jpeg_pixel(im, planes, x, y, out + im.out + 3 * ((long)y * im.w + x));
  }
  free(coef); free(samples); free(counters);
  return ZH_OK;
}
