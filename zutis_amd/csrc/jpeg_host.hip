// Host twin of the device JPEG decoder: the codec of jpeg_codec.h and its pixel arithmetic in three loops on the CPU, in the order of
// zh_jpeg_decode's launches.  HOST pointers throughout; no kernel and no HIP call in this file — it is what the CPU tests compare with
// jpeg_device.decode_np and what tools/host/jpeg_host_check.cpp runs under the host sanitizers (tools/README.md).  The scratch
// (coefficients, sample planes, MCU counters) is allocated here at exactly the sizes the device workspace has.
// zh_jpeg_decode_split_host: the passes of zh_jpeg_decode_split over the same rows with the same codec functions; a sequence's lanes run
// one after the other, which reaches the state the kernel's rounds settle in (lane i's state is a function of lane i - 1's alone).
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "jpeg_codec.h"

// the launches behind the entropy stage, shared by both entries: DESCRIPTOR / INCOMPLETE, then per image B and C
static void jpeg_host_pixels(const int* images, int B, const unsigned char* tables, int n_sets, long n_blocks, const short* coef, unsigned char* samples,
                             const int* counters, unsigned char* out, long out_bytes, int* status) {
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
}

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
  jpeg_host_pixels(images, B, tables, n_sets, n_blocks, coef, samples, counters, out, out_bytes, status);
  free(coef); free(samples); free(counters);
  return ZH_OK;
}

extern "C" int zh_jpeg_decode_split_host(const unsigned char* scan, long scan_bytes, const int* segments, int n_segments, const int* chunks, long n_chunks,
                                         int chunk_bytes, int passes, const int* images, int B, const unsigned char* tables, int n_sets, long n_blocks,
                                         unsigned char* out, long out_bytes, int* status) {
  ZH_CHECK_ARG(B >= 0 && B <= 65535, "zh_jpeg_decode_split_host: B = %d outside 0 .. 65535", B);
  if (B == 0) return ZH_OK;
  ZH_CHECK_ARG(scan_bytes >= 0 && scan_bytes <= 0x7fffffffL && out_bytes >= 0, "zh_jpeg_decode_split_host: scan_bytes / out_bytes outside 0 .. 2^31 - 1 / negative");
  ZH_CHECK_ARG(n_segments >= 0 && n_segments <= ZH_JPEG_MAX_SEGMENTS, "zh_jpeg_decode_split_host: n_segments = %d outside 0 .. %d", n_segments, ZH_JPEG_MAX_SEGMENTS);
  ZH_CHECK_ARG(n_chunks >= 0 && n_chunks <= ZH_JPEG_MAX_CHUNKS, "zh_jpeg_decode_split_host: n_chunks = %ld outside 0 .. %d", n_chunks, ZH_JPEG_MAX_CHUNKS);
  ZH_CHECK_ARG(chunk_bytes >= ZH_JPEG_CHUNK_BYTES_MIN && chunk_bytes <= 4096 && chunk_bytes % 16 == 0 && passes >= 1 && passes <= 64,
               "zh_jpeg_decode_split_host: chunk_bytes = %d (a multiple of 16 in %d .. 4096) / passes = %d (1 .. 64)", chunk_bytes, ZH_JPEG_CHUNK_BYTES_MIN, passes);
  ZH_CHECK_ARG(n_sets >= 1 && n_sets <= ZH_JPEG_MAX_TABLE_SETS, "zh_jpeg_decode_split_host: n_sets = %d outside 1 .. %d", n_sets, ZH_JPEG_MAX_TABLE_SETS);
  ZH_CHECK_ARG(n_blocks >= 1 && n_blocks < (1L << 24), "zh_jpeg_decode_split_host: n_blocks = %ld outside 1 .. 2^24 - 1", n_blocks);
  ZH_CHECK_ARG(scan && segments && chunks && images && tables && out && status, "zh_jpeg_decode_split_host: null pointer");
  ZH_CHECK_ARG(((uintptr_t)tables & 3) == 0, "zh_jpeg_decode_split_host: tables must be 4-byte aligned");
  const long n_seq = (n_chunks + ZH_JPEG_SPLIT_LANES - 1) / ZH_JPEG_SPLIT_LANES, nc = n_chunks > 0 ? n_chunks : 1, ns = n_seq > 0 ? n_seq : 1;
  short* coef = (short*)calloc((size_t)n_blocks * 64, sizeof(short));
  unsigned char* samples = (unsigned char*)malloc((size_t)n_blocks * 64);
  int* counters = (int*)calloc((size_t)B, sizeof(int));
  JpegState* st_in = (JpegState*)calloc((size_t)nc, sizeof(JpegState));
  JpegState* st_out = (JpegState*)calloc((size_t)nc, sizeof(JpegState));
  JpegState* hand = (JpegState*)calloc((size_t)ns * 2, sizeof(JpegState));
  int* cnt = (int*)calloc((size_t)nc, sizeof(int));
  int* first = (int*)calloc((size_t)nc, sizeof(int));
  if (!coef || !samples || !counters || !st_in || !st_out || !hand || !cnt || !first) {
    free(coef); free(samples); free(counters); free(st_in); free(st_out); free(hand); free(cnt); free(first);
    zh_set_error("zh_jpeg_decode_split_host: out of memory for %ld blocks and %ld chunks", n_blocks, n_chunks);
    return ZH_ERR_WORKSPACE;
  }
  memset(status, 0, (size_t)B * sizeof(int));
  const JpegLaunch L = {scan, scan_bytes, segments, n_segments, chunks, n_chunks, chunk_bytes, images, B, n_sets, n_blocks, out_bytes, n_blocks, 64 * n_blocks};
  // the synchronising passes
  for (int pass = 0; pass < passes; ++pass)
    for (long w = 0; w < n_seq; ++w) {
      JpegState last = {0, 0};
      for (long i = w * ZH_JPEG_SPLIT_LANES; i < n_chunks && i < (w + 1) * ZH_JPEG_SPLIT_LANES; ++i) {
        JpegChunk c; JpegImage im; JpegSegment s;
        int b;
        const bool ok = jpeg_chunk(L, i, c, im, s, &b) == 0, lane0 = i == w * ZH_JPEG_SPLIT_LANES;
        JpegState in = {ok ? c.ubits : 0, 0}, o = in;
        int n = 0;
        if (ok) {
          if (!c.first && !lane0) in = last;
          else if (pass > 0) {
            in = st_in[i];
            if (!c.first && w > 0) in = hand[((pass - 1) & 1) * n_seq + w - 1];
          }
          o = jpeg_chunk_lenient(scan, s.bits.end, c, im, tables + (long)im.tset * ZH_JPEG_TABLE_SET_BYTES, in, &n);
        }
        st_in[i] = in; st_out[i] = o; cnt[i] = n;
        last = o;
      }
      hand[(pass & 1) * n_seq + w] = last;
    }
  // the scan of the block counts: every chunk's first block inside its segment
  for (long i = 0, run = 0; i < n_chunks; ++i) {
    if (chunks[i * ZH_JPEG_CHUNK_WORDS + 3] == 1) run = 0;
    first[i] = (int)run;
    run = jpeg_block_sum((int)run, cnt[i]);
  }
  // the strict pass
  for (long i = 0; i < n_chunks; ++i) {
    JpegChunk c; JpegImage im; JpegSegment s;
    int b;
    const int rc = jpeg_chunk(L, i, c, im, s, &b);
    if (rc < 0) continue;
    if (rc > 0 || (!c.last && c.ubits + 8 * (int)(c.end - c.start - jpeg_chunk_pairs(scan, c, s.bits.end)) != c.uend)) { status[b] |= ZH_JPEG_STATUS_DESCRIPTOR; continue; }
    const JpegState pinned = {0, 0};
    int mcus;
    status[b] |= jpeg_chunk_strict(scan, c, im, s, tables + (long)im.tset * ZH_JPEG_TABLE_SET_BYTES, coef + im.block0 * 64, c.first ? pinned : st_in[i], first[i],
                                   cnt[i], c.last ? nullptr : &st_in[i + 1], &mcus);
    counters[b] += mcus;
  }
  // the DC sums of every segment
  for (long sg = 0; sg < n_segments; ++sg) {
    const int* row = segments + sg * ZH_JPEG_SEGMENT_WORDS;
    const int b = row[0];
    if (b < 0 || b >= B) continue;
    const JpegImage im = jpeg_launch_image(L, b);
    if (!im.ok) continue;
    JpegSegment s;
    int st;
    if (!jpeg_segment(row, im, scan, scan_bytes, s, &st)) { status[b] |= st; continue; }
    unsigned pred[3] = {0, 0, 0};
    for (long m = s.mcu; m < s.mcu_end; ++m)
      for (int j = 0; j < im.bpm; ++j) {
        short* blk = coef + (im.block0 + m * im.bpm + j) * 64;
        const int comp = j < im.lum ? 0 : j - im.lum + 1;
        pred[comp] = jpeg_dc_add(pred[comp], blk[0]);
        blk[0] = (short)pred[comp];
      }
  }
  jpeg_host_pixels(images, B, tables, n_sets, n_blocks, coef, samples, counters, out, out_bytes, status);
  free(coef); free(samples); free(counters); free(st_in); free(st_out); free(hand); free(cnt); free(first);
  return ZH_OK;
}

// Host twin of the device JPEG encoder (jpeg_enc.hip): the functions of jpeg_codec.h in the order of zh_jpeg_encode's three launches, a
// lane's work as a loop iteration; the scratch has the workspace's sizes.  tools/host/jpeg_enc_host_check.cpp runs it under the sanitizers.
extern "C" int zh_jpeg_encode_host(const unsigned char* images, long image_bytes, const long long* img_off, const int* hw, int B, int subsampling,
                                   long max_mcus, const unsigned short* quant, const long long* out_off, unsigned char* out, long out_bytes,
                                   long slot_bytes, int* lengths) {
  ZH_CHECK_ARG(B >= 0 && B <= 65535, "zh_jpeg_encode_host: B = %d outside 0 .. 65535", B);
  ZH_CHECK_ARG(subsampling == 0 || subsampling == 2, "zh_jpeg_encode_host: subsampling = %d is not 0 (4:4:4) or 2 (4:2:0)", subsampling);
  ZH_CHECK_ARG(image_bytes >= 0 && out_bytes >= 0 && slot_bytes >= 0 && max_mcus >= 0, "zh_jpeg_encode_host: negative count");
  if (B == 0) return ZH_OK;
  ZH_CHECK_ARG(max_mcus >= 1 && max_mcus <= (1L << 26), "zh_jpeg_encode_host: max_mcus = %ld outside 1 .. 2^26", max_mcus);
  ZH_CHECK_ARG(images && img_off && hw && quant && out_off && out && lengths, "zh_jpeg_encode_host: null pointer");
  for (int i = 0; i < 128; ++i) ZH_CHECK_ARG(quant[i] >= 1 && quant[i] <= 255, "zh_jpeg_encode_host: quant[%d] = %d outside 1 .. 255", i, (int)quant[i]);
  const int bpm = subsampling == 2 ? 6 : 3, iv_blocks = ZH_JPEG_ENC_INTERVAL_MCUS * bpm, iv_bytes = iv_blocks * ZH_JPEG_ENC_BLOCK_BYTES;
  short* coef = (short*)malloc((size_t)max_mcus * bpm * 64 * sizeof(short));
  unsigned* words = (unsigned*)malloc((size_t)iv_bytes);
  unsigned char* slot = (unsigned char*)malloc((size_t)iv_bytes * 2);
  if (!coef || !words || !slot) {
    free(coef); free(words); free(slot);
    zh_set_error("zh_jpeg_encode_host: out of memory for %ld MCUs", max_mcus);
    return ZH_ERR_WORKSPACE;
  }
  unsigned tables[4 * JPEG_ENC_TABLE_WORDS];
  for (int t = 0; t < 4; ++t) jpeg_enc_tables(t, tables + t * JPEG_ENC_TABLE_WORDS);
  for (int b = 0; b < B; ++b) {
    const JpegEncImage im = jpeg_enc_image(img_off, hw, out_off, b, subsampling, image_bytes, out_bytes, slot_bytes, max_mcus);
    if (!im.ok) { lengths[b] = -1; continue; }
    // A: coefficients
    for (long i = 0; i < im.mcus * im.bpm; ++i) jpeg_enc_block(im, images + im.off, quant, i / im.bpm, (int)(i % im.bpm), coef + i * 64);
    // B + C: every interval's bits, padded and stuffed, then into the slot behind the intervals in front of it
    long at = 0;
    unsigned char* dst = out + im.out;
    for (int iv = 0; iv < im.nint; ++iv) {
      const long mcu0 = (long)iv * ZH_JPEG_ENC_INTERVAL_MCUS, left = im.mcus - mcu0;
      const int nb = (int)(left < ZH_JPEG_ENC_INTERVAL_MCUS ? left : ZH_JPEG_ENC_INTERVAL_MCUS) * im.bpm;
      const short* c = coef + mcu0 * im.bpm * 64;
      memset(words, 0, (size_t)iv_bytes);
      unsigned bit = 0;
      for (int i = 0; i < nb; ++i) {
        const short* blk = c + i * 64;
        const int from = jpeg_enc_dc_from(i, im.bpm, im.lum);
        unsigned long long nz = 0;
        for (int k = 1; k < 64; ++k) nz |= (unsigned long long)(blk[k] != 0) << k;
        for (int k = 0; k < 64; ++k) {
          unsigned long long val;
          const int n = jpeg_enc_token(tables, i % im.bpm >= im.lum, k, k ? blk[k] : blk[0] - (from < 0 ? 0 : c[from * 64]), nz, &val);
          jpeg_enc_put(words, bit, val, n);
          bit += (unsigned)n;
        }
      }
      if (bit & 7u) { const int pad = 8 - (int)(bit & 7u); jpeg_enc_put(words, bit, (1ull << pad) - 1ull, pad); }
      const int nbytes = (int)((bit + 7u) >> 3);
      int len = 0;
      for (int i = 0; i < nbytes; ++i) {
        const unsigned v = jpeg_enc_byte(words, i);
        slot[len++] = (unsigned char)v;
        if (v == 0xFFu) slot[len++] = 0;
      }
      for (int i = 0; i < len; ++i)
        if (at + i < slot_bytes) dst[at + i] = slot[i];
      at += len;
      if (iv + 1 < im.nint) {
        if (at < slot_bytes) dst[at] = 0xFF;
        if (at + 1 < slot_bytes) dst[at + 1] = (unsigned char)(0xD0 + (iv & 7));
        at += 2;
      }
    }
    lengths[b] = (int)at;
  }
  free(coef); free(words); free(slot);
  return ZH_OK;
}
