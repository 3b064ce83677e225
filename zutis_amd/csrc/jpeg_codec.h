// The baseline JPEG decoder (zutis_amd/jpeg_device.py is the definition), written ONCE for the device kernels (jpeg.hip) and the host
// entry (jpeg_host.hip, which tools/host/jpeg_host_check.cpp runs under the host sanitizers).  Inline functions only.  The encoder's
// functions (jpeg_enc.hip, zh_jpeg_encode_host) follow the decoder's, with a list of their own.
//
//   jpeg_image         an image row of the launch, checked: nothing of an image whose row fails is read or written
//   jpeg_segment       a segment row, checked against the scan bytes and the image's MCUs
//   jpeg_step          ONE Huffman symbol of one segment: the state is (MCU, block in MCU, coefficient index k); the table is chosen by
//                      arithmetic on it (class = block past the luma blocks, AC = k != 0), so lanes at different positions of
//                      different images run the same instructions.  Every symbol advances k or ends the block, a block takes at most
//                      64 symbols, so jpeg_segment_steps() bounds the loop whatever the bytes say.
//   JpegBits           a 64-bit bit buffer over [pos, end) of the scan bytes, refilled four bytes at a time where none of them is FF,
//                      byte by byte (FF 00 -> FF) otherwise.  Nothing outside [pos, end) is read: past the end the buffer takes zero bits,
//                      counted in `fake`, and TRUNCATED is set once such a bit is consumed (read-ahead alone sets nothing).
//   jpeg_idct_block    dequantise + islow inverse DCT of one block (64-bit sums: damaged coefficients cannot overflow)
//   jpeg_pixel         fancy upsampling of the cropped chroma planes at one pixel + YCbCr -> RGB
#pragma once
#include "../../include/zutis_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JPEG_HD __host__ __device__ inline
#else
#define JPEG_HD inline
#endif

#define JPEG_HUFF_SET_BYTES (4 * ZH_JPEG_HUFF_TABLE_BYTES)      // the part of a table set the entropy stage reads (what lives in LDS)
#define JPEG_T_MAXCODE 512                                     // byte offsets inside one Huffman table
#define JPEG_T_VALOFF 584
#define JPEG_T_VALS 656

struct JpegImage {
  int w, h, nc, hs, vs, mcux, mcuy, tset, ri, bpm, lum;
  long block0, nblocks, out;
  bool ok;
};

JPEG_HD JpegImage jpeg_image(const int* r, int n_sets, long n_blocks, long out_bytes) {
  JpegImage im;
  im.w = r[0]; im.h = r[1]; im.nc = r[2]; im.hs = r[3]; im.vs = r[4]; im.mcux = r[5]; im.mcuy = r[6]; im.tset = r[7];
  im.block0 = r[8]; im.out = 16L * r[9]; im.ri = r[10];
  im.bpm = 0; im.lum = 0; im.nblocks = 0;
  im.ok = false;
  if (im.w < 1 || im.h < 1 || im.w > 65535 || im.h > 65535) return im;
  const bool grey = im.nc == 1 && im.hs == 1 && im.vs == 1;
  const bool colour = im.nc == 3 && (im.hs == 1 || im.hs == 2) && (im.vs == 1 || im.vs == 2) && !(im.hs == 1 && im.vs == 2);
  if (!grey && !colour) return im;
  if (im.mcux != (im.w + 8 * im.hs - 1) / (8 * im.hs) || im.mcuy != (im.h + 8 * im.vs - 1) / (8 * im.vs)) return im;
  if (im.tset < 0 || im.tset >= n_sets || im.ri < 0) return im;
  im.lum = im.hs * im.vs;
  im.bpm = im.lum + (im.nc == 3 ? 2 : 0);
  im.nblocks = (long)im.mcux * im.mcuy * im.bpm;
  if (im.block0 < 0 || im.block0 + im.nblocks > n_blocks) return im;
  if (r[9] < 0 || im.out + 3L * im.w * im.h > out_bytes) return im;
  im.ok = true;
  return im;
}

struct JpegBits {
  const unsigned char* p;
  long pos, end;
  unsigned long long buf;      // the next bits, from bit 63 down
  int n, fake, status;         // bits in buf; how many of them (the lowest) stand for bytes past the end
};

// after it: at least 32 bits in the buffer (a symbol takes at most 16 code bits and 11 more)
JPEG_HD void jpeg_refill(JpegBits& s) {
  if (s.n > 32) return;
  if (s.pos + 4 <= s.end) {
    unsigned w;
    __builtin_memcpy(&w, s.p + s.pos, 4);
    const unsigned inv = ~w;
    if (!((inv - 0x01010101u) & ~inv & 0x80808080u)) {          // no byte is FF: nothing to unstuff
      s.buf |= (unsigned long long)__builtin_bswap32(w) << (32 - s.n);
      s.n += 32;
      s.pos += 4;
      return;
    }
  }
  for (int i = 0; i < 4; ++i) {
    unsigned b = 0;
    if (s.pos < s.end) {
      b = s.p[s.pos++];
      if (b == 0xFFu) {
        if (s.pos < s.end && s.p[s.pos] == 0) ++s.pos;
        else { s.status |= ZH_JPEG_STATUS_MARKER; s.pos = s.end; }
      }
    } else {
      s.fake += 8;
    }
    s.buf |= (unsigned long long)b << (56 - s.n);
    s.n += 8;
  }
}

JPEG_HD void jpeg_consume(JpegBits& s, int c) {
  s.buf = c ? s.buf << c : s.buf;
  s.n -= c;
  if (s.n < s.fake) s.status |= ZH_JPEG_STATUS_TRUNCATED;
}

struct JpegSegment {
  JpegBits bits;
  int pred0, pred1, pred2;     // DC predictors of Y, Cb, Cr: 0 at the start of every segment
  int mcu, mcu_end, b, k;      // the state: MCU, block inside it, coefficient index (0: the DC symbol is next)
};

// The segment row `r` of image `im` over scan bytes [0, scan_bytes): false (and SEGMENT in *status) when it does not fit.
JPEG_HD bool jpeg_segment(const int* r, const JpegImage& im, const unsigned char* scan, long scan_bytes, JpegSegment& s, int* status) {
  const long lo = r[1], hi = r[2], first = r[3], total = (long)im.mcux * im.mcuy;
  s.bits.p = scan; s.bits.pos = lo; s.bits.end = hi; s.bits.buf = 0; s.bits.n = 0; s.bits.fake = 0; s.bits.status = 0;
  s.pred0 = s.pred1 = s.pred2 = 0;
  s.mcu = s.mcu_end = (int)first; s.b = 0; s.k = 0;
  if (lo < 0 || hi < lo || hi > scan_bytes || first < 0 || first >= total || (im.ri == 0 && first != 0)) {
    *status = ZH_JPEG_STATUS_SEGMENT;
    return false;
  }
  const long count = im.ri ? (im.ri < total - first ? im.ri : total - first) : total;
  s.mcu_end = (int)(first + count);
  *status = 0;
  return true;
}

JPEG_HD long jpeg_segment_steps(const JpegSegment& s, const JpegImage& im) { return 64L * (s.mcu_end - s.mcu) * im.bpm; }
JPEG_HD bool jpeg_segment_done(const JpegSegment& s) { return s.mcu >= s.mcu_end || s.bits.status != 0; }

// natural-order index of zigzag position k: eight positions to a 64-bit literal, picked by selects (a table would live in memory)
constexpr unsigned long long jpeg_zz8(unsigned long long a, unsigned long long b, unsigned long long c, unsigned long long d, unsigned long long e,
                                      unsigned long long f, unsigned long long g, unsigned long long h) {
  return a | b << 8 | c << 16 | d << 24 | e << 32 | f << 40 | g << 48 | h << 56;
}
JPEG_HD int jpeg_zigzag(int k) {
  const int g = (k >> 3) & 7;
  const unsigned long long w = g == 0   ? jpeg_zz8(0, 1, 8, 16, 9, 2, 3, 10)
                               : g == 1 ? jpeg_zz8(17, 24, 32, 25, 18, 11, 4, 5)
                               : g == 2 ? jpeg_zz8(12, 19, 26, 33, 40, 48, 41, 34)
                               : g == 3 ? jpeg_zz8(27, 20, 13, 6, 7, 14, 21, 28)
                               : g == 4 ? jpeg_zz8(35, 42, 49, 56, 57, 50, 43, 36)
                               : g == 5 ? jpeg_zz8(29, 22, 15, 23, 30, 37, 44, 51)
                               : g == 6 ? jpeg_zz8(58, 59, 52, 45, 38, 31, 39, 46)
                                        : jpeg_zz8(53, 60, 61, 54, 47, 55, 62, 63);
  return (int)((w >> (8 * (k & 7))) & 63);
}

// One symbol.  huff: the image's four Huffman tables; coef: the IMAGE's first block (int16 [nblocks, 64], zeroed): the block written is
// mcu * bpm + b with mcu < mcu_end <= the image's MCUs, the index inside it jpeg_zigzag() of k <= 63.
JPEG_HD void jpeg_step(JpegSegment& s, const JpegImage& im, const unsigned char* huff, short* coef) {
  JpegBits& bt = s.bits;
  jpeg_refill(bt);
  const int comp = s.b < im.lum ? 0 : s.b - im.lum + 1, ac = s.k != 0;
  const unsigned char* t = huff + (2 * (comp != 0) + ac) * ZH_JPEG_HUFF_TABLE_BYTES;
  const unsigned peek = (unsigned)(bt.buf >> 48);
  const unsigned e = ((const unsigned short*)t)[peek >> 8];
  int len = (int)(e >> 8), val = (int)(e & 255u);
  if (!e) {                                                       // a code of 9 .. 16 bits, or none
    const int* maxcode = (const int*)(t + JPEG_T_MAXCODE);
    const int* valoff = (const int*)(t + JPEG_T_VALOFF);
    for (int l = 9; l <= 16; ++l) {
      const int code = (int)(peek >> (16 - l));
      if (len == 0 && code <= maxcode[l]) { len = l; val = t[JPEG_T_VALS + ((code + valoff[l]) & 255)]; }
    }
    if (len == 0) { bt.status |= ZH_JPEG_STATUS_CODE; return; }
  }
  jpeg_consume(bt, len);
  const int r = ac ? val >> 4 : 0, sz = ac ? val & 15 : val;
  if (sz > (ac ? 10 : 11)) { bt.status |= ZH_JPEG_STATUS_BITS; return; }
  int v = sz ? (int)(bt.buf >> (64 - sz)) : 0;
  jpeg_consume(bt, sz);
  if (sz && v < (1 << (sz - 1))) v -= (1 << sz) - 1;
  if (bt.status) return;
  short* blk = coef + ((long)s.mcu * im.bpm + s.b) * 64;
  if (!ac) {
    int pred = comp == 0 ? s.pred0 : comp == 1 ? s.pred1 : s.pred2;
    pred += v;
    if (comp == 0) s.pred0 = pred; else if (comp == 1) s.pred1 = pred; else s.pred2 = pred;
    blk[0] = (short)pred;
    s.k = 1;
  } else if (sz == 0) {
    if (r == 15) {
      s.k += 16;
      if (s.k > 64) { bt.status |= ZH_JPEG_STATUS_INDEX; return; }
    } else {
      s.k = 64;                                                     // end of block
    }
  } else {
    s.k += r;
    if (s.k > 63) { bt.status |= ZH_JPEG_STATUS_INDEX; return; }
    blk[jpeg_zigzag(s.k)] = (short)v;
    ++s.k;
  }
  if (s.k >= 64) {
    s.k = 0;
    if (++s.b == im.bpm) { s.b = 0; ++s.mcu; }
  }
}

// ---- pixels
// one pass of the islow inverse DCT over eight values, descaled by `shift` bits with rounding (13-bit constants)
JPEG_HD void jpeg_idct8(const long long* in, int stride, long long* out, int shift) {
  const long long i0 = in[0], i1 = in[stride], i2 = in[2 * stride], i3 = in[3 * stride], i4 = in[4 * stride], i5 = in[5 * stride],
                  i6 = in[6 * stride], i7 = in[7 * stride];
  long long z1 = (i2 + i6) * 4433;
  const long long t2 = z1 - i6 * 15137, t3 = z1 + i2 * 6270;
  const long long t0 = (i0 + i4) * 8192, t1 = (i0 - i4) * 8192;
  const long long t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  long long a0 = i7, a1 = i5, a2 = i3, a3 = i1;
  z1 = a0 + a3;
  long long z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const long long z5 = (z3 + z4) * 9633;
  a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
  const long long half = 1LL << (shift - 1);
  out[0] = (t10 + a3 + half) >> shift;
  out[stride] = (t11 + a2 + half) >> shift;
  out[2 * stride] = (t12 + a1 + half) >> shift;
  out[3 * stride] = (t13 + a0 + half) >> shift;
  out[4 * stride] = (t13 - a0 + half) >> shift;
  out[5 * stride] = (t12 - a1 + half) >> shift;
  out[6 * stride] = (t11 - a2 + half) >> shift;
  out[7 * stride] = (t10 - a3 + half) >> shift;
}

// coef int16 [64] (natural order) x q u16 [64] -> 8 x 8 samples at dst (row stride `ld`): columns descaled by 11 bits, rows by 18, + 128
JPEG_HD void jpeg_idct_block(const short* coef, const unsigned short* q, unsigned char* dst, long ld) {
  long long x[64], w[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) x[i] = (long long)coef[i] * (long long)q[i];
#pragma unroll
  for (int c = 0; c < 8; ++c) jpeg_idct8(x + c, 8, w + c, 11);
#pragma unroll
  for (int r = 0; r < 8; ++r) jpeg_idct8(w + 8 * r, 1, x + 8 * r, 18);
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const long long v = x[8 * r + c] + 128;
      dst[r * ld + c] = (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
}

// where block j of the image (scan order) lies in its planes: the planes follow each other at samples + 64 * block0 — Y
// [mcuy vs 8, mcux hs 8], then Cb and Cr [mcuy 8, mcux 8]; q_class: 0 luma, 1 chroma
JPEG_HD long jpeg_block_place(const JpegImage& im, long j, long* ld, int* q_class) {
  const long mcu = j / im.bpm;
  const int b = (int)(j - mcu * im.bpm);
  const long my = mcu / im.mcux, mx = mcu - my * im.mcux;
  const long yw = (long)im.mcux * im.hs * 8, ysize = yw * im.mcuy * im.vs * 8, cw = (long)im.mcux * 8, csize = cw * im.mcuy * 8;
  if (b < im.lum) {
    const int by = b / im.hs, bx = b - by * im.hs;
    *ld = yw; *q_class = 0;
    return ((my * im.vs + by) * 8) * yw + (mx * im.hs + bx) * 8;
  }
  *ld = cw; *q_class = 1;
  return ysize + (b - im.lum) * csize + (my * 8) * cw + mx * 8;
}

// the chroma sample of pixel (x, y) from plane c [*, cld], cropped to cw x ch samples before it is upsampled
JPEG_HD int jpeg_chroma(const unsigned char* c, long cld, int cw, int ch, int hs, int vs, int x, int y) {
  if (hs == 1) return c[(long)y * cld + x];
  const int i = x >> 1;
  if (cw <= 2) return c[(long)(vs == 2 ? y >> 1 : y) * cld + i];          // a narrow component is replicated
  const int il = i > 0 ? i - 1 : 0, ir = i < cw - 1 ? i + 1 : cw - 1, in = (x & 1) ? ir : il;
  if (vs == 1) {
    const unsigned char* row = c + (long)y * cld;
    if (in == i) return row[i];                                          // the first and the last output
    return (3 * row[i] + row[in] + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int j = y >> 1, jn = (y & 1) ? (j < ch - 1 ? j + 1 : j) : (j > 0 ? j - 1 : j);
  const unsigned char *row = c + (long)j * cld, *nb = c + (long)jn * cld;
  const int cs = 3 * row[i] + nb[i], csn = 3 * row[in] + nb[in];
  const int bias = (x & 1) ? 7 : 8;
  if (in == i) return (4 * cs + bias) >> 4;
  return (3 * cs + csn + bias) >> 4;
}

JPEG_HD unsigned char jpeg_clamp8(int v) { return (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v); }

// pixel (x, y) of the image from its sample planes -> rgb[3]
JPEG_HD void jpeg_pixel(const JpegImage& im, const unsigned char* planes, int x, int y, unsigned char* rgb) {
  const long yw = (long)im.mcux * im.hs * 8, ysize = yw * im.mcuy * im.vs * 8, cld = (long)im.mcux * 8, csize = cld * im.mcuy * 8;
  const int Y = planes[(long)y * yw + x];
  if (im.nc == 1) { rgb[0] = rgb[1] = rgb[2] = (unsigned char)Y; return; }
  const int cw = (im.w + im.hs - 1) / im.hs, ch = (im.h + im.vs - 1) / im.vs;
  const int cb = jpeg_chroma(planes + ysize, cld, cw, ch, im.hs, im.vs, x, y) - 128;
  const int cr = jpeg_chroma(planes + ysize + csize, cld, cw, ch, im.hs, im.vs, x, y) - 128;
  rgb[0] = jpeg_clamp8(Y + ((91881 * cr + 32768) >> 16));               // F(1.402), F(x) = int(x 65536 + 0.5)
  rgb[1] = jpeg_clamp8(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)); // F(0.34414), F(0.71414)
  rgb[2] = jpeg_clamp8(Y + ((116130 * cb + 32768) >> 16));              // F(1.772)
}

// ---- a segment split among lanes (zh_jpeg_decode_split: include/zutis_hip.h has the method)
//   jpeg_chunk          a chunk row, checked against its segment, the row in front of it and the row behind it
//   jpeg_chunk_pairs    the FF 00 pairs of a chunk's bytes: what the unstuffed count of the NEXT row is checked with
//   jpeg_chunk_lenient  the symbols that start in a chunk, from any state, under rules that cannot fail: no status, nothing written
//   jpeg_chunk_strict   the same symbols under jpeg_step's rules: coefficients (DC as differences), status bits, the hand-over check
//   jpeg_dc_add         the wrapping DC sum
// A position is an unstuffed bit offset inside the segment; every loop is bounded by the bits of a chunk.
struct JpegLaunch {
  const unsigned char* scan;
  long scan_bytes;
  const int* segments;
  int n_segments;
  const int* chunks;
  long n_chunks;
  int chunk_bytes;
  const int* images;
  int B, n_sets;
  long n_blocks, out_bytes, max_image_blocks, max_image_pixels;
};

struct JpegState {
  int pos, bk;                 // the bit the next symbol starts at; block inside the MCU << 8 | coefficient index
};
JPEG_HD bool jpeg_state_equal(const JpegState& a, const JpegState& b) { return a.pos == b.pos && a.bk == b.bk; }

struct JpegChunk {
  int seg;                     // its segment row
  long start, end;             // its bytes [start, end) of the scan
  int ubits, uend;             // the unstuffed bits of the segment in front of it and in front of the next chunk (last: an upper bound)
  bool first, last;
};

#define JPEG_BLOCK_SUM_MAX (1 << 29)      // block counts are added saturating (a damaged scan may count anything): still associative
JPEG_HD int jpeg_block_sum(int a, int b) { return a + b > JPEG_BLOCK_SUM_MAX ? JPEG_BLOCK_SUM_MAX : a + b; }

JPEG_HD JpegImage jpeg_launch_image(const JpegLaunch& L, int b) {
  JpegImage im = jpeg_image(L.images + (long)b * ZH_JPEG_IMAGE_WORDS, L.n_sets, L.n_blocks, L.out_bytes);
  if (im.ok && (im.nblocks > L.max_image_blocks || (long)im.w * im.h > L.max_image_pixels)) im.ok = false;
  return im;
}

// Chunk row i.  0: it fits (c, im, s, *b are its chunk, image, segment and image index); -1: its segment or image cannot be told or
// fails its own check (whoever owns that row reports it); 1: the row does not fit — image *b gets DESCRIPTOR.
JPEG_HD int jpeg_chunk(const JpegLaunch& L, long i, JpegChunk& c, JpegImage& im, JpegSegment& s, int* b) {
  const int* r = L.chunks + i * ZH_JPEG_CHUNK_WORDS;
  c.seg = r[0];
  if (c.seg < 0 || c.seg >= L.n_segments) return -1;
  const int* srow = L.segments + (long)c.seg * ZH_JPEG_SEGMENT_WORDS;
  *b = srow[0];
  if (*b < 0 || *b >= L.B) return -1;
  im = jpeg_launch_image(L, *b);
  if (!im.ok) return -1;
  int st;
  if (!jpeg_segment(srow, im, L.scan, L.scan_bytes, s, &st)) return -1;
  const long lo = s.bits.pos, hi = s.bits.end;
  c.start = r[1]; c.ubits = r[2];
  c.end = hi; c.uend = 0; c.last = true;
  c.first = r[3] == 1;
  if ((r[3] != 0 && r[3] != 1) || hi - lo >= (1L << 28) || c.start < lo || c.start > hi) return 1;
  if (c.first) {
    if (c.start != lo || c.ubits != 0) return 1;
  } else {
    if (i == 0) return 1;
    const int* p = r - ZH_JPEG_CHUNK_WORDS;
    if (p[0] != c.seg || p[1] < lo || p[1] >= c.start || c.start - p[1] > L.chunk_bytes + 1) return 1;
    if (c.ubits < 0 || c.ubits > 8 * (c.start - lo) || (c.ubits & 7)) return 1;
  }
  if (i + 1 < L.n_chunks) {
    const int* q = r + ZH_JPEG_CHUNK_WORDS;
    if (q[0] == c.seg && q[3] == 0) { c.last = false; c.end = q[1]; c.uend = q[2]; }
  }
  if (c.end < c.start || c.end > hi || c.end - c.start > L.chunk_bytes + 1) return 1;
  if (c.last) c.uend = c.ubits + (int)(8 * (c.end - c.start));
  else if (c.uend < c.ubits || c.uend - c.ubits > 8 * (c.end - c.start)) return 1;
  return 0;
}

// FF 00 pairs whose FF lies in the chunk's bytes and whose 00 lies inside the segment
JPEG_HD int jpeg_chunk_pairs(const unsigned char* scan, const JpegChunk& c, long hi) {
  int n = 0;
  for (long q = c.start; q < c.end; ++q) n += scan[q] == 0xFFu && q + 1 < hi && scan[q + 1] == 0;
  return n;
}

// the bit buffer of the chunk's segment at unstuffed bit `pos` of it, c.ubits <= pos: read from the chunk's first byte
JPEG_HD void jpeg_chunk_bits(JpegBits& bt, const unsigned char* scan, const JpegChunk& c, long hi, int pos) {
  bt.p = scan; bt.pos = c.start; bt.end = hi; bt.buf = 0; bt.n = 0; bt.fake = 0; bt.status = 0;
  for (int skip = pos - c.ubits; skip > 0;) {
    jpeg_refill(bt);
    const int t = skip < 32 ? skip : 32;
    jpeg_consume(bt, t);
    skip -= t;
  }
}

// The symbols that start in [in.pos, c.uend) from state `in` -> the state behind them; *blocks: the blocks they complete.  A total
// function: an undefined code skips one bit, a category above the table's limit is clamped, an index past 63 ends the block; a state
// outside the chunk passes through.  It stops where the segment's bytes end.
JPEG_HD JpegState jpeg_chunk_lenient(const unsigned char* scan, long hi, const JpegChunk& c, const JpegImage& im, const unsigned char* huff,
                                     JpegState in, int* blocks) {
  *blocks = 0;
  int pos = in.pos, b = in.bk >> 8, k = in.bk & 255, n = 0;
  if (pos < c.ubits || pos >= c.uend || b < 0 || b >= im.bpm || k > 63) return in;
  JpegBits bt;
  jpeg_chunk_bits(bt, scan, c, hi, pos);
  const int limit = c.uend - c.ubits;                               // every iteration takes at least one bit
  for (int it = 0; it < limit && pos < c.uend && !(bt.status & ZH_JPEG_STATUS_TRUNCATED); ++it) {
    jpeg_refill(bt);
    const int ac = k != 0;
    const unsigned char* t = huff + (2 * (b >= im.lum) + ac) * ZH_JPEG_HUFF_TABLE_BYTES;
    const unsigned peek = (unsigned)(bt.buf >> 48);
    const unsigned e = ((const unsigned short*)t)[peek >> 8];
    int len = (int)(e >> 8), val = (int)(e & 255u);
    if (!e) {
      const int* maxcode = (const int*)(t + JPEG_T_MAXCODE);
      const int* valoff = (const int*)(t + JPEG_T_VALOFF);
      for (int l = 9; l <= 16; ++l) {
        const int code = (int)(peek >> (16 - l));
        if (len == 0 && code <= maxcode[l]) { len = l; val = t[JPEG_T_VALS + ((code + valoff[l]) & 255)]; }
      }
      if (len == 0) { jpeg_consume(bt, 1); ++pos; continue; }
    }
    jpeg_consume(bt, len);
    const int r = ac ? val >> 4 : 0, most = ac ? 10 : 11;
    int sz = ac ? val & 15 : val;
    sz = sz > most ? most : sz;
    jpeg_consume(bt, sz);
    pos += len + sz;
    if (!ac) k = 1;
    else if (sz == 0) k = r == 15 ? k + 16 : 64;
    else k += r + 1;
    if (k >= 64) {
      k = 0;
      if (++b == im.bpm) b = 0;
      ++n;
    }
  }
  *blocks = n;
  JpegState out = {pos, b << 8 | k};
  return out;
}

// The same symbols under jpeg_step's rules, from the state the synchronising passes left for the chunk.  first_block: the blocks of the
// segment the chunks in front of it complete (the scan of the lenient counts); want_blocks: its own lenient count; next: the state the
// next chunk starts from (null for the last chunk).  coef: the image's first block; DC values are written as DIFFERENCES (the
// predictors are taken as 0 at every symbol).  Returns the status bits: jpeg_step's, or UNSYNCED when the chunk ends clean in another
// state or with another count than the next chunk was given; *mcus: the segment's MCUs when this chunk completed its last block.
// Behind the segment's last block nothing is decoded, as zh_jpeg_decode leaves what follows it unread.
JPEG_HD int jpeg_chunk_strict(const unsigned char* scan, const JpegChunk& c, const JpegImage& im, const JpegSegment& s, const unsigned char* huff,
                              short* coef, JpegState in, int first_block, int want_blocks, const JpegState* next, int* mcus) {
  *mcus = 0;
  const long seg_blocks = (long)(s.mcu_end - s.mcu) * im.bpm;
  if (first_block >= seg_blocks) return 0;
  int pos = in.pos, n = 0;
  const int b = in.bk >> 8, k = in.bk & 255;
  if (pos < c.ubits || b != first_block % im.bpm || k > 63) return ZH_JPEG_STATUS_UNSYNCED;
  JpegSegment t = s;
  t.mcu = s.mcu + first_block / im.bpm; t.b = b; t.k = k;
  if (c.last || pos < c.uend) {
    jpeg_chunk_bits(t.bits, scan, c, s.bits.end, pos);
    const long limit = 8 * (c.end - c.start) + 2;                   // the chunk's bits, and the symbol that runs past the segment's end
    for (long it = 0; it < limit && (c.last || pos < c.uend) && !jpeg_segment_done(t); ++it) {
      t.pred0 = t.pred1 = t.pred2 = 0;
      while (t.bits.n <= 32) jpeg_refill(t.bits);                   // jpeg_step's own refill then adds nothing: the bits it takes are n0 - n
      const int n0 = t.bits.n, b0 = t.b, m0 = t.mcu;
      jpeg_step(t, im, huff, coef);
      pos += n0 - t.bits.n;
      n += t.b != b0 || t.mcu != m0;
    }
  }
  if (t.bits.status) return t.bits.status;
  if (t.mcu >= t.mcu_end) { *mcus = s.mcu_end - s.mcu; return 0; }
  if (!next) return 0;                                              // (a last chunk ends in one of the two ways above)
  const JpegState out = {pos, t.b << 8 | t.k};
  return jpeg_state_equal(out, *next) && n == want_blocks ? 0 : ZH_JPEG_STATUS_UNSYNCED;
}

// DC predictor + difference as the serial decoder's int sum wraps (32-bit two's complement)
JPEG_HD unsigned jpeg_dc_add(unsigned pred, short diff) { return pred + (unsigned)(int)diff; }

// ---- the baseline encoder (zh_jpeg_encode / zh_jpeg_encode_host: jpeg_device.scan_np is the definition; include/zutis_hip.h has the rules)
//   jpeg_enc_image      an image of the launch, checked: nothing of an image that fails is read or written
//   jpeg_enc_sample     one sample of a component on its edge-replicated MCU grid: colour conversion, h2v2 downsampling
//   jpeg_enc_block      one block of the scan: samples, islow forward DCT, quantisation, the dummy-block rule -> 64 zig-zag coefficients
//   jpeg_enc_tables     the Annex K Huffman codes by symbol
//   jpeg_enc_token      the bits ONE zig-zag position of a block puts into the scan, from the block's mask of nonzero AC positions alone
//   jpeg_enc_put        those bits into a word buffer, most significant first
#define JPEG_ENC_TABLE_WORDS 256                               // code << 8 | length by symbol; four tables: luma DC, luma AC, chroma DC, chroma AC
#define JPEG_ENC_BLOCK_BITS 1660                               // 11 + 11 of DC, 63 x (16 + 10) of AC: ZH_JPEG_ENC_BLOCK_BYTES rounded down

struct JpegEncImage {
  int h, w, hs, mcux, mcuy, lum, bpm, nint;                    // nint: restart intervals
  long mcus, off, out;
  bool ok;
};

JPEG_HD long jpeg_enc_intervals(long mcus) { return (mcus + ZH_JPEG_ENC_INTERVAL_MCUS - 1) / ZH_JPEG_ENC_INTERVAL_MCUS; }

JPEG_HD JpegEncImage jpeg_enc_image(const long long* img_off, const int* hw, const long long* out_off, int b, int sub, long image_bytes, long out_bytes,
                                    long slot_bytes, long max_mcus) {
  JpegEncImage im;
  im.h = hw[2 * b]; im.w = hw[2 * b + 1];
  im.hs = sub == 2 ? 2 : 1; im.lum = im.hs * im.hs; im.bpm = im.lum + 2;
  im.off = (long)img_off[b]; im.out = (long)out_off[b];
  im.mcux = im.mcuy = im.nint = 0; im.mcus = 0;
  im.ok = false;
  if (im.h < 1 || im.w < 1 || im.h > 65535 || im.w > 65535) return im;
  im.mcux = (im.w + 8 * im.hs - 1) / (8 * im.hs); im.mcuy = (im.h + 8 * im.hs - 1) / (8 * im.hs);
  im.mcus = (long)im.mcux * im.mcuy;
  im.nint = (int)jpeg_enc_intervals(im.mcus);
  if (im.mcus > max_mcus || im.mcus * im.bpm * 2 * ZH_JPEG_ENC_BLOCK_BYTES + 2L * im.nint > 0x7fffffffL) return im;      // the length is an int32
  if (im.off < 0 || im.off + 3L * im.h * im.w > image_bytes) return im;
  if (im.out < 0 || slot_bytes < 0 || im.out + slot_bytes > out_bytes) return im;
  im.ok = true;
  return im;
}

// component comp (0 Y, 1 Cb, 2 Cr) of the pixel at px
JPEG_HD int jpeg_enc_ycc(const unsigned char* px, int comp) {
  const int r = px[0], g = px[1], b = px[2];
  if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;                         // F(.299), F(.587), F(.114)
  if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;         // F(.16874), F(.33126), F(.5)
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;                          // F(.5), F(.41869), F(.08131)
}

// sample (x, y) of component comp on its padded grid; img: the image's first byte.  Luma and 4:4:4 chroma: the edge pixel repeats.  4:2:0
// chroma: the full-resolution plane repeats its last row and column, and the last DOWNSAMPLED row (ceil(h / 2) - 1) repeats below it.
JPEG_HD int jpeg_enc_sample(const JpegEncImage& im, const unsigned char* img, int comp, int x, int y) {
  if (comp == 0 || im.hs == 1) {
    const int xx = x < im.w ? x : im.w - 1, yy = y < im.h ? y : im.h - 1;
    return jpeg_enc_ycc(img + 3 * ((long)yy * im.w + xx), comp);
  }
  const int rows = (im.h + 1) >> 1, cy = y < rows ? y : rows - 1;
  const int y0 = 2 * cy < im.h ? 2 * cy : im.h - 1, y1 = 2 * cy + 1 < im.h ? 2 * cy + 1 : im.h - 1;
  const int x0 = 2 * x < im.w ? 2 * x : im.w - 1, x1 = 2 * x + 1 < im.w ? 2 * x + 1 : im.w - 1;
  const int s = jpeg_enc_ycc(img + 3 * ((long)y0 * im.w + x0), comp) + jpeg_enc_ycc(img + 3 * ((long)y0 * im.w + x1), comp) +
                jpeg_enc_ycc(img + 3 * ((long)y1 * im.w + x0), comp) + jpeg_enc_ycc(img + 3 * ((long)y1 * im.w + x1), comp);
  return (s + ((x & 1) ? 2 : 1)) >> 2;
}

// one pass of the islow forward DCT over eight values in place: the first (rows) scales up by 2 bits, the second (columns) back down
JPEG_HD void jpeg_fdct8(int* d, int stride, bool first) {
  const int t0 = d[0] + d[7 * stride], t7 = d[0] - d[7 * stride], t1 = d[stride] + d[6 * stride], t6 = d[stride] - d[6 * stride];
  const int t2 = d[2 * stride] + d[5 * stride], t5 = d[2 * stride] - d[5 * stride], t3 = d[3 * stride] + d[4 * stride], t4 = d[3 * stride] - d[4 * stride];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  const int sh = first ? 11 : 15, half = 1 << (sh - 1);
  d[0] = first ? (t10 + t11) * 4 : (t10 + t11 + 2) >> 2;
  d[4 * stride] = first ? (t10 - t11) * 4 : (t10 - t11 + 2) >> 2;
  int z1 = (t12 + t13) * 4433;
  d[2 * stride] = (z1 + t13 * 6270 + half) >> sh;
  d[6 * stride] = (z1 - t12 * 15137 + half) >> sh;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7 * stride] = (a4 + z1 + z3 + half) >> sh;
  d[5 * stride] = (a5 + z2 + z4 + half) >> sh;
  d[3 * stride] = (a6 + z2 + z3 + half) >> sh;
  d[stride] = (a7 + z1 + z4 + half) >> sh;
}

// Block j of MCU `mcu` -> zz[64], zig-zag order.  quant u16 [2, 64] natural order.  A luma block outside the component's real blocks is a
// dummy: AC 0, DC that of the real block libjpeg's chain of copies ends at — (by, 0) in a real block row, else block (0, 1) when that
// column is real, else block (0, 0).
JPEG_HD void jpeg_enc_block(const JpegEncImage& im, const unsigned char* img, const unsigned short* quant, long mcu, int j, short* zz) {
  const int my = (int)(mcu / im.mcux), mx = (int)(mcu - (long)my * im.mcux);
  const int comp = j < im.lum ? 0 : j - im.lum + 1;
  int bx = mx, by = my;
  bool dummy = false;
  if (comp == 0) {
    const int rows = (im.h + 7) >> 3, cols = (im.w + 7) >> 3;
    by = my * im.hs + j / im.hs; bx = mx * im.hs + j % im.hs;
    if (by >= rows) { dummy = true; by = my * im.hs; bx = mx * im.hs + 1 < cols ? mx * im.hs + 1 : mx * im.hs; }
    else if (bx >= cols) { dummy = true; bx = mx * im.hs; }
  }
  int d[64];
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int c = 0; c < 8; ++c) d[8 * r + c] = jpeg_enc_sample(im, img, comp, 8 * bx + c, 8 * by + r) - 128;
#pragma unroll
  for (int r = 0; r < 8; ++r) jpeg_fdct8(d + 8 * r, 1, true);
#pragma unroll
  for (int c = 0; c < 8; ++c) jpeg_fdct8(d + c, 8, false);
  const unsigned short* q = quant + (comp ? 64 : 0);
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    const int n = jpeg_zigzag(k), q8 = 8 * (int)q[n], v = d[n], a = ((v < 0 ? -v : v) + (q8 >> 1)) / q8;
    zz[k] = (short)(dummy && k ? 0 : v < 0 ? -a : a);
  }
}

// Annex K.3 as (codes per length 1 .. 16, values); table t: 0 luma DC, 1 luma AC, 2 chroma DC, 3 chroma AC -> out[symbol] = code << 8 | length
JPEG_HD void jpeg_enc_tables(int t, unsigned* out) {
  const unsigned char counts[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                       {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
  const unsigned char ac[2][162] = {
      {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
       0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
       0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
       0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
       0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
       0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
       0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
       0xfa},
      {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
       0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
       0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
       0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
       0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
       0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
       0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
       0xfa}};
  for (int i = 0; i < JPEG_ENC_TABLE_WORDS; ++i) out[i] = 0u;
  unsigned code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < counts[t][len - 1]; ++i, ++k, ++code) out[(t & 1) ? ac[t >> 1][k] : k] = code << 8 | (unsigned)len;     // a DC table's values are 0 .. 11 in order
    code <<= 1;
  }
}

JPEG_HD int jpeg_enc_size(int v) {
  const unsigned a = (unsigned)(v < 0 ? -v : v);
  return a ? 32 - __builtin_clz(a) : 0;
}

// the block, inside its restart interval, whose DC predicts block i's (blocks in scan order, bpm a MCU, the first `lum` luma): -1 at the first
JPEG_HD int jpeg_enc_dc_from(int i, int bpm, int lum) {
  const int j = i % bpm;
  if (j < lum) return j ? i - 1 : i >= bpm ? i - bpm + lum - 1 : -1;
  return i >= bpm ? i - bpm : -1;
}

// The bits zig-zag position k of a block adds to the scan -> *val (the first bit highest), their count returned (at most 3 x 11 + 16 + 10 =
// 59).  tables: the four of jpeg_enc_tables; k = 0: v is the DC DIFFERENCE; k >= 1: v is the coefficient and nz the mask of the block's
// nonzero AC positions (bit k for position k), from which the run in front of it follows; position 63 carries the EOB when it is zero.
JPEG_HD int jpeg_enc_token(const unsigned* tables, bool chroma, int k, int v, unsigned long long nz, unsigned long long* val) {
  const unsigned* dc = tables + (chroma ? 2 : 0) * JPEG_ENC_TABLE_WORDS;
  const unsigned* ac = dc + JPEG_ENC_TABLE_WORDS;
  *val = 0;
  int s = jpeg_enc_size(v);
  const int most = k ? 10 : 11;
  s = s > most ? most : s;                                     // (a coefficient of this encoder never exceeds it)
  const unsigned long long extra = (unsigned long long)(unsigned)(v < 0 ? v + (1 << s) - 1 : v) & ((1ull << s) - 1ull);
  if (k == 0) {
    const unsigned e = dc[s];
    *val = (unsigned long long)(e >> 8) << s | extra;
    return (int)(e & 255u) + s;
  }
  if (v == 0) {
    if (k != 63) return 0;
    *val = ac[0] >> 8;
    return (int)(ac[0] & 255u);
  }
  const unsigned long long below = nz & ((1ull << k) - 1ull);
  const int run = k - 1 - (below ? 63 - __builtin_clzll(below) : 0);
  const unsigned e = ac[((run & 15) << 4) | s], z = ac[0xF0];
  unsigned long long out = 0;
  int n = 0;
  for (int i = 0; i < 3; ++i)
    if (i < (run >> 4)) { out = out << (z & 255u) | (z >> 8); n += (int)(z & 255u); }
  *val = out << ((e & 255u) + s) | (unsigned long long)(e >> 8) << s | extra;
  return n + (int)(e & 255u) + s;
}

// OR the n <= 64 bits of val (the first highest) into words from bit `at`: bit 31 of words[0] is bit 0 of the stream.  The device
// kernels' words live in LDS and lanes share them, hence the atomic there.
#if defined(__HIP_DEVICE_COMPILE__)
#define JPEG_ENC_OR(p, v) atomicOr((p), (v))
#else
#define JPEG_ENC_OR(p, v) (*(p) |= (v))
#endif
JPEG_HD void jpeg_enc_put(unsigned* words, unsigned at, unsigned long long val, int n) {
  if (n <= 0) return;
  const unsigned long long top = val << (64 - n);
  const int s = (int)(at & 31u);
  unsigned* w = words + (at >> 5);
  const unsigned long long head = top >> s;
  const unsigned a = (unsigned)(head >> 32), b = (unsigned)head, c = s ? (unsigned)((top << (64 - s)) >> 32) : 0u;
  if (a) JPEG_ENC_OR(w, a);
  if (b) JPEG_ENC_OR(w + 1, b);
  if (c) JPEG_ENC_OR(w + 2, c);
}
JPEG_HD unsigned jpeg_enc_byte(const unsigned* words, int i) { return (words[i >> 2] >> (24 - 8 * (i & 3))) & 255u; }
