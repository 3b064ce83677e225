// Device PNG encoder (zutis_amd/png_device.py is the definition): the pictures the file drivers write — label maps, id maps, colour
// overlays — leave the GPU as the finished zlib stream of their PNG, so that a writer thread only frames it (chunk CRCs) and writes.
//
//   zh_png_deflate   launch A, one workgroup per ZH_PNG_SEGMENT_BYTES of an image's FILTERED bytes (filter type 2, Up, per row):
//                      1. filter: lane-strided over the segment, row / column from the flat index, byte minus the byte above, into LDS;
//                         the segment's Adler pair s1 = sum d, s2 = sum (len - i) d on the way;
//                      2. each lane owns 64 consecutive bytes: a 64-bit mask of run heads (byte != previous byte);
//                      3. a forward max-scan of the lanes' last heads and a backward min-scan of their first heads give every byte its
//                         run's start and end (clipped to the segment);
//                      4. the closed form of png_device.run_tokens gives each token's bits; an exclusive scan gives its bit offset;
//                      5. lanes OR their tokens into zeroed LDS words (LDS atomics: order-independent, so the bytes are deterministic);
//                      6. the segment goes out coalesced to a fixed-stride slot of the workspace with (bytes, s1, s2).
//                    launch B, one workgroup per segment again: sum the byte counts in front of it, copy the slot to its place in the
//                    contiguous stream; segment 0 also writes 78 01, the last one folds the Adler pairs (B = n + sum s2_j + s1_j (n -
//                    end_j), A = 1 + sum s1_j: the per-segment recurrence B += len A + s2, A += s1 in closed form), appends 03 00 and
//                    the checksum and stores the length.
//
// An image that does not fit (bytes outside `images`, more segments than the grid, a stream bound outside `out`, sizes below 1 or
// beyond 2^31 - 1 filtered bytes) is not read and nothing of its stream is written; its length is -1.  Bytes past a stream's length
// inside its stride are never written.  Every index is derived from checked sizes; every loop is bounded by them.
#include "common.h"

#define PNG_THREADS 256
#define PNG_PER_LANE (ZH_PNG_SEGMENT_BYTES / PNG_THREADS)     // 64: one bit of a 64-bit head mask per byte
#define PNG_SEG_BOUND ((9 * ZH_PNG_SEGMENT_BYTES + 13 + 7) / 8 + 4)      // png_device.segment_bound(ZH_PNG_SEGMENT_BYTES) = 18438
#define PNG_SLOT ((PNG_SEG_BOUND + 15) / 16 * 16)           // a segment's slot in the workspace: 18448 bytes
#define PNG_OUT_WORDS (PNG_SLOT / 4)
#define PNG_META 4                               // int32 per slot: bytes, s1, s2, 0
#define PNG_ADLER 65521u

static_assert(PNG_PER_LANE == 64, "one head-mask bit per byte of a lane");

// byte i of the segment in LDS: one pad word per lane's 64 bytes, so that the lanes' byte walks (stride 17 words) hit distinct banks
__device__ __forceinline__ int png_pad(int i) { return i + ((i >> 6) << 2); }

struct PngImage { long long off; int h, w, rowb, n, nseg; long long bound; bool ok; };

__device__ __forceinline__ long long png_segment_bound(int n) { return (9LL * n + 13 + 7) / 8 + 4; }

__device__ __forceinline__ PngImage png_image(const long long* img_off, const int* hw, const long long* out_off, int b, int c, long image_bytes,
                                               long out_bytes, int max_segments) {
  PngImage im;
  im.off = img_off[b];
  im.h = hw[2 * b];
  im.w = hw[2 * b + 1];
  im.ok = false;
  im.rowb = 0; im.n = 0; im.nseg = 0; im.bound = 0;
  if (im.h < 1 || im.w < 1 || (long long)im.w * c + 1 > 0x7fffffffLL) return im;
  const long long rowb = (long long)im.w * c + 1, n = rowb * im.h;
  if (n > 0x6fffffffLL) return im;                                            // 9 n / 8 and the framing stay below 2^31
  if (im.off < 0 || im.off + (rowb - 1) * im.h > (long long)image_bytes) return im;
  im.rowb = (int)rowb;
  im.n = (int)n;
  im.nseg = (int)((n + ZH_PNG_SEGMENT_BYTES - 1) / ZH_PNG_SEGMENT_BYTES);
  const int rest = im.n % ZH_PNG_SEGMENT_BYTES;
  im.bound = 2 + (long long)(im.n / ZH_PNG_SEGMENT_BYTES) * PNG_SEG_BOUND + (rest ? png_segment_bound(rest) : 0) + 6;
  if (im.nseg > max_segments || im.bound > 0x7fffffffLL) return im;
  const long long oo = out_off[b];
  if (oo < 0 || oo + im.bound > (long long)out_bytes) return im;
  im.ok = true;
  return im;
}

// (value, bits) of a literal / of a match of length 3 .. 258 at distance 1, as they enter the stream from bit 0 (RFC 1951 3.2.5, 3.2.6)
__device__ __forceinline__ void png_literal(unsigned v, unsigned& val, int& nb) {
  if (v < 144) { val = __brev(0x30u + v) >> 24; nb = 8; }
  else { val = __brev(0x190u + v - 144u) >> 23; nb = 9; }
}
__device__ __forceinline__ void png_match(int len, unsigned& val, int& nb) {
  int sym, eb;
  const int x = len - 3;
  if (len == 258) { sym = 285; eb = 0; }
  else if (x < 8) { sym = 257 + x; eb = 0; }
  else { eb = (31 - __clz(x)) - 2; sym = 265 + 4 * (eb - 1) + ((x >> eb) & 3); }
  const unsigned extra = (unsigned)x & ((1u << eb) - 1u);
  int cb;
  unsigned code;
  if (sym < 280) { code = __brev((unsigned)(sym - 256)) >> 25; cb = 7; }
  else { code = __brev(0xC0u + (unsigned)(sym - 280)) >> 24; cb = 8; }
  val = code | ((len == 258 ? 0u : extra) << cb);                            // the 5-bit distance code 0 adds zero bits
  nb = cb + eb + 5;
}

// The tokens of one lane's bytes [base, base + nv) of the segment.  EMIT = false: their bit count.  EMIT = true: OR them into `out` from
// bit offset `bit`.  heads: bit i = byte base + i starts a run; s0 / e_next: start of the run that holds byte `base` when it is not a head /
// the first head behind the lane's bytes (the segment's length when there is none).
template <bool EMIT>
__device__ __forceinline__ unsigned png_lane_tokens(const unsigned char* s_d, unsigned* out, unsigned long long heads, int base, int nv, int s0,
                                                    int e_next, unsigned bit) {
  unsigned long long acc = 0;          // bits not yet flushed, from bit (bit & 31) of word `word`
  int word = (int)(bit >> 5), have = (int)(bit & 31);
  unsigned total = 0;
  int i = 0, s = s0, e = heads ? base + __builtin_ctzll(heads) : e_next;
  while (i < nv) {
    const int pos = base + i;
    if ((heads >> i) & 1ull) {
      s = pos;
      const unsigned long long rest = i < 63 ? heads >> (i + 1) : 0ull;
      e = rest ? pos + 1 + __builtin_ctzll(rest) : e_next;
    }
    const int k = pos - s, L = e - s;
    unsigned val = 0;
    int nb = 0, step = 1;
    bool literal = k == 0;
    if (!literal) {
      const int j = k - 1, q = j / 258, m = j - q * 258, tail = L - 1 - 258 * q;
      if (tail < 3) literal = true;
      else {
        const int len = min(258, tail);
        if (m == 0) png_match(len, val, nb);
        step = len - m;                                                      // the rest of the match covers these bytes: no token
      }
    }
    if (literal) png_literal(s_d[png_pad(pos)], val, nb);
    if (EMIT && nb) {
      acc |= (unsigned long long)val << have;
      have += nb;
      if (have >= 32) {
        atomicOr(&out[word], (unsigned)acc);
        acc >>= 32;
        have -= 32;
        ++word;
      }
    }
    total += nb;
    i += step;
  }
  if (EMIT && have && acc) atomicOr(&out[word], (unsigned)acc);
  return total;
}

__global__ __launch_bounds__(PNG_THREADS) void png_segments_kernel(const unsigned char* images, long image_bytes, const long long* img_off,
                                                                   const int* hw, int c, int max_segments, const long long* out_off,
                                                                   long out_bytes, int* meta, unsigned char* slots) {
  __shared__ unsigned char s_d[ZH_PNG_SEGMENT_BYTES + PNG_THREADS * 4];
  __shared__ unsigned s_out[PNG_OUT_WORDS];
  __shared__ int s_a[PNG_THREADS];
  __shared__ int s_b[PNG_THREADS];
  const int b = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x;
  const PngImage im = png_image(img_off, hw, out_off, b, c, image_bytes, out_bytes, max_segments);
  if (!im.ok || seg >= im.nseg) return;                                      // block-uniform, in front of every barrier
  const int g0 = seg * ZH_PNG_SEGMENT_BYTES, len = min(ZH_PNG_SEGMENT_BYTES, im.n - g0);
  const unsigned char* img = images + im.off;

  for (int w = tid; w < PNG_OUT_WORDS; w += PNG_THREADS) s_out[w] = 0u;
  // 1. filter; byte g of the filtered data is row g / rowb, column g % rowb: column 0 is the filter byte, column x the image byte x - 1
  unsigned s1 = 0, s2 = 0;                                                   // 64 bytes a lane: s2 < 64 * 255 * 16384 < 2^32
  {
    int row = (g0 + tid) / im.rowb, col = (g0 + tid) - row * im.rowb;
    const int dq = PNG_THREADS / im.rowb, dr = PNG_THREADS - dq * im.rowb;
    for (int i = tid; i < len; i += PNG_THREADS) {
      unsigned d = 2u;
      if (col > 0) {
        const long long at = (long long)row * (im.rowb - 1) + (col - 1);
        const unsigned cur = img[at], up = row > 0 ? img[at - (im.rowb - 1)] : 0u;
        d = (cur - up) & 255u;
      }
      s_d[png_pad(i)] = (unsigned char)d;
      s1 += d;
      s2 += (unsigned)(len - i) * d;
      row += dq;
      col += dr;
      if (col >= im.rowb) { col -= im.rowb; ++row; }
    }
  }
  __syncthreads();
  // 2. the lane's 64 bytes: run heads
  const int base = tid * PNG_PER_LANE, nv = max(0, min(PNG_PER_LANE, len - base));
  unsigned long long heads = 0;
  if (nv > 0) {
    int prev = base > 0 ? (int)s_d[png_pad(base - 1)] : -1;                  // byte 0 of the segment always starts a run
    for (int i = 0; i < nv; ++i) {
      const int v = s_d[png_pad(base + i)];
      heads |= (unsigned long long)(v != prev) << i;
      prev = v;
    }
  }
  // 3. last head at or before each lane's bytes (forward max), first head behind them (backward min)
  s_a[tid] = heads ? base + 63 - __builtin_clzll(heads) : -1;
  s_b[tid] = heads ? base + __builtin_ctzll(heads) : len;
  __syncthreads();
  for (int o = 1; o < PNG_THREADS; o <<= 1) {
    const int a = tid >= o ? s_a[tid - o] : -1, z = tid + o < PNG_THREADS ? s_b[tid + o] : len;
    __syncthreads();
    s_a[tid] = max(s_a[tid], a);
    s_b[tid] = min(s_b[tid], z);
    __syncthreads();
  }
  const int s0 = tid > 0 ? s_a[tid - 1] : 0, e_next = tid + 1 < PNG_THREADS ? s_b[tid + 1] : len;
  __syncthreads();
  // 4. bits of the lane's tokens, their exclusive scan behind the block's 3 header bits
  const unsigned bits = png_lane_tokens<false>(s_d, s_out, heads, base, nv, s0, e_next, 0u);
  s_a[tid] = (int)bits;
  __syncthreads();
  for (int o = 1; o < PNG_THREADS; o <<= 1) {
    const int a = tid >= o ? s_a[tid - o] : 0;
    __syncthreads();
    s_a[tid] += a;
    __syncthreads();
  }
  const unsigned incl = (unsigned)s_a[tid], token_bits = (unsigned)s_a[PNG_THREADS - 1];
  // 5. emit: BFINAL = 0, BTYPE = 01 (bits 0, 1, 0), the tokens; end-of-block (7) and the stored block's header (3) are zero bits
  if (tid == 0) atomicOr(&s_out[0], 2u);
  png_lane_tokens<true>(s_d, s_out, heads, base, nv, s0, e_next, 3u + incl - bits);
  const int body = (int)((3u + token_bits + 10u + 7u) >> 3), nbytes = body + 4;        // then 00 00 FF FF
  __syncthreads();
  if (tid < 2) ((unsigned char*)s_out)[body + 2 + tid] = 0xFF;
  // the Adler pair of the segment
  s_b[tid] = (int)(s2 % PNG_ADLER);
  __syncthreads();                                                           // also: every s_a read above is done
  s_a[tid] = (int)s1;
  __syncthreads();
  for (int o = PNG_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) { s_a[tid] += s_a[tid + o]; s_b[tid] += s_b[tid + o]; }    // s1 <= 16384 * 255, s2 <= 256 * 65520
    __syncthreads();
  }
  // 6. the slot
  const long slot = (long)b * max_segments + seg;
  unsigned* dst = (unsigned*)(slots + slot * PNG_SLOT);
  for (int w = tid; w < (nbytes + 3) / 4; w += PNG_THREADS) dst[w] = s_out[w];
  if (tid == 0) {
    int* mt = meta + slot * PNG_META;
    mt[0] = nbytes;
    mt[1] = (int)((unsigned)s_a[0] % PNG_ADLER);
    mt[2] = (int)((unsigned)s_b[0] % PNG_ADLER);
    mt[3] = 0;
  }
}

__global__ __launch_bounds__(PNG_THREADS) void png_gather_kernel(long image_bytes, const long long* img_off, const int* hw, int c, int max_segments,
                                                                 const long long* out_off, long out_bytes, const int* meta,
                                                                 const unsigned char* slots, unsigned char* out, int* lengths) {
  __shared__ unsigned long long s_r[3][PNG_THREADS];
  const int b = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x;
  const PngImage im = png_image(img_off, hw, out_off, b, c, image_bytes, out_bytes, max_segments);
  if (!im.ok) {
    if (seg == 0 && tid == 0) lengths[b] = -1;
    return;
  }
  if (seg >= im.nseg) return;
  const bool last = seg == im.nseg - 1;
  const int* mt = meta + (long)b * max_segments * PNG_META;
  // bytes in front of this segment; the last segment also folds the Adler pairs of all of them
  unsigned long long front = 0, a = 0, bb = 0;
  for (int j = tid; j < im.nseg; j += PNG_THREADS) {
    if (j < seg) front += (unsigned)mt[j * PNG_META];
    if (last) {
      const unsigned long long e1 = (unsigned)mt[j * PNG_META + 1], e2 = (unsigned)mt[j * PNG_META + 2];
      const long long end = min((long long)(j + 1) * ZH_PNG_SEGMENT_BYTES, (long long)im.n);
      a += e1;                                                               // < 65521 each, at most 2^31 / 16384 segments
      bb = (bb + e2 + e1 * (unsigned long long)((im.n - end) % PNG_ADLER)) % PNG_ADLER;
    }
  }
  s_r[0][tid] = front; s_r[1][tid] = a; s_r[2][tid] = bb;
  __syncthreads();
  for (int o = PNG_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) { s_r[0][tid] += s_r[0][tid + o]; s_r[1][tid] += s_r[1][tid + o]; s_r[2][tid] += s_r[2][tid + o]; }
    __syncthreads();
  }
  front = s_r[0][0];
  const int nbytes = mt[seg * PNG_META];
  if (nbytes < 4 || nbytes > PNG_SEG_BOUND || 2 + front + nbytes + 6 > (unsigned long long)im.bound) return;      // never past the image's stride
  unsigned char* dst = out + out_off[b];
  const unsigned char* src = slots + ((long)b * max_segments + seg) * PNG_SLOT;
  for (int i = tid; i < nbytes; i += PNG_THREADS) dst[2 + front + i] = src[i];
  if (seg == 0 && tid < 2) dst[tid] = tid == 0 ? 0x78 : 0x01;
  if (last && tid == 0) {
    const unsigned A = (unsigned)((1ull + s_r[1][0]) % PNG_ADLER);
    const unsigned B = (unsigned)(((unsigned long long)(im.n % PNG_ADLER) + s_r[2][0]) % PNG_ADLER);
    unsigned char* t = dst + 2 + front + nbytes;
    t[0] = 0x03; t[1] = 0x00;                                                // a final empty fixed block
    t[2] = (unsigned char)(B >> 8); t[3] = (unsigned char)B; t[4] = (unsigned char)(A >> 8); t[5] = (unsigned char)A;
    lengths[b] = (int)(2 + front + nbytes + 6);
  }
}

extern "C" size_t zh_png_deflate_workspace_size(int B, int max_segments) {
  if (B < 1 || max_segments < 1) return 0;
  return (size_t)B * (size_t)max_segments * (PNG_SLOT + PNG_META * sizeof(int));
}

extern "C" int zh_png_deflate(const unsigned char* images, long image_bytes, const long long* img_off, const int* hw, int c, int B,
                              int max_segments, const long long* out_off, unsigned char* out, long out_bytes, int* lengths, void* workspace,
                              size_t workspace_bytes, hipStream_t stream) {
  ZH_CHECK_ARG(c == 1 || c == 3, "zh_png_deflate: c = %d is not 1 or 3", c);
  ZH_CHECK_ARG(B >= 0 && B <= 65535, "zh_png_deflate: B = %d outside 0 .. 65535", B);
  ZH_CHECK_ARG(max_segments >= 0 && image_bytes >= 0 && out_bytes >= 0, "zh_png_deflate: negative count");
  if (B == 0) return ZH_OK;
  ZH_CHECK_ARG(max_segments >= 1, "zh_png_deflate: max_segments = 0 for %d images (an image has at least one segment)", B);
  ZH_CHECK_ARG(images && img_off && hw && out_off && out && lengths && workspace, "zh_png_deflate: null pointer");
  ZH_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "zh_png_deflate: workspace must be 16-byte aligned");
  if (workspace_bytes < zh_png_deflate_workspace_size(B, max_segments)) {
    zh_set_error("zh_png_deflate: workspace holds %zu bytes, %zu needed", workspace_bytes, zh_png_deflate_workspace_size(B, max_segments));
    return ZH_ERR_WORKSPACE;
  }
  // slots first (16-byte aligned, PNG_SLOT is a multiple of 16), the (bytes, s1, s2, 0) words behind them
  unsigned char* slots = (unsigned char*)workspace;
  int* meta = (int*)(slots + (size_t)B * max_segments * PNG_SLOT);
  hipLaunchKernelGGL(png_segments_kernel, dim3(max_segments, B), dim3(PNG_THREADS), 0, stream, images, image_bytes, img_off, hw, c, max_segments,
                     out_off, out_bytes, meta, slots);
  ZH_CHECK_LAUNCH("zh_png_deflate (segments)");
  hipLaunchKernelGGL(png_gather_kernel, dim3(max_segments, B), dim3(PNG_THREADS), 0, stream, image_bytes, img_off, hw, c, max_segments, out_off,
                     out_bytes, (const int*)meta, (const unsigned char*)slots, out, lengths);
  ZH_CHECK_LAUNCH("zh_png_deflate (gather)");
  return ZH_OK;
}
