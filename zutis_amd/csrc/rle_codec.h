// The COCO run-length string format (pycocotools maskApi.c rleEncode + rleToString), defined ONCE for the host entry points
// (rle_host.hip), the device kernels (mask_rle.hip) and, by reference, the capacity helper of zutis_amd/rle.py.  Inline functions only;
// compiles as plain C++ too (tools/host/rle_host_check.cpp).  zutis_amd/rle.py::_to_string / _from_string are the readable Python
// restatement the tests hold this file against.
//
// A mask's runs are taken in column-major order and start with the run of zeros (length 0 when pixel 0 is set).  Run k is stored as
// the value x_k = run_k for k <= 2, run_k - run_{k-2} from the fourth on; a value is written as little-endian 5-bit groups, bit 5 of
// a character = "more groups follow", + 48.  The last group's bit 4 is the sign the reader extends, so a value takes the smallest n with
//       -2^(5n-1) <= x < 2^(5n-1):
//       n = 1: -16 .. 15     2: |x| < 2^9     3: < 2^14     4: < 2^19     5: -2^24 <= x < 2^24     6: < 2^29     7: < 2^34
// (15 -> "?", 16 -> "`0": a positive value whose top group has bit 4 set needs one more all-zero group; likewise -17 -> "ON").
//
// THE CHARACTER BOUND.  Runs lie in [0, H*W] and deltas in [-H*W, H*W], so
//   * H*W < 2^24: every value takes at most 5 characters.  A mask with nt transitions has nc = nt + 1 + lead <= nt + 2 values: its
//     string is at most 5 nt + 10 characters.  This is the range in which zh_mask_rle_kept's budget — mask mi's string starts at
//     5 * off(mi) + 16 * rank(mi), i.e. 5 nt + 16 characters to the next mask's slot, and `out` is checked for 5 nc — is GUARANTEED.
//     zh_mask_rle_fused_kept (string buffer: 5 (max_runs + 2) bytes of LDS) is always inside it: the mask's bits must fit 150 KB of LDS.
//   * 2^24 <= H*W < 2^31 (RLE_FIVE_CHAR_PIXELS and up; all that zh_mask_rle_kept's argument check asks for): at most 7 characters
//     per value.  The budget above then has 16 - 5 (1 + lead) spare characters per mask and no more: a mask whose values of 2^24 and
//     more in magnitude outnumber that (e.g. 17 runs A, A, 1, 1, A, A, 1, 1, ... with A = 2^24 + 2, about 151 M pixels: 6 * 17 - 5 =
//     97 characters against 5 * 16 + 16 = 96) does not fit its slot.  In this range zh_mask_rle_kept therefore MEASURES the string
//     first (the sum of rle_groups over the mask's values) and writes it only when it fits [cstart, min(cstart + 5 nt + 16,
//     out_capacity)); otherwise it reports -1 and writes no character (the host encodes that mask).  Below 2^24 the kernel takes no
//     such pass: the 5 nc check is exact enough there.  tests/test_rle_guard_gpu.py runs the 17-run list between two neighbours.
//   * the host buffers of rle.py (_host_capacity) allow 8 characters per value: enough for every |x| < 2^34; the host entry points
//     check `cap` for every value all the same and return -1.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RLE_HD __host__ __device__ inline
#else
#define RLE_HD inline
#endif

// masks of fewer pixels than this have no value of more than 5 characters (the character bound above)
#define RLE_FIVE_CHAR_PIXELS (1L << 24)

// number of 5-bit groups (= characters) of a value
RLE_HD int rle_groups(long x) {
  int n = 0;
  bool more = true;
  while (more) {
    const long ch = x & 0x1f;
    x >>= 5;
    more = (ch & 0x10) ? x != -1 : x != 0;
    ++n;
  }
  return n;
}

// the emitter: the characters of x at q (rle_groups(x) of them, the caller has made room); returns their number
template <class C>
RLE_HD int rle_put(C* q, long x) {
  C* const q0 = q;
  bool more = true;
  while (more) {
    long ch = x & 0x1f;
    x >>= 5;
    more = (ch & 0x10) ? x != -1 : x != 0;
    if (more) ch |= 0x20;
    *q++ = (C)(ch + 48);
  }
  return (int)(q - q0);
}

// the bounded emitter of the host side: x behind the `len` characters `out` holds; the new length, or -1 (nothing written past `cap`)
RLE_HD long rle_put_bounded(char* out, long len, long cap, long x) {
  const int n = rle_groups(x);
  if (n > cap - len) return -1;
  return len + rle_put(out + len, x);
}

// the delta rule: runs from the fourth on are stored as their difference from the run two places back
RLE_HD bool rle_is_delta(long k) { return k > 2; }
RLE_HD long rle_delta(long k, long run_k, long run_k2) { return rle_is_delta(k) ? run_k - run_k2 : run_k; }

// run k in [0, nt + 1 + lead) of a mask from its transition list p[0 .. nt) (column-major pixel indices where the value changes):
// run e spans [edge(e), edge(e + 1)) with edge(0) = 0, edge(i) = p[i - 1], edge(nt + 1) = H*W; lead (pixel 0 is set) puts an empty
// run of zeros in front
template <class I>
RLE_HD long rle_run(const int* p, I nt, bool lead, long HW, I k) {
  if (lead) { if (k == 0) return 0; --k; }
  const long lo = k == 0 ? 0 : p[k - 1], hi = k == nt ? HW : p[k];
  return hi - lo;
}
// ... and the value stored for it (run k - 2 is read only where the delta rule asks for it)
template <class I>
RLE_HD long rle_value(const int* p, I nt, bool lead, long HW, I k) {
  long x = rle_run(p, nt, lead, HW, k);
  if (rle_is_delta(k)) x -= rle_run(p, nt, lead, HW, (I)(k - 2));
  return x;
}
