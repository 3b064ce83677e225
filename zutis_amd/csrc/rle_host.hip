// Host-side COCO RLE (pycocotools maskApi.c rleEncode + rleToString restated): the reference encodes every kept instance mask with
// pycocotools.mask.encode(np.asfortranarray(m)) (networks/zutis.py:290,448).  HOST pointers throughout; no kernel and no HIP call in
// this file — three loops over rle_codec.h that write into caller-sized buffers against `cap`, which is what
// tools/host/rle_host_check.cpp runs under the host sanitizers (tools/README.md).
#include "common.h"
#include "rle_codec.h"

// mask u8 [H,W] row-major; runs are taken in column-major order starting with the zeros run.  Returns the string length, or -1 if
// `cap` is too small.
extern "C" long zh_rle_encode_host(const unsigned char* mask, int H, int W, char* out, long cap) {
  long len = 0, k = 0, run = 0, c1 = 0, c2 = 0;             // c1, c2: runs k - 1, k - 2
  unsigned char cur = 0;
  auto emit = [&] {
    len = rle_put_bounded(out, len, cap, rle_delta(k, run, c2));
    c2 = c1; c1 = run; ++k;
    return len >= 0;
  };
  for (int x = 0; x < W; ++x)
    for (int y = 0; y < H; ++y) {
      const unsigned char v = mask[(long)y * W + x] != 0;
      if (v != cur) { if (!emit()) return -1; run = 0; cur = v; }
      ++run;
    }
  emit();
  return len;
}

// RLE string from run lengths (pycocotools rleToString): counts int64 [n] -> chars; returns length or -1.
extern "C" long zh_rle_counts_to_string_host(const long long* counts, long n, char* out, long cap) {
  long len = 0;
  for (long i = 0; i < n && len >= 0; ++i) len = rle_put_bounded(out, len, cap, rle_delta(i, (long)counts[i], i > 1 ? (long)counts[i - 2] : 0));
  return len;
}

// The RLE strings of n masks straight from zh_mask_runs' output, one call (rle_from_transitions was one numpy diff + one ctypes call
// per mask: 18 us each, 0.3 ms of a 0.7-ms batch-1 instance predict for 17 kept masks).  positions int32 [n, stride] (column-major
// pixel indices where the value changes, the first nruns[2 i] of row i), nruns int32 [n, 2] = {transitions, value of pixel 0}; the
// runs are rle_codec.h's rle_run.  Strings are written back to back into `out`; offsets int64 [n + 1].  Masks with more than `stride`
// transitions get an empty string (offsets equal): the caller falls back to the mask encoder.  Returns the total length or -1 when
// `cap` is too small.  packed != 0: `positions` is zh_mask_runs_kept's packed list — row i starts where row i - 1 ended,
// min(transitions, stride) entries each.
extern "C" long zh_rle_from_transitions_host(const int* positions, long stride, int packed, const int* nruns, long n, long HW, char* out,
                                             long cap, long long* offsets) {
  long len = 0, at = 0;
  for (long i = 0; i < n; ++i) {
    offsets[i] = len;
    const long nt = nruns[2 * i];
    const int* p = packed ? positions + at : positions + i * stride;
    at += nt < stride ? nt : stride;
    if (nt > stride) continue;
    const bool lead = nruns[2 * i + 1] != 0;
    for (long k = 0; k < nt + 1 + (lead ? 1 : 0); ++k)
      if ((len = rle_put_bounded(out, len, cap, rle_value(p, nt, lead, HW, k))) < 0) return -1;
  }
  offsets[n] = len;
  return len;
}
