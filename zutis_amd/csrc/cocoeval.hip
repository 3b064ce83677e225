// COCO mask AP on the device (zutis_amd/coco_eval.py): what pycocotools' COCOeval.evaluate spends its time on for iouType "segm" —
// the IoU of every (detection, ground truth) pair of a group from the masks' run lengths (maskApi rleIou) and the greedy matching
// of COCOeval.evaluateImg per (group, area range, IoU threshold) — as three launches per call (trainer.py:255-292 -> cocoeval).
//
//   zh_rle_prefix    one wave per mask: a wave scan over the run counts (column-major, zeros first) gives every run's end position and
//                    the number of foreground pixels in front of it, and the mask's area.  A mask whose counts are negative or do
//                    not sum to its h * w gets its bit in `status` and takes no further part.
//   zh_rle_pair_iou  one wave per pair.  rleIou walks both run lists with two pointers, serially; here the lanes stride over the
//                    detection's foreground runs and the overlap of a run [s, e) with the ground truth is F_g(e) - F_g(s), F_g(x) =
//                    the ground truth's foreground in front of position x = one binary search over its run ends + the prefix array.
//                    The ground truth's two arrays are staged in LDS up to ZH_RLE_IOU_LDS_RUNS runs and searched in global memory above.
//   zh_coco_match    one lane per (group, area range, threshold): the T * A problems of a group share a wave, each lane runs
//                    evaluateImg's serial walk (csrc/assign.hip is the precedent for a serial solver per lane).
//
// Every loop is bounded by a count read from a descriptor the host built, every search by 32 steps; integers are exact and the
// IoU is ONE float64 division of two integers, so it is NumPy's bit for bit.
#include "common.h"

// ZH_RLE_IOU_LDS_RUNS = 1024 runs: 8 KB of LDS per wave, 20 waves a CU
#define CM_MAX_PROBLEMS 64         // T * A problems of a group = lanes of its wave
#define GROUP_WORDS 8              // det_off, D, gt_off, G, pair_off, 0, 0, 0

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- zh_rle_prefix --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rle_prefix_kernel(const int* counts, const int* run_off, const int* hw, int* run_end, int* run_fg,
                                                        int* area, int* status) {
  const int m = blockIdx.x, lane = threadIdx.x;
  const int o = run_off[m], n = run_off[m + 1] - o;
  long long end_carry = 0, fg_carry = 0;      // 64-bit: malformed counts may not wrap into a sum that looks right
  int bad = 0;
  for (int k0 = 0; k0 < n; k0 += 64) {
    const int k = k0 + lane;
    const int c = k < n ? counts[o + k] : 0;
    bad |= c < 0;
    long long e = c, f = (k & 1) ? c : 0;     // inclusive scans of the counts and of the foreground (odd) counts
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const long long pe = __shfl_up(e, s, 64), pf = __shfl_up(f, s, 64);
      if (lane >= s) { e += pe; f += pf; }
    }
    e += end_carry;
    f += fg_carry;
    if (k < n) {
      const long long before = f - ((k & 1) ? c : 0);
      bad |= e > 0x7fffffffLL;
      run_end[o + k] = (int)(e > 0x7fffffffLL ? 0x7fffffffLL : (e < 0 ? 0 : e));
      run_fg[o + k] = (int)(before > 0x7fffffffLL ? 0x7fffffffLL : (before < 0 ? 0 : before));
    }
    end_carry = __shfl(e, 63, 64);
    fg_carry = __shfl(f, 63, 64);
  }
  bad |= end_carry != (long long)hw[m];
  if (__ballot(bad) != 0ull) {
    if (lane == 0) { atomicOr(status + (m >> 5), 1 << (m & 31)); area[m] = 0; }
  } else if (lane == 0) {
    area[m] = (int)fg_carry;
  }
}

// ---- zh_rle_pair_iou ------------------------------------------------------------------------------------------------------------
// foreground of a mask in front of position x: k = number of run ends <= x (the run that holds x), bounded binary search
template <typename P>
__device__ __forceinline__ int rle_fg_before(P ends, P fgs, int n, int area, int x) {
  int lo = 0, hi = n;
  for (int step = 0; step < 32 && lo < hi; ++step) {
    const int mid = (lo + hi) >> 1;
    if (ends[mid] <= x) lo = mid + 1; else hi = mid;
  }
  if (lo >= n) return area;
  return fgs[lo] + ((lo & 1) ? x - (lo ? ends[lo - 1] : 0) : 0);
}

__global__ __launch_bounds__(64) void rle_pair_iou_kernel(const int* run_end, const int* run_fg, const int* run_off, const int* area,
                                                          const int* status, const int* groups, int n_groups, const int* det_mask,
                                                          const int* gt_mask, const int* gt_crowd, long n_pairs, int* inter, double* iou) {
  __shared__ int s_end[ZH_RLE_IOU_LDS_RUNS];
  __shared__ int s_fg[ZH_RLE_IOU_LDS_RUNS];
  const int lane = threadIdx.x;
  const long p = blockIdx.x;
  if (p >= n_pairs) return;
  // the group of pair p: the last one whose pair_off is <= p (groups without pairs share their successor's offset)
  int lo = 0, hi = n_groups;
  for (int step = 0; step < 32 && hi - lo > 1; ++step) {
    const int mid = (lo + hi) >> 1;
    if ((long)groups[GROUP_WORDS * mid + 4] <= p) lo = mid; else hi = mid;
  }
  const int* g = groups + GROUP_WORDS * lo;
  const int D = g[1], G = g[3];
  const long local = p - g[4];
  if (D <= 0 || G <= 0 || local < 0 || local >= (long)D * G) return;
  const int d = (int)(local / G), gi = (int)(local - (long)d * G);
  const int md = det_mask[g[0] + d], mg = gt_mask[g[2] + gi];
  if (((status[md >> 5] >> (md & 31)) | (status[mg >> 5] >> (mg & 31))) & 1) {       // a malformed mask: no pixels are read
    if (lane == 0) { inter[p] = -1; iou[p] = -1.0; }
    return;
  }
  const int od = run_off[md], nd = run_off[md + 1] - od;
  const int og = run_off[mg], ng = run_off[mg + 1] - og;
  const int ad = area[md], ag = area[mg];
  const bool staged = ng <= ZH_RLE_IOU_LDS_RUNS;
  if (staged) {
    for (int k = lane; k < ng; k += 64) { s_end[k] = run_end[og + k]; s_fg[k] = run_fg[og + k]; }
    __syncthreads();
  }
  int acc = 0;
  for (int k = 1 + 2 * lane; k < nd; k += 128) {          // the detection's foreground runs are its odd ones
    const int s = run_end[od + k - 1], e = run_end[od + k];
    if (e > s) {
      if (staged) acc += rle_fg_before(s_end, s_fg, ng, ag, e) - rle_fg_before(s_end, s_fg, ng, ag, s);
      else acc += rle_fg_before(run_end + og, run_fg + og, ng, ag, e) - rle_fg_before(run_end + og, run_fg + og, ng, ag, s);
    }
  }
  acc = wave_sum_i(acc);
  if (lane == 0) {
    // rleIou: no intersection is 0 whatever the union (an empty detection against an empty ground truth is 0, not 0 / 0)
    const long long uni = gt_crowd[g[2] + gi] ? (long long)ad : (long long)ad + (long long)ag - (long long)acc;
    inter[p] = acc;
    iou[p] = acc == 0 ? 0.0 : (double)acc / (double)uni;
  }
}

// ---- zh_coco_match --------------------------------------------------------------------------------------------------------------
// COCOeval.evaluateImg.  gt_order / gt_ignore [A][n_gt]: per area range the group's ground truths ignored-last (stable) as indices
// local to the group, and their ignore flags in that order.  taken u8 [n_gt][T * A]: this lane's matched flags, by sorted position.
__global__ __launch_bounds__(64) void coco_match_kernel(const double* iou, const int* groups, const int* det_mask, const int* area,
                                                        const int* gt_order, const int* gt_ignore, const int* gt_crowd, long n_gt,
                                                        const double* thresholds, int T, const double* area_ranges, int A, int* match,
                                                        unsigned char* ignore, unsigned char* taken) {
  const int lane = threadIdx.x;
  const int P = T * A;
  if (lane >= P) return;
  const int* g = groups + GROUP_WORDS * (long)blockIdx.x;
  const int det_off = g[0], D = g[1], gt_off = g[2], G = g[3];
  const long pair_off = g[4];
  const int a = lane / T, t = lane - a * T;
  const double thr = fmin(thresholds[t], 1.0 - 1e-10);
  const double a_lo = area_ranges[2 * a], a_hi = area_ranges[2 * a + 1];
  const int* ord = gt_order + (long)a * n_gt + gt_off;
  const int* ign = gt_ignore + (long)a * n_gt + gt_off;
  const int* crowd = gt_crowd + gt_off;
  unsigned char* tk = taken + (long)gt_off * P + lane;
  for (int j = 0; j < G; ++j) tk[(long)j * P] = 0;
  for (int d = 0; d < D; ++d) {
    const double* row = iou + pair_off + (long)d * G;
    double best = thr;
    int m = -1;
    for (int j = 0; j < G; ++j) {
      const int gl = ord[j];
      if (tk[(long)j * P] && !crowd[gl]) continue;          // matched at this threshold already, and not a crowd
      if (m > -1 && ign[m] == 0 && ign[j] == 1) break;      // a regular match is held and only ignored ones follow
      const double v = row[gl];
      if (v < best) continue;
      best = v;                                             // among equal IoUs the later one wins
      m = j;
    }
    const long o = (long)(det_off + d) * P + lane;
    if (m < 0) {
      const double ar = (double)area[det_mask[det_off + d]];
      match[o] = -1;
      ignore[o] = (ar < a_lo || ar > a_hi) ? 1 : 0;
    } else {
      tk[(long)m * P] = 1;
      match[o] = ord[m];
      ignore[o] = ign[m] ? 1 : 0;
    }
  }
}

extern "C" int zh_rle_iou_lds_runs(void) { return ZH_RLE_IOU_LDS_RUNS; }

extern "C" int zh_rle_prefix(const int* counts, const int* run_off, const int* hw, int n_masks, int* run_end, int* run_fg, int* area,
                             int* status, hipStream_t stream) {
  ZH_CHECK_ARG(n_masks >= 0, "zh_rle_prefix: negative mask count");
  if (n_masks == 0) return ZH_OK;                             // no empty grid
  ZH_CHECK_ARG(counts && run_off && hw && run_end && run_fg && area && status, "zh_rle_prefix: null pointer");
  hipLaunchKernelGGL(rle_prefix_kernel, dim3(n_masks), dim3(64), 0, stream, counts, run_off, hw, run_end, run_fg, area, status);
  ZH_CHECK_LAUNCH("zh_rle_prefix");
  return ZH_OK;
}

extern "C" int zh_rle_pair_iou(const int* run_end, const int* run_fg, const int* run_off, const int* area, const int* status,
                               const int* groups, int n_groups, const int* det_mask, const int* gt_mask, const int* gt_crowd,
                               long n_pairs, int* inter, double* iou, hipStream_t stream) {
  ZH_CHECK_ARG(n_groups >= 0 && n_pairs >= 0, "zh_rle_pair_iou: negative count");
  ZH_CHECK_ARG(n_pairs <= 0x7fffffffL, "zh_rle_pair_iou: %ld pairs in one call (at most 2^31 - 1: evaluate in chunks)", n_pairs);
  if (n_pairs == 0 || n_groups == 0) return ZH_OK;            // groups without detections or ground truths: nothing to launch
  ZH_CHECK_ARG(run_end && run_fg && run_off && area && status && groups && det_mask && gt_mask && gt_crowd && inter && iou,
               "zh_rle_pair_iou: null pointer");
  ZH_CHECK_ARG(((uintptr_t)iou & 7) == 0, "zh_rle_pair_iou: iou must be 8-byte aligned");
  hipLaunchKernelGGL(rle_pair_iou_kernel, dim3((unsigned)n_pairs), dim3(64), 0, stream, run_end, run_fg, run_off, area, status, groups,
                     n_groups, det_mask, gt_mask, gt_crowd, n_pairs, inter, iou);
  ZH_CHECK_LAUNCH("zh_rle_pair_iou");
  return ZH_OK;
}

extern "C" size_t zh_coco_match_workspace_size(long n_gt, int T, int A) {
  return (size_t)(n_gt > 0 ? n_gt : 0) * (size_t)(T > 0 ? T : 0) * (size_t)(A > 0 ? A : 0);
}

extern "C" int zh_coco_match(const double* iou, const int* groups, int n_groups, const int* det_mask, const int* area,
                             const int* gt_order, const int* gt_ignore, const int* gt_crowd, long n_gt, const double* thresholds, int T,
                             const double* area_ranges, int A, int* match, unsigned char* ignore, void* workspace,
                             size_t workspace_bytes, hipStream_t stream) {
  ZH_CHECK_ARG(n_groups >= 0 && n_gt >= 0, "zh_coco_match: negative count");
  ZH_CHECK_ARG(T > 0 && A > 0 && T * A <= CM_MAX_PROBLEMS, "zh_coco_match: T * A = %d problems per group (1 .. %d: the lanes of a wave)",
               T * A, CM_MAX_PROBLEMS);
  if (n_groups == 0) return ZH_OK;
  ZH_CHECK_ARG(groups && det_mask && area && thresholds && area_ranges && match && ignore, "zh_coco_match: null pointer");
  ZH_CHECK_ARG(n_gt == 0 || (iou && gt_order && gt_ignore && gt_crowd && workspace), "zh_coco_match: null ground-truth table");
  ZH_CHECK_ARG((((uintptr_t)iou | (uintptr_t)thresholds | (uintptr_t)area_ranges) & 7) == 0, "zh_coco_match: misaligned float64 table");
  if (workspace_bytes < zh_coco_match_workspace_size(n_gt, T, A)) {
    zh_set_error("zh_coco_match: workspace too small");
    return ZH_ERR_WORKSPACE;
  }
  hipLaunchKernelGGL(coco_match_kernel, dim3(n_groups), dim3(64), 0, stream, iou, groups, det_mask, area, gt_order, gt_ignore, gt_crowd,
                     n_gt, thresholds, T, area_ranges, A, match, ignore, (unsigned char*)workspace);
  ZH_CHECK_LAUNCH("zh_coco_match");
  return ZH_OK;
}
