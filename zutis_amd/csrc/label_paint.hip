// Semantic ground truth from annotations (zutis_amd/annotation_labels.py): the label maps the reference's COCO datasets open at
// {dir_dataset}/annotations/semantic_segmentation_masks/{stem}.png (datasets/coco2017.py:134, datasets/coco20k.py:178), painted from
// the annotations' run lengths as zh_rle_prefix leaves them.
//
//   zh_runs_label_maps   B images in one launch, one lane per output pixel of a 32 x 8 tile, as a GATHER: the lane's column-major position
//                        p = x * h + y is looked up in the run ends of each entry of its image's paint list, walked from the last entry
//                        to the first — the pixel is covered when the index of the first run end greater than p is odd — and the walk
//                        stops at the first hit ("last") or at the second ("ignore").  Every pixel has one writer and reads only what the
//                        launch does not write: no atomics, no order between workgroups, the same bytes every time.
//
// The list has no cap: the workgroup stages LP_STAGE entries at a time in LDS, from the list's end — per entry where its runs start, how
// many there are, its label, and whether it can touch the tile at all (the columns between its first and its last covered position,
// read from run_end, against the tile's 32 columns).  A pass that leaves every lane of the tile done ends the walk.  Runs are read
// from global memory through the cache, so there is no cap on the runs of a mask either.
// Every loop is bounded by a count the launch checks against the arrays' lengths, every search by 32 steps.
#include "common.h"

#define LP_THREADS (ZH_LABEL_TILE_W * ZH_LABEL_TILE_H)    // a 32 x 8 tile: a wave stores two 32-byte row segments
#define LP_STAGE 256      // list entries staged per pass: one per thread, 3 KB of LDS

__global__ __launch_bounds__(LP_THREADS) void runs_label_maps_kernel(const int* run_end, const int* run_off, const int* status, int n_masks,
                                                                      long n_runs, const int* list_off, const int* list_mask,
                                                                      const unsigned char* list_label, int n_list, const int* hw, const long long* out_off,
                                                                      long out_bytes, int overlap, int ignore_value, unsigned char* out) {
  __shared__ int s_o[LP_STAGE];        // first run of the entry's mask, -1: the entry cannot touch this tile (or is not painted)
  __shared__ int s_n[LP_STAGE];        // its number of runs
  __shared__ int s_label[LP_STAGE];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int h = hw[2 * b], w = hw[2 * b + 1];
  if (h < 1 || w < 1 || (long)h * w > 0x7fffffffL) return;                     // block-uniform, as every exit in front of a barrier
  const int tiles_x = (w + ZH_LABEL_TILE_W - 1) / ZH_LABEL_TILE_W, tiles_y = (h + ZH_LABEL_TILE_H - 1) / ZH_LABEL_TILE_H;
  if ((long)blockIdx.x >= (long)tiles_x * tiles_y) return;
  const long long base = out_off[b];
  if (base < 0 || base + (long long)h * w > (long long)out_bytes) return;       // an image that does not fit its buffer is not written
  const int x0 = ((int)blockIdx.x % tiles_x) * ZH_LABEL_TILE_W, y0 = ((int)blockIdx.x / tiles_x) * ZH_LABEL_TILE_H;
  const int x = x0 + (tid & (ZH_LABEL_TILE_W - 1)), y = y0 + tid / ZH_LABEL_TILE_W;
  const bool inb = x < w && y < h;
  const int p = inb ? x * h + y : 0;                                           // < h * w <= 2^31 - 1
  const int c_lo = x0, c_hi = min(x0 + ZH_LABEL_TILE_W, w) - 1;                          // the tile's columns
  const int l0 = list_off[b], l1 = (l0 < 0 || list_off[b + 1] > n_list) ? l0 : list_off[b + 1];    // a list outside the arrays: empty
  int hits = 0, label = 0;
  bool done = !inb;
  for (int hi = l1; hi > l0; hi -= LP_STAGE) {
    const int lo = max(l0, hi - LP_STAGE), n = hi - lo;
    if (tid < n) {
      const int m = list_mask[lo + tid];
      int o = -1, nr = 0;
      if (m >= 0 && m < n_masks && !((status[m >> 5] >> (m & 31)) & 1)) {      // a mask zh_rle_prefix flagged paints nothing
        const int ro = run_off[m];
        nr = run_off[m + 1] - ro;
        if (ro >= 0 && nr >= 2 && (long)ro + nr <= n_runs) {                   // fewer than two runs: no pixel
          const int first = run_end[ro];                                       // covered positions lie in [first, last)
          const int last = (nr & 1) ? run_end[ro + nr - 2] : run_end[ro + nr - 1];
          if (last > first && first / h <= c_hi && (last - 1) / h >= c_lo) o = ro;
        }
      }
      s_o[tid] = o;
      s_n[tid] = nr;
      s_label[tid] = list_label[lo + tid];
    }
    __syncthreads();
    if (!done) {
      for (int k = n - 1; k >= 0; --k) {                                       // the last entry first
        const int o = s_o[k];
        if (o < 0) continue;
        const int nr = s_n[k];
        int a = 0, z = nr;                                                     // a = number of run ends <= p = the run that holds p
        for (int step = 0; step < 32 && a < z; ++step) {
          const int mid = (a + z) >> 1;
          if (run_end[o + mid] <= p) a = mid + 1; else z = mid;
        }
        if (a < nr && (a & 1)) {                                               // odd runs are foreground
          if (hits == 0) label = s_label[k];
          ++hits;
          if (overlap == ZH_OVERLAP_LAST) { done = true; break; }
          if (hits == 2) { label = ignore_value; done = true; break; }
        }
      }
    }
    if (__syncthreads_and(done)) break;                                        // also the barrier in front of the next pass's staging
  }
  if (inb) out[base + (long long)y * w + x] = (unsigned char)label;
}

extern "C" int zh_runs_label_maps(const int* run_end, const int* run_off, const int* status, int n_masks, long n_runs, const int* list_off,
                                  const int* list_mask, const unsigned char* list_label, int n_list, const int* hw, const long long* out_off,
                                  int B, int max_tiles, int overlap, int ignore_value, unsigned char* out, long out_bytes, hipStream_t stream) {
  ZH_CHECK_ARG(B >= 0 && B <= 65535, "zh_runs_label_maps: B = %d outside 0 .. 65535", B);
  ZH_CHECK_ARG(n_masks >= 0 && n_runs >= 0 && n_list >= 0 && out_bytes >= 0 && max_tiles >= 0, "zh_runs_label_maps: negative count");
  ZH_CHECK_ARG(overlap == ZH_OVERLAP_LAST || overlap == ZH_OVERLAP_IGNORE, "zh_runs_label_maps: overlap = %d is not ZH_OVERLAP_LAST / _IGNORE", overlap);
  ZH_CHECK_ARG(ignore_value >= 0 && ignore_value <= 255, "zh_runs_label_maps: ignore_value = %d is not a byte", ignore_value);
  if (B == 0 || max_tiles == 0) return ZH_OK;                                   // no image, or none with a pixel: nothing to launch
  ZH_CHECK_ARG(run_off && status && list_off && hw && out_off && out, "zh_runs_label_maps: null pointer");
  ZH_CHECK_ARG((n_runs == 0 || run_end) && (n_list == 0 || (list_mask && list_label)), "zh_runs_label_maps: null pointer");
  hipLaunchKernelGGL(runs_label_maps_kernel, dim3(max_tiles, B), dim3(LP_THREADS), 0, stream, run_end, run_off, status, n_masks, n_runs,
                     list_off, list_mask, list_label, n_list, hw, out_off, out_bytes, overlap, ignore_value, out);
  ZH_CHECK_LAUNCH("zh_runs_label_maps");
  return ZH_OK;
}
