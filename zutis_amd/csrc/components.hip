// Mask components on the device — the last four lines of bilateral_solver_output, utils/bilateral_solver.py:185-193: fill the holes of
// `soft > 0.5` (scipy.ndimage.binary_fill_holes), label its 4-connected components (ndimage.label), count every label, background
// included, and keep the label that is SECOND largest under the key (count, label); all ones when there is no object.  Integers only:
// every output is a pure function of the input (zutis_amd/components.py is the definition, scipy agrees with it outside count ties).
//
//   zh_second_largest_component   B images of one size, blockIdx.y = image, in ten launches whose geometry (B, H, W) alone decides;
//                                 nothing is read back, no workgroup waits on another: a phase boundary is a kernel boundary.
//
// One union-find forest per image over BOTH classes: par[p] <= p always, a union links the larger root under the smaller one with an
// atomic min, so a component's representative ends as its smallest linear index y * W + x — its first pixel in raster order, which is
// what scipy numbers components by — whatever order the unions arrive in.
//   1 tile      a ZH_CCL_TILE_H x ZH_CCL_TILE_W tile in LDS: classify (soft > threshold, NaN is background | binary != 0), join each pixel
//               with its left / upper neighbour of the same class (LDS atomics), flatten, store par (global index of the tile's
//               representative: the tile's raster order is monotonic in the image's) and the class byte; zero the border marks.
//   2 seams     one lane per pixel just right of / below a tile border: the same join across the border, in global memory.
//   3 flatten   par[p] = root(p); a background pixel on the image's border marks its root as open.
//   4 holes     a background pixel whose root is not open is a hole (class 2): joined with its four neighbours, all of them filled
//               foreground (a background neighbour is in the same hole), so the holes fuse the foreground components around them.
//   5 flags     par[p] = root(p) again; flag the filled pixels that are their own root (= one per component) and sum the flags of each
//               1024-pixel block; zero the counts.
//   6 scan      one workgroup per image: exclusive scan of the block sums, nr_objects = the total.
//   7 ranks     per block an exclusive scan of its flags plus the block's offset: rank of each representative = its label - 1.
//   8 labels    label(p) = rank(par[p]) + 1 or 0; counts[label] += 1, equal labels merged inside the wave (ballot) and then inside the
//               workgroup (a 16-slot LDS table) before the global atomic: a blob sends one add per 1024 pixels, not one per pixel.
//   9 select    one workgroup per image: top two of (count << 32 | label) over labels 0 .. nr, the second is kept.
//  10 mask      mask(p) = label(p) == chosen (or 1 in the fallback).
// Every index is formed from coordinates inside the image or is an entry of par (all H * W of which launch 1 writes, each <= its own
// index); every loop is bounded by a count the entry fixes, the finds by par[x] < x for every x that is no root.
#include "common.h"

#define CCL_TILE (ZH_CCL_TILE_H * ZH_CCL_TILE_W)
#define CCL_TILE_THREADS 256
#define CCL_BLOCK 1024          // pixels (= threads) of one scan block
#define CCL_SLOTS 16            // (label, count) pairs a workgroup merges in LDS before it adds to global memory
#define CCL_MERGE_ROUNDS 8      // distinct labels of one wave merged by ballot; the lanes left after that add their own 1

#define CCL_WG __HIP_MEMORY_SCOPE_WORKGROUP
#define CCL_AGENT __HIP_MEMORY_SCOPE_AGENT

template <int SCOPE>
__device__ __forceinline__ int ccl_find(int* par, int i) {
  for (;;) {                                                   // par[x] < x for every x that is no root: at most i steps
    const int p = __hip_atomic_load(&par[i], __ATOMIC_RELAXED, SCOPE);
    if (p == i) return i;
    i = p;
  }
}

// Join the components of a and b.  The larger root is linked under the smaller; when it stopped being a root in the meantime (another
// lane linked it first: the min went to whichever is smaller) the walk goes on from where it pointed.  Lock-free: a lane repeats only
// after another lane's min has lowered an entry, and entries only ever go down.
template <int SCOPE>
__device__ __forceinline__ void ccl_union(int* par, int a, int b) {
  for (;;) {
    a = ccl_find<SCOPE>(par, a);
    b = ccl_find<SCOPE>(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(&par[a], b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) return;
    a = old;
  }
}

struct CclWs { int* par; int* aux; int* cnt; int* bsum; unsigned char* cls; };

static inline size_t ccl_align(size_t n) { return (n + 255) & ~(size_t)255; }
__host__ __device__ static inline int ccl_blocks(long n) { return (int)((n + CCL_BLOCK - 1) / CCL_BLOCK); }
__host__ __device__ static inline long ccl_labels(long n) { return (n + 1) / 2 + 1; }        // labels 0 .. nr, nr <= ceil(n / 2) (a checkerboard)

// the slices of one image's workspace: par, aux int32 [N]; counts int32 [(N + 1) / 2 + 1]; block sums int32; class bytes [N]
struct CclLayout { size_t par, aux, cnt, bsum, cls, total; };
static inline CclLayout ccl_layout(long n) {
  CclLayout l;
  l.par = 0;
  l.aux = l.par + ccl_align((size_t)n * 4);
  l.cnt = l.aux + ccl_align((size_t)n * 4);
  l.bsum = l.cnt + ccl_align((size_t)ccl_labels(n) * 4);
  l.cls = l.bsum + ccl_align((size_t)ccl_blocks(n) * 4);
  l.total = l.cls + ccl_align((size_t)n);
  return l;
}
__device__ __forceinline__ CclWs ccl_ws(unsigned char* ws, size_t per_image, CclLayout l) {
  unsigned char* base = ws + (size_t)blockIdx.y * per_image;
  CclWs w = {(int*)(base + l.par), (int*)(base + l.aux), (int*)(base + l.cnt), (int*)(base + l.bsum), base + l.cls};
  return w;
}

// exclusive scan of one int per thread over a CCL_BLOCK-thread workgroup; total = the workgroup's sum.  s_w: 16 ints of LDS.
__device__ __forceinline__ int ccl_block_scan(int v, int* s_w, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();                                             // s_w may still be read from a previous call
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
  for (int k = 0; k < waves; ++k) {
    const int t = s_w[k];
    if (k < wave) before += t;
    all += t;
  }
  *total = all;
  return before + inc - v;
}

// 1: a tile in LDS
__global__ __launch_bounds__(CCL_TILE_THREADS) void ccl_tile_kernel(const double* soft, const unsigned char* binary, double threshold, int H,
                                                                     int W, int tiles_x, unsigned char* ws, size_t per_image, CclLayout lay) {
  __shared__ int s_par[CCL_TILE];
  __shared__ unsigned char s_cls[CCL_TILE];
  const CclWs w = ccl_ws(ws, per_image, lay);
  const long N = (long)H * W, img = (long)blockIdx.y * N;
  const int x0 = ((int)blockIdx.x % tiles_x) * ZH_CCL_TILE_W, y0 = ((int)blockIdx.x / tiles_x) * ZH_CCL_TILE_H;
  for (int i = threadIdx.x; i < CCL_TILE; i += CCL_TILE_THREADS) {
    const int x = x0 + i % ZH_CCL_TILE_W, y = y0 + i / ZH_CCL_TILE_W;
    unsigned char c = 0;
    if (x < W && y < H) {
      const long p = (long)y * W + x;
      c = soft ? (soft[img + p] > threshold ? 1 : 0) : (binary[img + p] != 0 ? 1 : 0);      // a NaN compares false: background
    }
    s_cls[i] = c;
    s_par[i] = i;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CCL_TILE; i += CCL_TILE_THREADS) {
    const int lx = i % ZH_CCL_TILE_W, ly = i / ZH_CCL_TILE_W;
    if (x0 + lx >= W || y0 + ly >= H) continue;
    const unsigned char c = s_cls[i];
    if (lx > 0 && s_cls[i - 1] == c) ccl_union<CCL_WG>(s_par, i, i - 1);
    if (ly > 0 && s_cls[i - ZH_CCL_TILE_W] == c) ccl_union<CCL_WG>(s_par, i, i - ZH_CCL_TILE_W);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CCL_TILE; i += CCL_TILE_THREADS) {
    const int x = x0 + i % ZH_CCL_TILE_W, y = y0 + i / ZH_CCL_TILE_W;
    if (x >= W || y >= H) continue;
    const int r = ccl_find<CCL_WG>(s_par, i);                  // r <= i, inside the image as i is
    const int p = y * W + x;
    w.par[p] = (y0 + r / ZH_CCL_TILE_W) * W + x0 + r % ZH_CCL_TILE_W;
    w.aux[p] = 0;
    w.cls[p] = s_cls[i];
  }
}

// 2: the tile borders.  Lane t < n_v: the pixel right of a vertical border; the others: the pixel below a horizontal one.
__global__ __launch_bounds__(256) void ccl_seam_kernel(int H, int W, int tiles_x, int tiles_y, unsigned char* ws, size_t per_image, CclLayout lay) {
  const CclWs w = ccl_ws(ws, per_image, lay);
  const long n_v = (long)(tiles_x - 1) * H, n_h = (long)(tiles_y - 1) * W;
  long t = (long)blockIdx.x * 256 + threadIdx.x;
  int p, q;
  if (t < n_v) {
    const int x = ((int)(t / H) + 1) * ZH_CCL_TILE_W, y = (int)(t % H);
    p = y * W + x;
    q = p - 1;
  } else {
    t -= n_v;
    if (t >= n_h) return;
    const int y = ((int)(t / W) + 1) * ZH_CCL_TILE_H, x = (int)(t % W);
    p = y * W + x;
    q = p - W;
  }
  if (w.cls[p] == w.cls[q]) ccl_union<CCL_AGENT>(w.par, p, q);
}

// 3: flatten; open background
__global__ __launch_bounds__(256) void ccl_open_kernel(int H, int W, unsigned char* ws, size_t per_image, CclLayout lay) {
  const CclWs w = ccl_ws(ws, per_image, lay);
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)H * W) return;
  const int p = (int)t, x = p % W, y = p / W;
  const int r = ccl_find<CCL_AGENT>(w.par, p);
  if (r != p) __hip_atomic_store(&w.par[p], r, __ATOMIC_RELAXED, CCL_AGENT);    // a shortcut to an ancestor: finds through p stay right
  if (w.cls[p] == 0 && (x == 0 || y == 0 || x == W - 1 || y == H - 1)) w.aux[r] = 1;
}

// 4: holes.  par[p] of a background pixel is still the root launch 3 left — or, for a hole's own root that a neighbour has already
// linked on, a former root of the filled foreground (only those are ever joined here), whose mark is 0 like the hole's: either way the
// mark read is the component's.  Open background is never touched.
__global__ __launch_bounds__(256) void ccl_hole_kernel(int H, int W, unsigned char* ws, size_t per_image, CclLayout lay) {
  const CclWs w = ccl_ws(ws, per_image, lay);
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)H * W) return;
  const int p = (int)t, x = p % W, y = p / W;
  if (w.cls[p] != 0) return;
  const int r = __hip_atomic_load(&w.par[p], __ATOMIC_RELAXED, CCL_AGENT);
  // aux is 0 for every pixel after launch 1 and launch 3 sets it at roots of background that has a border pixel only: a foreground
  // root's mark and a hole root's mark are both 0, an open root's is 1
  if (w.aux[r]) return;
  w.cls[p] = 2;                                                // read by no other lane of this launch
  if (x > 0) ccl_union<CCL_AGENT>(w.par, p, p - 1);             // a hole has no pixel on the border: the guards never fail
  if (x < W - 1) ccl_union<CCL_AGENT>(w.par, p, p + 1);
  if (y > 0) ccl_union<CCL_AGENT>(w.par, p, p - W);
  if (y < H - 1) ccl_union<CCL_AGENT>(w.par, p, p + W);
}

// 5: flatten; representative flags and their block sums; zero the counts
__global__ __launch_bounds__(CCL_BLOCK) void ccl_flag_kernel(int H, int W, unsigned char* ws, size_t per_image, CclLayout lay) {
  __shared__ int s_w[16];
  const CclWs w = ccl_ws(ws, per_image, lay);
  const long N = (long)H * W, t = (long)blockIdx.x * CCL_BLOCK + threadIdx.x, n_cnt = ccl_labels(N);
  int flag = 0;
  if (t < N) {
    const int p = (int)t;
    const int r = ccl_find<CCL_AGENT>(w.par, p);
    if (r != p) __hip_atomic_store(&w.par[p], r, __ATOMIC_RELAXED, CCL_AGENT);
    flag = (w.cls[p] != 0 && r == p) ? 1 : 0;
    w.aux[p] = flag;
    if (t < n_cnt) w.cnt[t] = 0;
    if (t + N < n_cnt) w.cnt[t + N] = 0;                         // n_cnt <= N + 1
  }
  int total;
  ccl_block_scan(flag, s_w, &total);
  if (threadIdx.x == 0) w.bsum[blockIdx.x] = total;
}

// 6: exclusive scan of the block sums, one workgroup per image
__global__ __launch_bounds__(CCL_BLOCK) void ccl_scan_kernel(int n_blocks, int* stats, unsigned char* ws, size_t per_image, CclLayout lay) {
  __shared__ int s_w[16];
  const CclWs w = ccl_ws(ws, per_image, lay);
  int carry = 0;
  for (int base = 0; base < n_blocks; base += CCL_BLOCK) {
    const int i = base + (int)threadIdx.x;
    const int v = i < n_blocks ? w.bsum[i] : 0;
    int total;
    const int ex = ccl_block_scan(v, s_w, &total);
    if (i < n_blocks) w.bsum[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) stats[4 * blockIdx.y] = carry;
}

// 7: rank of every representative
__global__ __launch_bounds__(CCL_BLOCK) void ccl_rank_kernel(int H, int W, unsigned char* ws, size_t per_image, CclLayout lay) {
  __shared__ int s_w[16];
  const CclWs w = ccl_ws(ws, per_image, lay);
  const long N = (long)H * W, t = (long)blockIdx.x * CCL_BLOCK + threadIdx.x;
  const int flag = t < N ? w.aux[t] : 0;
  int total;
  const int ex = ccl_block_scan(flag, s_w, &total);
  if (t < N) w.aux[t] = w.bsum[blockIdx.x] + ex;
}

__device__ __forceinline__ int ccl_label(const CclWs& w, int p) { return w.cls[p] != 0 ? w.aux[w.par[p]] + 1 : 0; }

// 8: labels, filled mask, counts
__global__ __launch_bounds__(CCL_BLOCK) void ccl_label_kernel(int H, int W, unsigned char* filled_out, int* labels_out, unsigned char* ws,
                                                               size_t per_image, CclLayout lay) {
  __shared__ int s_lab[CCL_SLOTS];
  __shared__ int s_cnt[CCL_SLOTS];
  const CclWs w = ccl_ws(ws, per_image, lay);
  const long N = (long)H * W, t = (long)blockIdx.x * CCL_BLOCK + threadIdx.x, img = (long)blockIdx.y * N;
  if (threadIdx.x < CCL_SLOTS) { s_lab[threadIdx.x] = -1; s_cnt[threadIdx.x] = 0; }
  __syncthreads();
  int key = -1;
  if (t < N) {
    key = ccl_label(w, (int)t);
    if (labels_out) labels_out[img + t] = key;
    if (filled_out) filled_out[img + t] = w.cls[t] != 0 ? 1 : 0;
  }
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(key >= 0);
  for (int round = 0; todo; ++round) {
    int k = key, n = 1;
    bool add = false;
    if (round == CCL_MERGE_ROUNDS) {                           // many labels in this wave (noise): the lanes left add their own 1
      add = (todo >> lane) & 1;
      todo = 0;
    } else {
      const int leader = __ffsll((long long)todo) - 1;
      k = __shfl(key, leader);
      const unsigned long long same = __ballot(key == k);
      n = __popcll(same);
      add = lane == leader;
      todo &= ~same;
    }
    if (add) {
      bool placed = false;
      for (int probe = 0; probe < CCL_SLOTS && !placed; ++probe) {
        const int slot = (k + probe) & (CCL_SLOTS - 1);
        const int old = atomicCAS(&s_lab[slot], -1, k);
        if (old == -1 || old == k) {
          atomicAdd(&s_cnt[slot], n);
          placed = true;
        }
      }
      if (!placed) atomicAdd(&w.cnt[k], n);                     // k <= nr < ccl_labels(N)
    }
  }
  __syncthreads();
  if (threadIdx.x < CCL_SLOTS && s_lab[threadIdx.x] >= 0) atomicAdd(&w.cnt[s_lab[threadIdx.x]], s_cnt[threadIdx.x]);
}

// 9: the second largest of (count, label) over labels 0 .. nr; stats = {nr, label, count, fallback}
__global__ __launch_bounds__(256) void ccl_select_kernel(int H, int W, int* stats, unsigned char* ws, size_t per_image, CclLayout lay) {
  __shared__ long long s_1[256];
  __shared__ long long s_2[256];
  const CclWs w = ccl_ws(ws, per_image, lay);
  int* st = stats + 4 * blockIdx.y;
  const long N = (long)H * W;
  long nr = st[0];
  if (nr < 0 || nr >= ccl_labels(N)) nr = ccl_labels(N) - 1;    // cannot happen: the counts are not read past their end all the same
  long long a1 = -1, a2 = -1;                                   // -1: none (every key is >= 0)
  for (long i = threadIdx.x; i <= nr; i += 256) {
    const long long k = ((long long)w.cnt[i] << 32) | i;
    if (k > a1) { a2 = a1; a1 = k; } else if (k > a2) a2 = k;
  }
  s_1[threadIdx.x] = a1;
  s_2[threadIdx.x] = a2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const long long b1 = s_1[threadIdx.x + o], b2 = s_2[threadIdx.x + o];
      a1 = s_1[threadIdx.x];
      a2 = s_2[threadIdx.x];
      const long long lo = a1 < b1 ? a1 : b1, hi2 = a2 > b2 ? a2 : b2;
      s_1[threadIdx.x] = a1 > b1 ? a1 : b1;
      s_2[threadIdx.x] = lo > hi2 ? lo : hi2;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const long long second = s_2[0];
    if (nr == 0 || second < 0) {                                // no object: all ones (bilateral_solver.py:192-193)
      st[1] = -1;
      st[2] = (int)N;
      st[3] = 1;
    } else {
      st[1] = (int)(second & 0x7fffffff);
      st[2] = (int)(second >> 32);
      st[3] = 0;
    }
  }
}

// 10: the mask
__global__ __launch_bounds__(256) void ccl_mask_kernel(int H, int W, const int* stats, unsigned char* mask_out, unsigned char* ws, size_t per_image,
                                                        CclLayout lay) {
  const CclWs w = ccl_ws(ws, per_image, lay);
  const long N = (long)H * W, t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= N) return;
  const int chosen = stats[4 * blockIdx.y + 1], fallback = stats[4 * blockIdx.y + 3];
  mask_out[(long)blockIdx.y * N + t] = (fallback || ccl_label(w, (int)t) == chosen) ? 1 : 0;
}

extern "C" size_t zh_components_workspace_size(int H, int W) {
  if (H < 1 || W < 1 || (long)H * W > 0x7fffffffL) return 0;
  return ccl_layout((long)H * W).total;
}

extern "C" int zh_second_largest_component(const double* soft, const unsigned char* binary, double threshold, int B, int H, int W,
                                           unsigned char* mask_out, unsigned char* filled_out, int* labels_out, int* stats, void* workspace,
                                           size_t workspace_bytes, hipStream_t stream) {
  ZH_CHECK_ARG((soft != nullptr) != (binary != nullptr), "zh_second_largest_component: exactly one of soft and binary is given");
  ZH_CHECK_ARG(B >= 0 && B <= 65535, "zh_second_largest_component: B = %d outside 0 .. 65535", B);
  ZH_CHECK_ARG(H >= 1 && W >= 1 && (long)H * W <= 0x7fffffffL, "zh_second_largest_component: H x W = %d x %d is not 1 .. 2^31 - 1 pixels", H, W);
  ZH_CHECK_ARG(threshold == threshold, "zh_second_largest_component: threshold is NaN");
  if (B == 0) return ZH_OK;
  ZH_CHECK_ARG(mask_out && stats && workspace, "zh_second_largest_component: null pointer");
  ZH_CHECK_ARG(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)stats & 3) == 0, "zh_second_largest_component: workspace / stats not 4-byte aligned");
  const long N = (long)H * W;
  const CclLayout lay = ccl_layout(N);
  if (workspace_bytes < (size_t)B * lay.total) {
    zh_set_error("zh_second_largest_component: workspace holds %zu bytes, %zu needed", workspace_bytes, (size_t)B * lay.total);
    return ZH_ERR_WORKSPACE;
  }
  const int tiles_x = zh_cdiv(W, ZH_CCL_TILE_W), tiles_y = zh_cdiv(H, ZH_CCL_TILE_H);
  const long n_tiles = (long)tiles_x * tiles_y, n_seam = (long)(tiles_x - 1) * H + (long)(tiles_y - 1) * W;
  const int n_blocks = ccl_blocks(N), n_256 = zh_cdiv(N, 256);
  ZH_CHECK_ARG(n_tiles <= 0x7fffffffL, "zh_second_largest_component: %ld tiles", n_tiles);
  unsigned char* ws = (unsigned char*)workspace;
  const size_t per = lay.total;
  hipLaunchKernelGGL(ccl_tile_kernel, dim3((unsigned)n_tiles, B), dim3(CCL_TILE_THREADS), 0, stream, soft, binary, threshold, H, W, tiles_x, ws, per, lay);
  if (n_seam > 0)
    hipLaunchKernelGGL(ccl_seam_kernel, dim3(zh_cdiv(n_seam, 256), B), dim3(256), 0, stream, H, W, tiles_x, tiles_y, ws, per, lay);
  hipLaunchKernelGGL(ccl_open_kernel, dim3(n_256, B), dim3(256), 0, stream, H, W, ws, per, lay);
  hipLaunchKernelGGL(ccl_hole_kernel, dim3(n_256, B), dim3(256), 0, stream, H, W, ws, per, lay);
  hipLaunchKernelGGL(ccl_flag_kernel, dim3(n_blocks, B), dim3(CCL_BLOCK), 0, stream, H, W, ws, per, lay);
  hipLaunchKernelGGL(ccl_scan_kernel, dim3(1, B), dim3(CCL_BLOCK), 0, stream, n_blocks, stats, ws, per, lay);
  hipLaunchKernelGGL(ccl_rank_kernel, dim3(n_blocks, B), dim3(CCL_BLOCK), 0, stream, H, W, ws, per, lay);
  hipLaunchKernelGGL(ccl_label_kernel, dim3(n_blocks, B), dim3(CCL_BLOCK), 0, stream, H, W, filled_out, labels_out, ws, per, lay);
  hipLaunchKernelGGL(ccl_select_kernel, dim3(1, B), dim3(256), 0, stream, H, W, stats, ws, per, lay);
  hipLaunchKernelGGL(ccl_mask_kernel, dim3(n_256, B), dim3(256), 0, stream, H, W, stats, mask_out, ws, per, lay);
  ZH_CHECK_LAUNCH("zh_second_largest_component");
  return ZH_OK;
}
