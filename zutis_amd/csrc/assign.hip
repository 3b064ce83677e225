// The two host trips of the training criterion, on the device (zutis_amd/criterion.py, assignment="device"):
//   * zh_linear_assignment: scipy.optimize.linear_sum_assignment (criterion.py:133) for every (image, layer) of one criterion call in
//     one launch, on the costs buffer exactly as zh_mask_match_cost lays it out; a second, single-workgroup launch compacts the matches
//     to the (b, l, q, i) pairs zh_mask_match_grad reads and forms the mask loss (criterion.py:145,150).
//   * zh_pack_masks_u8: the ragged list of ground-truth instance masks -> gt_u8 [n_tot, H, W] and inst_off, in one launch.
//
// The solver is scipy's: the rectangular shortest-augmenting-path method (Crouse's form of Jonker-Volgenant) in float64 on the float32
// costs, every sum in scipy's operand order (there is no product, so nothing contracts to an FMA), and scipy's tie rule.  That rule is
// what makes the result scipy's when cost rows are bit-identical (random_duplicate produces identical GT masks): a search step scans
// the not-yet-scanned columns in the order of `remaining` (initially nc-1 .. 0; the chosen slot is overwritten with the last live
// entry) and among the columns of minimal reduced path cost takes the LAST UNASSIGNED one in scan order, or, when none is unassigned,
// the FIRST one.  The wave's arg-min therefore orders candidates by (value, unassigned, scan position): a total order with one
// winner, so lanes may own scan positions in any pattern.
//
// One wavefront per problem (workgroup = 64 threads): lanes own scan positions lane, lane + 64, ...; the duals, shortest, path,
// row4col, col4row, the scanned flags and `remaining` live in LDS; costs are read from global memory (a 10 x 100 problem is 4 KB and
// stays in cache).  __syncthreads() of a one-wave workgroup is no s_barrier, only the LDS ordering the compiler must keep.
#include "common.h"

// ZH_ASSIGN_MAX_DIM caps max(n_b, Q): 32 bytes per column + 16 per row of LDS state = 48 KB at the cap (64 KB per workgroup)
#define AS_COL_BYTES 32   // v f64, shortest f64, path i32, row4col i32, remaining i32, SC i32
#define AS_ROW_BYTES 16   // u f64, col4row i32, SR i32

// (value, score): smaller value wins; on equal values the higher score — unassigned columns score above every assigned one and
// later scan positions above earlier ones, assigned columns score earlier positions higher
__device__ __forceinline__ bool as_better(double va, int sa, double vb, int sb) { return va < vb || (va == vb && sa > sb); }

__global__ __launch_bounds__(64) void linear_assignment_kernel(const float* costs, const int* inst_off, const int* skip, int L, int Q,
                                                               int lds_bytes, int* match, double* psum, int* status) {
  extern __shared__ double as_lds[];
  const int lane = threadIdx.x;
  const int p = blockIdx.x, b = p / L, l = p - b * L;
  const int n_b = inst_off[b + 1] - inst_off[b];
  const long row0 = (long)L * inst_off[b] + (long)l * n_b;        // first row of this problem in costs [.., Q] / match
  if (lane == 0) psum[p] = 0.0;
  if (n_b <= 0) return;
  if (skip[b] != 0) {
    for (int i = lane; i < n_b; i += 64) match[row0 + i] = -1;
    return;
  }
  const float* c = costs + row0 * Q;
  // scipy's validity test, stricter: NaN and -inf as scipy, +inf as well (it would need scipy's infeasibility exit)
  int bad = 0;
  for (int k = lane; k < n_b * Q; k += 64) bad |= !(fabsf(c[k]) <= 3.402823466e38f);
  // (a problem larger than the n_max the launch sized its LDS for is refused the same way: no pairs, the status bit)
  if ((n_b > Q ? n_b : Q) * AS_COL_BYTES + (n_b > Q ? Q : n_b) * AS_ROW_BYTES > lds_bytes) bad = 1;
  if (__ballot(bad) != 0ull) {
    if (lane == 0) atomicOr(status, ZH_STATUS_NONFINITE);
    for (int i = lane; i < n_b; i += 64) match[row0 + i] = -1;
    return;
  }
  // rows of the solve = the shorter side: a tall problem is solved transposed, as scipy does
  const bool tr = Q < n_b;
  const int nr = tr ? Q : n_b, nc = tr ? n_b : Q;
  const long rs = tr ? 1 : Q, cs = tr ? Q : 1;                     // cost(i, j) = c[i * rs + j * cs]
  double* v = as_lds;                    // [nc]
  double* shortest = v + nc;             // [nc]
  double* u = shortest + nc;             // [nr]
  int* path = (int*)(u + nr);            // [nc]
  int* row4col = path + nc;              // [nc]
  int* remaining = row4col + nc;         // [nc]
  int* SC = remaining + nc;              // [nc]
  int* col4row = SC + nc;                // [nr]
  int* SR = col4row + nr;                // [nr]
  for (int j = lane; j < nc; j += 64) { v[j] = 0.0; path[j] = -1; row4col[j] = -1; }
  for (int i = lane; i < nr; i += 64) { u[i] = 0.0; col4row[i] = -1; }
  __syncthreads();

  for (int cur = 0; cur < nr; ++cur) {
    // ---- shortest augmenting path from row `cur`
    for (int j = lane; j < nc; j += 64) { remaining[j] = nc - j - 1; SC[j] = 0; shortest[j] = INFINITY; }
    for (int i = lane; i < nr; i += 64) SR[i] = 0;
    __syncthreads();
    double min_val = 0.0;
    int i = cur, sink = -1, num_remaining = nc;
    while (sink < 0 && num_remaining > 0) {
      if (lane == 0) SR[i] = 1;
      const double ui = u[i];
      double bv = INFINITY;
      int bs = -0x7fffffff, bpos = -1;
      for (int it = lane; it < num_remaining; it += 64) {
        const int j = remaining[it];
        const double r = min_val + (double)c[i * rs + j * cs] - ui - v[j];
        double s = shortest[j];
        if (r < s) { path[j] = i; shortest[j] = r; s = r; }
        const int score = row4col[j] < 0 ? ZH_ASSIGN_MAX_DIM + it : -it;
        if (as_better(s, score, bv, bs)) { bv = s; bs = score; bpos = it; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const int os = __shfl_xor(bs, o, 64), op = __shfl_xor(bpos, o, 64);
        if (as_better(ov, os, bv, bs)) { bv = ov; bs = os; bpos = op; }
      }
      min_val = bv;
      const int j = remaining[bpos];
      const int rj = row4col[j];
      const int last = remaining[num_remaining - 1];
      if (rj < 0) sink = j; else i = rj;
      __syncthreads();
      if (lane == 0) { SC[j] = 1; remaining[bpos] = last; }
      --num_remaining;
      __syncthreads();
    }
    // ---- dual updates (scipy's operand order)
    if (lane == 0) u[cur] += min_val;
    for (int k = lane; k < nr; k += 64)
      if (SR[k] && k != cur) u[k] += min_val - shortest[col4row[k]];
    for (int j = lane; j < nc; j += 64)
      if (SC[j]) v[j] -= min_val - shortest[j];
    __syncthreads();
    // ---- augment along the path
    if (lane == 0) {
      int j = sink;
      for (int guard = 0; guard <= nr && j >= 0; ++guard) {
        const int k = path[j];
        row4col[j] = k;
        const int t = col4row[k];
        col4row[k] = j;
        j = t;
        if (k == cur) break;
      }
    }
    __syncthreads();
  }
  // ---- matched query per instance (-1: none, only in a tall problem), the matched costs summed in instance order in float64
  for (int i = lane; i < n_b; i += 64) match[row0 + i] = tr ? row4col[i] : col4row[i];
  __syncthreads();
  if (lane == 0) {
    double s = 0.0;
    for (int i = 0; i < n_b; ++i) {
      const int q = tr ? row4col[i] : col4row[i];
      if (q >= 0) s += (double)c[(long)i * Q + q];
    }
    psum[p] = s;
  }
}

// match [L * n_tot] (the row order of costs = (b, l, i) order) -> pairs int32 [n_pairs, 4] = (b, l, q, i) compacted in that order,
// n_pairs, mask_loss = f32(sum of the problems' float64 sums in (b, l) order / B).  One workgroup.
__global__ __launch_bounds__(256) void assignment_finish_kernel(const int* match, const double* psum, const int* inst_off, int B, int L,
                                                                int* pairs, int* n_pairs, float* mask_loss) {
  __shared__ int wave_cnt[4];
  __shared__ int base_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long R = (long)L * inst_off[B];
  if (threadIdx.x == 0) base_s = 0;
  __syncthreads();
  for (long r0 = 0; r0 < R; r0 += 256) {
    const long r = r0 + threadIdx.x;
    const int q = r < R ? match[r] : -1;
    const unsigned long long m = __ballot(q >= 0);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int rank = base_s + __popcll(m & ((1ull << lane) - 1ull));
    for (int k = 0; k < wave; ++k) rank += wave_cnt[k];
    if (q >= 0) {
      int b = 0;
      while ((long)L * inst_off[b + 1] <= r) ++b;
      const int n_b = inst_off[b + 1] - inst_off[b];
      const int rr = (int)(r - (long)L * inst_off[b]);
      const int l = rr / n_b;
      *(int4*)(pairs + 4 * (long)rank) = make_int4(b, l, q, rr - l * n_b);
    }
    __syncthreads();
    if (threadIdx.x == 0) base_s += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int p = 0; p < B * L; ++p) tot += psum[p];
    *n_pairs = base_s;
    *mask_loss = (float)(tot / (double)B);
  }
}

extern "C" int zh_linear_assignment_max_dim(void) { return ZH_ASSIGN_MAX_DIM; }

extern "C" size_t zh_linear_assignment_workspace_size(int B, int L, int n_tot) {
  return (size_t)B * L * sizeof(double) + (size_t)L * (n_tot > 0 ? n_tot : 0) * sizeof(int);
}

extern "C" int zh_linear_assignment(const float* costs, const int* inst_off, const int* skip, int B, int L, int Q, int n_max, int n_tot,
                                    int* pairs, int* n_pairs, float* mask_loss, int* status, void* workspace, size_t workspace_bytes,
                                    hipStream_t stream) {
  ZH_CHECK_ARG(inst_off && skip && n_pairs && mask_loss && status && workspace, "zh_linear_assignment: null pointer");
  ZH_CHECK_ARG(B > 0 && L > 0 && Q > 0 && n_max >= 0 && n_tot >= 0 && n_max <= n_tot, "zh_linear_assignment: bad shape");
  ZH_CHECK_ARG(n_tot == 0 || (costs && pairs), "zh_linear_assignment: null costs / pairs");
  ZH_CHECK_ARG(((uintptr_t)pairs & 15) == 0, "zh_linear_assignment: pairs must be 16-byte aligned");
  ZH_CHECK_ARG(Q <= ZH_ASSIGN_MAX_DIM && n_max <= ZH_ASSIGN_MAX_DIM, "zh_linear_assignment: max(n_max = %d, Q = %d) exceeds the cap of %d (LDS state)",
               n_max, Q, ZH_ASSIGN_MAX_DIM);
  ZH_CHECK_ARG(workspace_bytes >= zh_linear_assignment_workspace_size(B, L, n_tot), "zh_linear_assignment: workspace too small");
  double* psum = (double*)workspace;
  int* match = (int*)(psum + (long)B * L);
  const int nc = n_max > Q ? n_max : Q, nr = n_max > Q ? Q : n_max;
  const size_t lds = (size_t)nc * AS_COL_BYTES + (size_t)nr * AS_ROW_BYTES;
  hipLaunchKernelGGL(linear_assignment_kernel, dim3(B * L), dim3(64), lds, stream, costs, inst_off, skip, L, Q, (int)lds,
                     match, psum, status);
  ZH_CHECK_LAUNCH("zh_linear_assignment");
  hipLaunchKernelGGL(assignment_finish_kernel, dim3(1), dim3(256), 0, stream, match, psum, inst_off, B, L, pairs, n_pairs, mask_loss);
  ZH_CHECK_LAUNCH("zh_linear_assignment");
  return ZH_OK;
}

// ================================================================================================================================
// Ground-truth packing
// ================================================================================================================================
#define PK_IMAGES 32      // images per launch: their source pointers and offsets travel as kernel arguments (no table copy)
#define PK_CHUNK 2048     // output bytes per workgroup step

struct PackArgs {
  const void* src[PK_IMAGES];
  int off[PK_IMAGES + 1];  // instance offsets of the launch's images, off[k + 1] - off[k] = count
  int b0;
};

// blockIdx.y = image of the launch, blockIdx.x walks its count * HW elements; 8 outputs per thread as one 8-byte store when the
// image's source and destination are 8-byte aligned, bytes otherwise.  An image whose source IS its destination is left alone.
template <int ES>
__global__ __launch_bounds__(256) void pack_masks_kernel(PackArgs a, long HW, unsigned char* gt, int* inst_off) {
  const int k = blockIdx.y;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    inst_off[a.b0 + k + 1] = a.off[k + 1];
    if (a.b0 + k == 0) inst_off[0] = a.off[0];
  }
  const long n = (long)(a.off[k + 1] - a.off[k]) * HW;
  unsigned char* dst = gt + (long)a.off[k] * HW;
  const unsigned char* src = (const unsigned char*)a.src[k];
  if (n <= 0 || (const void*)src == (const void*)dst) return;
  const bool vec = (((uintptr_t)src | (uintptr_t)dst) & 7) == 0;
  const long n8 = vec ? n / 8 : 0;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n8; e += (long)gridDim.x * 256) {
    unsigned long long o = 0;
    if (ES == 1) {
      const unsigned long long w = ((const unsigned long long*)src)[e];
#pragma unroll
      for (int t = 0; t < 8; ++t) o |= (unsigned long long)(((w >> (8 * t)) & 0xffull) != 0) << (8 * t);
    } else {
#pragma unroll
      for (int t = 0; t < 8; ++t) o |= (unsigned long long)(((const unsigned long long*)src)[8 * e + t] != 0) << (8 * t);
    }
    ((unsigned long long*)dst)[e] = o;
  }
  for (long e = n8 * 8 + (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256)
    dst[e] = ES == 1 ? (src[e] != 0) : (((const unsigned long long*)src)[e] != 0);
}

extern "C" int zh_pack_masks_u8(const void* const* src, const int* counts, int B, int elem_size, long HW, unsigned char* gt_u8,
                                int* inst_off, hipStream_t stream) {
  ZH_CHECK_ARG(src && counts && inst_off, "zh_pack_masks_u8: null pointer");
  ZH_CHECK_ARG(B > 0 && HW > 0, "zh_pack_masks_u8: bad shape");
  ZH_CHECK_ARG(elem_size == 1 || elem_size == 8, "zh_pack_masks_u8: element size %d (1 = bool / uint8, 8 = int64)", elem_size);
  long tot = 0;
  for (int b = 0; b < B; ++b) {
    ZH_CHECK_ARG(counts[b] >= 0, "zh_pack_masks_u8: negative count");
    ZH_CHECK_ARG(counts[b] == 0 || (src[b] && gt_u8), "zh_pack_masks_u8: null source / gt_u8");
    ZH_CHECK_ARG(elem_size == 1 || ((uintptr_t)src[b] & 7) == 0, "zh_pack_masks_u8: misaligned int64 source");
    tot += counts[b];
    ZH_CHECK_ARG(tot <= 0x7fffffffL, "zh_pack_masks_u8: too many instances");
  }
  int off = 0;
  for (int b0 = 0; b0 < B; b0 += PK_IMAGES) {
    PackArgs a;
    a.b0 = b0;
    const int nb = B - b0 < PK_IMAGES ? B - b0 : PK_IMAGES;
    a.off[0] = off;
    int cmax = 0;
    for (int k = 0; k < PK_IMAGES; ++k) {
      a.src[k] = k < nb ? src[b0 + k] : nullptr;
      const int cnt = k < nb ? counts[b0 + k] : 0;
      const bool in_place = cnt > 0 && a.src[k] == (const void*)(gt_u8 + (long)off * HW);     // nothing to copy: inst_off only
      cmax = (!in_place && cnt > cmax) ? cnt : cmax;
      off += cnt;
      a.off[k + 1] = off;
    }
    long gx = ((long)cmax * HW + PK_CHUNK - 1) / PK_CHUNK;
    gx = gx < 1 ? 1 : (gx > 4096 ? 4096 : gx);
    if (elem_size == 1)
      hipLaunchKernelGGL(pack_masks_kernel<1>, dim3((unsigned)gx, nb), dim3(256), 0, stream, a, HW, gt_u8, inst_off);
    else
      hipLaunchKernelGGL(pack_masks_kernel<8>, dim3((unsigned)gx, nb), dim3(256), 0, stream, a, HW, gt_u8, inst_off);
    ZH_CHECK_LAUNCH("zh_pack_masks_u8");
  }
  return ZH_OK;
}
