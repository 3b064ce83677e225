// Instance-prediction kernels (networks/zutis.py:374-420): per-query mask statistics, masked mean of the
// text-space patch tokens, and the per-query class / score.  The reference materialises
// patch_tokens[:,None] * binary_masks[...,None] = B x Q x hw x 512 fp32 (2.9 GB at B=8, zutis.py:404-406);
// here the masked mean is a streaming reduction that reads each image's tokens from L2.
#include "common.h"

// ---- per (image, query): size = #(p > thr), conf = sum(p * (p > thr)) / (size + 1e-7)   (zutis.py:390-397)
// range_flag (optional): bit 0 is set when any proposal lies outside [0, 1] (or is a NaN) — the reference's two asserts on the
// mask proposals (zutis.py:385-386), checked by the host at the predict's one synchronisation instead of with a reduction + copy of its own
// One workgroup per (image, query) row, 4 pixels per thread and pass (round 4: a wave per row walked its 4800 pixels in 75 dependent
// passes, 25 workgroups at batch 1: 26 us for 1.9 MB).  The sums are integers (counts) and a float sum whose order is fixed by the
// shape: per thread ascending pixels, then the fixed tree of block_sum4.
__device__ __forceinline__ float stats_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void instance_stats_kernel(const float* mp, long stride_b, float thr, long rows, int Q, int M,
                                                             float* sizes, float* conf, unsigned char* binary, int* range_flag) {
  __shared__ float red[4];
  const long r = blockIdx.x;                                      // r = b*Q + q
  const int b = (int)(r / Q), q = (int)(r % Q);
  const float* p = mp + (long)b * stride_b + (long)q * M;
  unsigned char* bo = binary + r * M;
  float cnt = 0.f, s = 0.f;
  bool bad = false;
  const bool vec = (M % 4 == 0) && ((((uintptr_t)p) & 15) == 0) && ((((uintptr_t)bo) & 3) == 0);
  if (vec) {
    for (int m = threadIdx.x * 4; m < M; m += 1024) {
      const f32x4 v = *(const f32x4*)(p + m);
      unsigned pk = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bad |= !(v[e] >= 0.f && v[e] <= 1.f);
        const bool on = v[e] > thr;
        cnt += on ? 1.f : 0.f;
        s += on ? v[e] : 0.f;
        pk |= (on ? 1u : 0u) << (8 * e);
      }
      *(unsigned*)(bo + m) = pk;
    }
  } else {
    for (int m = threadIdx.x; m < M; m += 256) {
      const float v = p[m];
      bad |= !(v >= 0.f && v <= 1.f);
      const bool on = v > thr;
      cnt += on ? 1.f : 0.f;
      s += on ? v : 0.f;
      bo[m] = on ? 1 : 0;
    }
  }
  cnt = stats_block_sum(cnt, red);
  s = stats_block_sum(s, red);
  if (threadIdx.x == 0) { sizes[r] = cnt; conf[r] = s / (cnt + 1e-7f); }
  if (range_flag && __ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(range_flag, ZH_STATUS_RANGE);
}

extern "C" int zh_instance_mask_stats(const float* mask_proposals, long stride_image, float threshold, int B, int Q, int M,
                                      float* sizes, float* confidence, unsigned char* binary, int* range_flag, hipStream_t stream) {
  ZH_CHECK_ARG(mask_proposals && sizes && confidence && binary && B > 0 && Q > 0 && M > 0, "zh_instance_mask_stats: bad arguments");
  const long rows = (long)B * Q;
  ZH_CHECK_ARG(rows < (1L << 31), "zh_instance_mask_stats: too many rows");
  hipLaunchKernelGGL(instance_stats_kernel, dim3((unsigned)rows), dim3(256), 0, stream, mask_proposals, stride_image, threshold, rows, Q, M,
                     sizes, confidence, binary, range_flag);
  ZH_CHECK_LAUNCH("zh_instance_mask_stats");
  return ZH_OK;
}

// ---- avg[b,q,:] = sum_m binary[b,q,m] * tokens[b,m,:] / (size[b,q] + 1e-7)   (zutis.py:404-406)
// block = (tile of QT queries, image, chunk of MCH pixels); thread owns CPT channels; the tile's mask bytes of the chunk are
// staged in LDS.  Per-chunk partial sums go to the workspace [chunks][B*Q][E] and masked_mean_reduce_kernel adds them in chunk
// order (deterministic, independent of the batch) and divides.  (Round 3: the first version walked ALL pixels in one block per
// (query tile, image) — 10 blocks at batch 1, the COCO-20K evaluation's regime, 4800 dependent iterations: 1.8 ms of the
// 3.5 ms instance predict.)
#define QT 10      // (round 4: 20 queries per block with 16 rows of loads in flight: 31 -> 60 us — 190 blocks, one round, each twice as long)
#define MCH 64     // pixels per block (round 4: 128 -> 64: twice the workgroups, half the dependent load rounds per workgroup)
template <int CPT>
__global__ __launch_bounds__(256) void masked_mean_kernel(const float* tokens, const unsigned char* binary, float* partial, int Q, int M, int E,
                                                          long rows) {
  __shared__ unsigned char sm[QT][MCH];
  const int b = blockIdx.y, q0 = blockIdx.x * QT, m0 = blockIdx.z * MCH;
  const int nq = min(QT, Q - q0), mc = min(MCH, M - m0);
  const float* tk = tokens + (long)b * M * E;
  float acc[QT][CPT];
#pragma unroll
  for (int q = 0; q < QT; ++q)
#pragma unroll
    for (int c = 0; c < CPT; ++c) acc[q][c] = 0.f;
  for (int i = threadIdx.x; i < QT * MCH; i += 256) {
    const int q = i / MCH, m = i - q * MCH;
    sm[q][m] = (q < nq && m < mc) ? binary[((long)b * Q + q0 + q) * M + m0 + m] : 0;
  }
  __syncthreads();
#pragma unroll 8                                         // eight rows of loads in flight (same summation order per accumulator; 16: 208 VGPRs)
  for (int m = 0; m < mc; ++m) {
    float v[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int ch = threadIdx.x + 256 * c;
      v[c] = ch < E ? tk[(long)(m0 + m) * E + ch] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      const float f = sm[q][m] ? 1.f : 0.f;
#pragma unroll
      for (int c = 0; c < CPT; ++c) acc[q][c] += f * v[c];
    }
  }
  float* po = partial + ((long)blockIdx.z * rows + (long)b * Q + q0) * E;
  for (int q = 0; q < nq; ++q)
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int ch = threadIdx.x + 256 * c;
      if (ch < E) po[(long)q * E + ch] = acc[q][c];
    }
}
__global__ __launch_bounds__(256) void masked_mean_reduce_kernel(const float* partial, const float* sizes, float* avg, long rows, int E, int chunks) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * E) return;
  float s = 0.f;
#pragma unroll 8
  for (int z = 0; z < chunks; ++z) s += partial[(long)z * rows * E + i];
  avg[i] = s * (1.0f / (sizes[i / E] + 1e-7f));
}

extern "C" size_t zh_masked_mean_workspace_size(int B, int Q, int M, int E) {
  return (size_t)zh_cdiv(M, MCH) * B * Q * E * sizeof(float);
}
extern "C" int zh_masked_mean_tokens(const float* tokens, const unsigned char* binary, const float* sizes, float* avg,
                                     int B, int Q, int M, int E, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  ZH_CHECK_ARG(tokens && binary && sizes && avg && B > 0 && Q > 0 && M > 0 && E > 0, "zh_masked_mean_tokens: bad arguments");
  ZH_CHECK_ARG(E <= 1024 && B < 65536, "zh_masked_mean_tokens: E=%d > 1024 unsupported", E);
  const int chunks = zh_cdiv(M, MCH);
  ZH_CHECK_ARG(chunks < 65536, "zh_masked_mean_tokens: M=%d too large", M);
  if (!workspace || workspace_bytes < zh_masked_mean_workspace_size(B, Q, M, E)) {
    zh_set_error("zh_masked_mean_tokens: workspace too small (%zu < %zu)", workspace_bytes, zh_masked_mean_workspace_size(B, Q, M, E));
    return ZH_ERR_WORKSPACE;
  }
  float* partial = (float*)workspace;
  const long rows = (long)B * Q;
  dim3 grid(zh_cdiv(Q, QT), B, chunks);
  if (E <= 256) hipLaunchKernelGGL(masked_mean_kernel<1>, grid, dim3(256), 0, stream, tokens, binary, partial, Q, M, E, rows);
  else if (E <= 512) hipLaunchKernelGGL(masked_mean_kernel<2>, grid, dim3(256), 0, stream, tokens, binary, partial, Q, M, E, rows);
  else hipLaunchKernelGGL(masked_mean_kernel<4>, grid, dim3(256), 0, stream, tokens, binary, partial, Q, M, E, rows);
  hipLaunchKernelGGL(masked_mean_reduce_kernel, dim3(zh_cdiv(rows * E, 256)), dim3(256), 0, stream, partial, sizes, avg, rows, E, chunks);
  ZH_CHECK_LAUNCH("zh_masked_mean_tokens");
  return ZH_OK;
}

// ---- per (image, query): v = avg / (||avg|| + 1e-7); prob_n = sigmoid(T * text_n . v);
//      category = argmax_n (first max), score = conf * max_n prob      (zutis.py:409-420)
__global__ __launch_bounds__(256) void instance_classify_kernel(const float* avg, const float* text, const float* conf, float temperature,
                                                                int n, int E, long long* category, float* score) {
  __shared__ float sv[1024];
  __shared__ float red[4];
  __shared__ int bestk[4];
  __shared__ int besti[4];
  const long r = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* a = avg + r * E;
  float q = 0.f;
  for (int c = threadIdx.x; c < E; c += 256) { const float v = a[c]; sv[c] = v; q += v * v; }
  q = wave_sum(q);
  if (lane == 0) red[wave] = q;
  __syncthreads();
  const float inv = 1.0f / (sqrtf((red[0] + red[1]) + (red[2] + red[3])) + 1e-7f);
  int bk = -1;                                            // key of the best class: the bits of its probability, sign cleared
  int bi = 0x7fffffff;
  // CPP classes per pass (cls, cls + 4, ...): their rows are loaded together — one class at a time was 21 dependent passes of
  // load -> reduce -> exp per wave, 48 us for 100 queries x 81 classes at batch 1.  Each class's dot product keeps its summation
  // order and the classes are compared in ascending order, as before: bit-identical categories and scores.
  constexpr int CPP = 6;                                  // classes per pass and wave (round 4: 3 -> 6, 81 classes in 4 passes instead of 7)
  for (int cls = wave; cls < n; cls += 4 * CPP) {
    const float* t[CPP];
    float d[CPP];
#pragma unroll
    for (int j = 0; j < CPP; ++j) { t[j] = text + (long)(cls + 4 * j < n ? cls + 4 * j : cls) * E; d[j] = 0.f; }
    for (int c = lane; c < E; c += 64) {                     // (unrolled by 8 — 48 loads in flight — this kernel ran 40 us instead of 22)
      const float x = sv[c] * inv;
#pragma unroll
      for (int j = 0; j < CPP; ++j) d[j] += t[j][c] * x;
    }
#pragma unroll
    for (int j = 0; j < CPP; ++j) {
      const float dj = wave_sum(d[j]);
      const float pr = 1.0f / (1.0f + expf(-temperature * dj));
      // classes ascend within a wave -> first max kept.  A probability is +0 .. 1 or NaN; as the integer bits with the sign cleared
      // it orders the same and every NaN ranks above 1: the first NaN is kept, as torch.argmax / max take a NaN as the maximum
      const int key = __float_as_int(pr) & 0x7fffffff;
      if (cls + 4 * j < n && key > bk) { bk = key; bi = cls + 4 * j; }
    }
  }
  if (lane == 0) { bestk[wave] = bk; besti[wave] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int k = bestk[0];
    int i = besti[0];
    for (int w = 1; w < 4; ++w)
      if (bestk[w] > k || (bestk[w] == k && besti[w] < i)) { k = bestk[w]; i = besti[w]; }
    category[r] = i;
    score[r] = conf[r] * __int_as_float(k);
  }
}

extern "C" int zh_instance_classify(const float* avg, const float* text, const float* confidence, float temperature,
                                    int rows, int n_classes, int E, long long* category, float* score, hipStream_t stream) {
  ZH_CHECK_ARG(avg && text && confidence && category && score && rows > 0 && n_classes > 0 && E > 0 && E <= 1024,
               "zh_instance_classify: bad arguments");
  hipLaunchKernelGGL(instance_classify_kernel, dim3(rows), dim3(256), 0, stream, avg, text, confidence, temperature, n_classes, E,
                     category, score);
  ZH_CHECK_LAUNCH("zh_instance_classify");
  return ZH_OK;
}

// ---- pairwise mask IoU on bit-packed masks: iou[i][j] = |a_i & a_j| / (|a_i | a_j| + 1e-7)  (utils/iou.py:6-37)
//      masks u8 {0,1} [n, P] -> inter/union counts int32 [n, n] (exact integers; the float divide happens on the host
//      in float64 exactly as numpy does).
__global__ __launch_bounds__(256) void mask_pack_kernel(const unsigned char* masks, unsigned long long* packed, long P, long W64, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;   // one thread per 64-bit word
  if (idx >= total) return;
  const long n = idx / W64, w = idx - n * W64;
  const unsigned char* m = masks + n * P + w * 64;
  unsigned long long bits = 0;
  const long lim = P - w * 64 < 64 ? P - w * 64 : 64;
  if (lim == 64 && (((uintptr_t)m) & 15) == 0) {
    // four 16-byte loads instead of 64 byte loads (66 us for 100 masks of 480 x 640 at batch 1): a word of four {0,1} bytes
    // b0..b3 times 0x01020408 has b0 | b1 << 1 | b2 << 2 | b3 << 3 in bits 24..27 (the other partial products land on
    // distinct lower bits: no carries)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint4 v = *(const uint4*)(m + q * 16);
      const unsigned w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned t = ((w4[k] & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w4[k];
        const unsigned nz = (t >> 7) & 0x01010101u;
        bits |= (unsigned long long)(((nz * 0x01020408u) >> 24) & 0xFu) << (q * 16 + k * 4);
      }
    }
  } else {
    for (long i = 0; i < lim; ++i) bits |= (unsigned long long)(m[i] != 0) << i;
  }
  packed[idx] = bits;
}

// A block = a 4 x 4 tile of mask pairs (i0 .. i0+3) x (j0 .. j0+3), tiles on or above the diagonal: a pass loads eight 64-bit words
// per thread for sixteen (intersection, union) popcounts (round 4: one block per pair loaded two words per popcount pair, 390 MB of L2
// reads for 100 masks of 480 x 640: 30 us).  Integer sums: any order gives the same counts.
#define IOU_T 4
__global__ __launch_bounds__(256) void mask_iou_counts_kernel(const unsigned long long* packed, int n, long W64, int* inter, int* uni) {
  const int ti = blockIdx.x, tj = blockIdx.y;
  if (tj < ti) return;
  const int i0 = ti * IOU_T, j0 = tj * IOU_T;
  int ci[IOU_T][IOU_T], cu[IOU_T][IOU_T];
#pragma unroll
  for (int a = 0; a < IOU_T; ++a)
#pragma unroll
    for (int b = 0; b < IOU_T; ++b) { ci[a][b] = 0; cu[a][b] = 0; }
#pragma unroll 4                                             // 32 loads in flight per thread (19 dependent rounds for 480 x 640 otherwise)
  for (long w = threadIdx.x; w < W64; w += 256) {
    unsigned long long x[IOU_T], y[IOU_T];
#pragma unroll
    for (int a = 0; a < IOU_T; ++a) {
      x[a] = packed[(long)min(i0 + a, n - 1) * W64 + w];
      y[a] = packed[(long)min(j0 + a, n - 1) * W64 + w];
    }
#pragma unroll
    for (int a = 0; a < IOU_T; ++a)
#pragma unroll
      for (int b = 0; b < IOU_T; ++b) { ci[a][b] += __popcll(x[a] & y[b]); cu[a][b] += __popcll(x[a] | y[b]); }
  }
  __shared__ int red[4][2 * IOU_T * IOU_T];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < IOU_T; ++a)
#pragma unroll
    for (int b = 0; b < IOU_T; ++b) {
      int v = ci[a][b], u = cu[a][b];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { v += __shfl_xor(v, o, 64); u += __shfl_xor(u, o, 64); }
      if (lane == 0) { red[wave][2 * (a * IOU_T + b)] = v; red[wave][2 * (a * IOU_T + b) + 1] = u; }
    }
  __syncthreads();
  if (threadIdx.x < IOU_T * IOU_T) {
    const int a = threadIdx.x / IOU_T, b = threadIdx.x % IOU_T;
    const int i = i0 + a, j = j0 + b;
    if (i < n && j < n) {
      const int k = 2 * (a * IOU_T + b);
      const int I = red[0][k] + red[1][k] + red[2][k] + red[3][k], U = red[0][k + 1] + red[1][k + 1] + red[2][k + 1] + red[3][k + 1];
      inter[(long)i * n + j] = I; inter[(long)j * n + i] = I;
      uni[(long)i * n + j] = U; uni[(long)j * n + i] = U;
    }
  }
}

extern "C" size_t zh_mask_iou_workspace_size(int n, long pixels) { return (size_t)n * ((pixels + 63) / 64) * 8; }

extern "C" int zh_mask_iou_counts(const unsigned char* masks, int n, long pixels, int* inter, int* uni,
                                  void* workspace, size_t workspace_bytes, hipStream_t stream) {
  ZH_CHECK_ARG(masks && inter && uni && n > 0 && pixels > 0 && n < 65536, "zh_mask_iou_counts: bad arguments");
  const long W64 = (pixels + 63) / 64;
  if (!workspace || workspace_bytes < zh_mask_iou_workspace_size(n, pixels)) {
    zh_set_error("zh_mask_iou_counts: workspace too small");
    return ZH_ERR_WORKSPACE;
  }
  hipLaunchKernelGGL(mask_pack_kernel, dim3(zh_cdiv((long)n * W64, 256)), dim3(256), 0, stream, masks, (unsigned long long*)workspace, pixels, W64, (long)n * W64);
  const int nt = zh_cdiv(n, IOU_T);
  hipLaunchKernelGGL(mask_iou_counts_kernel, dim3(nt, nt), dim3(256), 0, stream, (const unsigned long long*)workspace, n, W64, inter, uni);
  ZH_CHECK_LAUNCH("zh_mask_iou_counts");
  return ZH_OK;
}

// ---- greedy per-category mask NMS on the device (networks/zutis.py:211-299, copy at coco20k_eval.py:54-136).
// One workgroup per image; inputs are the exact integer intersection / union counts of zh_mask_iou_counts, so every IoU is
// inter / (union + 1e-7) in float64 exactly as utils/iou.py:30-32 computes it on boolean masks.  Control flow of the
// reference, restated over the Q x Q counts:
//   for every category present, ascending, skipping 0 (background):
//     active = queries of that category, s = their scores
//     while active: best = argmax s (the reference takes the LAST element of an ascending np.argsort; equal maxima: the
//                   largest query index here — numpy's choice among exact ties is unspecified); emit (best, s[best]);
//                   for the others: s *= w(IoU(m, best)), w = hard: 0 if IoU > thr else 1; linear: (1 - IoU) if IoU > thr
//                   else 1; gaussian: exp(-IoU^2 / sigma); drop those with s <= score_threshold
//     emitted entries whose mask is empty are skipped (zutis.py:281-282).
// Scores are carried in float64: the reference's float32 scores are promoted by the first float64 weight (linear / gaussian)
// and stay float32 under hard NMS, where the only products are x1 / x0 — both representations hold the same values, and every
// comparison agrees except one: a score equal to float32(score_threshold).  float32(0.001) is 0.0010000000475 as a double, so
// `s > score_thr` here, in float64, KEEPS such a candidate; the reference's float32 score against a Python float drops it under
// NumPy 2 promotion (both sides become float32(0.001)) and keeps it under NumPy 1 (value-based: compared in float64).
#define NMS_MAXQ 1024
__global__ __launch_bounds__(256) void mask_nms_kernel(const int* inter, const int* uni, const float* scores, const long long* cats,
                                                       int Q, int nms_type, double thr, double sigma, double score_thr,
                                                       int* out_idx, double* out_score, long long* out_cat, int* out_count,
                                                       double* packed, const int* range_flag, int* zero_word) {
  __shared__ double s_sc[NMS_MAXQ];
  __shared__ long long s_cat[NMS_MAXQ];
  __shared__ unsigned char s_act[NMS_MAXQ];
  __shared__ double r_val[256];
  __shared__ long long r_key[256];
  __shared__ int s_best, s_n;
  __shared__ long long s_cur;
  const int img = blockIdx.x, tid = threadIdx.x;
  if (zero_word && img == 0 && tid == 0) *zero_word = 0;     // (the cursor of the run / string kernel launched behind this one)
  inter += (long)img * Q * Q; uni += (long)img * Q * Q;
  scores += (long)img * Q; cats += (long)img * Q;
  out_idx += (long)img * Q; out_score += (long)img * Q; out_cat += (long)img * Q;
  for (int q = tid; q < Q; q += 256) { s_cat[q] = cats[q]; s_act[q] = 0; }
  if (tid == 0) { s_n = 0; s_cur = 0; }        // categories <= 0 are never processed (0 = background)
  __syncthreads();
  for (;;) {
    // next category: the smallest id greater than the one just processed
    long long mine = 0x7FFFFFFFFFFFFFFFll;
    for (int q = tid; q < Q; q += 256)
      if (s_cat[q] > s_cur && s_cat[q] < mine) mine = s_cat[q];
    r_key[tid] = mine;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if (tid < st && r_key[tid + st] < r_key[tid]) r_key[tid] = r_key[tid + st];
      __syncthreads();
    }
    const long long cur = r_key[0];
    __syncthreads();
    if (cur == 0x7FFFFFFFFFFFFFFFll) break;
    if (tid == 0) s_cur = cur;
    for (int q = tid; q < Q; q += 256) {
      s_act[q] = s_cat[q] == cur;
      s_sc[q] = (double)scores[q];
    }
    __syncthreads();
    for (;;) {
      // argmax over the active set; key = (score, index) so equal maxima resolve to the largest index
      double bv = -1.0; int bi = -1;
      for (int q = tid; q < Q; q += 256)
        if (s_act[q] && (s_sc[q] > bv || (s_sc[q] == bv && q > bi))) { bv = s_sc[q]; bi = q; }
      r_val[tid] = bv; r_key[tid] = bi;
      __syncthreads();
      for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
          const double ov = r_val[tid + st]; const long long oi = r_key[tid + st];
          if (oi >= 0 && (r_key[tid] < 0 || ov > r_val[tid] || (ov == r_val[tid] && oi > r_key[tid]))) { r_val[tid] = ov; r_key[tid] = oi; }
        }
        __syncthreads();
      }
      const int best = (int)r_key[0];
      const double best_s = r_val[0];
      __syncthreads();
      if (best < 0) break;
      if (tid == 0) {
        s_act[best] = 0;
        if (inter[(long)best * Q + best] > 0) {         // area of the mask = |m & m|: empty masks are not emitted
          const int n = s_n++;
          out_idx[n] = best; out_score[n] = best_s; out_cat[n] = cur;
        }
      }
      __syncthreads();
      for (int q = tid; q < Q; q += 256) {
        if (!s_act[q]) continue;
        const double iou = (double)inter[(long)q * Q + best] / ((double)uni[(long)q * Q + best] + 1e-7);
        double s = s_sc[q];
        if (nms_type == 0) { if (iou > thr) s = s * 0.0; }
        else if (nms_type == 1) { if (iou > thr) s = s * (1.0 - iou); }
        else s = s * exp(-(iou * iou) / sigma);
        s_sc[q] = s;
        if (!(s > score_thr)) s_act[q] = 0;
      }
      __syncthreads();
    }
  }
  if (tid == 0) out_count[img] = s_n;
  // packed (optional): everything the host needs from this image in ONE row of float64 — [index | score | category | every query's
  // category | count, range flag] (small integers are exact in float64) — so that one device -> host copy fetches it
  if (packed) {
    __syncthreads();
    double* row = packed + (long)img * (4 * Q + 2);
    const int n = s_n;
    for (int q = tid; q < Q; q += 256) {
      row[q] = q < n ? (double)out_idx[q] : -1.0;
      row[Q + q] = q < n ? out_score[q] : 0.0;
      row[2 * Q + q] = q < n ? (double)out_cat[q] : 0.0;
      row[3 * Q + q] = (double)s_cat[q];
    }
    if (tid == 0) { row[4 * Q] = (double)n; row[4 * Q + 1] = range_flag ? (double)*range_flag : 0.0; }
  }
}

// The same loop for Q <= NMS_WAVE_MAXQ candidates with ONE wave per image doing the selection (round 4).  The block-wide form above
// spends its time in __syncthreads: ~11 per selection step (an 8-level argmax tree + 3), ~100 steps for the COCO-20K fixture: 52 us for
// 100 candidates.  Here the whole workgroup first turns the image's integer counts into the Q x Q float64 IoU table in LDS (one
// division per pair, done once, in parallel: the table replaces two loads and a float64 division per candidate and step) and notes which
// masks are empty; then wave 0 alone runs the loop: a lane owns candidates lane, lane + 64, the argmax is a wave reduction of
// (score, index) keys (nms_wave_argmax below), no barrier.  Same arithmetic (float64 scores, IoU = inter / (union + 1e-7) in float64), same tie rule (largest
// index among equal maxima), same emission order.
#define NMS_WAVE_MAXQ 128
// argmax of (score, index) keys over a wave: four DPP steps inside each row of 16 lanes (quad xor 1, quad xor 2, half-row mirror, row
// mirror: both lanes of a pair take the same winner, so after them every lane holds its row's), then the four rows' winners by
// v_readlane — ~40 VALU instructions instead of six rounds of three ds_bpermute (each a trip through the LDS crossbar).
__device__ __forceinline__ void nms_take(double& bv, int& bi, double ov, int oi) {
  if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi > bi))) { bv = ov; bi = oi; }
}
template <int CTRL>
__device__ __forceinline__ void nms_dpp_step(double& bv, int& bi) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, bv);
  const int lo = (int)(unsigned)u, hi = (int)(unsigned)(u >> 32);
  const int olo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  const int ohi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  const int oi = __builtin_amdgcn_update_dpp(bi, bi, CTRL, 0xf, 0xf, false);
  nms_take(bv, bi, __builtin_bit_cast(double, ((unsigned long long)(unsigned)ohi << 32) | (unsigned)olo), oi);
}
__device__ __forceinline__ void nms_wave_argmax(double& bv, int& bi) {
  nms_dpp_step<0xB1>(bv, bi);                                 // quad_perm [1,0,3,2]
  nms_dpp_step<0x4E>(bv, bi);                                 // quad_perm [2,3,0,1]
  nms_dpp_step<0x141>(bv, bi);                                // row_half_mirror
  nms_dpp_step<0x140>(bv, bi);                                // row_mirror
  const unsigned long long u = __builtin_bit_cast(unsigned long long, bv);
  const int lo = (int)(unsigned)u, hi = (int)(unsigned)(u >> 32);
  double rv[4]; int ri[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned l = (unsigned)__builtin_amdgcn_readlane(lo, 16 * r), h = (unsigned)__builtin_amdgcn_readlane(hi, 16 * r);
    rv[r] = __builtin_bit_cast(double, ((unsigned long long)h << 32) | l);
    ri[r] = __builtin_amdgcn_readlane(bi, 16 * r);
  }
  bv = rv[0]; bi = ri[0];
#pragma unroll
  for (int r = 1; r < 4; ++r) nms_take(bv, bi, rv[r], ri[r]);
}
__global__ __launch_bounds__(256) void mask_nms_wave_kernel(const int* inter, const int* uni, const float* scores, const long long* cats,
                                                            int Q, int nms_type, double thr, double sigma, double score_thr,
                                                            int* out_idx, double* out_score, long long* out_cat, int* out_count,
                                                            double* packed, const int* range_flag, int* zero_word) {
  extern __shared__ double s_iou[];                          // [Q][Q] IoU, then [Q] scores of the kept, [Q] (as int) indices / categories
  __shared__ unsigned char s_empty[NMS_WAVE_MAXQ];
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (zero_word && img == 0 && tid == 0) *zero_word = 0;     // (the cursor of the run / string kernel launched behind this one)
  inter += (long)img * Q * Q; uni += (long)img * Q * Q;
  scores += (long)img * Q; cats += (long)img * Q;
  out_idx += (long)img * Q; out_score += (long)img * Q; out_cat += (long)img * Q;
#pragma unroll 8                                             // eight pairs of loads in flight (40 dependent round trips for Q = 100 otherwise: ~25 of this kernel's 37 us)
  for (int i = tid; i < Q * Q; i += 256) s_iou[i] = (double)inter[i] / ((double)uni[i] + 1e-7);
  for (int q = tid; q < Q; q += 256) s_empty[q] = inter[q * Q + q] <= 0;       // area of the mask = |m & m|: empty masks are not emitted
  __syncthreads();
  if (tid >= 64) return;                                      // wave 0 selects
  constexpr int PL = NMS_WAVE_MAXQ / 64;                     // candidates per lane
  long long cat[PL];
  double sc[PL];
  bool act[PL];
  double sc0[PL];       // the candidates' own scores, read once (they were a dependent global load in front of every category's loop: ~1.5 us x 9)
#pragma unroll
  for (int e = 0; e < PL; ++e) { const int q = lane + 64 * e; cat[e] = q < Q ? cats[q] : 0; sc0[e] = q < Q ? (double)scores[q] : 0.0; }
  int n_out = 0;
  long long cur = 0;                                          // categories <= 0 are never processed (0 = background)
  for (;;) {
    long long mine = 0x7FFFFFFFFFFFFFFFll;
#pragma unroll
    for (int e = 0; e < PL; ++e)
      if (cat[e] > cur && cat[e] < mine) mine = cat[e];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const long long t = __shfl_xor(mine, o, 64); mine = t < mine ? t : mine; }
    if (mine == 0x7FFFFFFFFFFFFFFFll) break;
    cur = mine;
#pragma unroll
    for (int e = 0; e < PL; ++e) { const int q = lane + 64 * e; act[e] = q < Q && cat[e] == cur; sc[e] = sc0[e]; }
    for (;;) {
      double bv = -1.0; int bi = -1;                          // key = (score, index): equal maxima resolve to the largest index
#pragma unroll
      for (int e = 0; e < PL; ++e) {
        const int q = lane + 64 * e;
        if (act[e] && (sc[e] > bv || (sc[e] == bv && q > bi))) { bv = sc[e]; bi = q; }
      }
      nms_wave_argmax(bv, bi);
      if (bi < 0) break;
      const int best = bi;
      if (!s_empty[best]) {
        if (lane == 0) { out_idx[n_out] = best; out_score[n_out] = bv; out_cat[n_out] = cur; }
        ++n_out;
      }
#pragma unroll
      for (int e = 0; e < PL; ++e) {
        const int q = lane + 64 * e;
        if (q == best) act[e] = false;
        if (!act[e]) continue;
        const double iou = s_iou[q * Q + best];
        double v = sc[e];
        if (nms_type == 0) { if (iou > thr) v = v * 0.0; }
        else if (nms_type == 1) { if (iou > thr) v = v * (1.0 - iou); }
        else v = v * exp(-(iou * iou) / sigma);
        sc[e] = v;
        if (!(v > score_thr)) act[e] = false;
      }
    }
  }
  if (lane == 0) out_count[img] = n_out;
  if (packed) {
    __builtin_amdgcn_s_waitcnt(0);                           // lane 0's global stores above, re-read below by the other lanes of this wave
    __threadfence_block();
    double* row = packed + (long)img * (4 * Q + 2);
    for (int q = lane; q < Q; q += 64) {
      row[q] = q < n_out ? (double)out_idx[q] : -1.0;
      row[Q + q] = q < n_out ? out_score[q] : 0.0;
      row[2 * Q + q] = q < n_out ? (double)out_cat[q] : 0.0;
      row[3 * Q + q] = (double)cats[q];
    }
    if (lane == 0) { row[4 * Q] = (double)n_out; row[4 * Q + 1] = range_flag ? (double)*range_flag : 0.0; }
  }
}

extern "C" int zh_mask_nms(const int* inter, const int* uni, const float* scores, const long long* category_ids, int B, int Q,
                           int nms_type, double nms_threshold, double sigma, double score_threshold,
                           int* out_index, double* out_score, long long* out_category, int* out_count, double* packed, const int* range_flag,
                           int* zero_word, hipStream_t stream) {
  ZH_CHECK_ARG(inter && uni && scores && category_ids && out_index && out_score && out_category && out_count,
               "zh_mask_nms: null pointer");
  ZH_CHECK_ARG(B > 0 && Q > 0 && Q <= NMS_MAXQ, "zh_mask_nms: need 0 < Q <= %d", NMS_MAXQ);
  ZH_CHECK_ARG(nms_type >= 0 && nms_type <= 2, "zh_mask_nms: nms_type %d not in {0 hard, 1 linear, 2 gaussian}", nms_type);
  if (Q <= NMS_WAVE_MAXQ) {
    const size_t lds = (size_t)Q * Q * sizeof(double);
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)mask_nms_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(mask_nms_wave_kernel, dim3(B), dim3(256), lds, stream, inter, uni, scores, category_ids, Q, nms_type, nms_threshold, sigma,
                       score_threshold, out_index, out_score, out_category, out_count, packed, range_flag, zero_word);
  } else
  hipLaunchKernelGGL(mask_nms_kernel, dim3(B), dim3(256), 0, stream, inter, uni, scores, category_ids, Q, nms_type, nms_threshold, sigma,
                     score_threshold, out_index, out_score, out_category, out_count, packed, range_flag, zero_word);
  ZH_CHECK_LAUNCH("zh_mask_nms");
  return ZH_OK;
}
