// COCO RLE of the kept instance masks on the device: run extraction (zh_mask_runs / zh_mask_runs_kept), the string kernel over
// the packed run list (zh_mask_rle_kept) and the one-launch fused form (zh_mask_rle_fused_kept).  The string format itself — group
// count, emitter, delta rule, run k of a transition list — is rle_codec.h's, shared with the host entry points (rle_host.hip).
#include "common.h"
#include "rle_codec.h"

// ---- run-length transitions + box + area of selected masks ON THE DEVICE (replaces the B x Q x H x W mask D2H in front of
//      pycocotools.mask.encode / masks_to_boxes, networks/zutis.py:288-294,446-452).  COCO RLE runs are column-major:
//      the mask is cut into 64-column panels staged through LDS (coalesced row reads); the value changes per column segment are
//      counted, prefix-summed, and the column-major pixel positions where the value changes are written.
//      counts = diff([0, positions..., H*W]) with a leading 0-run inserted when pixel 0 is set (host, tiny).
// One block per (mask, 64-column panel), TWO launches (round 4).  Round 3's single launch had every panel's block count the transitions of
// ALL columns left of its panel from global memory (the last panel re-read 90 % of the mask) and the first panel's block scan the whole
// mask once more for the box and the area: 55 us for 17 kept masks of 480 x 640, the critical path being those two long blocks.  Now
//   launch 1 (count): a block stages its panel [H][64] in LDS (coalesced row reads), four threads per column count the transitions of
//                     their quarter of the rows (the H-1 -> 0 wrap to the previous column included), and the panel's own pixels give its
//                     part of the box / area: per-panel results into a small table;
//   launch 2 (emit):  a block sums the counts of the panels to its left (<= W / 64 integers), stages its panel again, a 256-entry scan
//                     in (column, segment) order places its transitions and a second walk writes the column-major positions; the
//                     last panel's block writes the total, the first one folds the per-panel boxes / areas.
#define RUNS_PANEL 64
#define RUNS_SEG 4
__device__ __forceinline__ unsigned zh_nz_bytes(unsigned w) {   // 0x01 in every byte of w that is non-zero
  const unsigned t = ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w;
  return (t >> 7) & 0x01010101u;
}
// count != NULL (zh_mask_runs_kept): entry mi = b * Q + j is the j-th kept query of image b — sel[mi] is its query index (zh_mask_nms'
// out_index), entries j >= count[b] do nothing: the NMS result never visits the host before the runs are extracted.
struct RunsArgs {
  const unsigned char* masks; const int* sel; const int* count; int Q, H, W, max_runs, npanel;
  int* positions; int* nruns; int* box_area;
  int* pcount;       // [n][npanel] transitions per panel
  int* pbox;         // [n][npanel][5] xmin, ymin, xmax, ymax, area of the panel's pixels
  long packed_cap;   // > 0 (kept form only): `positions` is ONE list of that many ints, the kept masks' transitions back to back
};
// stages the panel (values normalised to {0,1}) and returns, per thread = (column c = tid / 4, row quarter sg = tid % 4), the number of
// transitions of its segment and the value in front of it
__device__ __forceinline__ int runs_stage_and_count(const RunsArgs& a, const unsigned char* m, unsigned char* sm, int x0, int pw, int& y0, int& y1,
                                                    unsigned char& prev0) {
  const int tid = threadIdx.x, H = a.H, W = a.W;
  const bool vec = (W % 16 == 0) && (((uintptr_t)m & 15) == 0);
  if (vec && pw % 16 == 0) {
    constexpr int cpr = RUNS_PANEL / 16;
#pragma unroll 8
    for (int i = tid; i < H * cpr; i += 256) {
      const int y = i / cpr, c16 = i - y * cpr;
      uint4 v = {0u, 0u, 0u, 0u};
      if (c16 * 16 < pw) v = *(const uint4*)(m + (long)y * W + x0 + c16 * 16);
      uint4 o = {zh_nz_bytes(v.x), zh_nz_bytes(v.y), zh_nz_bytes(v.z), zh_nz_bytes(v.w)};
      *(uint4*)(sm + (long)y * RUNS_PANEL + c16 * 16) = o;
    }
  } else {
    for (int i = tid; i < H * RUNS_PANEL; i += 256) {
      const int y = i / RUNS_PANEL, c = i - y * RUNS_PANEL;
      sm[i] = c < pw ? (m[(long)y * W + x0 + c] != 0) : 0;
    }
  }
  __syncthreads();
  const int c = tid / RUNS_SEG, sg = tid % RUNS_SEG;
  const int hs = (H + RUNS_SEG - 1) / RUNS_SEG;
  y0 = min(H, sg * hs); y1 = min(H, y0 + hs);
  prev0 = 0;
  int mine = 0;
  if (c < pw && y0 < y1) {
    if (y0 > 0) prev0 = sm[(y0 - 1) * RUNS_PANEL + c];
    else if (c > 0) prev0 = sm[(H - 1) * RUNS_PANEL + c - 1];
    else prev0 = x0 > 0 ? (unsigned char)(m[(long)(H - 1) * W + x0 - 1] != 0) : sm[0];   // pixel 0 starts the list: no transition
    unsigned char prev = prev0;
#pragma unroll 8
    for (int y = y0; y < y1; ++y) {
      const unsigned char v = sm[y * RUNS_PANEL + c];
      mine += v != prev;
      prev = v;
    }
  }
  return mine;
}
__device__ __forceinline__ const unsigned char* runs_mask(const RunsArgs& a, int mi) {
  return a.masks + (a.count ? (long)(mi / a.Q) * a.Q + a.sel[mi] : (long)a.sel[mi]) * a.H * a.W;
}
__global__ __launch_bounds__(256) void mask_runs_count_kernel(RunsArgs a) {
  extern __shared__ unsigned char sm[];                    // [H][64] panel
  __shared__ int s_cnt, s_minx, s_maxx, s_miny, s_maxy, s_area;
  const int tid = threadIdx.x, mi = blockIdx.x, pnl = blockIdx.y;
  if (a.count && mi % a.Q >= a.count[mi / a.Q]) return;   // whole workgroup, before any barrier
  const unsigned char* m = runs_mask(a, mi);
  const int x0 = pnl * RUNS_PANEL, pw = min(RUNS_PANEL, a.W - x0);
  if (tid == 0) { s_cnt = 0; s_minx = a.W; s_maxx = -1; s_miny = a.H; s_maxy = -1; s_area = 0; }
  int y0, y1; unsigned char prev0;
  const int mine = runs_stage_and_count(a, m, sm, x0, pw, y0, y1, prev0);   // (contains the barrier that publishes the initial values)
  // box / area of the panel's own pixels: thread = (column, row quarter)
  const int c = tid / RUNS_SEG;
  int area = 0, miny = a.H, maxy = -1;
  if (c < pw)
    for (int y = y0; y < y1; ++y)
      if (sm[y * RUNS_PANEL + c]) { ++area; miny = min(miny, y); maxy = max(maxy, y); }
  if (mine) atomicAdd(&s_cnt, mine);
  if (area) { atomicAdd(&s_area, area); atomicMin(&s_minx, x0 + c); atomicMax(&s_maxx, x0 + c); atomicMin(&s_miny, miny); atomicMax(&s_maxy, maxy); }
  __syncthreads();
  if (tid == 0) {
    a.pcount[(long)mi * a.npanel + pnl] = s_cnt;
    int* b = a.pbox + ((long)mi * a.npanel + pnl) * 5;
    b[0] = s_minx; b[1] = s_miny; b[2] = s_maxx; b[3] = s_maxy; b[4] = s_area;
  }
}
__global__ __launch_bounds__(256) void mask_runs_emit_kernel(RunsArgs a) {
  extern __shared__ unsigned char sm[];
  __shared__ int s_red[256];
  const int tid = threadIdx.x, mi = blockIdx.x, pnl = blockIdx.y;
  if (a.count && mi % a.Q >= a.count[mi / a.Q]) return;
  const unsigned char* m = runs_mask(a, mi);
  int* pos = a.positions + (long)mi * a.max_runs;
  long room = a.max_runs;                                  // entries this mask may write
  if (a.packed_cap > 0) {
    // packed form: mask mi's list starts where the lists of the kept masks in front of it (image-major, kept order) end; each of those
    // is min(its transitions, max_runs) long — summed here from the count kernel's per-panel counts (<= B*Q*npanel ints, L2-resident)
    long part = 0;
    for (int mp = tid; mp < mi; mp += 256) {
      if (mp % a.Q >= a.count[mp / a.Q]) continue;
      int t = 0;
      for (int p = 0; p < a.npanel; ++p) t += a.pcount[(long)mp * a.npanel + p];
      part += min(t, a.max_runs);
    }
    s_red[tid] = (int)part;                                // < 2^31: B*Q*max_runs is checked by the host entry
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if (tid < st) s_red[tid] += s_red[tid + st];
      __syncthreads();
    }
    const long off = s_red[0];
    __syncthreads();
    pos = a.positions + off;
    room = min((long)a.max_runs, a.packed_cap - off);      // <= 0: the list does not fit any more (the host sees it from the counts)
  }
  const int x0 = pnl * RUNS_PANEL, pw = min(RUNS_PANEL, a.W - x0);
  int base = 0;
  for (int p = 0; p < pnl; ++p) base += a.pcount[(long)mi * a.npanel + p];
  int y0, y1; unsigned char prev0;
  const int mine = runs_stage_and_count(a, m, sm, x0, pw, y0, y1, prev0);
  s_red[tid] = mine;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {                      // inclusive scan (Hillis - Steele), entry e = column * RUNS_SEG + segment == tid
    const int t = tid >= d ? s_red[tid - d] : 0;
    __syncthreads();
    s_red[tid] += t;
    __syncthreads();
  }
  const int total = base + s_red[255];
  if (mine) {
    const int c = tid / RUNS_SEG;
    int o = base + s_red[tid] - mine;
    unsigned char prev = prev0;
#pragma unroll 8
    for (int y = y0; y < y1; ++y) {
      const unsigned char v = sm[y * RUNS_PANEL + c];
      if (v != prev) { if (o < room) pos[o] = (x0 + c) * a.H + y; ++o; }
      prev = v;
    }
  }
  if (pnl == a.npanel - 1 && tid == 0) {
    a.nruns[mi * 2] = total;                               // number of transitions (may exceed max_runs => host fallback)
    a.nruns[mi * 2 + 1] = m[0] != 0;                       // value of pixel 0
  }
  if (pnl == 0 && tid == 0) {                              // fold the per-panel boxes / areas
    int minx = a.W, miny = a.H, maxx = -1, maxy = -1, area = 0;
    for (int p = 0; p < a.npanel; ++p) {
      const int* b = a.pbox + ((long)mi * a.npanel + p) * 5;
      minx = min(minx, b[0]); miny = min(miny, b[1]); maxx = max(maxx, b[2]); maxy = max(maxy, b[3]); area += b[4];
    }
    int* o = a.box_area + mi * 5;
    o[0] = minx; o[1] = miny; o[2] = maxx; o[3] = maxy; o[4] = area;
  }
}

static int launch_mask_runs(const char* what, RunsArgs a, int n, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  const size_t lds = ((size_t)a.H * RUNS_PANEL + 15) & ~(size_t)15;
  ZH_CHECK_ARG(lds <= 150 * 1024, "%s: H=%d too tall for the LDS panel", what, a.H);
  a.npanel = zh_cdiv(a.W, RUNS_PANEL);
  ZH_CHECK_ARG(a.npanel <= 65535, "%s: mask too wide", what);
  const size_t need = (size_t)n * a.npanel * 6 * sizeof(int);
  if (!workspace || workspace_bytes < need) {
    zh_set_error("%s: workspace too small (%zu < %zu)", what, workspace_bytes, need);
    return ZH_ERR_WORKSPACE;
  }
  a.pcount = (int*)workspace;
  a.pbox = a.pcount + (size_t)n * a.npanel;
  if (lds > 64 * 1024) {
    (void)hipFuncSetAttribute((const void*)mask_runs_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipFuncSetAttribute((const void*)mask_runs_emit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  }
  hipLaunchKernelGGL(mask_runs_count_kernel, dim3(n, a.npanel), dim3(256), lds, stream, a);
  hipLaunchKernelGGL(mask_runs_emit_kernel, dim3(n, a.npanel), dim3(256), lds, stream, a);
  ZH_CHECK_LAUNCH(what);
  return ZH_OK;
}
extern "C" size_t zh_mask_runs_workspace_size(int n, int W) { return (size_t)n * zh_cdiv(W, RUNS_PANEL) * 6 * sizeof(int); }

extern "C" int zh_mask_runs(const unsigned char* masks, const int* sel, int n_sel, int H, int W, int max_runs,
                            int* positions, int* nruns, int* box_area, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  ZH_CHECK_ARG(masks && sel && positions && nruns && box_area && n_sel > 0 && H > 0 && W > 0 && max_runs > 0, "zh_mask_runs: bad arguments");
  ZH_CHECK_ARG((long)H * W < (1L << 31), "zh_mask_runs: mask too large");
  RunsArgs a{masks, sel, nullptr, 1, H, W, max_runs, 0, positions, nruns, box_area, nullptr, nullptr, 0};
  return launch_mask_runs("zh_mask_runs", a, n_sel, workspace, workspace_bytes, stream);
}

extern "C" int zh_mask_runs_kept(const unsigned char* masks, const int* kept_index, const int* kept_count, int B, int Q, int H, int W, int max_runs,
                                 int* positions, long packed_capacity, int* nruns, int* box_area, void* workspace, size_t workspace_bytes,
                                 hipStream_t stream) {
  ZH_CHECK_ARG(masks && kept_index && kept_count && positions && nruns && box_area && B > 0 && Q > 0 && H > 0 && W > 0 && max_runs > 0,
               "zh_mask_runs_kept: bad arguments");
  ZH_CHECK_ARG((long)H * W < (1L << 31) && (long)B * Q < (1L << 31), "zh_mask_runs_kept: mask / batch too large");
  ZH_CHECK_ARG(packed_capacity >= 0 && (packed_capacity == 0 || (long)B * Q * max_runs < (1L << 31)),
               "zh_mask_runs_kept: packed_capacity=%ld (needs B*Q*max_runs < 2^31)", packed_capacity);
  RunsArgs a{masks, kept_index, kept_count, Q, H, W, max_runs, 0, positions, nruns, box_area, nullptr, nullptr, packed_capacity};
  return launch_mask_runs("zh_mask_runs_kept", a, B * Q, workspace, workspace_bytes, stream);
}

// ---- COCO RLE strings of the kept masks, on the device (pycocotools rleEncode + rleToString, the strings of zutis.py:290,448).
// Input: zh_mask_runs_kept's packed list (column-major pixel indices where the value changes) and its nruns table.  One workgroup per
// kept mask; runs, values and characters are rle_codec.h's (rle_value, rle_groups, rle_put) — the number of groups is a function of the
// value alone, so a block scan of the group counts places every run's characters.  Mask mi's string starts at 5 * off(mi) + 16 * rank(mi)
// in `out` (off = the start of its list in the packed positions, rank = kept masks in front of it: both follow from nruns and the
// counts, on the host too; what that budget guarantees: rle_codec.h, "the character bound"), out_len[mi] = its length, or -1 when the
// mask has more than max_runs transitions or its list / string lies past a capacity (the host encodes that mask itself).
struct RleArgs {
  const int* positions; long packed_cap; const int* nruns; const int* count; int Q, max_runs; long HW;
  unsigned char* out; long out_cap; int* out_len;
};
#define RLE_LDS_RUNS 8192
__global__ __launch_bounds__(256) void mask_rle_kernel(RleArgs a) {
  __shared__ int s_a[256], s_b[256];
  __shared__ int s_w[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mi = blockIdx.x;
  if (mi % a.Q >= a.count[mi / a.Q]) return;               // whole workgroup, before any barrier
  int part = 0, rank = 0;
  for (int mp = tid; mp < mi; mp += 256)
    if (mp % a.Q < a.count[mp / a.Q]) { part += min(a.nruns[2 * mp], a.max_runs); ++rank; }
  s_a[tid] = part; s_b[tid] = rank;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) { s_a[tid] += s_a[tid + st]; s_b[tid] += s_b[tid + st]; }
    __syncthreads();
  }
  const long off = s_a[0], cstart = 5L * s_a[0] + 16L * s_b[0];
  const int nt = a.nruns[2 * mi], lead = a.nruns[2 * mi + 1] != 0 ? 1 : 0;
  const int nc = nt + 1 + lead;
  // H*W < 2^24: a value takes at most 5 characters, so 5 nc bounds the string and the slot of 5 nt + 16 holds it (rle_codec.h, "the
  // character bound").  Larger masks: the string is measured below, before a character is written.
  const bool big = a.HW >= RLE_FIVE_CHAR_PIXELS;
  if (nt > a.max_runs || off + nt > a.packed_cap || (!big && cstart + 5L * nc > a.out_cap)) {
    if (tid == 0) a.out_len[mi] = -1;
    return;
  }
  // the mask's list goes to LDS in one sweep of wide loads (every run is read four times below: 25 -> ~10 us for the fixture's
  // 1750-transition masks); lists longer than the LDS copy are read where they lie
  __shared__ int s_p[RLE_LDS_RUNS];
  const int* p = a.positions + off;
  if (nt <= RLE_LDS_RUNS) {
    for (int i = tid; i < nt; i += 256) s_p[i] = p[i];
    __syncthreads();
    p = s_p;
  }
  if (big) {
    // values of 2^24 and more in magnitude take 6 or 7 characters: the string's true length against its window
    // [cstart, min(cstart + 5 nt + 16, out_cap)) — the neighbour's slot starts behind it — decides, for the whole workgroup
    __shared__ long s_len[4];
    long len = 0;
    for (int k = tid; k < nc; k += 256) len += rle_groups(rle_value(p, nt, lead != 0, a.HW, k));
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) len += __shfl_xor(len, d, 64);
    if (lane == 0) s_len[wave] = len;
    __syncthreads();
    len = s_len[0] + s_len[1] + s_len[2] + s_len[3];
    if (len > min(5L * nt + 16, a.out_cap - cstart)) {
      if (tid == 0) a.out_len[mi] = -1;
      return;
    }
  }
  unsigned char* o = a.out + cstart;
  int base = 0;
  for (int k0 = 0; k0 < nc; k0 += 256) {
    const int k = k0 + tid;
    long x = 0;
    int n = 0;
    if (k < nc) { x = rle_value(p, nt, lead != 0, a.HW, k); n = rle_groups(x); }
    int inc = n;                                            // inclusive scan: within the wave by shuffles, across the four waves through LDS
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
    __syncthreads();                                        // (the previous chunk's s_w reads are done)
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int wbase = 0;
    for (int w = 0; w < wave; ++w) wbase += s_w[w];
    const int total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    if (k < nc) rle_put(o + base + wbase + inc - n, x);
    base += total;
  }
  if (tid == 0) a.out_len[mi] = base;
}
extern "C" int zh_mask_rle_kept(const int* positions, long packed_capacity, const int* nruns, const int* kept_count, int B, int Q, int max_runs,
                                long HW, unsigned char* out, long out_capacity, int* out_len, hipStream_t stream) {
  ZH_CHECK_ARG(positions && nruns && kept_count && out && out_len && B > 0 && Q > 0 && max_runs > 0 && HW > 0 && packed_capacity > 0 &&
               out_capacity > 0, "zh_mask_rle_kept: bad arguments");
  ZH_CHECK_ARG((long)B * Q * max_runs < (1L << 31) / 5 && HW < (1L << 31), "zh_mask_rle_kept: B*Q*max_runs or H*W too large");
  RleArgs a{positions, packed_capacity, nruns, kept_count, Q, max_runs, HW, out, out_capacity, out_len};
  hipLaunchKernelGGL(mask_rle_kernel, dim3(B * Q), dim3(256), 0, stream, a);
  ZH_CHECK_LAUNCH("zh_mask_rle_kept");
  return ZH_OK;
}

// ---- the same three steps (runs, box / area, RLE string) of a kept mask in ONE workgroup and ONE launch (round 4; the batch-1 predict's tail was
// count 27 + emit 18 + string 21 us, each a chain of a dozen dependent ~1-us steps on 17 busy workgroups).  With one workgroup per mask the
// per-pixel walk of the panel kernels would be 17 CUs doing what 170 did, so everything here is word-parallel on the mask's BITS (row-major,
// H*W/8 bytes in LDS: 38 KB for 480x640; copied from the IoU step's bit-packed workspace when the caller has it, else packed from the bytes
// with 16-byte loads).  A transition of the column-major order is a bit of T = B xor (B moved down one row) (row 0 against the last row of
// the column to the left).  A thread owns (32-column panel p, 16-row chunk s):
//   pass 1: its 16 words of T go through a bit-sliced vertical counter (5 planes, registers): per-column counts of the chunk -> part[s][c];
//   then a per-column prefix over the chunks (in place) and a block scan over the columns give every (column, chunk)'s place in the list;
//   pass 2: the 16 words again (registers); per column that has a transition in the chunk, its rows in ascending order -> list[place++];
//   string: mask_rle_kernel's steps from the LDS list into an LDS buffer (one pass: the length falls out of the scan), an atomic cursor
//           places it in `out` (order of arrival: the host reads every string's offset from `info`), a coalesced copy writes it.
// No LDS read-modify-write anywhere.  info int32 [B*Q][8] = {string offset, string length (-1: not encoded — more than max_runs
// transitions or `out` full), xmin, ymin, xmax, ymax, area, transitions}; rows of slots past an image's count are not written.
struct FusedRleArgs {
  const unsigned char* masks; const unsigned long long* bits; const int* sel; const int* count; int Q, H, W, max_runs;
  unsigned char* out; long out_cap; int* cursor; int* info;
};
#define FRLE_ROWS 16                                         // rows per chunk (= counts per (chunk, column) fit the 5-plane counter)
__device__ __forceinline__ unsigned rle_bits4(unsigned w) {  // bit k = byte k of w is non-zero
  const unsigned nz = zh_nz_bytes(w);
  return (nz & 1u) | ((nz >> 7) & 2u) | ((nz >> 14) & 4u) | ((nz >> 21) & 8u);
}
struct FrleLayout { long n64; int P, S, Wp; size_t o_part, o_coloff, o_list, total; };
__host__ __device__ static inline FrleLayout frle_layout(int H, int W, int max_runs) {
  FrleLayout L;
  L.n64 = ((long)H * W + 63) >> 6;
  L.P = (W + 31) >> 5;                                       // 32-column panels
  L.Wp = ((W + 63) >> 6) * 64; L.S = (H + FRLE_ROWS - 1) / FRLE_ROWS;
  L.o_part = (size_t)(L.n64 + 2) * 8;                        // u64 bits[n64 + 2] (two zero words behind the last: funnel reads)
  size_t r0 = L.o_part + (size_t)L.S * L.Wp * 2;             // u16 part[S][Wp]
  const size_t cb = ((size_t)5 * (max_runs + 2) + 15) & ~(size_t)15;
  if (r0 < cb) r0 = cb;                                      // the string is built over bits + part once they are dead
  L.o_coloff = r0;
  L.o_list = L.o_coloff + (size_t)L.Wp * 4;                  // int coloff[Wp]
  L.total = L.o_list + (size_t)max_runs * 4;                 // int list[max_runs]
  return L;
}
__global__ __launch_bounds__(1024) void mask_rle_fused_kernel(FusedRleArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
  __shared__ int s_w[16], s_red[5][16];
  __shared__ int s_off;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x, nw = nthr >> 6, mi = blockIdx.x;
  if (mi % a.Q >= a.count[mi / a.Q]) return;                // whole workgroup, before any barrier
  const int H = a.H, W = a.W;
  const long HW = (long)H * W;
  const long mask_index = (long)(mi / a.Q) * a.Q + a.sel[mi];
  const FrleLayout L = frle_layout(H, W, a.max_runs);
  unsigned long long* Bw = (unsigned long long*)dyn;
  unsigned* B32 = (unsigned*)dyn;                            // bit (f & 31) of B32[f >> 5] = pixel f (row-major) is set
  unsigned short* part = (unsigned short*)(dyn + L.o_part);
  int* coloff = (int*)(dyn + L.o_coloff);
  int* list = (int*)(dyn + L.o_list);
  if (a.bits) {
    const unsigned long long* src = a.bits + mask_index * L.n64;
    for (long i = tid; i < L.n64; i += nthr) Bw[i] = src[i];
    for (long i = L.n64 + tid; i < L.n64 + 2; i += nthr) Bw[i] = 0;
  } else {
    const unsigned char* m = a.masks + mask_index * HW;
    unsigned short* B16 = (unsigned short*)dyn;
    const long n16 = (HW + 15) >> 4;
    if (HW % 16 == 0 && ((uintptr_t)m & 15) == 0) {
#pragma unroll 8
      for (long i = tid; i < n16; i += nthr) {
        const uint4 v = ((const uint4*)m)[i];
        B16[i] = (unsigned short)(rle_bits4(v.x) | (rle_bits4(v.y) << 4) | (rle_bits4(v.z) << 8) | (rle_bits4(v.w) << 12));
      }
    } else {
      for (long i = tid; i < n16; i += nthr) {
        unsigned b = 0;
        for (int k = 0; k < 16; ++k)
          if (16 * i + k < HW && m[16 * i + k]) b |= 1u << k;
        B16[i] = (unsigned short)b;
      }
    }
    for (long i = n16 + tid; i < (L.n64 + 2) * 4; i += nthr) B16[i] = 0;
  }
  for (int i = tid; i < L.S * L.Wp / 2; i += nthr) ((unsigned*)part)[i] = 0;
  __syncthreads();
  // 32 columns of row y, from column 32 p on (bits past the row's end are 0)
  auto rowword = [&](int y, int p) -> unsigned {
    const long f0 = (long)y * W + 32L * p;
    const int sh = (int)(f0 & 31);
    const unsigned lo = B32[f0 >> 5], hi = B32[(f0 >> 5) + 1];
    unsigned w = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
    const int nb = W - 32 * p;
    if (nb < 32) w &= (1u << nb) - 1u;
    return w;
  };
  // the 16 words of T of item (p, chunk sc) (rows past H: 0); row 0 is compared with the LAST row one column to the left (column 0 of the
  // mask: pixel 0 itself, no transition)
  auto item_words = [&](int p, int sc, unsigned (&t)[FRLE_ROWS], int& area, int& miny, int& maxy, unsigned& ored) {
    const int y0 = sc * FRLE_ROWS;
    unsigned prev;
    if (y0 == 0) {
      const unsigned last = rowword(H - 1, p);
      prev = (last << 1) | (p ? rowword(H - 1, p - 1) >> 31 : (rowword(0, 0) & 1u));
    } else prev = rowword(y0 - 1, p);
    const int nb = min(32, W - 32 * p);
    const unsigned cmask = nb < 32 ? (1u << nb) - 1u : ~0u;
#pragma unroll
    for (int i = 0; i < FRLE_ROWS; ++i) {
      const int y = y0 + i;
      unsigned cur = 0;
      t[i] = 0;
      if (y < H) {
        cur = rowword(y, p);
        t[i] = (cur ^ prev) & cmask;
        prev = cur;
        if (cur) { area += __popc(cur); miny = min(miny, y); maxy = y; ored |= cur; }
      }
    }
  };
  // ---- pass 1: per-column transition counts of every (chunk, panel); area, box
  const int nitems = L.P * L.S;
  int area = 0, miny = H, maxy = -1, minx = W, maxx = -1;
  unsigned t_first[FRLE_ROWS];                               // the thread's first item's words, kept for pass 2 (most shapes: its only item)
  for (int it = tid; it < nitems; it += nthr) {
    const int p = it % L.P, sc = it / L.P;
    unsigned t[FRLE_ROWS], ored = 0;
    item_words(p, sc, t, area, miny, maxy, ored);
    if (it == tid) {
#pragma unroll
      for (int i = 0; i < FRLE_ROWS; ++i) t_first[i] = t[i];
    }
    if (ored) { minx = min(minx, 32 * p + __ffs((int)ored) - 1); maxx = max(maxx, 32 * p + 31 - __clz((int)ored)); }
    unsigned c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;         // bit j of (c4 c3 c2 c1 c0) = transitions of column j so far (<= 16)
#pragma unroll
    for (int i = 0; i < FRLE_ROWS; ++i) {
      unsigned carry = t[i], x;
      x = c0 & carry; c0 ^= carry; carry = x;
      x = c1 & carry; c1 ^= carry; carry = x;
      x = c2 & carry; c2 ^= carry; carry = x;
      x = c3 & carry; c3 ^= carry; carry = x;
      c4 ^= carry;
    }
    unsigned any = c0 | c1 | c2 | c3 | c4;
    unsigned short* pc = part + (long)sc * L.Wp + 32 * p;
    while (any) {
      const int j = __ffs((int)any) - 1;
      any &= any - 1;
      pc[j] = (unsigned short)(((c0 >> j) & 1u) | (((c1 >> j) & 1u) << 1) | (((c2 >> j) & 1u) << 2) | (((c3 >> j) & 1u) << 3) | (((c4 >> j) & 1u) << 4));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    area += __shfl_xor(area, o, 64);
    miny = min(miny, __shfl_xor(miny, o, 64)); maxy = max(maxy, __shfl_xor(maxy, o, 64));
    minx = min(minx, __shfl_xor(minx, o, 64)); maxx = max(maxx, __shfl_xor(maxx, o, 64));
  }
  if (lane == 0) { s_red[0][wave] = area; s_red[1][wave] = miny; s_red[2][wave] = maxy; s_red[3][wave] = minx; s_red[4][wave] = maxx; }
  __syncthreads();
  // ---- per column: exclusive prefix over the chunks (in place), then a block scan of the column totals -> coloff
  int ctot = 0;
  if (tid < L.Wp) {
    for (int sc = 0; sc < L.S; ++sc) { const int v = part[(long)sc * L.Wp + tid]; part[(long)sc * L.Wp + tid] = (unsigned short)ctot; ctot += v; }
  }
  int inc = ctot;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int wbase = 0, nt = 0;
  for (int w = 0; w < nw; ++w) { if (w < wave) wbase += s_w[w]; nt += s_w[w]; }
  if (tid < L.Wp) coloff[tid] = wbase + inc - ctot;
  int* info = a.info + (long)mi * 8;
  if (tid == 0) {
    int A = 0, y0 = H, y1 = -1, x0 = W, x1 = -1;
    for (int w = 0; w < nw; ++w) { A += s_red[0][w]; y0 = min(y0, s_red[1][w]); y1 = max(y1, s_red[2][w]); x0 = min(x0, s_red[3][w]); x1 = max(x1, s_red[4][w]); }
    info[2] = x0; info[3] = y0; info[4] = x1; info[5] = y1; info[6] = A; info[7] = nt;
  }
  if (nt > a.max_runs) {
    if (tid == 0) { info[0] = 0; info[1] = -1; }
    return;
  }
  const int lead = (int)(B32[0] & 1u), nc = nt + 1 + lead;
  __syncthreads();
  // ---- pass 2: the same threads write their transitions to their places in the list, column by column
  for (int it = tid; it < nitems; it += nthr) {
    const int p = it % L.P, sc = it / L.P, y0 = sc * FRLE_ROWS;
    unsigned t[FRLE_ROWS], ored = 0;
    if (it == tid) {
#pragma unroll
      for (int i = 0; i < FRLE_ROWS; ++i) t[i] = t_first[i];
    } else {
      int d0 = 0, d1 = 0, d2 = 0;
      item_words(p, sc, t, d0, d1, d2, ored);
    }
    unsigned any = 0;
#pragma unroll
    for (int i = 0; i < FRLE_ROWS; ++i) any |= t[i];
    const unsigned short* pc = part + (long)sc * L.Wp + 32 * p;
    const int* co = coloff + 32 * p;
    // per column with a transition: its 16 row bits gathered into one word, then one store per set bit; the NEXT column's place is
    // requested from LDS before this column's stores (the two loads were a third of the pass when they sat in front of every column)
    int j = any ? __ffs((int)any) - 1 : 0;
    int o = co[j] + pc[j];
    while (any) {
      any &= any - 1;
      const int jn = any ? __ffs((int)any) - 1 : j;
      const int on = co[jn] + pc[jn];
      unsigned cw = 0;
#pragma unroll
      for (int i = 0; i < FRLE_ROWS; ++i) cw |= ((t[i] >> j) & 1u) << i;
      const int v = (32 * p + j) * H + y0;
      while (cw) { list[o++] = v + __ffs((int)cw) - 1; cw &= cw - 1; }
      j = jn; o = on;
    }
  }
  __syncthreads();
  // ---- the string (see mask_rle_kernel) into LDS, over the dead bits / counts
  unsigned char* cbuf = dyn;
  int base = 0;
  for (int k0 = 0; k0 < nc; k0 += 2 * nthr) {                 // two consecutive runs per thread and step (half the barriers)
    const int k = k0 + 2 * tid;
    long xa = 0, xb = 0;
    int na = 0, nb = 0;
    if (k < nc) { xa = rle_value(list, nt, lead != 0, HW, k); na = rle_groups(xa); }
    if (k + 1 < nc) { xb = rle_value(list, nt, lead != 0, HW, k + 1); nb = rle_groups(xb); }
    int in2 = na + nb;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(in2, d, 64); if (lane >= d) in2 += t; }
    __syncthreads();                                        // (the previous step's s_w reads are done)
    if (lane == 63) s_w[wave] = in2;
    __syncthreads();
    int wb = 0, total = 0;
    for (int w = 0; w < nw; ++w) { if (w < wave) wb += s_w[w]; total += s_w[w]; }
    unsigned char* q = cbuf + base + wb + in2 - na - nb;
    if (k < nc) rle_put(q, xa);
    if (k + 1 < nc) rle_put(q + na, xb);
    base += total;
  }
  if (tid == 0) {
    const int off = atomicAdd(a.cursor, base);
    const bool fits = (long)off + base <= a.out_cap;
    info[0] = off; info[1] = fits ? base : -1;
    s_off = fits ? off : -1;
  }
  __syncthreads();
  if (s_off < 0) return;
  unsigned char* o = a.out + s_off;
  for (int i = tid; i < base; i += nthr) o[i] = cbuf[i];
}
static size_t rle_fused_lds(int H, int W, int max_runs) { return frle_layout(H, W, max_runs).total; }
extern "C" int zh_mask_rle_fused_supported(int H, int W, int max_runs) {
  return H > 0 && W > 0 && W <= 1024 && max_runs > 0 && (long)H * W < (1L << 31) && rle_fused_lds(H, W, max_runs) <= 150 * 1024;
}
extern "C" int zh_mask_rle_fused_kept(const unsigned char* masks, const unsigned long long* bits, const int* kept_index, const int* kept_count,
                                      int B, int Q, int H, int W, int max_runs, unsigned char* out, long out_capacity, int* cursor, int* info,
                                      hipStream_t stream) {
  ZH_CHECK_ARG((masks || bits) && kept_index && kept_count && out && cursor && info && B > 0 && Q > 0 && out_capacity > 0 && (long)B * Q < (1L << 31),
               "zh_mask_rle_fused_kept: bad arguments");
  ZH_CHECK_ARG(zh_mask_rle_fused_supported(H, W, max_runs), "zh_mask_rle_fused_kept: H=%d W=%d max_runs=%d not supported (W <= 1024, bits + tables + list <= 150 KB of LDS)",
               H, W, max_runs);
  FusedRleArgs a{masks, bits, kept_index, kept_count, Q, H, W, max_runs, out, out_capacity, cursor, info};
  const size_t lds = rle_fused_lds(H, W, max_runs);
  if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)mask_rle_fused_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(mask_rle_fused_kernel, dim3(B * Q), dim3(((W + 63) / 64) * 64), lds, stream, a);     // >= one thread per column (W <= 1024)
  ZH_CHECK_LAUNCH("zh_mask_rle_fused_kept");
  return ZH_OK;
}
