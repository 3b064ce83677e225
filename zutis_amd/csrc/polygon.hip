// Polygon annotations to COCO run lengths on the device (zutis_amd/polygons.py): rle.from_polygons — pycocotools' rleFrPoly per
// polygon and the union of an annotation's polygons — for a whole annotation file in ONE launch, one workgroup per annotation.
//
//   walk    the lanes stride over the points of a polygon's walk at 5 x the resolution.  Point j is a closed-form function of its
//           edge (binary search in the prefix of the edges' step counts, held in LDS) and of its place on it, exactly as
//           rle._polygon_boundary steps it: the flip rule (dx == dy goes with dx > dy), t = n - d under flip, slope 0 on an edge of
//           no length, (int) by truncation.  The crossing between the points j - 1 and j passes the column-centre filter, its row
//           is clamped, and x * h + ceil(y) goes through a wave-ballot compaction into LDS.  Built with -ffp-contract=off: every
//           double operation is one IEEE operation, the divisions are true divisions.
//   sort    bitonic in LDS, all exchanges ascending, so that a range of any length sorts in place (the places past its end act as
//           +infinity and never move).  Position x lies inside a polygon exactly when an odd number of its crossings lie at or
//           before x: the crossing of rank r starts the polygon (r even) or ends it (r odd); equal positions cancel in pairs, which
//           is rleFrPoly's merging of what a zero-length run separates.  Crossings at h * w change no pixel and are not kept.
//   union   the events (position << 1 | end) of all polygons of the annotation are sorted once more, a scan gives the coverage after
//           each, and a run boundary lies wherever the coverage moves between 0 and positive across one position (equal positions
//           taken together).  The counts are the differences of the boundaries from 0 to h * w: rle._counts' canonical form.
//
// Every loop is bounded by a size the host packed (and the kernel checks again) or by the LDS capacity; an annotation outside them
// gets n_runs = -1 and is left to the host.
#include "common.h"

// ZH_POLYGON_LDS_CROSSINGS = 4096: 16 KB keys + 8 KB coverage + 16 KB boundaries, 3 workgroups a CU
#define PG_THREADS 256
#define PG_WAVES (PG_THREADS / 64)
#define PG_MAX_STEPS (1 << 22)          // points of one polygon's walk (zutis_amd/polygons.py MAX_STEPS)

// point d of the edge that starts at vertex e of a k-vertex polygon (the host keeps |scaled coordinate| <= 2^24, polygons.py MAX_COORD:
// every int32 expression here is exact)
__device__ __forceinline__ void pg_point(const int* xs, const int* ys, int k, int e, int d, int& u, int& v) {
  const int e1 = e + 1 == k ? 0 : e + 1;
  int x0 = xs[e], y0 = ys[e], x1 = xs[e1], y1 = ys[e1];
  const int dx = abs(x1 - x0), dy = abs(y0 - y1);
  const bool major = dx >= dy;
  const bool flip = major ? x0 > x1 : y0 > y1;
  if (flip) { int t = x0; x0 = x1; x1 = t; t = y0; y0 = y1; y1 = t; }
  if (major) {
    const double s = dx ? (double)(y1 - y0) / (double)dx : 0.0;
    const int t = flip ? dx - d : d;
    u = t + x0;
    v = (int)((double)y0 + s * (double)t + .5);
  } else {
    const double s = (double)(x1 - x0) / (double)dy;
    const int t = flip ? dy - d : d;
    v = t + y0;
    u = (int)((double)x0 + s * (double)t + .5);
  }
}

__device__ __forceinline__ void pg_exchange(unsigned* a, int i, int l, int n) {
  if (l < n) {
    const unsigned x = a[i], y = a[l];
    if (x > y) { a[i] = y; a[l] = x; }
  }
}

// a[0 .. n) ascending, by the whole workgroup (n is the same in every lane)
__device__ __forceinline__ void pg_sort(unsigned* a, int n, int tid) {
  int m = 1;
  while (m < n) m <<= 1;                                  // n <= ZH_POLYGON_LDS_CROSSINGS: at most 12 doublings
  for (int k = 2; k <= m; k <<= 1) {
    const int half = k >> 1;
    for (int t = tid; t < (m >> 1); t += PG_THREADS) {    // mirror exchange within blocks of k
      const int i = ((t / half) * k) + (t % half);
      pg_exchange(a, i, i ^ (k - 1), n);
    }
    __syncthreads();
    for (int j = half >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (m >> 1); t += PG_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        pg_exchange(a, i, i | j, n);
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(PG_THREADS) void polygon_runs_kernel(const int* xs, const int* ys, const int* step_pref, const int* vert_off,
                                                                  const int* poly_off, const int* hw, const int* flags,
                                                                  const int* out_off, int* counts, int* n_runs) {
  __shared__ unsigned s_key[ZH_POLYGON_LDS_CROSSINGS];
  __shared__ short s_cov[ZH_POLYGON_LDS_CROSSINGS];
  __shared__ int s_bnd[ZH_POLYGON_LDS_CROSSINGS];         // the walk's step prefix first (at most CROSSINGS / 2 edges), then the boundaries
  __shared__ int s_n, s_wsum[PG_WAVES];
  int* s_pref = s_bnd;
  const int a = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = hw[2 * a], w = hw[2 * a + 1];
  const long long HW = (long long)h * (long long)w;
  const int cap_out = out_off[a + 1] - out_off[a];
  const int p0 = poly_off[a], n_poly = poly_off[a + 1] - p0;
  int* out = counts + out_off[a];
  bool bad = flags[a] != 0 || h < 1 || w < 1 || HW > 0x7fffffffLL || cap_out < 1 || n_poly < 0;      // the same in every lane
  if (tid == 0) s_n = 0;
  __syncthreads();
  for (int p = 0; p < n_poly && !bad; ++p) {
    const int v0 = vert_off[p0 + p], k = vert_off[p0 + p + 1] - v0;
    const int base = s_n;
    if (k < 1 || k > ZH_POLYGON_LDS_CROSSINGS / 2 || base > ZH_POLYGON_LDS_CROSSINGS) { bad = true; break; }
    const int* pref = step_pref + v0 + (p0 + p);
    for (int i = tid; i <= k; i += PG_THREADS) s_pref[i] = pref[i];
    __syncthreads();
    const int N = s_pref[k];
    if (N < k || N > PG_MAX_STEPS) { bad = true; break; }
    const int* px = xs + v0;
    const int* py = ys + v0;
    for (int jb = 1 + wave * 64; jb < N; jb += PG_THREADS) {                 // the same trip count in every lane of a wave
      const int j = jb + lane;
      bool keep = false;
      unsigned pos = 0;
      if (j < N) {
        int lo = 0, hi = k;                                                   // the edge of point j: s_pref[lo] <= j < s_pref[lo + 1]
        for (int step = 0; step < 32 && hi - lo > 1; ++step) {
          const int mid = (lo + hi) >> 1;
          if (s_pref[mid] <= j) lo = mid; else hi = mid;
        }
        const int d = j - s_pref[lo];
        int u0, q0, u1, q1;
        pg_point(px, py, k, lo, d, u1, q1);
        if (d > 0) pg_point(px, py, k, lo, d - 1, u0, q0);
        else if (lo > 0) pg_point(px, py, k, lo - 1, s_pref[lo] - s_pref[lo - 1] - 1, u0, q0);   // the last point of the edge before
        else { u0 = u1; q0 = q1; }                                            // (j >= 1 lies past point 0 of edge 0: not reached)
        if (u1 != u0) {
          double xd = (double)(u1 < u0 ? u1 : u1 - 1);
          xd = (xd + .5) / 5.0 - .5;
          if (floor(xd) == xd && xd >= 0.0 && xd <= (double)(w - 1)) {
            double yd = (double)(q1 < q0 ? q1 : q0);
            yd = (yd + .5) / 5.0 - .5;
            yd = yd < 0.0 ? 0.0 : (yd > (double)h ? (double)h : yd);
            const long long at = (long long)(int)xd * (long long)h + (long long)(int)ceil(yd);
            keep = at < HW;                                                   // a crossing at h * w changes no pixel
            pos = (unsigned)at;
          }
        }
      }
      const unsigned long long m = __ballot(keep);
      if (m != 0ull) {
        int b = 0;
        if (lane == 0) b = atomicAdd(&s_n, __popcll(m));
        b = __shfl(b, 0, 64) + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && b < ZH_POLYGON_LDS_CROSSINGS) s_key[b] = pos;
      }
    }
    __syncthreads();
    const int end = s_n;
    if (end > ZH_POLYGON_LDS_CROSSINGS) { bad = true; break; }
    pg_sort(s_key + base, end - base, tid);
    __syncthreads();
    for (int i = base + tid; i < end; i += PG_THREADS) s_key[i] = (s_key[i] << 1) | (unsigned)((i - base) & 1);
    __syncthreads();
  }
  if (bad) {                                               // `bad` is the same in every lane: it comes from descriptors and from s_n behind a barrier
    if (tid == 0) n_runs[a] = -1;
    return;
  }
  const int n = s_n;
  if (n_poly > 1) pg_sort(s_key, n, tid);
  __syncthreads();
  // coverage after each event
  int carry = 0;
  for (int t0 = 0; t0 < n; t0 += PG_THREADS) {
    const int i = t0 + tid;
    int c = i < n ? ((s_key[i] & 1u) ? -1 : 1) : 0;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const int up = __shfl_up(c, s, 64);
      if (lane >= s) c += up;
    }
    if (lane == 63) s_wsum[wave] = c;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int q = 0; q < PG_WAVES; ++q) {
      const int t = s_wsum[q];
      if (q < wave) before += t;
      total += t;
    }
    if (i < n) s_cov[i] = (short)(carry + before + c);
    carry += total;
    __syncthreads();
  }
  // boundaries: the last event of a position, where the coverage before the position's first event and after its last differ in sign
  int nb = 0;
  for (int t0 = 0; t0 < n; t0 += PG_THREADS) {
    const int i = t0 + tid;
    bool isb = false;
    unsigned pos = 0;
    if (i < n) {
      pos = s_key[i] >> 1;
      if (i == n - 1 || (s_key[i + 1] >> 1) != pos) {
        int lo = 0, hi = i;                                // first event of this position: the first key >= pos << 1
        for (int step = 0; step < 32 && lo < hi; ++step) {
          const int mid = (lo + hi) >> 1;
          if ((s_key[mid] >> 1) < pos) lo = mid + 1; else hi = mid;
        }
        const int cov0 = lo > 0 ? (int)s_cov[lo - 1] : 0;
        isb = (cov0 > 0) != ((int)s_cov[i] > 0);
      }
    }
    const unsigned long long m = __ballot(isb);
    if (lane == 0) s_wsum[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int q = 0; q < PG_WAVES; ++q) {
      const int t = s_wsum[q];
      if (q < wave) before += t;
      total += t;
    }
    if (isb) s_bnd[nb + before + __popcll(m & ((1ull << lane) - 1ull))] = (int)pos;     // < n <= ZH_POLYGON_LDS_CROSSINGS
    nb += total;
    __syncthreads();
  }
  if (nb + 1 > cap_out) {                                  // the host's bound holds at least the crossings: not reached
    if (tid == 0) n_runs[a] = -1;
    return;
  }
  for (int r = tid; r <= nb; r += PG_THREADS) {
    const int from = r ? s_bnd[r - 1] : 0;
    const int to = r < nb ? s_bnd[r] : (int)HW;
    out[r] = to - from;
  }
  if (tid == 0) n_runs[a] = nb + 1;
}

extern "C" int zh_polygon_lds_crossings(void) { return ZH_POLYGON_LDS_CROSSINGS; }

extern "C" int zh_polygon_runs(const int* xs, const int* ys, const int* step_pref, const int* vert_off, const int* poly_off, const int* hw,
                               const int* flags, const int* out_off, int n_annotations, int* counts, int* n_runs, hipStream_t stream) {
  ZH_CHECK_ARG(n_annotations >= 0, "zh_polygon_runs: negative annotation count");
  if (n_annotations == 0) return ZH_OK;                    // no empty grid
  ZH_CHECK_ARG(xs && ys && step_pref && vert_off && poly_off && hw && flags && out_off && counts && n_runs, "zh_polygon_runs: null pointer");
  hipLaunchKernelGGL(polygon_runs_kernel, dim3(n_annotations), dim3(PG_THREADS), 0, stream, xs, ys, step_pref, vert_off, poly_off, hw,
                     flags, out_off, counts, n_runs);
  ZH_CHECK_LAUNCH("zh_polygon_runs");
  return ZH_OK;
}
