// dkm_ordered.hip -- the reference's own summation order (KMeans
// sums="reference"): per-Subset partial sums as one sequential chain per
// (Subset, cluster, column) in ascending row order (`partials[label] += row`,
// cluster/kmeans/base.py:166-181), and the arity tree that merges them
// (`_merge`, base.py:137-141, 184-191).  No floating-point atomic, and no
// result depends on the grid or the block size: two runs give the same bits.
//
// Grouping (a stable counting sort of the row indices by (Subset, label);
// rows are already in Subset order, so it is one stable sort by label inside
// every Subset):
//   k_ord_tiles    tiles of ORD_T rows that never cross a Subset boundary:
//                  first tile of every Subset (one block, a scan over S);
//   k_ord_hist     one wave per tile: LDS histogram of the k + 1 bins (bin k
//                  = labels outside [0, k): grouped last, never summed);
//   k_ord_scan     one block per Subset, a thread per bin: the tiles' counts
//                  become exclusive prefixes in tile order, the bins' totals
//                  the segment offsets and (as integers) the partial's counts;
//   k_ord_scatter  one wave per tile walks its rows 64 at a time in row
//                  order; equal labels rank by ballot / mbcnt (ascending
//                  lane = ascending row), so the order inside a segment is
//                  the row order.
// Chains:
//   k_ord_chain    G lanes per (segment, block of G columns): lane = column,
//                  so the lanes of a group read one row contiguously; the
//                  loads of ORD_U rows are issued together, the adds follow
//                  strictly in order from +0.0 (fp32 rows: fp32 adds, stored
//                  widened, which is exact).
//   k_merge_tree   one thread per element walks the host-built schedule.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "dkm_internal.h"

namespace dkm {

namespace {

constexpr int ORD_T = 2048;     // rows per grouping tile
constexpr int ORD_KMAX = 8191;  // k + 1 bins of 4 B in 32 KB of LDS
constexpr int ORD_U = 8;        // rows whose loads a chain issues together
constexpr int ORD_CB = 256;     // threads per k_ord_chain / k_ord_scan block

// Workspace carve-up (every part 256-B aligned).
struct OrdView {
  int32_t *sorted;  // [n]            row indices grouped by (Subset, label)
  int32_t *seg;     // [S (k + 1)]    first sorted position of (Subset, bin)
  int32_t *tile0;   // [S + 1]        first tile of every Subset
  int32_t *hist;    // [tiles (k+1)]  per-tile counts, then in-Subset prefixes
  int64_t max_tiles;
};

int64_t ord_max_tiles(int64_t n, int64_t S) { return n / ORD_T + S; }

size_t ord_bytes(int64_t n, int64_t S, int64_t k) {
  size_t b = 0;
  b += (size_t)round_up(std::max<int64_t>(n, 1) * 4, 256);
  b += (size_t)round_up(S * (k + 1) * 4, 256);
  b += (size_t)round_up((S + 1) * 4, 256);
  b += (size_t)round_up(ord_max_tiles(n, S) * (k + 1) * 4, 256);
  return b;
}

OrdView ord_view(void *ws, int64_t n, int64_t S, int64_t k) {
  OrdView v;
  char *p = (char *)ws;
  v.sorted = (int32_t *)p;
  p += round_up(std::max<int64_t>(n, 1) * 4, 256);
  v.seg = (int32_t *)p;
  p += round_up(S * (k + 1) * 4, 256);
  v.tile0 = (int32_t *)p;
  p += round_up((S + 1) * 4, 256);
  v.hist = (int32_t *)p;
  v.max_tiles = ord_max_tiles(n, S);
  return v;
}

bool ord_shape_ok(int64_t n, int64_t S, int64_t k, int64_t d) {
  return n >= 0 && n < INT32_MAX && S >= 1 && k >= 1 && k <= ORD_KMAX &&
         d >= 1 && d < INT32_MAX && S * (k + 1) < INT32_MAX &&
         ord_max_tiles(n, S) < INT32_MAX;
}

// Rows [lo, hi) of Subset s, clamped to [0, n] (offsets that are not the
// ascending 0 .. n the contract asks for never index outside the arrays).
__device__ __forceinline__ void subset_rows(const int64_t *off, int64_t s,
                                            int64_t n, int64_t *lo,
                                            int64_t *hi) {
  const int64_t a = off[s], b = off[s + 1];
  *lo = a < 0 ? 0 : (a > n ? n : a);
  *hi = b < *lo ? *lo : (b > n ? n : b);
}

// Subset of tile t: tile0[s] <= t < tile0[s + 1].
__device__ __forceinline__ int tile_subset(const int32_t *tile0, int S,
                                           int t) {
  int lo = 0, hi = S;  // tile0[lo] <= t < tile0[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile0[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int bin_of(int32_t lab, int k) {
  return (unsigned)lab < (unsigned)k ? lab : k;
}

}  // namespace

// tile0[s] = tiles of the Subsets before s (exclusive scan, one block).
__global__ void __launch_bounds__(1024)
    k_ord_tiles(const int64_t *__restrict__ off, int S, int64_t n,
                int32_t *__restrict__ tile0, int64_t max_tiles) {
  __shared__ int64_t part[1024];
  const int per = (S + 1023) / 1024;
  const int s0 = min(S, (int)threadIdx.x * per), s1 = min(S, s0 + per);
  int64_t sum = 0;
  for (int s = s0; s < s1; ++s) {
    int64_t lo, hi;
    subset_rows(off, s, n, &lo, &hi);
    sum += (hi - lo + ORD_T - 1) / ORD_T;
  }
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int st = 1; st < 1024; st <<= 1) {  // Hillis-Steele inclusive scan
    const int64_t v = (int)threadIdx.x >= st ? part[threadIdx.x - st] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int64_t run = part[threadIdx.x] - sum;
  for (int s = s0; s < s1; ++s) {
    int64_t lo, hi;
    subset_rows(off, s, n, &lo, &hi);
    tile0[s] = (int32_t)min(run, max_tiles);
    run += (hi - lo + ORD_T - 1) / ORD_T;
  }
  if (threadIdx.x == 1023) tile0[S] = (int32_t)min(part[1023], max_tiles);
}

// Per-tile histogram of the k + 1 bins (one wave per tile).
__global__ void __launch_bounds__(64)
    k_ord_hist(const int32_t *__restrict__ lab,
               const int64_t *__restrict__ off, int S, int64_t n, int k,
               const int32_t *__restrict__ tile0, int32_t *__restrict__ hist) {
  extern __shared__ int bins[];
  const int t = blockIdx.x;
  if (t >= tile0[S]) return;
  const int s = tile_subset(tile0, S, t);
  int64_t lo, hi;
  subset_rows(off, s, n, &lo, &hi);
  const int64_t r0 = lo + (int64_t)(t - tile0[s]) * ORD_T;
  const int64_t r1 = min(hi, r0 + ORD_T);
  for (int c = threadIdx.x; c <= k; c += 64) bins[c] = 0;
  __syncthreads();
  for (int64_t r = r0 + threadIdx.x; r < r1; r += 64)
    atomicAdd(&bins[bin_of(lab[r], k)], 1);
  __syncthreads();
  int32_t *h = hist + (int64_t)t * (k + 1);
  for (int c = threadIdx.x; c <= k; c += 64) h[c] = bins[c];
}

// Per Subset: the tiles' counts of every bin -> exclusive prefixes in tile
// order; the bins' totals -> segment offsets (seg) and the partial's counts.
__global__ void __launch_bounds__(ORD_CB)
    k_ord_scan(const int64_t *__restrict__ off, int S, int64_t n, int k,
               int64_t d, const int32_t *__restrict__ tile0,
               int32_t *__restrict__ hist, int32_t *__restrict__ seg,
               double *__restrict__ partials) {
  extern __shared__ int tot[];  // [k + 1] totals, then their exclusive scan
  __shared__ int part[ORD_CB];
  const int64_t len = (int64_t)k * (d + 1);
  for (int s = blockIdx.x; s < S; s += gridDim.x) {
    int64_t lo, hi;
    subset_rows(off, s, n, &lo, &hi);
    const int t0 = tile0[s], t1 = tile0[s + 1];
    __syncthreads();
    for (int c = threadIdx.x; c <= k; c += ORD_CB) {
      int run = 0;
      for (int t = t0; t < t1; t += 8) {  // 8 tiles' loads issued together
        int32_t *h = hist + (int64_t)t * (k + 1) + c;
        int v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          v[u] = t + u < t1 ? h[(int64_t)u * (k + 1)] : 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (t + u < t1) h[(int64_t)u * (k + 1)] = run;
          run += v[u];
        }
      }
      tot[c] = run;
      if (c < k) partials[(int64_t)s * len + (int64_t)k * d + c] = (double)run;
    }
    __syncthreads();
    const int per = (k + 1 + ORD_CB - 1) / ORD_CB;
    const int c0 = min(k + 1, (int)threadIdx.x * per);
    const int c1 = min(k + 1, c0 + per);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += tot[c];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int st = 1; st < ORD_CB; st <<= 1) {
      const int v = (int)threadIdx.x >= st ? part[threadIdx.x - st] : 0;
      __syncthreads();
      part[threadIdx.x] += v;
      __syncthreads();
    }
    int run = (int)lo + part[threadIdx.x] - sum;
    for (int c = c0; c < c1; ++c) {
      seg[(int64_t)s * (k + 1) + c] = run;
      run += tot[c];
    }
  }
}

// Stable scatter of a tile's rows to their segments (one wave per tile).
__global__ void __launch_bounds__(64)
    k_ord_scatter(const int32_t *__restrict__ lab,
                  const int64_t *__restrict__ off, int S, int64_t n, int k,
                  const int32_t *__restrict__ tile0,
                  const int32_t *__restrict__ hist,
                  const int32_t *__restrict__ seg,
                  int32_t *__restrict__ sorted) {
  extern __shared__ int cur[];  // [k + 1] next position of every bin
  const int t = blockIdx.x;
  if (t >= tile0[S]) return;
  const int s = tile_subset(tile0, S, t);
  int64_t lo, hi;
  subset_rows(off, s, n, &lo, &hi);
  const int64_t r0 = lo + (int64_t)(t - tile0[s]) * ORD_T;
  const int64_t r1 = min(hi, r0 + ORD_T);
  const int32_t *h = hist + (int64_t)t * (k + 1);
  const int32_t *sg = seg + (int64_t)s * (k + 1);
  for (int c = threadIdx.x; c <= k; c += 64) cur[c] = sg[c] + h[c];
  const int lane = threadIdx.x;
  for (int64_t q = r0; q < r1; q += 64) {
    __syncthreads();  // the previous 64 rows' positions are taken
    const int64_t r = q + lane;
    const bool valid = r < r1;
    const int c = valid ? bin_of(lab[r], k) : -1;
    uint64_t todo = __ballot(valid);
    while (todo) {  // wave-uniform: one pass per distinct bin of these rows
      const int leader = __ffsll((unsigned long long)todo) - 1;
      const int lc = __shfl(c, leader);
      const bool mine = c == lc;
      const uint64_t m = __ballot(mine);
      const int base = cur[lc];
      if (mine) {
        const int rank = __builtin_amdgcn_mbcnt_hi(
            (uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
        const int64_t pos = (int64_t)base + rank;
        if (pos >= 0 && pos < n) sorted[pos] = (int32_t)r;
        // every bin is met once per 64 rows: no other pass reads cur[lc]
        // before the barrier above
        if (lane == leader) cur[lc] = base + __popcll(m);
      }
      todo &= ~m;
    }
  }
}

// One sequential chain per (Subset, cluster, column), ascending row order.
template <class TX, int G>
__global__ void __launch_bounds__(ORD_CB)
    k_ord_chain(const TX *__restrict__ X, int64_t n, int64_t ldx, int d,
                int k, int S,
                const int32_t *__restrict__ sorted,
                const int32_t *__restrict__ seg,
                double *__restrict__ partials) {
  constexpr int GPB = ORD_CB / G;  // groups per block
  const int gl = threadIdx.x % G;
  const int64_t ncb = (d + G - 1) / G;
  const int64_t items = (int64_t)S * k * ncb;
  const int64_t len = (int64_t)k * (d + 1);
  for (int64_t it = (int64_t)blockIdx.x * GPB + threadIdx.x / G; it < items;
       it += (int64_t)gridDim.x * GPB) {
    const int64_t cb = it % ncb, sc = it / ncb;
    const int64_t c = sc % k, s = sc / k;
    const int32_t *sg = seg + s * (k + 1) + c;
    const int64_t a = sg[0], b = sg[1];
    const int t = (int)(cb * G) + gl;
    const int tc = t < d ? t : d - 1;
    TX acc = (TX)0;  // +0.0: the reference's integer 0 placeholder
    for (int64_t q = a; q < b; q += ORD_U) {
      TX x[ORD_U];
      // unconditional loads from clamped positions (see k_seg_sums): the
      // values past the segment are never added
#pragma unroll
      for (int u = 0; u < ORD_U; ++u) {
        const int64_t pos = q + u < b ? q + u : b - 1;
        const int64_t row = sorted[pos];
        x[u] = X[(row >= 0 && row < n ? row : 0) * ldx + tc];
      }
#pragma unroll
      for (int u = 0; u < ORD_U; ++u)
        if (q + u < b) acc = acc + x[u];
    }
    if (t < d) partials[s * len + c * d + t] = (double)acc;
  }
}

// The arity tree: every thread folds its element through the schedule.
// Operand i < n_partials is partials[i], else scratch slot i - n_partials;
// an op is [dst, count, src_0 .. src_{count-1}], dst < 0 = acc.
__global__ void __launch_bounds__(256)
    k_merge_tree(const double *__restrict__ partials, int64_t n_partials,
                 int64_t len, const int32_t *__restrict__ sched, int n_ops,
                 int64_t n_f32, double *scratch, double *__restrict__ acc) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= len) return;
  if (n_ops == 0) {
    acc[e] = partials[e];
    return;
  }
  auto at = [&](int i) -> double {
    return i < n_partials ? partials[(int64_t)i * len + e]
                          : scratch[((int64_t)i - n_partials) * len + e];
  };
  const int32_t *p = sched;
  const bool f32 = e < n_f32;
  for (int op = 0; op < n_ops; ++op) {
    const int dst = p[0], cnt = p[1];
    double r;
    if (f32) {
      float a = (float)at(p[2]);
      for (int j = 1; j < cnt; ++j) a = a + (float)at(p[2 + j]);
      r = (double)a;
    } else {
      double a = at(p[2]);
      for (int j = 1; j < cnt; ++j) a = a + at(p[2 + j]);
      r = a;
    }
    (dst < 0 ? acc : scratch + (int64_t)dst * len)[e] = r;
    p += 2 + cnt;
  }
}

template <class TX>
static int ordered_sums(const TX *X, int64_t n, int64_t d, int64_t ldx,
                        const int32_t *labels, int64_t k,
                        const int64_t *subset_off, int64_t S, void *ws,
                        size_t ws_b, double *partials, hipStream_t s) {
  if (!subset_off || !partials || !ws || !ord_shape_ok(n, S, k, d) ||
      (n > 0 && (!X || !labels || ldx < d)))
    return fail(DKM_E_ARG, "ordered sums: bad arguments");
  if (ws_b < ord_bytes(n, S, k))
    return fail(DKM_E_WORKSPACE, "ordered sums: workspace too small");
  const OrdView v = ord_view(ws, n, S, k);
  const size_t lds = (size_t)(k + 1) * 4;
  const unsigned tiles = (unsigned)std::max<int64_t>(1, v.max_tiles);
  k_ord_tiles<<<1, 1024, 0, s>>>(subset_off, (int)S, n, v.tile0, v.max_tiles);
  k_ord_hist<<<tiles, 64, lds, s>>>(labels, subset_off, (int)S, n, (int)k,
                                    v.tile0, v.hist);
  k_ord_scan<<<(unsigned)std::min<int64_t>(S, 65535), ORD_CB, lds, s>>>(
      subset_off, (int)S, n, (int)k, d, v.tile0, v.hist, v.seg, partials);
  k_ord_scatter<<<tiles, 64, lds, s>>>(labels, subset_off, (int)S, n, (int)k,
                                       v.tile0, v.hist, v.seg, v.sorted);
  if (int r = check_launch("ordered sums: grouping")) return r;
#define DKM_ORD(GG)                                                          \
  {                                                                          \
    const int64_t items = S * k * ((d + GG - 1) / GG);                       \
    const int64_t g = std::max<int64_t>(                                     \
        1, std::min<int64_t>((items + ORD_CB / GG - 1) / (ORD_CB / GG),      \
                             1 << 20));                                      \
    k_ord_chain<TX, GG><<<(unsigned)g, ORD_CB, 0, s>>>(                      \
        X, n, ldx, (int)d, (int)k, (int)S, v.sorted, v.seg, partials);          \
  }
  if (d <= 8) DKM_ORD(8)
  else if (d <= 16) DKM_ORD(16)
  else if (d <= 32) DKM_ORD(32)
  else DKM_ORD(64)
#undef DKM_ORD
  return check_launch("ordered sums: chains");
}

}  // namespace dkm

using namespace dkm;

extern "C" {

size_t dkm_ordered_workspace_bytes(int64_t n, int64_t n_subsets, int64_t k,
                                   int64_t d) {
  if (!ord_shape_ok(n, n_subsets, k, d)) return 0;
  return ord_bytes(n, n_subsets, k);
}

int dkm_ordered_sums_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                         const int32_t *labels, int64_t k,
                         const int64_t *subset_off, int64_t n_subsets,
                         void *ws, size_t ws_bytes, double *partials,
                         void *stream) {
  return ordered_sums<double>(X, n, d, ldx, labels, k, subset_off, n_subsets,
                              ws, ws_bytes, partials, (hipStream_t)stream);
}

int dkm_ordered_sums_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                         const int32_t *labels, int64_t k,
                         const int64_t *subset_off, int64_t n_subsets,
                         void *ws, size_t ws_bytes, double *partials,
                         void *stream) {
  return ordered_sums<float>(X, n, d, ldx, labels, k, subset_off, n_subsets,
                             ws, ws_bytes, partials, (hipStream_t)stream);
}

int dkm_merge_tree(const double *partials, int64_t n_partials, int64_t len,
                   const int32_t *schedule, int64_t n_ops, int64_t sums_f32,
                   double *scratch, double *acc, void *stream) {
  if (!partials || !acc || n_partials < 1 || n_partials >= INT32_MAX ||
      len < 1 || n_ops < 0 || n_ops >= INT32_MAX || sums_f32 < 0 ||
      sums_f32 > len || (n_ops > 0 && !schedule) ||
      (n_ops == 0 && n_partials != 1))
    return fail(DKM_E_ARG, "merge tree: bad arguments");
  k_merge_tree<<<(unsigned)((len + 255) / 256), 256, 0,
                 (hipStream_t)stream>>>(partials, n_partials, len, schedule,
                                        (int)n_ops, sums_f32, scratch, acc);
  return check_launch("dkm_merge_tree");
}

}  // extern "C"

// Code-object preload (dkm_preload): the runtime loads this file's kernels
// on first use of any of them; an attribute query here does it up front.
namespace dkm {
DKM_TU_FLAGS(ordered, 0)
__global__ void k_tu_ordered() {}
int preload_ordered() {
  hipFuncAttributes a;
  const bool ok =
      hipFuncGetAttributes(&a, (const void *)k_tu_ordered) == hipSuccess;
  return ok ? 0 : 1;
}
}  // namespace dkm
