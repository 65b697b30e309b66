// dkm_dbscan.hip -- the graph half of DBSCAN on the epsilon query's distance
// arithmetic: core points, connected components of the core
// points, border points, labels.  Reference: _compute_labels of
// cluster/dbscan/classes.py:162-191 on the lists of _compute_neighbours
// (:124-141), with one region.
//
// No neighbour list and no n x n object exists: every pass recomputes the
// distances.  Rows arrive ordered by grid cell (the caller's stable sort;
// orig_index[i] = the Dataset row of ordered row i), so 64 consecutive rows
// -- a tile -- lie close together and a tile pair whose bounding boxes are
// further apart than eps is skipped.
//
//   k_db_box      wave per tile: the bounding box of its rows over the first
//                 min(d, DB_BD) features.
//   k_db_pair<MAXD, 0>  lane = query row (in VGPRs for d <= 64), wave-uniform
//                 fit row read by scalar loads, fit tiles partitioned over
//                 blockIdx.y: the shape of k_radius.  64 fit tiles are tested
//                 against the query tile's box at once (lane = fit tile, one
//                 ballot), the survivors scanned.  Counts neighbours.
//   k_db_core     core[i] = count[i] >= min_samples.
//   k_db_pair<MAXD, 1>  the same loop over the core fit rows only.  A core
//                 query unions itself with every core neighbour before it
//                 (each pair is seen from both ends); a non-core query keeps
//                 the smallest (distance, original index) core neighbour of
//                 its partition.
//   k_db_attach   a non-core row's partitions merged: attach[i] = that core
//                 row, or -1.
//   k_db_comp / k_db_stats / k_db_survive / k_db_scan / k_db_labels
//                 (dkm_dbscan_finalize) roots, border rows attached, size and
//                 smallest original index per component, components below
//                 min_samples dropped, survivors ranked by smallest index.
//
// Union-find: parent[i] <= i always (a root is hooked under a smaller root,
// path halving writes a grandparent), and every value parent[i] ever held is
// an ancestor of i from then on.  Non-core rows never enter it: a border row
// within eps of two clusters must not bridge them.
#include "dkm_internal.h"

#include <algorithm>
#include <cmath>

namespace dkm {

namespace {

constexpr int NB = 256;    // threads per block (4 waves)
constexpr int DB_BD = 16;  // features of a tile's bounding box
// the link pass's per-partition (distance, row) of the non-core rows
constexpr size_t DB_PART_BYTES = 768u << 10;
typedef const __attribute__((address_space(4))) double cdouble;
typedef const __attribute__((address_space(4))) int cint;

// A coherent read of the forest: bypasses the per-CU cache, so a thread sees
// every hook that an atomic already made (a stale root would make its CAS
// fail again and again).
__device__ __forceinline__ int uf_load(int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x, halving the path behind it.
__device__ __forceinline__ int uf_find(int *parent, int x) {
  // Ends: p < x whenever x is not a root, so x strictly decreases; it is
  // bounded below by 0.  No read waits for another thread.
  for (;;) {
    const int p = uf_load(parent + x);
    if (p == x) return x;
    const int gp = uf_load(parent + p);
    // gp <= p < x is an ancestor of x; atomicMin keeps parent[x] decreasing
    // whatever other threads write meanwhile
    if (gp != p) atomicMin(parent + x, gp);
    x = p;
  }
}

// One component for a and b: the larger root goes under the smaller.
__device__ __forceinline__ void uf_union(int *parent, int a, int b) {
  // Ends: a failed CAS means another thread hooked `hi` under a smaller row
  // (progress elsewhere); this thread goes on from that row, `old` < hi, and
  // from lo < hi, so max(a, b) strictly decreases from one round to the
  // next: at most n rounds, none of them waiting for anybody.
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    a = old;
    b = lo;
  }
}

__global__ void __launch_bounds__(NB)
    k_db_box(const double *__restrict__ X, int n, int64_t ldx, int bd, int T,
             double *__restrict__ box) {
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * (NB / 64) + (threadIdx.x >> 6);
  if (tile >= T) return;  // wave-uniform
  const int64_t i = (int64_t)tile * 64 + lane;
  const bool live = i < n;
  for (int t = 0; t < bd; ++t) {
    double lo = live ? X[i * ldx + t] : INFINITY;
    double hi = live ? lo : -INFINITY;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      lo = fmin(lo, __shfl_xor(lo, off, WAVE));
      hi = fmax(hi, __shfl_xor(hi, off, WAVE));
    }
    if (lane == 0) {
      box[(int64_t)tile * 2 * DB_BD + t] = lo;
      box[(int64_t)tile * 2 * DB_BD + DB_BD + t] = hi;
    }
  }
}

// MODE 0: cnt[q] += neighbours of q in this partition.
// MODE 1: unions of the core rows; (pdist, pidx)[p][q] of the non-core rows.
template <int MAXD, int MODE>
__global__ void __launch_bounds__(NB)
    k_db_pair(const double *__restrict__ X, int n, int64_t ldx, int d,
              double eps, int bd, const double *__restrict__ box, int T,
              int tpp, int noprune, unsigned *__restrict__ cnt,
              const int *__restrict__ core, const int *__restrict__ orig,
              int *__restrict__ parent, double *__restrict__ pdist,
              int *__restrict__ pidx, int npad) {
  const int lane = threadIdx.x & 63;
  const int tq = blockIdx.x * (NB / 64) +
                 __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = blockIdx.y;
  if (tq >= T) return;  // wave-uniform
  const int q = tq * 64 + lane;  // < npad <= INT32_MAX
  const bool live = q < n;
  const double *qrow = X + (int64_t)(live ? q : 0) * ldx;
  double qv[MAXD > 0 ? MAXD : 8];
  if constexpr (MAXD > 0) {
#pragma unroll
    for (int t = 0; t < MAXD; ++t) qv[t] = t < d ? qrow[t] : 0.0;
  }
  cdouble *xc = (cdouble *)X;
  cdouble *bq = (cdouble *)box + (int64_t)tq * 2 * DB_BD;
  cint *corec = (cint *)core;
  cint *origc = (cint *)orig;
  const double e2 = eps * eps;
  // the epsilon predicate of k_radius (dkm_neighbors.hip): eps <= 0 takes
  // nothing; r clear of eps^2 by a relative 2^-48 is decided on r, the band
  // between by the reference's sqrt and compare
  const double e2lo = eps > 0 ? e2 * (1.0 - 0x1.0p-48) : -1.0;
  const double e2hi = eps > 0 ? e2 * (1.0 + 0x1.0p-48) : -1.0;
  // a tile pair is skipped when the squared gap of its boxes is above this:
  // the gap bounds every distance of the pair from below, and 2^-40 is far
  // above the rounding of the gap and of r (eps <= 0: every pair)
  const double lim = eps > 0 ? e2 * (1.0 + 0x1.0p-40) : -1.0;
  unsigned mine = 0;
  const bool mycore = (MODE == 1 && live) ? core[q] != 0 : false;
  double bdist = INFINITY;
  int borig = INT32_MAX, bj = -1;
  const int t0 = p * tpp;
  const int t1 = std::min(T, t0 + tpp);
  // Ends: tb advances by 64 up to t1.
  for (int tb = t0; tb < t1; tb += 64) {
    const int tf = tb + lane;
    bool hit = tf < t1;
    if (hit && !noprune) {
      const double *bf = box + (int64_t)tf * 2 * DB_BD;
      double gap2 = 0.0;
      for (int t = 0; t < bd; ++t) {
        const double g = fmax(fmax(bf[t] - bq[DB_BD + t], bq[t] - bf[DB_BD + t]),
                              0.0);
        gap2 = gap2 + g * g;
      }
      hit = !(gap2 > lim);
    }
    unsigned long long m = __ballot(hit);
    // Ends: every round clears the lowest set bit of m (wave-uniform).
    while (m) {
      const int b = __builtin_ctzll(m);
      m &= m - 1;
      const int j0 = (tb + b) * 64;
      const int j1 = std::min(n, j0 + 64);
      for (int j = j0; j < j1; ++j) {
        if constexpr (MODE == 1) {
          if (!corec[j]) continue;  // wave-uniform: only core rows link
        }
        double r;
        if constexpr (MAXD > 0)
          r = exact_sqdist_reg<MAXD>(qv, xc + (int64_t)j * ldx, d);
        else
          r = pw_sum(SqDiff<double>{qrow, X + (int64_t)j * ldx}, d);
        const bool in = r < e2lo || (r <= e2hi && sqrt(r) < eps);
        if (live && in) {
          if constexpr (MODE == 0) {
            ++mine;
          } else {
            if (mycore) {
              if (j < q) uf_union(parent, q, j);
            } else {
              const double dist = sqrt(r);
              const int oj = origc[j];
              if (dist < bdist || (dist == bdist && oj < borig)) {
                bdist = dist;
                borig = oj;
                bj = j;
              }
            }
          }
        }
      }
    }
  }
  if constexpr (MODE == 0) {
    if (live && mine) atomicAdd(cnt + q, mine);
  } else {
    if (live && !mycore) {
      pdist[(int64_t)p * npad + q] = bdist;
      pidx[(int64_t)p * npad + q] = bj;
    }
  }
}

__global__ void __launch_bounds__(NB)
    k_db_core(const unsigned *__restrict__ cnt, int n, unsigned min_samples,
              int *__restrict__ core) {
  const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
  if (i < n) core[i] = cnt[i] >= min_samples ? 1 : 0;
}

__global__ void __launch_bounds__(NB)
    k_db_init(int n, int *__restrict__ parent) {
  const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
  if (i < n) parent[i] = (int)i;
}

__global__ void __launch_bounds__(NB)
    k_db_attach(const int *__restrict__ core, const int *__restrict__ orig,
                const double *__restrict__ pdist,
                const int *__restrict__ pidx, int n, int npad, int P,
                int *__restrict__ attach) {
  const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
  if (i >= n) return;
  if (core[i]) {
    attach[i] = -1;
    return;
  }
  double bdist = INFINITY;
  int borig = INT32_MAX, bj = -1;
  for (int p = 0; p < P; ++p) {
    const int j = pidx[(int64_t)p * npad + i];
    if (j < 0) continue;
    const double dist = pdist[(int64_t)p * npad + i];
    const int oj = orig[j];
    if (dist < bdist || (dist == bdist && oj < borig)) {
      bdist = dist;
      borig = oj;
      bj = j;
    }
  }
  attach[i] = bj;
}

// comp[i] = the row that names i's component: a core row's root, a border
// row's core neighbour's root, a lone non-core row itself (it is nobody's
// root: only core rows are hooked).  The forest is final here, and only
// path halving writes it.
__global__ void __launch_bounds__(NB)
    k_db_comp(const int *__restrict__ core, const int *__restrict__ attach,
              int *__restrict__ parent, int n, int *__restrict__ comp,
              int *__restrict__ minidx, int *__restrict__ size,
              int *__restrict__ surv) {
  const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
  if (i >= n) return;
  int c = (int)i;
  if (core[i])
    c = uf_find(parent, (int)i);
  else if (attach[i] >= 0)
    c = uf_find(parent, attach[i]);
  comp[i] = c;
  minidx[i] = INT32_MAX;
  size[i] = 0;
  surv[i] = 0;
}

__global__ void __launch_bounds__(NB)
    k_db_stats(const int *__restrict__ comp, const int *__restrict__ orig,
               int n, int *__restrict__ minidx, int *__restrict__ size) {
  const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
  if (i >= n) return;
  const int c = comp[i];
  atomicMin(minidx + c, orig[i]);
  atomicAdd(size + c, 1);
}

// surv[o] = 1 where original row o is the smallest row of a component that
// stays (size >= min_samples).
__global__ void __launch_bounds__(NB)
    k_db_survive(const int *__restrict__ comp,
                 const int *__restrict__ minidx,
                 const int *__restrict__ size, int n, unsigned min_samples,
                 int *__restrict__ surv) {
  const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
  if (i >= n) return;
  // (orig_index is a permutation of 0 .. n - 1; anything else is dropped
  // here instead of written out of bounds)
  if (comp[i] == (int)i && (unsigned)size[i] >= min_samples &&
      (unsigned)minidx[i] < (unsigned)n)
    surv[minidx[i]] = 1;
}

// One block: surv <- its exclusive prefix sum (the rank of every surviving
// component by smallest row), *n_clusters <- the total.
constexpr int SCAN_B = 1024;
__global__ void __launch_bounds__(SCAN_B)
    k_db_scan(int *__restrict__ surv, int n, int *__restrict__ n_clusters) {
  __shared__ int wsum[SCAN_B / 64];
  __shared__ int carry_s;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  // Ends: c0 advances by SCAN_B up to n (block-uniform).
  for (int64_t c0 = 0; c0 < n; c0 += SCAN_B) {
    const int64_t i = c0 + threadIdx.x;
    const int v = i < n ? surv[i] : 0;
    int s = v;  // inclusive scan within the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(s, off, WAVE);
      if (lane >= off) s += o;
    }
    if (lane == 63) wsum[w] = s;
    __syncthreads();
    int before = carry_s;
    for (int u = 0; u < w; ++u) before += wsum[u];
    if (i < n) surv[i] = before + s - v;
    __syncthreads();
    if (threadIdx.x == SCAN_B - 1) carry_s = before + s;
    __syncthreads();
  }
  if (threadIdx.x == 0) *n_clusters = carry_s;
}

__global__ void __launch_bounds__(NB)
    k_db_labels(const int *__restrict__ comp, const int *__restrict__ orig,
                const int *__restrict__ minidx, const int *__restrict__ size,
                const int *__restrict__ rank, int n, unsigned min_samples,
                int32_t *__restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
  if (i >= n) return;
  const int c = comp[i], o = orig[i], mi = minidx[c];
  if ((unsigned)o >= (unsigned)n || (unsigned)mi >= (unsigned)n) return;
  labels[o] = (unsigned)size[c] >= min_samples ? rank[mi] : -1;
}

int maxd_of(int64_t d) {
  return d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : d <= 64 ? 64 : 0;
}

// Query tiles x P partitions of `tpp` fit tiles: about 4096 waves, no
// partition below 4 tiles, and the link pass's P x npad partials within
// DB_PART_BYTES (P = 1 from 49152 rows on, where the query tiles alone
// approach a thousand waves).
void db_grid(int64_t n, int *T, int *tpp, int *P) {
  const int64_t tiles = (n + 63) / 64;
  int64_t p = std::max<int64_t>(1, (4096 + tiles - 1) / tiles);
  p = std::min<int64_t>(p, std::max<int64_t>(1, tiles / 4));
  p = std::min<int64_t>(
      p, std::max<int64_t>(1, (int64_t)(DB_PART_BYTES / 12) / (tiles * 64)));
  const int64_t per = (tiles + p - 1) / p;
  *T = (int)tiles;
  *tpp = (int)per;
  *P = (int)((tiles + per - 1) / per);
}

struct DbWs {
  double *box;      // T x 2 x DB_BD
  unsigned *cnt;    // npad neighbour counts; then comp (finalize)
  int *minidx, *size, *surv;  // npad each
  double *pdist;    // P x npad
  int *pidx;        // P x npad
};

size_t db_layout(int64_t n, char *base, DbWs *w) {
  int T, tpp, P;
  db_grid(std::max<int64_t>(n, 1), &T, &tpp, &P);
  const size_t npad = (size_t)T * 64;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += (bytes + 255) & ~(size_t)255;
    return base ? base + at : nullptr;
  };
  char *a = take((size_t)T * 2 * DB_BD * 8), *b = take(npad * 4),
       *c = take(npad * 4), *d = take(npad * 4), *e = take(npad * 4),
       *f = take((size_t)P * npad * 8), *g = take((size_t)P * npad * 4);
  if (w) *w = DbWs{(double *)a, (unsigned *)b, (int *)c, (int *)d, (int *)e,
                   (double *)f, (int *)g};
  return o;
}

int db_args(const char *who, const double *X, int64_t n, int64_t d,
            int64_t ldx, double eps, int64_t min_samples, const void *ws,
            size_t ws_bytes) {
  if (n < 0 || d < 1 || ldx < d || n > INT32_MAX - 64 || d > INT32_MAX)
    return fail(DKM_E_ARG, std::string(who) + ": bad n/d/ld");
  if (std::isnan(eps)) return fail(DKM_E_ARG, std::string(who) + ": eps is NaN");
  if (min_samples < 0)
    return fail(DKM_E_ARG, std::string(who) + ": min_samples < 0");
  if (n > 0 && !X) return fail(DKM_E_ARG, std::string(who) + ": NULL X");
  if (n > 0 && (!ws || ws_bytes < dkm_dbscan_workspace_bytes(n, d)))
    return fail(DKM_E_WORKSPACE, std::string(who) + ": workspace smaller than "
                                 "dkm_dbscan_workspace_bytes()");
  return 0;
}

unsigned clamp_min_samples(int64_t ms) {
  return (unsigned)std::min<int64_t>(std::max<int64_t>(ms, 0), INT32_MAX);
}

template <int MODE>
int db_pair(const double *X, int n, int64_t ldx, int d, double eps,
            int noprune, const DbWs &w, const int *core, const int *orig,
            int *parent, hipStream_t s) {
  int T, tpp, P;
  db_grid(n, &T, &tpp, &P);
  const int bd = std::min(d, DB_BD), npad = T * 64;
  const dim3 g((unsigned)((T + 3) / 4), (unsigned)P);
#define DB_LAUNCH(M)                                                          \
  k_db_pair<M, MODE><<<g, NB, 0, s>>>(X, n, ldx, d, eps, bd, w.box, T, tpp,   \
                                      noprune, w.cnt, core, orig, parent,     \
                                      w.pdist, w.pidx, npad)
  switch (maxd_of(d)) {
    case 8: DB_LAUNCH(8); break;
    case 16: DB_LAUNCH(16); break;
    case 32: DB_LAUNCH(32); break;
    case 64: DB_LAUNCH(64); break;
    default: DB_LAUNCH(0); break;
  }
#undef DB_LAUNCH
  return check_launch(MODE == 0 ? "dbscan core pass" : "dbscan link pass");
}

int db_boxes(const double *X, int n, int64_t ldx, int d, const DbWs &w,
             hipStream_t s) {
  const int T = (n + 63) / 64;
  k_db_box<<<(unsigned)((T + 3) / 4), NB, 0, s>>>(X, n, ldx,
                                                   std::min(d, DB_BD), T,
                                                   w.box);
  return check_launch("dbscan boxes");
}

unsigned row_blocks(int64_t n) { return (unsigned)((n + NB - 1) / NB); }

}  // namespace
}  // namespace dkm

using namespace dkm;

extern "C" {

size_t dkm_dbscan_workspace_bytes(int64_t n, int64_t d) {
  if (n < 0 || d < 1 || n > INT32_MAX - 64) return 0;
  return db_layout(n, nullptr, nullptr);
}

int dkm_dbscan_core_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                        double eps, int64_t min_samples, int flags, void *ws,
                        size_t ws_bytes, int32_t *core_out, void *stream) {
  if (int r = db_args("dbscan core", X, n, d, ldx, eps, min_samples, ws,
                      ws_bytes))
    return r;
  if (n == 0) return 0;
  if (!core_out) return fail(DKM_E_ARG, "dbscan core: NULL core_out");
  hipStream_t s = (hipStream_t)stream;
  DbWs w;
  db_layout(n, (char *)ws, &w);
  if (hipMemsetAsync(w.cnt, 0, (size_t)n * 4, s) != hipSuccess)
    return fail(DKM_E_LAUNCH, "dbscan core: memset");
  if (int r = db_boxes(X, (int)n, ldx, (int)d, w, s)) return r;
  if (int r = db_pair<0>(X, (int)n, ldx, (int)d, eps,
                         flags & DKM_DBSCAN_NOPRUNE ? 1 : 0, w, nullptr,
                         nullptr, nullptr, s))
    return r;
  k_db_core<<<row_blocks(n), NB, 0, s>>>(w.cnt, (int)n,
                                         clamp_min_samples(min_samples),
                                         core_out);
  return check_launch("dbscan core flags");
}

int dkm_dbscan_link_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                        double eps, int flags, void *ws, size_t ws_bytes,
                        const int32_t *core, const int32_t *orig_index,
                        int32_t *parent, int32_t *attach, void *stream) {
  if (int r = db_args("dbscan link", X, n, d, ldx, eps, 0, ws, ws_bytes))
    return r;
  if (n == 0) return 0;
  if (!core || !orig_index || !parent || !attach)
    return fail(DKM_E_ARG, "dbscan link: NULL core/orig_index/parent/attach");
  hipStream_t s = (hipStream_t)stream;
  DbWs w;
  db_layout(n, (char *)ws, &w);
  int T, tpp, P;
  db_grid(n, &T, &tpp, &P);
  k_db_init<<<row_blocks(n), NB, 0, s>>>((int)n, parent);
  if (int r = check_launch("dbscan link init")) return r;
  if (int r = db_boxes(X, (int)n, ldx, (int)d, w, s)) return r;
  if (int r = db_pair<1>(X, (int)n, ldx, (int)d, eps,
                         flags & DKM_DBSCAN_NOPRUNE ? 1 : 0, w, core,
                         orig_index, parent, s))
    return r;
  k_db_attach<<<row_blocks(n), NB, 0, s>>>(core, orig_index, w.pdist, w.pidx,
                                           (int)n, T * 64, P, attach);
  return check_launch("dbscan attach");
}

int dkm_dbscan_finalize(int64_t n, int64_t min_samples, void *ws,
                        size_t ws_bytes, const int32_t *core,
                        const int32_t *orig_index, int32_t *parent,
                        const int32_t *attach, int32_t *labels,
                        int32_t *n_clusters, void *stream) {
  if (n < 0 || n > INT32_MAX - 64 || min_samples < 0)
    return fail(DKM_E_ARG, "dbscan finalize: bad n/min_samples");
  if (!n_clusters) return fail(DKM_E_ARG, "dbscan finalize: NULL n_clusters");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    if (hipMemsetAsync(n_clusters, 0, 4, s) != hipSuccess)
      return fail(DKM_E_LAUNCH, "dbscan finalize: memset");
    return 0;
  }
  if (!core || !orig_index || !parent || !attach || !labels)
    return fail(DKM_E_ARG, "dbscan finalize: NULL array");
  if (!ws || ws_bytes < dkm_dbscan_workspace_bytes(n, 1))
    return fail(DKM_E_WORKSPACE, "dbscan finalize: workspace smaller than "
                                 "dkm_dbscan_workspace_bytes()");
  DbWs w;
  db_layout(n, (char *)ws, &w);
  int *comp = (int *)w.cnt;
  const unsigned ms = clamp_min_samples(min_samples);
  const unsigned g = row_blocks(n);
  k_db_comp<<<g, NB, 0, s>>>(core, attach, parent, (int)n, comp, w.minidx,
                             w.size, w.surv);
  k_db_stats<<<g, NB, 0, s>>>(comp, orig_index, (int)n, w.minidx, w.size);
  k_db_survive<<<g, NB, 0, s>>>(comp, w.minidx, w.size, (int)n, ms, w.surv);
  k_db_scan<<<1, SCAN_B, 0, s>>>(w.surv, (int)n, n_clusters);
  k_db_labels<<<g, NB, 0, s>>>(comp, orig_index, w.minidx, w.size, w.surv,
                               (int)n, ms, labels);
  return check_launch("dbscan finalize");
}

}  // extern "C"

// Code-object preload (dkm_preload), as in the other files.
namespace dkm {
DKM_TU_FLAGS(dbscan, 0)
__global__ void k_tu_dbscan() {}
int preload_dbscan() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, (const void *)k_tu_dbscan) == hipSuccess ? 0
                                                                           : 1;
}
}  // namespace dkm
