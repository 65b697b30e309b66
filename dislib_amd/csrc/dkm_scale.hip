// dkm_scale.hip -- StandardScaler on resident samples: column statistics and
// the scaling itself (reference dislib/preprocessing/classes.py:114-147).
// Three pure HBM streams; no floating-point atomic anywhere.
//
//   k_col_stats   sums="fast": column sums of x, or of (x - mean)^2, in fp64.
//                 A block owns a contiguous range of rows; a thread keeps one
//                 column piece (16 B of a row where d, ldx and the base allow,
//                 one element otherwise) and one fp64 accumulator per element
//                 of it in registers, over every SC_RP-th row of the range;
//                 the loads of SC_U rows are issued together.  One LDS
//                 reduction per block, in a fixed order, writes the block's
//                 partial into the workspace;
//   k_col_final   out[j] = the blocks' partials of column j, in a fixed
//                 order (a block per column).  The grid of k_col_stats
//                 depends on (n, d) only: two runs give the same bits.
//   k_col_chain   sums="reference": one sequential chain per (Subset, column)
//                 in row order from +0.0 -- k_ord_chain (dkm_ordered.hip) for
//                 a single cluster, so without the grouping pass: lane =
//                 column, the loads of CH_U rows are issued together, the
//                 adds follow strictly in order.  x, or (x - mean)^2 with the
//                 subtraction and the square rounded in the sample dtype.
//   k_scale       Y = (X - mean) / sqrt(var): the sqrt once per column piece
//                 of a thread (in the statistics' dtype), one IEEE divide per
//                 element (in the promoted dtype, as numpy).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "dkm_internal.h"

namespace dkm {

namespace {

constexpr int SC_B = 256;       // threads per block
constexpr int SC_U = 4;         // rows whose loads a thread issues together
constexpr int SC_GRID = 2048;   // most blocks (8 per CU)
constexpr int CH_U = 16;        // rows whose loads a chain issues together

// V elements of T moved as one piece (16 B for the sample dtype's V).
template <class T, int V>
struct alignas(sizeof(T) * V < 16 ? sizeof(T) * V : 16) Pack {
  T v[V];
};

template <class T>
constexpr int vec_of() { return 16 / (int)sizeof(T); }

// The grid of the streams: a function of (n, d) only.
int64_t scale_grid(int64_t n, int64_t d) {
  if (n <= 0) return 0;
  const int64_t work = (n * d + 16383) / 16384;
  return std::max<int64_t>(1, std::min<int64_t>(work, SC_GRID));
}

bool vec_ok(const void *p, int64_t ld, int64_t d, int v) {
  return ((uintptr_t)p % 16) == 0 && ld % v == 0 && d % v == 0;
}

bool scale_shape_ok(int64_t n, int64_t d, int64_t ldx) {
  return n >= 0 && d >= 1 && d < INT32_MAX && (n == 0 || ldx >= d) &&
         n < (INT64_MAX / 16) / std::max<int64_t>(1, std::max(ldx, d));
}

}  // namespace

// Column sums of f(x) over the block's rows -> part[blockIdx.x * d + j].
// cv = d / V column pieces; they are taken SC_B at a time (one pass over the
// rows per chunk; one chunk up to d = 256 V).  In a chunk of w pieces the
// thread (r, c) = (tid / w, tid % w) adds rows r, r + rp, ... (rp = SC_B / w)
// of the block's range to its V accumulators.
template <class TX, int V, bool SQ>
__global__ void __launch_bounds__(SC_B)
    k_col_stats(const TX *__restrict__ X, int64_t n, int d, int64_t ldx,
                const double *__restrict__ mean, double *__restrict__ part) {
  __shared__ double sm[SC_B * V];
  const int tid = threadIdx.x;
  const int cv = d / V;
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t row0 = min(n, (int64_t)blockIdx.x * per);
  const int64_t row1 = min(n, row0 + per);
  for (int c0 = 0; c0 < cv; c0 += SC_B) {
    const int w = min(SC_B, cv - c0);
    const int rp = SC_B / w;
    const bool live = tid < rp * w;
    const int c = c0 + tid % w;
    double acc[V], m[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      acc[v] = 0.0;
      m[v] = SQ && live ? mean[(int64_t)c * V + v] : 0.0;
    }
    if (live) {
      const TX *col = X + (int64_t)c * V;
      for (int64_t r = row0 + tid / w; r < row1; r += (int64_t)rp * SC_U) {
        Pack<TX, V> x[SC_U];
        // unconditional loads from clamped rows: the values past the range
        // are never added
#pragma unroll
        for (int u = 0; u < SC_U; ++u) {
          const int64_t ru = r + (int64_t)u * rp;
          x[u] = *(const Pack<TX, V> *)(col + (ru < row1 ? ru : r) * ldx);
        }
#pragma unroll
        for (int u = 0; u < SC_U; ++u)
          if (r + (int64_t)u * rp < row1) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
              if (SQ) {
                const double t = (double)x[u].v[v] - m[v];
                acc[v] = acc[v] + t * t;
              } else {
                acc[v] = acc[v] + (double)x[u].v[v];
              }
            }
          }
      }
    }
    __syncthreads();  // the previous chunk's reads of sm are done
#pragma unroll
    for (int v = 0; v < V; ++v) sm[tid * V + v] = acc[v];
    __syncthreads();
    if (tid < w) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        double s = sm[tid * V + v];
        for (int r = 1; r < rp; ++r) s = s + sm[(r * w + tid) * V + v];
        part[(int64_t)blockIdx.x * d + (int64_t)c * V + v] = s;
      }
    }
  }
}

// out[j] = sum over the nb blocks' partials of column j (fixed order: thread
// t folds blocks t, t + SC_B, ..., then a tree over the threads).
__global__ void __launch_bounds__(SC_B)
    k_col_final(const double *__restrict__ part, int64_t nb, int64_t d,
                double *__restrict__ out) {
  __shared__ double sm[SC_B];
  for (int64_t j = blockIdx.x; j < d; j += gridDim.x) {
    double s = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += SC_B) s = s + part[b * d + j];
    __syncthreads();
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int st = SC_B / 2; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st)
        sm[threadIdx.x] = sm[threadIdx.x] + sm[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[j] = sm[0];
  }
}

// One sequential chain per (Subset, column), ascending row order.
template <class TX, int G, bool SQ>
__global__ void __launch_bounds__(SC_B)
    k_col_chain(const TX *__restrict__ X, int64_t n, int64_t ldx, int d,
                const TX *__restrict__ mean, const int64_t *__restrict__ off,
                int64_t S, double *__restrict__ partials, int64_t ldp) {
  constexpr int GPB = SC_B / G;  // groups per block
  const int gl = threadIdx.x % G;
  const int64_t ncb = (d + G - 1) / G;
  const int64_t items = S * ncb;
  for (int64_t it = (int64_t)blockIdx.x * GPB + threadIdx.x / G; it < items;
       it += (int64_t)gridDim.x * GPB) {
    const int64_t cb = it % ncb, s = it / ncb;
    // rows [a, b) of Subset s, clamped to [0, n]
    const int64_t o0 = off[s], o1 = off[s + 1];
    const int64_t a = o0 < 0 ? 0 : (o0 > n ? n : o0);
    const int64_t b = o1 < a ? a : (o1 > n ? n : o1);
    const int t = (int)(cb * G) + gl;
    const int tc = t < d ? t : d - 1;
    const TX m = SQ ? mean[tc] : (TX)0;
    TX acc = (TX)0;  // +0.0
    for (int64_t q = a; q < b; q += CH_U) {
      TX x[CH_U];
#pragma unroll
      for (int u = 0; u < CH_U; ++u)
        x[u] = X[(q + u < b ? q + u : b - 1) * ldx + tc];
#pragma unroll
      for (int u = 0; u < CH_U; ++u)
        if (q + u < b) {
          if (SQ) {
            const TX e = x[u] - m;  // rounded in the sample dtype
            const TX e2 = e * e;    // np.square: one rounding
            acc = acc + e2;
          } else {
            acc = acc + x[u];
          }
        }
    }
    if (t < d) partials[s * ldp + t] = (double)acc;
  }
}

// Y = (X - mean) / sqrt(var).  TS: the statistics' dtype (the sqrt is taken
// in it); TY: numpy's promotion of TX and TS (the subtraction and the divide
// are taken in it).  The mapping of threads to rows and column pieces is
// k_col_stats'; a thread reads every element it writes before it writes it,
// and no other thread touches it: Y may be X.
template <class TX, class TS, class TY, int V>
__global__ void __launch_bounds__(SC_B)
    k_scale(const TX *X, int64_t n, int d, int64_t ldx,
            const TS *__restrict__ mean, const TS *__restrict__ var, TY *Y,
            int64_t ldy) {
  const int tid = threadIdx.x;
  const int cv = d / V;
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t row0 = min(n, (int64_t)blockIdx.x * per);
  const int64_t row1 = min(n, row0 + per);
  for (int c0 = 0; c0 < cv; c0 += SC_B) {
    const int w = min(SC_B, cv - c0);
    const int rp = SC_B / w;
    if (tid >= rp * w) continue;
    const int c = c0 + tid % w;
    TY m[V], sd[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      m[v] = (TY)mean[(int64_t)c * V + v];
      sd[v] = (TY)std::sqrt(var[(int64_t)c * V + v]);
    }
    const TX *col = X + (int64_t)c * V;
    TY *ycol = Y + (int64_t)c * V;
    for (int64_t r = row0 + tid / w; r < row1; r += (int64_t)rp * SC_U) {
      Pack<TX, V> x[SC_U];
#pragma unroll
      for (int u = 0; u < SC_U; ++u) {
        const int64_t ru = r + (int64_t)u * rp;
        x[u] = *(const Pack<TX, V> *)(col + (ru < row1 ? ru : r) * ldx);
      }
#pragma unroll
      for (int u = 0; u < SC_U; ++u) {
        const int64_t ru = r + (int64_t)u * rp;
        if (ru < row1) {
          Pack<TY, V> y;
#pragma unroll
          for (int v = 0; v < V; ++v) y.v[v] = ((TY)x[u].v[v] - m[v]) / sd[v];
          *(Pack<TY, V> *)(ycol + ru * ldy) = y;
        }
      }
    }
  }
}

template <class TX>
static int col_stats(const TX *X, int64_t n, int64_t d, int64_t ldx,
                     const double *mean, void *ws, size_t ws_b, double *out,
                     hipStream_t s) {
  if (!out || !scale_shape_ok(n, d, ldx) || (n > 0 && !X))
    return fail(DKM_E_ARG, "column statistics: bad arguments");
  const int64_t nb = scale_grid(n, d);
  if (nb > 0 && (!ws || ws_b < (size_t)nb * d * 8))
    return fail(DKM_E_WORKSPACE, "column statistics: workspace too small");
  constexpr int V = vec_of<TX>();
  if (nb > 0) {
    const bool vec = vec_ok(X, ldx, d, V);
#define DKM_CS(VV, SS)                                                     \
  k_col_stats<TX, VV, SS><<<(unsigned)nb, SC_B, 0, s>>>(X, n, (int)d, ldx, \
                                                        mean, (double *)ws)
    if (mean) {
      if (vec) DKM_CS(V, true);
      else DKM_CS(1, true);
    } else {
      if (vec) DKM_CS(V, false);
      else DKM_CS(1, false);
    }
#undef DKM_CS
    if (int r = check_launch("column statistics")) return r;
  }
  k_col_final<<<(unsigned)std::min<int64_t>(d, 65535), SC_B, 0, s>>>(
      (const double *)ws, nb, d, out);
  return check_launch("column statistics: final sum");
}

template <class TX>
static int col_chain(const TX *X, int64_t n, int64_t d, int64_t ldx,
                     const TX *mean, const int64_t *off, int64_t S,
                     double *partials, int64_t ldp, hipStream_t s) {
  if (!off || !partials || S < 1 || S >= INT32_MAX || ldp < d ||
      !scale_shape_ok(n, d, ldx) || (n > 0 && !X))
    return fail(DKM_E_ARG, "column chains: bad arguments");
#define DKM_CC(GG)                                                           \
  {                                                                          \
    const int64_t items = S * ((d + GG - 1) / GG);                           \
    const int64_t g = std::max<int64_t>(                                     \
        1, std::min<int64_t>((items + SC_B / GG - 1) / (SC_B / GG),          \
                             1 << 20));                                      \
    if (mean)                                                                \
      k_col_chain<TX, GG, true><<<(unsigned)g, SC_B, 0, s>>>(                \
          X, n, ldx, (int)d, mean, off, S, partials, ldp);                   \
    else                                                                     \
      k_col_chain<TX, GG, false><<<(unsigned)g, SC_B, 0, s>>>(               \
          X, n, ldx, (int)d, mean, off, S, partials, ldp);                   \
  }
  if (d <= 8) DKM_CC(8)
  else if (d <= 16) DKM_CC(16)
  else if (d <= 32) DKM_CC(32)
  else DKM_CC(64)
#undef DKM_CC
  return check_launch("column chains");
}

template <class TX, class TS, class TY>
static int scale_transform(const TX *X, int64_t n, int64_t d, int64_t ldx,
                           const TS *mean, const TS *var, TY *Y, int64_t ldy,
                           hipStream_t s) {
  if (!mean || !var || !scale_shape_ok(n, d, ldx) ||
      !scale_shape_ok(n, d, ldy) || (n > 0 && (!X || !Y)))
    return fail(DKM_E_ARG, "scale transform: bad arguments");
  const int64_t nb = scale_grid(n, d);
  if (nb == 0) return 0;
  constexpr int V = vec_of<TX>();
  // Y's pieces are V elements of TY (16 B or more): 16-B aligned like X's
  if (vec_ok(X, ldx, d, V) && ((uintptr_t)Y % 16) == 0 &&
      (ldy * (int64_t)sizeof(TY)) % 16 == 0)
    k_scale<TX, TS, TY, V><<<(unsigned)nb, SC_B, 0, s>>>(X, n, (int)d, ldx,
                                                         mean, var, Y, ldy);
  else
    k_scale<TX, TS, TY, 1><<<(unsigned)nb, SC_B, 0, s>>>(X, n, (int)d, ldx,
                                                         mean, var, Y, ldy);
  return check_launch("scale transform");
}

}  // namespace dkm

using namespace dkm;

extern "C" {

size_t dkm_scale_workspace_bytes(int64_t n, int64_t d) {
  if (n < 0 || d < 1 || d >= INT32_MAX) return 0;
  return (size_t)round_up(std::max<int64_t>(1, scale_grid(n, d)) * d * 8, 256);
}

int dkm_col_stats_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                      const double *mean, void *ws, size_t ws_bytes,
                      double *out, void *stream) {
  return col_stats<double>(X, n, d, ldx, mean, ws, ws_bytes, out,
                           (hipStream_t)stream);
}

int dkm_col_stats_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                      const double *mean, void *ws, size_t ws_bytes,
                      double *out, void *stream) {
  return col_stats<float>(X, n, d, ldx, mean, ws, ws_bytes, out,
                          (hipStream_t)stream);
}

int dkm_col_chain_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                      const double *mean, const int64_t *subset_off,
                      int64_t n_subsets, double *partials, int64_t ldp,
                      void *stream) {
  return col_chain<double>(X, n, d, ldx, mean, subset_off, n_subsets,
                           partials, ldp, (hipStream_t)stream);
}

int dkm_col_chain_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                      const float *mean, const int64_t *subset_off,
                      int64_t n_subsets, double *partials, int64_t ldp,
                      void *stream) {
  return col_chain<float>(X, n, d, ldx, mean, subset_off, n_subsets, partials,
                          ldp, (hipStream_t)stream);
}

int dkm_scale_transform_f64(const double *X, int64_t n, int64_t d,
                            int64_t ldx, const double *mean,
                            const double *var, double *Y, int64_t ldy,
                            void *stream) {
  return scale_transform<double, double, double>(X, n, d, ldx, mean, var, Y,
                                                 ldy, (hipStream_t)stream);
}

int dkm_scale_transform_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                            const float *mean, const float *var, float *Y,
                            int64_t ldy, void *stream) {
  return scale_transform<float, float, float>(X, n, d, ldx, mean, var, Y, ldy,
                                              (hipStream_t)stream);
}

int dkm_scale_transform_f32_f64(const float *X, int64_t n, int64_t d,
                                int64_t ldx, const double *mean,
                                const double *var, double *Y, int64_t ldy,
                                void *stream) {
  return scale_transform<float, double, double>(X, n, d, ldx, mean, var, Y,
                                                ldy, (hipStream_t)stream);
}

int dkm_scale_transform_f64_f32(const double *X, int64_t n, int64_t d,
                                int64_t ldx, const float *mean,
                                const float *var, double *Y, int64_t ldy,
                                void *stream) {
  return scale_transform<double, float, double>(X, n, d, ldx, mean, var, Y,
                                                ldy, (hipStream_t)stream);
}

}  // extern "C"

// Code-object preload (dkm_preload): see dkm_ordered.hip.
namespace dkm {
DKM_TU_FLAGS(scale, 0)
__global__ void k_tu_scale() {}
int preload_scale() {
  hipFuncAttributes a;
  const bool ok =
      hipFuncGetAttributes(&a, (const void *)k_tu_scale) == hipSuccess;
  return ok ? 0 : 1;
}
}  // namespace dkm
