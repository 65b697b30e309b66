// dkm_gm.hip -- GaussianMixture (full covariances) on resident samples: the
// E-step and the two M-step passes of one EM iteration (reference
// dislib/cluster/gm/base.py:19-29, :103-117, :201-307), all in fp64 on
// v_mfma_f64_16x16x4_f64.  fp32 rows are widened in the loads.  No fast-math,
// no floating-point atomic: every cross-block sum is block partials added in
// a fixed order, and every grid is a function of (n, d, K) only, so the same
// input gives the same bits from run to run.
//
// Operand layout of the f64 MFMA (lane l, c = l & 15, g = l >> 4): A[c][g],
// B[g][c], result register r = D[g + 4 r][c].  A wave is the unit of work
// everywhere; no kernel stages anything in LDS.
//
//   k_gm_estep       a wave owns RT tiles of 16 rows.  Lane (c, g) keeps
//                    x[row c][4 q + g] of its rows in registers for every
//                    component (D4 = the q's; d > 128 reloads them).  Per
//                    component k: xm = x - mu_k once, then per 16-column
//                    panel of P_k  y = xm P_k  with the panel's elements read
//                    from global memory (L1/L2: K d^2 fp64 is small), the
//                    rows of P_k below an upper-triangular panel skipped,
//                    ss += y^2 per lane and one 16-lane butterfly per row.
//                    wlp = -(d log 2pi + ss) / 2 + (log det + log w)_k is
//                    parked in resp[row][k] by lane c = k & 15 of the row's
//                    group, which is the lane that reads it back: the
//                    second part (max, sum of exp, log, resp = exp(wlp - lse),
//                    first-maximum argmax of resp) runs over k = c, c + 16, ..
//                    with 16-lane butterflies, without a barrier.
//   k_gm_sums        [nk | resp^T X]: M = components, N = the columns of
//                    [X | 1], summed over a chunk of rows, 4 rows per MFMA;
//                    a wave owns (row chunk, 16 components, 4 column panels).
//   k_gm_cov         sum_n r_nk (x_n - mu_k)(x_n - mu_k)^T around the given
//                    means (the second pass): a wave owns (row chunk, k, 4 of
//                    the 16 x 16 tiles on or above the diagonal).
//   k_gm_*_final     the chunks' partials added in a fixed order (16 slices
//                    of the chunks, then the slices in order); the covariance
//                    tiles are mirrored below the diagonal here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "dkm_internal.h"

namespace dkm {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int GM_B = 256;            // threads per block
constexpr int GM_W = GM_B / WAVE;    // waves per block
constexpr int GM_ROWS = 512;         // rows of an M-step chunk, at least
constexpr int GM_CHUNKS = 2048;      // most M-step chunks
constexpr int GM_NJ = 4;             // tiles a wave accumulates
constexpr int64_t GM_COV_WS = int64_t(64) << 20;  // covariance partials, about
constexpr double LOG_2PI = 1.8378770664093453;    // np.log(2 * np.pi)

__device__ inline f64x4 mfma(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// The sum / maximum over the 16 lanes of a row group, the same bits in each.
__device__ inline double sum16(double v) {
  v = v + __shfl_xor(v, 1);
  v = v + __shfl_xor(v, 2);
  v = v + __shfl_xor(v, 4);
  v = v + __shfl_xor(v, 8);
  return v;
}

__device__ inline double max16(double v) {
  v = fmax(v, __shfl_xor(v, 1));
  v = fmax(v, __shfl_xor(v, 2));
  v = fmax(v, __shfl_xor(v, 4));
  v = fmax(v, __shfl_xor(v, 8));
  return v;
}

bool gm_shape_ok(int64_t n, int64_t d, int64_t ldx, int64_t k) {
  return n >= 0 && d >= 1 && d <= 32768 && k >= 1 && k <= (1 << 20) &&
         (n == 0 || ldx >= d) && k * d * d < (int64_t(1) << 40) &&
         n < (INT64_MAX / 16) / std::max<int64_t>(k, std::max(ldx, d));
}

int64_t estep_rt(int64_t d) { return d > 64 && d <= 128 ? 1 : 2; }

int64_t estep_blocks(int64_t n, int64_t d) {
  const int64_t rpb = GM_W * 16 * estep_rt(d);
  return (n + rpb - 1) / rpb;
}

// M-step row chunks: a function of (n, d, K) only.
int64_t sums_chunks(int64_t n) {
  return std::max<int64_t>(
      1, std::min<int64_t>((n + GM_ROWS - 1) / GM_ROWS, GM_CHUNKS));
}

int64_t cov_tiles(int64_t d) {
  const int64_t p = (d + 15) / 16;
  return p * (p + 1) / 2;
}

int64_t cov_chunks(int64_t n, int64_t d, int64_t k) {
  const int64_t cap =
      std::max<int64_t>(8, GM_COV_WS / (k * cov_tiles(d) * 2048));
  return std::max<int64_t>(1, std::min(sums_chunks(n), cap));
}

// rows of a chunk: a multiple of 4
__host__ __device__ inline int64_t chunk_rows(int64_t n, int64_t nrc) {
  return ((n + nrc - 1) / nrc + 3) / 4 * 4;
}

}  // namespace

template <class TX, int D4, int RT>
__global__ void __launch_bounds__(GM_B)
    k_gm_estep(const TX *__restrict__ X, int64_t n, int d, int64_t ldx,
               const double *__restrict__ mu, const double *__restrict__ P,
               const double *__restrict__ ldw, int K, int upper, double *resp,
               int64_t *__restrict__ labels, double *__restrict__ part) {
  __shared__ double sw[GM_W];
  constexpr int NX = D4 > 0 ? D4 : 1;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int64_t base = ((int64_t)blockIdx.x * GM_W + w) * (16 * RT);
  const int nq = (d + 3) / 4;
  // the row this lane supplies to the A operand of tile t (clamped: rows
  // past n repeat the last one and are never written)
  const TX *xr[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
    xr[t] = X + std::min<int64_t>(base + 16 * t + c, n - 1) * ldx;
  double x[RT][NX];
  if (D4 > 0) {
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int q = 0; q < NX; ++q) {
        const int i = 4 * q + g;
        x[t][q] = q < nq && i < d ? (double)xr[t][i] : 0.0;
      }
  }
  const double cst = (double)d * LOG_2PI;
  for (int k = 0; k < K; ++k) {
    const double *Pk = P + (int64_t)k * d * d;
    const double *muk = mu + (int64_t)k * d;
    double xm[RT][NX];
    if (D4 > 0) {
#pragma unroll
      for (int q = 0; q < NX; ++q) {
        const int i = 4 * q + g;
        const double m = q < nq && i < d ? muk[i] : 0.0;
#pragma unroll
        for (int t = 0; t < RT; ++t) xm[t][q] = x[t][q] - m;
      }
    }
    double ss[RT][4];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) ss[t][r] = 0.0;
    for (int j0 = 0; j0 < d; j0 += 16) {
      const int j = j0 + c;
      const bool jok = j < d;
      // P_k upper triangular: rows past the panel's last column are zero
      const int iend = upper ? std::min(d, j0 + 16) : d;
      const int qend = (iend + 3) / 4;
      f64x4 acc[RT];
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
      if (D4 > 0) {
#pragma unroll
        for (int q = 0; q < NX; ++q)
          if (q < qend) {
            const int i = 4 * q + g;
            const double b = jok && i < d ? Pk[(int64_t)i * d + j] : 0.0;
#pragma unroll
            for (int t = 0; t < RT; ++t) acc[t] = mfma(xm[t][q], b, acc[t]);
          }
      } else {
        for (int q = 0; q < qend; ++q) {
          const int i = 4 * q + g;
          const bool iok = i < d;
          const double m = iok ? muk[i] : 0.0;
          const double b = jok && iok ? Pk[(int64_t)i * d + j] : 0.0;
#pragma unroll
          for (int t = 0; t < RT; ++t) {
            const double a = iok ? (double)xr[t][i] - m : 0.0;
            acc[t] = mfma(a, b, acc[t]);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) ss[t][r] = ss[t][r] + acc[t][r] * acc[t][r];
    }
    const double lk = ldw[k];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double s = sum16(ss[t][r]);
        const int64_t row = base + 16 * t + g + 4 * r;
        if ((k & 15) == c && row < n)
          resp[row * K + k] = -0.5 * (cst + s) + lk;
      }
  }
  // the rows of this lane's group over k = c, c + 16, ...: every lane reads
  // back what it wrote itself
  double tot = 0.0;
#pragma unroll
  for (int t = 0; t < RT; ++t)
    for (int r = 0; r < 4; ++r) {
      const int64_t row = base + 16 * t + g + 4 * r;
      const bool ok = row < n;
      double *rr = resp + (ok ? row : 0) * K;
      const int kl = ok ? K : 0;
      double mx = -INFINITY;
      for (int k = c; k < kl; k += 16) mx = fmax(mx, rr[k]);
      mx = max16(mx);
      double s = 0.0;
      for (int k = c; k < kl; k += 16) s = s + exp(rr[k] - mx);
      s = sum16(s);
      const double lse = log(s) + mx;
      double best = -1.0;
      int bi = INT32_MAX;
      for (int k = c; k < kl; k += 16) {
        const double v = exp(rr[k] - lse);
        rr[k] = v;
        if (v > best) {
          best = v;
          bi = k;
        }
      }
      // numpy's argmax: the first maximum
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const double ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ob > best || (ob == best && oi < bi)) {
          best = ob;
          bi = oi;
        }
      }
      if (ok && c == 0 && labels) labels[row] = bi == INT32_MAX ? 0 : bi;
      if (ok) tot = tot + lse;
    }
  tot = tot + __shfl_xor(tot, 16);
  tot = tot + __shfl_xor(tot, 32);
  if (lane == 0) sw[w] = tot;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = sw[0];
    for (int i = 1; i < GM_W; ++i) s = s + sw[i];
    part[blockIdx.x] = s;
  }
}

// out[0] = the blocks' partials in a fixed order (one block).
__global__ void __launch_bounds__(GM_B)
    k_gm_scalar_final(const double *__restrict__ part, int64_t nb,
                      double *__restrict__ out) {
  __shared__ double sm[GM_B];
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += GM_B) s = s + part[b];
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int st = GM_B / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st)
      sm[threadIdx.x] = sm[threadIdx.x] + sm[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sm[0];
}

// part[(rc K + k)(d + 1) + j] = sum over the chunk's rows of resp[., k] times
// column j of [X | 1].
template <class TX>
__global__ void __launch_bounds__(GM_B)
    k_gm_sums(const TX *__restrict__ X, int64_t n, int d, int64_t ldx,
              const double *__restrict__ resp, int K, int64_t nrc,
              double *__restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int c = lane & 15, g = lane >> 4;
  const int np = (d + 1 + 15) / 16, njc = (np + GM_NJ - 1) / GM_NJ;
  const int kp = (K + 15) / 16;
  const int64_t wid = (int64_t)blockIdx.x * GM_W + (threadIdx.x >> 6);
  const int jc = (int)(wid % njc);
  const int kq = (int)((wid / njc) % kp);
  const int64_t rc = wid / ((int64_t)njc * kp);
  if (rc >= nrc) return;
  const int64_t per = chunk_rows(n, nrc);
  const int64_t row0 = std::min(n, rc * per), row1 = std::min(n, row0 + per);
  const int k = kq * 16 + c;
  const bool kok = k < K;
  f64x4 acc[GM_NJ];
#pragma unroll
  for (int p = 0; p < GM_NJ; ++p) acc[p] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int64_t r0 = row0; r0 < row1; r0 += 4) {
    const int64_t row = r0 + g;
    const bool ok = row < row1;
    const double a = ok && kok ? resp[row * K + k] : 0.0;
#pragma unroll
    for (int p = 0; p < GM_NJ; ++p) {
      const int j = (jc * GM_NJ + p) * 16 + c;
      if (jc * GM_NJ + p < np) {
        const double b =
            !ok ? 0.0 : j < d ? (double)X[row * ldx + j] : j == d ? 1.0 : 0.0;
        acc[p] = mfma(a, b, acc[p]);
      }
    }
  }
#pragma unroll
  for (int p = 0; p < GM_NJ; ++p) {
    const int j = (jc * GM_NJ + p) * 16 + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kk = kq * 16 + g + 4 * r;
      if (kk < K && j <= d)
        part[(rc * K + kk) * (int64_t)(d + 1) + j] = acc[p][r];
    }
  }
}

// The sum over p of part[p len + e] for the 16 elements e of a block: thread
// (slice s = tid / 16, element tid % 16) folds chunks s, s + 16, ...; the
// slices are then added in order.  Valid in the threads of slice 0.
__device__ inline double fold_parts(const double *__restrict__ part,
                                    int64_t nparts, int64_t len, int64_t e,
                                    double *sm) {
  const int s = threadIdx.x >> 4;
  double v = 0.0;
  if (e < len)
    for (int64_t p = s; p < nparts; p += 16) v = v + part[p * len + e];
  sm[threadIdx.x] = v;
  __syncthreads();
  if (s == 0)
    for (int i = 1; i < 16; ++i) v = v + sm[i * 16 + threadIdx.x];
  return v;
}

// out = [nk (K) | resp^T X (K x d)]
__global__ void __launch_bounds__(GM_B)
    k_gm_sums_final(const double *__restrict__ part, int64_t nrc, int K, int d,
                    double *__restrict__ out) {
  __shared__ double sm[GM_B];
  const int64_t len = (int64_t)K * (d + 1);
  const int64_t e = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
  const double v = fold_parts(part, nrc, len, e, sm);
  if (threadIdx.x < 16 && e < len) {
    const int64_t k = e / (d + 1), j = e % (d + 1);
    out[j == d ? k : K + k * d + j] = v;
  }
}

// tile ti of the tiles on or above the diagonal, row-major: (ap, bp)
__device__ inline void cov_tile(int ti, int np, int *ap, int *bp) {
  int a = 0;
  while (ti >= np - a) {
    ti -= np - a;
    ++a;
  }
  *ap = a;
  *bp = a + ti;
}

// part[((rc K + k) T + ti) 256 + 16 a + b] = sum over the chunk's rows of
// r_nk (x_a - mu_ka)(x_b - mu_kb) for the elements (a, b) of tile ti.
template <class TX>
__global__ void __launch_bounds__(GM_B)
    k_gm_cov(const TX *__restrict__ X, int64_t n, int d, int64_t ldx,
             const double *__restrict__ resp, const double *__restrict__ mu,
             int K, int64_t nrc, double *__restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int c = lane & 15, g = lane >> 4;
  const int np = (d + 15) / 16, T = np * (np + 1) / 2;
  const int ntc = (T + GM_NJ - 1) / GM_NJ;
  const int64_t wid = (int64_t)blockIdx.x * GM_W + (threadIdx.x >> 6);
  const int tc = (int)(wid % ntc);
  const int k = (int)((wid / ntc) % K);
  const int64_t rc = wid / ((int64_t)ntc * K);
  if (rc >= nrc) return;
  const int64_t per = chunk_rows(n, nrc);
  const int64_t row0 = std::min(n, rc * per), row1 = std::min(n, row0 + per);
  int ja[GM_NJ], jb[GM_NJ];
  double ma[GM_NJ], mb[GM_NJ];
  f64x4 acc[GM_NJ];
#pragma unroll
  for (int t = 0; t < GM_NJ; ++t) {
    int ap = 0, bp = 0;
    if (tc * GM_NJ + t < T) cov_tile(tc * GM_NJ + t, np, &ap, &bp);
    ja[t] = ap * 16 + c;
    jb[t] = bp * 16 + c;
    ma[t] = ja[t] < d ? mu[(int64_t)k * d + ja[t]] : 0.0;
    mb[t] = jb[t] < d ? mu[(int64_t)k * d + jb[t]] : 0.0;
    acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  }
  for (int64_t r0 = row0; r0 < row1; r0 += 4) {
    const int64_t row = r0 + g;
    const bool ok = row < row1;
    const double r = ok ? resp[row * K + k] : 0.0;
    const TX *xr = X + (ok ? row : row0) * ldx;
#pragma unroll
    for (int t = 0; t < GM_NJ; ++t)
      if (tc * GM_NJ + t < T) {
        const double da = ok && ja[t] < d ? (double)xr[ja[t]] - ma[t] : 0.0;
        const double db = ok && jb[t] < d ? (double)xr[jb[t]] - mb[t] : 0.0;
        acc[t] = mfma(r * da, db, acc[t]);
      }
  }
#pragma unroll
  for (int t = 0; t < GM_NJ; ++t)
    if (tc * GM_NJ + t < T) {
      double *o = part + ((rc * K + k) * (int64_t)T + tc * GM_NJ + t) * 256;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[(g + 4 * r) * 16 + c] = acc[t][r];
    }
}

// cov[k][a][b] = cov[k][b][a] = the chunks' partials of (a <= b).
__global__ void __launch_bounds__(GM_B)
    k_gm_cov_final(const double *__restrict__ part, int64_t nrc, int K, int d,
                   double *__restrict__ cov) {
  __shared__ double sm[GM_B];
  const int np = (d + 15) / 16, T = np * (np + 1) / 2;
  const int64_t len = (int64_t)K * T * 256;
  const int64_t e = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
  const double v = fold_parts(part, nrc, len, e, sm);
  if (threadIdx.x < 16 && e < len) {
    const int64_t k = e / ((int64_t)T * 256);
    const int ti = (int)((e / 256) % T), el = (int)(e % 256);
    int ap, bp;
    cov_tile(ti, np, &ap, &bp);
    const int a = ap * 16 + el / 16, b = bp * 16 + el % 16;
    if (a <= b && b < d) {
      double *ck = cov + k * d * d;
      ck[(int64_t)a * d + b] = v;
      ck[(int64_t)b * d + a] = v;
    }
  }
}

// resp[i][k] = labels[i] == k
__global__ void __launch_bounds__(GM_B)
    k_gm_onehot(const int32_t *__restrict__ labels, int64_t n, int K,
                double *__restrict__ resp) {
  const int64_t total = n * K;
  for (int64_t e = (int64_t)blockIdx.x * GM_B + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * GM_B)
    resp[e] = labels[e / K] == (int32_t)(e % K) ? 1.0 : 0.0;
}

namespace {

size_t gm_ws_bytes(int64_t n, int64_t d, int64_t k) {
  int64_t b = std::max<int64_t>(1, estep_blocks(n, d)) * 8;
  b = std::max(b, sums_chunks(n) * k * (d + 1) * 8);
  b = std::max(b, cov_chunks(n, d, k) * k * cov_tiles(d) * 2048);
  return (size_t)round_up(b, 256);
}

template <class TX>
int gm_estep(const TX *X, int64_t n, int64_t d, int64_t ldx,
             const double *means, const double *pc, const double *ldw,
             int64_t k, int flags, void *ws, size_t ws_b, double *resp,
             int64_t *labels, double *lpn, hipStream_t s) {
  if (!gm_shape_ok(n, d, ldx, k) || !means || !pc || !ldw || !lpn ||
      (flags & ~DKM_GM_UPPER) || (n > 0 && (!X || !resp)))
    return fail(DKM_E_ARG, "gm E-step: bad arguments");
  const int64_t nb = estep_blocks(n, d);
  if (nb > INT32_MAX) return fail(DKM_E_ARG, "gm E-step: n too large");
  if (!ws || ws_b < gm_ws_bytes(n, d, k))
    return fail(DKM_E_WORKSPACE, "gm E-step: workspace too small");
  const int up = flags & DKM_GM_UPPER ? 1 : 0;
  if (nb > 0) {
#define DKM_GE(DD, RR)                                                      \
  k_gm_estep<TX, DD, RR><<<(unsigned)nb, GM_B, 0, s>>>(                     \
      X, n, (int)d, ldx, means, pc, ldw, (int)k, up, resp, labels,          \
      (double *)ws)
    if (d <= 16) DKM_GE(4, 2);
    else if (d <= 32) DKM_GE(8, 2);
    else if (d <= 64) DKM_GE(16, 2);
    else if (d <= 128) DKM_GE(32, 1);
    else DKM_GE(0, 2);
#undef DKM_GE
    if (int r = check_launch("gm E-step")) return r;
  }
  k_gm_scalar_final<<<1, GM_B, 0, s>>>((const double *)ws, nb, lpn);
  return check_launch("gm E-step: final sum");
}

template <class TX>
int gm_sums(const TX *X, int64_t n, int64_t d, int64_t ldx, const double *resp,
            int64_t k, void *ws, size_t ws_b, double *out, hipStream_t s) {
  if (!gm_shape_ok(n, d, ldx, k) || !out || (n > 0 && (!X || !resp)))
    return fail(DKM_E_ARG, "gm M-step sums: bad arguments");
  if (!ws || ws_b < gm_ws_bytes(n, d, k))
    return fail(DKM_E_WORKSPACE, "gm M-step sums: workspace too small");
  const int64_t nrc = n > 0 ? sums_chunks(n) : 0;
  if (nrc > 0) {
    const int64_t np = (d + 1 + 15) / 16, njc = (np + GM_NJ - 1) / GM_NJ;
    const int64_t waves = nrc * ((k + 15) / 16) * njc;
    const int64_t nb = (waves + GM_W - 1) / GM_W;
    if (nb > INT32_MAX) return fail(DKM_E_ARG, "gm M-step sums: too large");
    k_gm_sums<TX><<<(unsigned)nb, GM_B, 0, s>>>(X, n, (int)d, ldx, resp,
                                                (int)k, nrc, (double *)ws);
    if (int r = check_launch("gm M-step sums")) return r;
  }
  const int64_t len = k * (d + 1);
  k_gm_sums_final<<<(unsigned)((len + 15) / 16), GM_B, 0, s>>>(
      (const double *)ws, nrc, (int)k, (int)d, out);
  return check_launch("gm M-step sums: final sum");
}

template <class TX>
int gm_cov(const TX *X, int64_t n, int64_t d, int64_t ldx, const double *resp,
           const double *means, int64_t k, void *ws, size_t ws_b, double *cov,
           hipStream_t s) {
  if (!gm_shape_ok(n, d, ldx, k) || !means || !cov ||
      (n > 0 && (!X || !resp)))
    return fail(DKM_E_ARG, "gm M-step covariances: bad arguments");
  if (!ws || ws_b < gm_ws_bytes(n, d, k))
    return fail(DKM_E_WORKSPACE,
                "gm M-step covariances: workspace too small");
  const int64_t nrc = n > 0 ? cov_chunks(n, d, k) : 0;
  const int64_t T = cov_tiles(d);
  if (nrc > 0) {
    const int64_t waves = nrc * k * ((T + GM_NJ - 1) / GM_NJ);
    const int64_t nb = (waves + GM_W - 1) / GM_W;
    if (nb > INT32_MAX)
      return fail(DKM_E_ARG, "gm M-step covariances: too large");
    k_gm_cov<TX><<<(unsigned)nb, GM_B, 0, s>>>(X, n, (int)d, ldx, resp, means,
                                               (int)k, nrc, (double *)ws);
    if (int r = check_launch("gm M-step covariances")) return r;
  }
  const int64_t len = k * T * 256;
  if ((len + 15) / 16 > INT32_MAX)
    return fail(DKM_E_ARG, "gm M-step covariances: too large");
  k_gm_cov_final<<<(unsigned)((len + 15) / 16), GM_B, 0, s>>>(
      (const double *)ws, nrc, (int)k, (int)d, cov);
  return check_launch("gm M-step covariances: final sum");
}

}  // namespace

}  // namespace dkm

using namespace dkm;

extern "C" {

size_t dkm_gm_workspace_bytes(int64_t n, int64_t d, int64_t k) {
  if (!gm_shape_ok(n, d, d, k)) return 0;
  return gm_ws_bytes(n, d, k);
}

int dkm_gm_estep_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                     const double *means, const double *precisions_chol,
                     const double *log_det_w, int64_t k, int flags, void *ws,
                     size_t ws_bytes, double *resp, int64_t *labels,
                     double *log_prob_sum, void *stream) {
  return gm_estep<double>(X, n, d, ldx, means, precisions_chol, log_det_w, k,
                          flags, ws, ws_bytes, resp, labels, log_prob_sum,
                          (hipStream_t)stream);
}

int dkm_gm_estep_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                     const double *means, const double *precisions_chol,
                     const double *log_det_w, int64_t k, int flags, void *ws,
                     size_t ws_bytes, double *resp, int64_t *labels,
                     double *log_prob_sum, void *stream) {
  return gm_estep<float>(X, n, d, ldx, means, precisions_chol, log_det_w, k,
                         flags, ws, ws_bytes, resp, labels, log_prob_sum,
                         (hipStream_t)stream);
}

int dkm_gm_mstep_sums_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                          const double *resp, int64_t k, void *ws,
                          size_t ws_bytes, double *out, void *stream) {
  return gm_sums<double>(X, n, d, ldx, resp, k, ws, ws_bytes, out,
                         (hipStream_t)stream);
}

int dkm_gm_mstep_sums_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                          const double *resp, int64_t k, void *ws,
                          size_t ws_bytes, double *out, void *stream) {
  return gm_sums<float>(X, n, d, ldx, resp, k, ws, ws_bytes, out,
                        (hipStream_t)stream);
}

int dkm_gm_mstep_cov_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                         const double *resp, const double *means, int64_t k,
                         void *ws, size_t ws_bytes, double *cov,
                         void *stream) {
  return gm_cov<double>(X, n, d, ldx, resp, means, k, ws, ws_bytes, cov,
                        (hipStream_t)stream);
}

int dkm_gm_mstep_cov_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                         const double *resp, const double *means, int64_t k,
                         void *ws, size_t ws_bytes, double *cov,
                         void *stream) {
  return gm_cov<float>(X, n, d, ldx, resp, means, k, ws, ws_bytes, cov,
                       (hipStream_t)stream);
}

int dkm_gm_onehot(const int32_t *labels, int64_t n, int64_t k, double *resp,
                  void *stream) {
  if (n < 0 || k < 1 || k > INT32_MAX || (n > 0 && (!labels || !resp)) ||
      n >= INT64_MAX / 16 / k)
    return fail(DKM_E_ARG, "gm one-hot: bad arguments");
  if (n == 0) return 0;
  const int64_t nb = std::min<int64_t>((n * k + GM_B - 1) / GM_B, 65536);
  k_gm_onehot<<<(unsigned)nb, GM_B, 0, (hipStream_t)stream>>>(labels, n,
                                                              (int)k, resp);
  return check_launch("gm one-hot");
}

}  // extern "C"

// Code-object preload (dkm_preload): see dkm_ordered.hip.
namespace dkm {
DKM_TU_FLAGS(gm, 0)
__global__ void k_tu_gm() {}
int preload_gm() {
  hipFuncAttributes a;
  const bool ok = hipFuncGetAttributes(&a, (const void *)k_tu_gm) == hipSuccess;
  return ok ? 0 : 1;
}
}  // namespace dkm
