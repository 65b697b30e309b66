// dkm_als.hip -- alternating least squares on a resident CSR ratings matrix:
// one half-step (reference dislib/recommendation/als/base.py:225-242, with
// the normal equations solved exactly instead of by cg), the squared error
// of base.py:246-253 and the item means of base.py:162.  All arithmetic is
// fp64; fp32 factors are widened in the loads.  No fast-math, no
// floating-point atomic: every sum has an order that depends on the inputs'
// shapes only, so the same input gives the same bits from run to run.
//
//   k_als_update     one block (4 waves) per CSR row.  The factor rows of the
//                    row's non-zero entries are gathered ALS_CH at a time into
//                    an LDS tile T (ALS_CH x P, P = n_f padded to 16, zero
//                    rows for stored zeros and past the end).  The 16 x 16
//                    tiles (I <= J) of the Gram matrix T^T T are dealt to the
//                    waves round robin and accumulated in registers over all
//                    chunks with v_mfma_f64_16x16x4_f64 (operands A[c][g] =
//                    T[k0 + g][16 I + c], B[g][c] = T[k0 + g][16 J + c],
//                    lane = 16 g + c, result register r = D[g + 4 r][c]);
//                    thread j < n_f keeps v[j] = sum_k T[k][j] r[k].  The
//                    lower triangle of A = Gram + lambda n_c I then goes to
//                    LDS with v as one more row below it, a right-looking
//                    Cholesky factors the augmented matrix in place (which
//                    leaves z = L^-1 v in the extra row), and one backward
//                    substitution gives y, stored as fp32.
//   k_als_sse        one wave per CSR row: lanes take the row's entries,
//                    each a full fp64 dot of the two fp32 factor rows; a
//                    64-lane butterfly; (sum, count) per row to the
//                    workspace.  k_als_sse_final adds them in a fixed order.
//   k_als_row_means  one wave per row: mean of the stored entries (zeros
//                    included; NaN for an empty row).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "dkm_internal.h"

namespace dkm {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int ALS_B = 256;             // threads per block
constexpr int ALS_W = ALS_B / WAVE;    // waves per block
constexpr int ALS_CH = DKM_ALS_CHUNK;  // gathered rows per chunk
static_assert(ALS_CH % 4 == 0 && ALS_CH <= ALS_B, "chunk: whole MFMA steps");

__device__ inline double sum64(double v) {
  v = v + __shfl_xor(v, 1);
  v = v + __shfl_xor(v, 2);
  v = v + __shfl_xor(v, 4);
  v = v + __shfl_xor(v, 8);
  v = v + __shfl_xor(v, 16);
  v = v + __shfl_xor(v, 32);
  return v;
}

// LDS doubles of k_als_update for NT column tiles: A with the v row
// ((P + 1) x (P + 1): the odd stride spreads a column over the banks), the
// gather tile, its ratings, the diagonal of L.
constexpr size_t update_lds(int nt) {
  const size_t p = size_t(nt) * 16;
  return ((p + 1) * (p + 1) + ALS_CH * p + ALS_CH + p) * sizeof(double);
}
static_assert(update_lds(DKM_ALS_MAX_NF / 16) <= 160 * 1024, "LDS budget");

bool als_csr_ok(const int64_t *indptr, const int32_t *indices,
                const double *data, int64_t n_rows) {
  return n_rows >= 0 && n_rows <= INT32_MAX && indptr &&
         (n_rows == 0 || (indices && data));
}

}  // namespace

template <class TX, int NT>
__global__ void __launch_bounds__(ALS_B)
    k_als_update(const int64_t *__restrict__ indptr,
                 const int32_t *__restrict__ indices,
                 const double *__restrict__ data, const TX *__restrict__ X,
                 int64_t m, int nf, int64_t ldx, double lambda,
                 float *__restrict__ Y) {
  constexpr int P = NT * 16, LDA = P + 1;
  constexpr int NTP = NT * (NT + 1) / 2, MAXP = (NTP + ALS_W - 1) / ALS_W;
  extern __shared__ double als_sm[];
  double *A = als_sm;                  // rows 0 .. nf (row nf = v), lower
  double *T = A + (P + 1) * LDA;       // ALS_CH x P
  double *rt = T + ALS_CH * P;         // ratings of the chunk (0 = no entry)
  double *dg = rt + ALS_CH;            // diagonal of L
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int c = lane & 15, g = lane >> 4;
  const int64_t row = blockIdx.x;
  const int64_t e0 = indptr[row], e1 = indptr[row + 1];

  // the tiles (ti, tj), ti <= tj, of this wave: t = w, w + ALS_W, ...
  int ti[MAXP], tj[MAXP];
  f64x4 acc[MAXP];
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    int i = 0, rem = w + ALS_W * p;
    while (i < NT - 1 && rem >= NT - i) {
      rem -= NT - i;
      ++i;
    }
    ti[p] = i;
    tj[p] = std::min(i + rem, NT - 1);
    acc[p] = f64x4{0.0, 0.0, 0.0, 0.0};
  }

  int nc = 0;
  double vacc = 0.0;
  for (int64_t eb = e0; eb < e1; eb += ALS_CH) {
    for (int q = tid; q < ALS_CH * P; q += ALS_B) {
      const int kk = q / P, j = q % P;
      const int64_t e = eb + kk;
      double val = 0.0;
      if (e < e1 && j < nf) {
        const int64_t ix = indices[e];
        if (data[e] != 0.0 && ix >= 0 && ix < m)
          val = (double)X[ix * ldx + j];
      }
      T[kk * P + j] = val;
    }
    if (tid < ALS_CH) {
      const int64_t e = eb + tid;
      double r = 0.0;
      if (e < e1) {
        const int64_t ix = indices[e];
        if (ix >= 0 && ix < m) r = data[e];
      }
      rt[tid] = r;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < ALS_CH; ++kk) nc += rt[kk] != 0.0 ? 1 : 0;
    if (tid < nf) {
#pragma unroll
      for (int kk = 0; kk < ALS_CH; ++kk)
        vacc = fma(T[kk * P + tid], rt[kk], vacc);
    }
#pragma unroll
    for (int k0 = 0; k0 < ALS_CH; k0 += 4) {
      const double *tr = T + (k0 + g) * P + c;
#pragma unroll
      for (int p = 0; p < MAXP; ++p) {
        if (w + ALS_W * p < NTP)
          acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(
              tr[ti[p] * 16], tr[tj[p] * 16], acc[p], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  float *y = Y + row * (int64_t)nf;
  if (nc == 0) {  // no non-zero entry: zeros (base.py:228)
    if (tid < nf) y[tid] = 0.0f;
    return;
  }

  // A[b][a] = Gram[a][b] for a in tile ti, b in tile tj (b >= a is the lower
  // triangle; the rest of a diagonal tile lands above it, unused)
  const double reg = lambda * (double)nc;
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    if (w + ALS_W * p < NTP) {
      const int b = tj[p] * 16 + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int a = ti[p] * 16 + g + 4 * r;
        if (a < nf && b < nf)
          A[b * LDA + a] = a == b ? acc[p][r] + reg : acc[p][r];
      }
    }
  }
  if (tid < nf) A[nf * LDA + tid] = vacc;
  __syncthreads();

  // Cholesky of the augmented matrix, column by column
  const int tx = tid & 15, ty = tid >> 4;
  for (int j = 0; j < nf; ++j) {
    const double l = sqrt(A[j * LDA + j]);
    if (tid == j) dg[j] = l;
    if (tid > j && tid <= nf) A[tid * LDA + j] = A[tid * LDA + j] / l;
    __syncthreads();
    for (int i = j + 1 + ty; i <= nf; i += 16) {
      const double lij = A[i * LDA + j];
      const int kmax = i < nf ? i : nf - 1;
      for (int k = j + 1 + tx; k <= kmax; k += 16)
        A[i * LDA + k] = fma(-lij, A[k * LDA + j], A[i * LDA + k]);
    }
    __syncthreads();
  }

  // L^T y = z, z in row nf
  double *z = A + nf * LDA;
  double yv = 0.0;
  for (int j = nf - 1; j >= 0; --j) {
    const double yj = z[j] / dg[j];
    if (tid < j) z[tid] = fma(-A[j * LDA + tid], yj, z[tid]);
    if (tid == j) yv = yj;
    __syncthreads();
  }
  if (tid < nf) y[tid] = (float)yv;
}

// part[2 (row - r0)] = sum over the row's non-zero entries of
// (r - users[row - r0 + uoff] . items[col])^2, part[.. + 1] = their count.
__global__ void __launch_bounds__(ALS_B)
    k_als_sse(const int64_t *__restrict__ indptr,
              const int32_t *__restrict__ indices,
              const double *__restrict__ data, int64_t r0, int64_t r1,
              int64_t uoff, const float *__restrict__ U,
              const float *__restrict__ I, int64_t ni, int nf,
              double *__restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int64_t row = r0 + (int64_t)blockIdx.x * ALS_W + (threadIdx.x >> 6);
  if (row >= r1) return;
  const float *u = U + (row - r0 + uoff) * nf;
  double s = 0.0, cnt = 0.0;
  for (int64_t e = indptr[row] + lane; e < indptr[row + 1]; e += WAVE) {
    const double r = data[e];
    const int64_t ix = indices[e];
    if (r != 0.0 && ix >= 0 && ix < ni) {
      const float *it = I + ix * nf;
      double dot = 0.0;
      for (int f = 0; f < nf; ++f) dot = fma((double)u[f], (double)it[f], dot);
      const double diff = r - dot;
      s = fma(diff, diff, s);
      cnt = cnt + 1.0;
    }
  }
  s = sum64(s);
  cnt = sum64(cnt);
  if (lane == 0) {
    part[2 * (row - r0)] = s;
    part[2 * (row - r0) + 1] = cnt;
  }
}

// out[0 .. 1] = the rows' (sum, count) added up: thread t folds rows t,
// t + ALS_B, ...; a tree over the threads then.
__global__ void __launch_bounds__(ALS_B)
    k_als_sse_final(const double *__restrict__ part, int64_t nrows,
                    double *__restrict__ out) {
  __shared__ double sm[2][ALS_B];
  double s = 0.0, cnt = 0.0;
  for (int64_t p = threadIdx.x; p < nrows; p += ALS_B) {
    s = s + part[2 * p];
    cnt = cnt + part[2 * p + 1];
  }
  sm[0][threadIdx.x] = s;
  sm[1][threadIdx.x] = cnt;
  __syncthreads();
  for (int h = ALS_B / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      sm[0][threadIdx.x] = sm[0][threadIdx.x] + sm[0][threadIdx.x + h];
      sm[1][threadIdx.x] = sm[1][threadIdx.x] + sm[1][threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = sm[0][0];
    out[1] = sm[1][0];
  }
}

__global__ void __launch_bounds__(ALS_B)
    k_als_row_means(const int64_t *__restrict__ indptr,
                    const double *__restrict__ data, int64_t n_rows,
                    double *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * ALS_W + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const int64_t e0 = indptr[row], e1 = indptr[row + 1];
  double s = 0.0;
  for (int64_t e = e0 + lane; e < e1; e += WAVE) s = s + data[e];
  s = sum64(s);
  if (lane == 0)
    out[row] = e1 > e0 ? s / (double)(e1 - e0) : __builtin_nan("");
}

namespace {

template <class TX>
int als_update(const int64_t *indptr, const int32_t *indices,
               const double *data, int64_t n_rows, const TX *X, int64_t m,
               int64_t n_f, int64_t ldx, double lambda, float *Y,
               hipStream_t s) {
  if (!als_csr_ok(indptr, indices, data, n_rows) || n_f < 1 ||
      n_f > DKM_ALS_MAX_NF || m < 0 || m > INT32_MAX || ldx < n_f ||
      (n_rows > 0 && (!X || !Y)) || !(lambda == lambda))
    return fail(DKM_E_ARG, "als update: bad arguments");
  if (n_rows == 0) return 0;
  const int nt = (int)((n_f + 15) / 16);
  const void *kf = nullptr;
  switch (nt) {
#define DKM_AU(N)                                  \
  case N:                                          \
    kf = (const void *)k_als_update<TX, N>;        \
    break;
    DKM_AU(1) DKM_AU(2) DKM_AU(3) DKM_AU(4)
    DKM_AU(5) DKM_AU(6) DKM_AU(7) DKM_AU(8)
#undef DKM_AU
    default:
      return fail(DKM_E_ARG, "als update: n_f");
  }
  const size_t lds = update_lds(nt);
  if (hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return fail(DKM_E_LAUNCH, "als update: LDS attribute");
  hipLaunchKernelGGL(
      (void (*)(const int64_t *, const int32_t *, const double *, const TX *,
                int64_t, int, int64_t, double, float *))kf,
      dim3((unsigned)n_rows), dim3(ALS_B), lds, s, indptr, indices, data, X, m,
      (int)n_f, ldx, lambda, Y);
  return check_launch("als update");
}

}  // namespace

}  // namespace dkm

using namespace dkm;

extern "C" {

size_t dkm_als_workspace_bytes(int64_t n_rows, int64_t n_f) {
  if (n_rows < 0 || n_rows > INT32_MAX || n_f < 1 || n_f > DKM_ALS_MAX_NF)
    return 0;
  return (size_t)(2 * std::max<int64_t>(n_rows, 1)) * sizeof(double);
}

int dkm_als_update_f64(const int64_t *indptr, const int32_t *indices,
                       const double *data, int64_t n_rows, const double *X,
                       int64_t m, int64_t n_f, int64_t ldx, double lambda,
                       float *Y, void *stream) {
  return als_update<double>(indptr, indices, data, n_rows, X, m, n_f, ldx,
                            lambda, Y, (hipStream_t)stream);
}

int dkm_als_update_f32(const int64_t *indptr, const int32_t *indices,
                       const double *data, int64_t n_rows, const float *X,
                       int64_t m, int64_t n_f, int64_t ldx, double lambda,
                       float *Y, void *stream) {
  return als_update<float>(indptr, indices, data, n_rows, X, m, n_f, ldx,
                           lambda, Y, (hipStream_t)stream);
}

int dkm_als_sse(const int64_t *indptr, const int32_t *indices,
                const double *data, int64_t row_begin, int64_t row_end,
                int64_t user_offset, const float *users, int64_t n_users,
                const float *items, int64_t n_items, int64_t n_f, void *ws,
                size_t ws_bytes, double *out, void *stream) {
  const int64_t nr = row_end - row_begin;
  if (!indptr || row_begin < 0 || nr < 0 || row_end > INT32_MAX ||
      user_offset < 0 || n_users < 0 || nr + user_offset > n_users ||
      n_items < 0 || n_items > INT32_MAX || n_f < 1 ||
      n_f > DKM_ALS_MAX_NF || !out ||
      (nr > 0 && (!indices || !data || !users || !items)))
    return fail(DKM_E_ARG, "als sse: bad arguments");
  if (!ws || ws_bytes < dkm_als_workspace_bytes(nr, n_f))
    return fail(DKM_E_WORKSPACE, "als sse: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  if (nr > 0) {
    k_als_sse<<<(unsigned)((nr + ALS_W - 1) / ALS_W), ALS_B, 0, s>>>(
        indptr, indices, data, row_begin, row_end, user_offset, users, items,
        n_items, (int)n_f, (double *)ws);
    if (int r = check_launch("als sse")) return r;
  }
  k_als_sse_final<<<1, ALS_B, 0, s>>>((const double *)ws, nr, out);
  return check_launch("als sse: final sum");
}

int dkm_als_row_means(const int64_t *indptr, const double *data,
                      int64_t n_rows, double *out, void *stream) {
  if (!indptr || n_rows < 0 || n_rows > INT32_MAX || (n_rows > 0 && !out))
    return fail(DKM_E_ARG, "als row means: bad arguments");
  if (n_rows == 0) return 0;
  k_als_row_means<<<(unsigned)((n_rows + ALS_W - 1) / ALS_W), ALS_B, 0,
                    (hipStream_t)stream>>>(indptr, data, n_rows, out);
  return check_launch("als row means");
}

}  // extern "C"

// Code-object preload (dkm_preload): see dkm_ordered.hip.
namespace dkm {
DKM_TU_FLAGS(als, 0)
__global__ void k_tu_als() {}
int preload_als() {
  hipFuncAttributes a;
  const bool ok = hipFuncGetAttributes(&a, (const void *)k_tu_als) == hipSuccess;
  return ok ? 0 : 1;
}
}  // namespace dkm
