// dkm_pca.hip -- PCA on the resident dense samples: the
// mean and the scatter matrix in ONE read of X, and the projection of rows
// onto the principal axes.  All arithmetic is fp64 on v_mfma_f64_16x16x4_f64;
// fp32 rows are widened in the loads.  No fast-math, no floating-point atomic,
// no grid-wide barrier: every cross-block sum is block partials added in a
// fixed order and every grid is a function of the shapes only, so the same
// input gives the same bits from run to run.
//
// Operands of the f64 MFMA (lane l, c = l & 15, g = l >> 4): A[m = c][k = g],
// B[k = g][n = c], result register r = D[g + 4 r][c].  Both kernels stage
// their operands in LDS in the layout [k / 4][m or n][k % 4] (dkm_svm.hip's),
// so that a wave's operand read is 64 consecutive doubles.
//
//   k_pca_gram        G = sum over the rows of a^T a for the augmented rows
//                     a = [x - p | 1] of width da = d + 1 (p: a pivot near the
//                     mean, so that G[:d,:d] - s s^T / n does not cancel):
//                     G[:d,:d] is the shifted scatter, column d is s = sum(x -
//                     p) and the corner is n.  Here k is the ROW of X.  G is
//                     cut into 64 x 64 macro tiles; a block of four waves owns
//                     one (macro tile (I, J) on or above the diagonal, row
//                     chunk) and each wave a 16 x 64 strip of it in four
//                     accumulators for the whole chunk.  Per slab of 16 rows
//                     the block loads the I and J column panels (one panel on
//                     the diagonal) into registers -- a wave reads 4 rows x 16
//                     columns per load, 128-byte pieces -- subtracts p and
//                     writes 64 consecutive doubles per wave into LDS.  LDS is
//                     double-buffered: the loads of slab s + 1 are issued
//                     before the MFMAs of slab s and stored after them, one
//                     barrier per slab.  16 x 16 tiles wholly below the
//                     diagonal or past column d are multiplied (no branch in
//                     the loop) but never stored.
//   k_pca_gram_final  the chunks' partials added in a fixed order (16 slices
//                     of the chunks, then the slices in order), written to
//                     both halves of the symmetric (d + 1) x (d + 1) matrix.
//   k_pca_project     Y = (X - mean) V^T.  Here k is the FEATURE.  A block
//                     owns 64 rows (16 per wave); per panel of 64 components
//                     it walks the features in slabs of 16, staging the
//                     centred rows and the matching slab of V, with the same
//                     register prefetch; a wave stores 16 consecutive
//                     components of a row.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "dkm_internal.h"

namespace dkm {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int PC_B = 256;              // threads per block: four waves
constexpr int PC_T = 64;               // a macro tile / panel: 4 MFMA tiles
constexpr int PC_S = 16;               // rows (gram) / features (project) per slab
constexpr int PC_G = PC_T * 4 + 16;    // doubles per group of four k in LDS
constexpr int PC_PANEL = (PC_S / 4) * PC_G;  // one staged panel
constexpr int PC_ROWS = 512;           // rows of a chunk, at least
constexpr int64_t PC_WS = int64_t(64) << 20;  // the partials, about
constexpr int64_t PC_TILE_BYTES = PC_T * PC_T * 8;
static_assert(PC_B == 4 * WAVE && PC_T * PC_S == 4 * PC_B,
              "four elements per thread and panel");

__device__ inline f64x4 mfma(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

bool pca_shape_ok(int64_t n, int64_t d, int64_t ldx) {
  return n >= 1 && d >= 1 && d <= DKM_PCA_MAX_D && ldx >= d &&
         n < (INT64_MAX / 16) / ldx;
}

int64_t pca_panels(int64_t d) { return (d + 1 + PC_T - 1) / PC_T; }

int64_t pca_pairs(int64_t d) {
  const int64_t p = pca_panels(d);
  return p * (p + 1) / 2;
}

// Row chunks: a function of (n, d) only.
int64_t pca_chunks(int64_t n, int64_t d) {
  const int64_t cap =
      std::max<int64_t>(8, PC_WS / (pca_pairs(d) * PC_TILE_BYTES));
  return std::max<int64_t>(
      1, std::min<int64_t>((n + PC_ROWS - 1) / PC_ROWS, cap));
}

// rows of a chunk: whole slabs
__host__ __device__ inline int64_t pca_chunk_rows(int64_t n, int64_t nrc) {
  return ((n + nrc - 1) / nrc + PC_S - 1) / PC_S * PC_S;
}

size_t pca_ws_bytes(int64_t n, int64_t d) {
  return (size_t)round_up(pca_chunks(n, d) * pca_pairs(d) * PC_TILE_BYTES, 256);
}

// macro tile `ti` of the tiles on or above the diagonal, row-major: (I, J)
__device__ inline void pca_pair(int ti, int np, int *ip, int *jp) {
  int a = 0;
  while (ti >= np - a) {
    ti -= np - a;
    ++a;
  }
  *ip = a;
  *jp = a + ti;
}

}  // namespace

// part[(rc pairs + pair) 4096 + 64 i + j] = the sum over the chunk's rows of
// a[I 64 + i] a[J 64 + j] for the 16 x 16 tiles of the pair that hold an
// element on or above the diagonal and left of column da; the others are not
// written.
template <class TX>
__global__ void __launch_bounds__(PC_B)
    k_pca_gram(const TX *__restrict__ X, int64_t n, int d, int64_t ldx,
               const double *__restrict__ pivot, int npan, int64_t nrc,
               double *__restrict__ part) {
  __shared__ double lds[2 * 2 * PC_PANEL];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int c = lane & 15, g = lane >> 4;
  const int da = d + 1;
  const int npairs = npan * (npan + 1) / 2;
  const int pair = (int)(blockIdx.x % npairs);
  const int64_t rc = blockIdx.x / npairs;
  int I, J;
  pca_pair(pair, npan, &I, &J);
  const bool diag = I == J;
  const int nP = diag ? 1 : 2;
  const int64_t per = pca_chunk_rows(n, nrc);
  const int64_t row0 = std::min(n, rc * per), row1 = std::min(n, row0 + per);
  const int ns = (int)((row1 - row0 + PC_S - 1) / PC_S);

  // staging: wave w takes rows 4 w .. 4 w + 3 of a slab, lane l row l & 3 and
  // columns (l >> 2) + 16 v of each panel: the wave's LDS store of one v is
  // 64 consecutive doubles
  const int sr = 4 * w + (lane & 3);
  int col[2][4];
  double pv[2][4];
#pragma unroll
  for (int P = 0; P < 2; ++P)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      col[P][v] = (P ? J : I) * PC_T + (lane >> 2) + 16 * v;
      pv[P][v] = col[P][v] < d ? pivot[col[P][v]] : 0.0;
    }
  double raw[2][4];
  auto load = [&](int s) {
    const int64_t row = row0 + (int64_t)s * PC_S + sr;
    const bool ok = row < row1;
    const TX *xr = X + (ok ? row : row0) * ldx;
#pragma unroll
    for (int P = 0; P < 2; ++P)
      if (P < nP) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int j = col[P][v];
          raw[P][v] = !ok ? 0.0
                      : j < d ? (double)xr[j] - pv[P][v]
                      : j == d ? 1.0 : 0.0;
        }
      }
  };
  auto store = [&](int buf) {
    double *base = lds + buf * 2 * PC_PANEL + w * PC_G + lane;
#pragma unroll
    for (int P = 0; P < 2; ++P)
      if (P < nP) {
#pragma unroll
        for (int v = 0; v < 4; ++v) base[P * PC_PANEL + 64 * v] = raw[P][v];
      }
  };

  // the tiles this wave stores: strip rows I 64 + 16 w .. + 15 against tiles t
  // of panel J.  The loop below multiplies all four tiles without a branch
  // (a conditional MFMA costs accumulator copies on every slab, and the
  // flops of a skipped tile stay below the byte floor of the slab)
  const bool wave_on = I * PC_T + 16 * w < da;
  bool ton[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
    ton[t] = wave_on && J * PC_T + 16 * t < da && (!diag || t >= w);
  f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};

  if (ns > 0) {
    load(0);
    store(0);
  }
  __syncthreads();
  for (int s = 0; s < ns; ++s) {
    const bool more = s + 1 < ns;
    if (more) load(s + 1);
    const double *As = lds + (s & 1) * 2 * PC_PANEL;
    const double *Bs = diag ? As : As + PC_PANEL;
#pragma unroll
    for (int q = 0; q < PC_S / 4; ++q) {
      const double a = As[q * PC_G + (16 * w + c) * 4 + g];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[t] = mfma(a, Bs[q * PC_G + (16 * t + c) * 4 + g], acc[t]);
    }
    if (more) store((s + 1) & 1);
    __syncthreads();
  }

  double *o = part + ((int64_t)rc * npairs + pair) * (PC_T * PC_T);
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (ton[t]) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        o[(16 * w + g + 4 * r) * PC_T + 16 * t + c] = acc[t][r];
    }
}

// G[a][b] = G[b][a] = the chunks' partials of (a <= b < da).  Thread (slice
// s = tid / 16, element tid % 16) folds chunks s, s + 16, ...; the slices are
// then added in order by the threads of slice 0.
__global__ void __launch_bounds__(PC_B)
    k_pca_gram_final(const double *__restrict__ part, int64_t nrc, int npan,
                     int d, double *__restrict__ G) {
  __shared__ double sm[PC_B];
  const int da = d + 1;
  const int64_t len = (int64_t)npan * (npan + 1) / 2 * (PC_T * PC_T);
  const int64_t e = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
  int I, J;
  pca_pair((int)(e / (PC_T * PC_T)), npan, &I, &J);
  const int el = (int)(e % (PC_T * PC_T));
  const int a = I * PC_T + el / PC_T, b = J * PC_T + el % PC_T;
  // tiles the Gram kernel skipped hold no element with a <= b < da
  const bool ok = a <= b && b < da;
  const int s = threadIdx.x >> 4;
  double v = 0.0;
  if (ok)
    for (int64_t p = s; p < nrc; p += 16) v = v + part[p * len + e];
  sm[threadIdx.x] = v;
  __syncthreads();
  if (s == 0 && ok) {
    for (int i = 1; i < 16; ++i) v = v + sm[i * 16 + threadIdx.x];
    G[(int64_t)a * da + b] = v;
    G[(int64_t)b * da + a] = v;
  }
}

// Y[row][j] = sum_f (x[row][f] - mean[f]) V[j][f], j < nc.
template <class TX>
__global__ void __launch_bounds__(PC_B)
    k_pca_project(const TX *__restrict__ X, int64_t n, int d, int64_t ldx,
                  const double *__restrict__ mean, const double *__restrict__ V,
                  int nc, double *__restrict__ Y, int64_t ldy) {
  __shared__ double lds[2 * 2 * PC_PANEL];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int c = lane & 15, g = lane >> 4;
  const int64_t rb = (int64_t)blockIdx.x * PC_T;
  const int ns = (d + PC_S - 1) / PC_S;

  // staging: element e = tid + 256 u of a 64 x 16 slab is (row or component
  // e / 16, feature e % 16): 16 consecutive features per row, 128-byte pieces
  const int sf = tid & 15, si = tid >> 4;
  const TX *xr[4];
  bool xok[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t row = rb + si + 16 * u;
    xok[u] = row < n;
    xr[u] = X + (xok[u] ? row : 0) * ldx;
  }
  double rx[4], rv[4];
  auto load = [&](int s, int j0) {
    const int f = s * PC_S + sf;
    const bool fok = f < d;
    const double m = fok ? mean[f] : 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      rx[u] = fok && xok[u] ? (double)xr[u][f] - m : 0.0;
      const int j = j0 + si + 16 * u;
      rv[u] = fok && j < nc ? V[(int64_t)j * d + f] : 0.0;
    }
  };
  auto store = [&](int buf) {
    double *base = lds + buf * 2 * PC_PANEL + (sf >> 2) * PC_G + (sf & 3);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      base[(si + 16 * u) * 4] = rx[u];
      base[PC_PANEL + (si + 16 * u) * 4] = rv[u];
    }
  };

  for (int j0 = 0; j0 < nc; j0 += PC_T) {
    f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    load(0, j0);      // the previous panel's slabs are read: its last barrier
    store(0);
    __syncthreads();
    for (int s = 0; s < ns; ++s) {
      const bool more = s + 1 < ns;
      if (more) load(s + 1, j0);
      const double *As = lds + (s & 1) * 2 * PC_PANEL;
      const double *Bs = As + PC_PANEL;
#pragma unroll
      for (int q = 0; q < PC_S / 4; ++q) {
        const double a = As[q * PC_G + (16 * w + c) * 4 + g];
#pragma unroll
        for (int t = 0; t < 4; ++t)
          acc[t] = mfma(a, Bs[q * PC_G + (16 * t + c) * 4 + g], acc[t]);
      }
      if (more) store((s + 1) & 1);
      __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = j0 + 16 * t + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = rb + 16 * w + g + 4 * r;
        if (row < n && j < nc) Y[row * ldy + j] = acc[t][r];
      }
    }
  }
}

namespace {

template <class TX>
int pca_gram(const TX *X, int64_t n, int64_t d, int64_t ldx,
             const double *pivot, void *ws, size_t ws_b, double *G,
             hipStream_t s) {
  if (!pca_shape_ok(n, d, ldx) || !X || !pivot || !G)
    return fail(DKM_E_ARG, "pca gram: bad arguments");
  if (!ws || ws_b < pca_ws_bytes(n, d))
    return fail(DKM_E_WORKSPACE, "pca gram: workspace too small");
  const int64_t nrc = pca_chunks(n, d), npan = pca_panels(d);
  const int64_t pairs = pca_pairs(d);
  if (nrc * pairs > INT32_MAX)
    return fail(DKM_E_ARG, "pca gram: too large");
  k_pca_gram<TX><<<(unsigned)(nrc * pairs), PC_B, 0, s>>>(
      X, n, (int)d, ldx, pivot, (int)npan, nrc, (double *)ws);
  if (int r = check_launch("pca gram")) return r;
  k_pca_gram_final<<<(unsigned)(pairs * (PC_T * PC_T / 16)), PC_B, 0, s>>>(
      (const double *)ws, nrc, (int)npan, (int)d, G);
  return check_launch("pca gram: final sum");
}

template <class TX>
int pca_project(const TX *X, int64_t n, int64_t d, int64_t ldx,
                const double *mean, const double *V, int64_t c, double *Y,
                int64_t ldy, hipStream_t s) {
  if (!pca_shape_ok(n, d, ldx) || c < 1 || c > DKM_PCA_MAX_D || ldy < c ||
      n >= (INT64_MAX / 16) / ldy || !X || !mean || !V || !Y)
    return fail(DKM_E_ARG, "pca project: bad arguments");
  const int64_t nb = (n + PC_T - 1) / PC_T;
  if (nb > INT32_MAX) return fail(DKM_E_ARG, "pca project: n too large");
  k_pca_project<TX><<<(unsigned)nb, PC_B, 0, s>>>(X, n, (int)d, ldx, mean, V,
                                                  (int)c, Y, ldy);
  return check_launch("pca project");
}

}  // namespace

}  // namespace dkm

using namespace dkm;

extern "C" {

size_t dkm_pca_workspace_bytes(int64_t n, int64_t d) {
  if (!pca_shape_ok(n, d, d)) return 0;
  return pca_ws_bytes(n, d);
}

int dkm_pca_gram_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                     const double *pivot, void *ws, size_t ws_bytes, double *G,
                     void *stream) {
  return pca_gram<double>(X, n, d, ldx, pivot, ws, ws_bytes, G,
                          (hipStream_t)stream);
}

int dkm_pca_gram_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                     const double *pivot, void *ws, size_t ws_bytes, double *G,
                     void *stream) {
  return pca_gram<float>(X, n, d, ldx, pivot, ws, ws_bytes, G,
                         (hipStream_t)stream);
}

int dkm_pca_project_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                        const double *mean, const double *V, int64_t c,
                        double *Y, int64_t ldy, void *stream) {
  return pca_project<double>(X, n, d, ldx, mean, V, c, Y, ldy,
                             (hipStream_t)stream);
}

int dkm_pca_project_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                        const double *mean, const double *V, int64_t c,
                        double *Y, int64_t ldy, void *stream) {
  return pca_project<float>(X, n, d, ldx, mean, V, c, Y, ldy,
                            (hipStream_t)stream);
}

}  // extern "C"

// Code-object preload (dkm_preload): see dkm_ordered.hip.
namespace dkm {
DKM_TU_FLAGS(pca, 0)
__global__ void k_tu_pca() {}
int preload_pca() {
  hipFuncAttributes a;
  const bool ok = hipFuncGetAttributes(&a, (const void *)k_tu_pca) == hipSuccess;
  return ok ? 0 : 1;
}
}  // namespace dkm
