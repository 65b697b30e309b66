// dkm_qr.hip -- tall-skinny QR (TSQR) of the implicit matrix A = [1 | X | y]
// (or [X | y]) of the resident dense samples, in ONE read of X (DESIGN.md
// 3.25): the w x w upper-triangular fp64 factor R with A^T A = R^T R, from
// which LinearRegression solves its least squares on the host without ever
// forming the normal equations.  w = d + 1 + ones <= DKM_TSQR_MAX_W.  All
// arithmetic is fp64 (fp32 rows are widened in the loads); no fast-math, no
// floating-point atomic; every grid, tile and reduction order is a function
// of (n, w) only, so the same input gives the same bits from run to run.
//
// The columns are padded to wp = 16 ceil(w / 16) (padding columns are zero
// and give tau = 0).  A workgroup of four waves keeps a running R in LDS,
// packed by block rows (block row I: 16 rows of the wp - 16 I columns from
// the diagonal block on, 72 KiB at wp = 128), and streams tiles of QR_T = 64
// rows through the structured Householder factorisation of [R; tile]:
// reflector j of a 16-column panel is [e_j; v] with v in the tile's rows
// only, so it touches row j of R and the tile and leaves R triangular.  Per
// panel p:
//
//   qr_panel   wave 0: lane (c = l & 15, g = l >> 4) holds rows g + 4 i of
//              column c of the tile's panel in registers; row j of the
//              diagonal block of R is read and written in step j only and
//              stays in LDS.  Unblocked
//              Householder, column by column: the norm and the 15 dots
//              v_j . a_c of all columns at once are 16 local products and two
//              xor shuffles over g; v_j reaches the lanes by one shuffle per
//              row.  A zero column gives tau = 0 and no division.  For c < j
//              the same dot IS v_c . v_j, so the 16 x 16 compact-WY factor
//              T (Q = I - V T V^T) grows in the same loop, row c of T on
//              lane c.  V overwrites the tile's panel.
//   qr_update  wave q of the trailing 16-column blocks: on
//              v_mfma_f64_16x16x4_f64 (lane l: A[m = c][k = g],
//              B[k = g][n = c], result register r = D[g + 4 r][c]),
//              Z = R_pq + V^T tile_q (16 steps over the 64 rows),
//              W = T^T Z (4 steps; step r takes k = g + 4 r, which IS the
//              result layout of Z, so Z never leaves the registers),
//              R_pq -= W and tile_q -= V W (4 row blocks x 4 steps, W again
//              from its registers).
//
//   k_tsqr_panel  one workgroup per contiguous row range (the ranges: a
//                 function of n); [1 | x | y] is assembled in the load
//                 (the ones and y columns never exist in HBM), rows past the
//                 range are zero rows, and the global loads of tile t + 1 are
//                 issued into registers before tile t is factored.  The R of
//                 the range goes to the workspace as a full wp x wp matrix.
//   k_tsqr_merge  a workgroup stacks up to QR_FAN of those Rs, in range
//                 order, through the same routine (an R is a 'tile' of wp
//                 rows, 64 at a time); the levels repeat until one R is left,
//                 whose rows are negated where the diagonal is negative.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "dkm_internal.h"

namespace dkm {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int QR_B = 256;        // threads per block: four waves
constexpr int QR_T = 64;         // rows of a tile
constexpr int QR_P = 16;         // columns of a panel
constexpr int QR_PAD = 4;        // tile row stride wp + 4: 2-way banks at most
constexpr int QR_RANGE = 2048;   // rows of a range, at least
constexpr int QR_RANGES = 512;   // ranges, at most
constexpr int QR_FAN = 8;        // Rs one merge workgroup stacks
constexpr int QR_RAW = 4 * (DKM_TSQR_MAX_W / QR_P);  // prefetched per thread
static_assert(QR_B == 4 * WAVE && QR_T * QR_P == 4 * QR_B && QR_P == 16,
              "four elements per thread and panel of a tile");

__device__ inline f64x4 mfma(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

__host__ __device__ inline int qr_wp(int w) {
  return (w + QR_P - 1) / QR_P * QR_P;
}

// packed R: doubles before block row I
__host__ __device__ inline int qr_roff(int I, int wp) {
  return 16 * (I * wp - 8 * I * (I - 1));
}

__host__ __device__ inline int qr_lds_doubles(int wp) {
  return qr_roff(wp / QR_P, wp) + QR_T * (wp + QR_PAD) + QR_P * QR_P;
}

bool qr_shape_ok(int64_t n, int64_t d, int64_t ldx, int ones) {
  return n >= 1 && d >= 1 && (ones == 0 || ones == 1) &&
         d + 1 + ones <= DKM_TSQR_MAX_W && ldx >= d &&
         n < (INT64_MAX / 16) / ldx;
}

// Row ranges: a function of n only.
int64_t qr_ranges(int64_t n) {
  return std::max<int64_t>(
      1, std::min<int64_t>((n + QR_RANGE - 1) / QR_RANGE, QR_RANGES));
}

// rows of a range: whole tiles
int64_t qr_range_rows(int64_t n, int64_t nr) {
  return ((n + nr - 1) / nr + QR_T - 1) / QR_T * QR_T;
}

// the ranges' Rs, then the Rs of the first merge level (the levels alternate
// between the two)
size_t qr_ws_bytes(int64_t n, int64_t w) {
  const int64_t nr = qr_ranges(n), wp = qr_wp((int)w);
  return (size_t)round_up((nr + (nr + QR_FAN - 1) / QR_FAN) * wp * wp * 8,
                          256);
}

// Wave 0: Householder on [diagonal block of R; the tile's panel], V into the
// panel, T into tf (tf[16 i + j] = T[i][j]).  Rp: the diagonal block, row
// stride rs; tl: the panel's first column, row stride ld.  Row j of R is read
// and written in step j only, and row c of T only by lane c (g = 0), so both
// stay in LDS.
__device__ __forceinline__ void qr_panel(double *Rp, int rs, double *tl,
                                         int ld, double *tf, int lane) {
  const int c = lane & 15, g = lane >> 4;
  double x[16], vv[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = tl[(g + 4 * i) * ld + c];
#pragma unroll 1
  for (int j = 0; j < 16; ++j) {
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) ss = ss + x[i] * x[i];
    ss = ss + __shfl_xor(ss, 16);
    ss = ss + __shfl_xor(ss, 32);
    const double xn2 = __shfl(ss, j);
    const double alpha = Rp[j * rs + j], rjc = Rp[j * rs + c];
    // a zero column below the diagonal: H = I (tau = 0, v = 0), no division
    double tau = 0.0, beta = alpha, scale = 1.0;
    if (xn2 != 0.0) {
      beta = -copysign(sqrt(alpha * alpha + xn2), alpha);
      tau = (beta - alpha) / beta;
      scale = 1.0 / (alpha - beta);
    }
    if (c == j) {
#pragma unroll
      for (int i = 0; i < 16; ++i) x[i] = x[i] * scale;
    }
    double dot = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      vv[i] = __shfl(x[i], (lane & 48) | j);
      dot = dot + vv[i] * x[i];
    }
    dot = dot + __shfl_xor(dot, 16);
    dot = dot + __shfl_xor(dot, 32);
    // c > j: v_j . (column c); c < j: v_c . v_j, an entry of V^T V
    const double ts = tau * (rjc + dot);
    if (c > j) {
#pragma unroll
      for (int i = 0; i < 16; ++i) x[i] = x[i] - ts * vv[i];
    }
    if (g == 0 && c >= j) Rp[j * rs + c] = c == j ? beta : rjc - ts;
    // T[0:j, j] = -tau T[0:j, 0:j] (V^T v_j)[0:j]; T[j][j] = tau: lane c adds
    // to row c of T (zero left of the diagonal, and at and below row j)
    double acc = 0.0;
#pragma unroll 1
    for (int k = 0; k < j; ++k) {
      const double gk = __shfl(dot, k);
      if (g == 0) acc = acc + tf[c * 16 + k] * gk;
    }
    if (g == 0) tf[c * 16 + j] = c == j ? tau : -tau * acc;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) tl[(g + 4 * i) * ld + c] = x[i];
}

// One wave: apply the panel (V at `V`, T in tf) to the trailing block whose
// part of R is Rq (row stride rs) and whose tile columns start at C.
__device__ __forceinline__ void qr_update(double *Rq, int rs, const double *V,
                                          double *C, int ld, const double *tf,
                                          int lane) {
  const int c = lane & 15, g = lane >> 4;
  f64x4 r0, z, wm = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int r = 0; r < 4; ++r) r0[r] = Rq[(g + 4 * r) * rs + c];
  z = r0;
#pragma unroll
  for (int s = 0; s < QR_T / 4; ++s)
    z = mfma(V[(4 * s + g) * ld + c], C[(4 * s + g) * ld + c], z);
#pragma unroll
  for (int r = 0; r < 4; ++r) wm = mfma(tf[(g + 4 * r) * 16 + c], z[r], wm);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    Rq[(g + 4 * r) * rs + c] = r0[r] - wm[r];
    wm[r] = -wm[r];
  }
#pragma unroll
  for (int b = 0; b < QR_T / 16; ++b) {
    f64x4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = C[(16 * b + g + 4 * r) * ld + c];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      acc = mfma(V[(16 * b + c) * ld + g + 4 * r], wm[r], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) C[(16 * b + g + 4 * r) * ld + c] = acc[r];
  }
}

// The block: [R; tile] <- its R factor (the tile is left holding reflectors).
// Ends with a barrier.
__device__ __forceinline__ void qr_factor(double *R, double *tile, double *tf,
                                          int wp) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int np = wp / QR_P, ld = wp + QR_PAD;
  for (int p = 0; p < np; ++p) {
    double *Rp = R + qr_roff(p, wp);
    const int rs = wp - QR_P * p;
    if (wv == 0) qr_panel(Rp, rs, tile + QR_P * p, ld, tf, lane);
    __syncthreads();
    for (int q = p + 1 + wv; q < np; q += QR_B / WAVE)
      qr_update(Rp + QR_P * (q - p), rs, tile + QR_P * p, tile + QR_P * q, ld,
                tf, lane);
    __syncthreads();
  }
}

// Stream nt tiles through the running R.  elem(t, r, col): entry (row r of
// tile t, column col < wp).  Thread tid takes rows (tid >> 4) + 16 v, v < 4,
// of column 16 P + (tid & 15) of every panel P: 128-byte pieces of a row.
template <class ELEM>
__device__ __forceinline__ void qr_stream(double *sm, int wp, int64_t nt,
                                          const ELEM &elem) {
  const int tid = threadIdx.x, np = wp / QR_P, ld = wp + QR_PAD;
  double *R = sm, *tile = R + qr_roff(np, wp), *tf = tile + QR_T * ld;
  for (int e = tid; e < qr_roff(np, wp); e += QR_B) R[e] = 0.0;
  double raw[QR_RAW];
  auto load = [&](int64_t t) {
#pragma unroll
    for (int u = 0; u < QR_RAW; ++u)
      if ((u >> 2) < np)
        raw[u] = elem(t, (tid >> 4) + 16 * (u & 3),
                      QR_P * (u >> 2) + (tid & 15));
  };
  if (nt > 0) load(0);
  __syncthreads();
  for (int64_t t = 0; t < nt; ++t) {
#pragma unroll
    for (int u = 0; u < QR_RAW; ++u)
      if ((u >> 2) < np)
        tile[((tid >> 4) + 16 * (u & 3)) * ld + QR_P * (u >> 2) + (tid & 15)] =
            raw[u];
    __syncthreads();
    if (t + 1 < nt) load(t + 1);   // in flight while tile t is factored
    qr_factor(R, tile, tf, wp);
  }
}

// entry (i, j) of the packed R, j at or right of row i's diagonal block
__device__ inline double qr_r_at(const double *R, int wp, int i, int j) {
  const int I = i >> 4;
  return R[qr_roff(I, wp) + (i & 15) * (wp - QR_P * I) + j - QR_P * I];
}

// the packed R as a full wp x wp matrix (zero left of the diagonal blocks;
// the diagonal blocks hold their own zeros)
__device__ void qr_write_full(const double *R, int wp, double *out) {
  for (int e = threadIdx.x; e < wp * wp; e += QR_B) {
    const int i = e / wp, j = e % wp;
    out[e] = j >= (i & ~15) ? qr_r_at(R, wp, i, j) : 0.0;
  }
}

}  // namespace

// ws[range] <- the R of rows [range per, (range + 1) per) of A.
template <class TX>
__global__ void __launch_bounds__(QR_B)
    k_tsqr_panel(const TX *__restrict__ X, const double *__restrict__ y,
                 int64_t n, int d, int64_t ldx, int ones, int wp, int64_t per,
                 double *__restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) double qr_sm[];
  const int64_t row0 = std::min(n, (int64_t)blockIdx.x * per);
  const int64_t row1 = std::min(n, row0 + per);
  const int64_t nt = (row1 - row0 + QR_T - 1) / QR_T;
  auto elem = [&](int64_t t, int r, int col) -> double {
    const int64_t row = row0 + t * QR_T + r;
    const int j = col - ones;
    if (row >= row1 || j > d) return 0.0;
    if (j < 0) return 1.0;
    return j < d ? (double)X[row * ldx + j] : y[row];
  };
  qr_stream(qr_sm, wp, nt, elem);
  qr_write_full(qr_sm, wp, ws + (int64_t)blockIdx.x * wp * wp);
}

// dst[block] <- the R of src[block QR_FAN .. + QR_FAN) stacked (cnt in all),
// as a full wp x wp matrix; last != 0 (one block): dst is the w x w result,
// its diagonal non-negative.
__global__ void __launch_bounds__(QR_B)
    k_tsqr_merge(const double *__restrict__ src, int cnt, int wp, int w,
                 int last, double *__restrict__ dst) {
  extern __shared__ __attribute__((aligned(16))) double qr_sm[];
  const int k0 = blockIdx.x * QR_FAN, k1 = std::min(cnt, k0 + QR_FAN);
  const int nch = (wp + QR_T - 1) / QR_T;
  auto elem = [&](int64_t t, int r, int col) -> double {
    const int k = k0 + (int)(t / nch), row = (int)(t % nch) * QR_T + r;
    // row `row` of an R is zero left of its diagonal
    return row < wp && col >= row ? src[((int64_t)k * wp + row) * wp + col]
                                  : 0.0;
  };
  qr_stream(qr_sm, wp, (int64_t)(k1 - k0) * nch, elem);
  if (!last) {
    qr_write_full(qr_sm, wp, dst + (int64_t)blockIdx.x * wp * wp);
    return;
  }
  for (int e = threadIdx.x; e < w * w; e += QR_B) {
    const int i = e / w, j = e % w;
    double v = 0.0;
    if (j >= i) {
      v = qr_r_at(qr_sm, wp, i, j);
      if (qr_r_at(qr_sm, wp, i, i) < 0.0) v = -v;
    }
    dst[e] = v;
  }
}

namespace {

template <class TX>
int tsqr(const TX *X, int64_t n, int64_t d, int64_t ldx, const double *y,
         int ones, void *ws, size_t ws_b, double *R, hipStream_t s) {
  if (!qr_shape_ok(n, d, ldx, ones) || !X || !y || !R)
    return fail(DKM_E_ARG, "tsqr: bad arguments");
  const int w = (int)d + 1 + ones, wp = qr_wp(w);
  if (!ws || ws_b < qr_ws_bytes(n, w))
    return fail(DKM_E_WORKSPACE, "tsqr: workspace too small");
  const int64_t nr = qr_ranges(n), per = qr_range_rows(n, nr);
  const int lds = qr_lds_doubles(wp) * 8;
  if (hipFuncSetAttribute((const void *)k_tsqr_panel<TX>,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          lds) != hipSuccess ||
      hipFuncSetAttribute((const void *)k_tsqr_merge,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          lds) != hipSuccess)
    return fail(DKM_E_LAUNCH, "tsqr: LDS attribute");
  double *a = (double *)ws, *b = a + nr * wp * wp;
  k_tsqr_panel<TX><<<(unsigned)nr, QR_B, lds, s>>>(X, y, n, (int)d, ldx, ones,
                                                   wp, per, a);
  if (int r = check_launch("tsqr panel")) return r;
  for (int cnt = (int)nr;;) {
    const int nb = (cnt + QR_FAN - 1) / QR_FAN;
    k_tsqr_merge<<<(unsigned)nb, QR_B, lds, s>>>(a, cnt, wp, w, nb == 1,
                                                 nb == 1 ? R : b);
    if (int r = check_launch("tsqr merge")) return r;
    if (nb == 1) return 0;
    std::swap(a, b);
    cnt = nb;
  }
}

}  // namespace

}  // namespace dkm

using namespace dkm;

extern "C" {

size_t dkm_tsqr_workspace_bytes(int64_t n, int64_t w) {
  if (n < 1 || w < 2 || w > DKM_TSQR_MAX_W) return 0;
  return qr_ws_bytes(n, w);
}

int dkm_tsqr_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                 const double *y, int ones, void *ws, size_t ws_bytes,
                 double *R, void *stream) {
  return tsqr<double>(X, n, d, ldx, y, ones, ws, ws_bytes, R,
                      (hipStream_t)stream);
}

int dkm_tsqr_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                 const double *y, int ones, void *ws, size_t ws_bytes,
                 double *R, void *stream) {
  return tsqr<float>(X, n, d, ldx, y, ones, ws, ws_bytes, R,
                     (hipStream_t)stream);
}

}  // extern "C"

// Code-object preload (dkm_preload): see dkm_ordered.hip.
namespace dkm {
DKM_TU_FLAGS(qr, 0)
__global__ void k_tu_qr() {}
int preload_qr() {
  hipFuncAttributes a;
  const bool ok = hipFuncGetAttributes(&a, (const void *)k_tu_qr) == hipSuccess;
  return ok ? 0 : 1;
}
}  // namespace dkm
