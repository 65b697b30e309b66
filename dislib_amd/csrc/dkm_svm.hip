// dkm_svm.hip -- the kernels of CascadeSVM (binary C-SVC, reference
// dislib/classification/csvm/base.py, whose nodes run libsvm): kernel-matrix
// rows of a node, working-set selection, the local SMO solver, the update of
// the optimality vector, decision values and the reference's convergence
// quantity W.  A node is an index list into the resident samples: no sample
// row is copied.  All arithmetic is fp64; fp32 rows are widened in the loads.
// No fast-math, no floating-point atomic, no grid-wide barrier: every sum has
// an order that depends on the shapes only, so the same input gives the same
// bits from run to run, and every loop has a bound known at launch.
//
// The solver state of a node of m rows is alpha[m] and f[m] with
// f_i = y_i * (dual gradient)_i = sum_j alpha_j y_j K_ij - y_i, so that
// libsvm's -y_i G_i is -f_i, and an update of alpha is f += K^T (y o dalpha).
//
//   k_svm_norms   one thread per row: ||x||^2 as an fma chain over the row.
//   k_svm_panel   dot products of up to SV_TA "A" rows with a panel of SV_TB
//                 "B" rows per block on v_mfma_f64_16x16x4_f64.  Both
//                 operands are staged in LDS SV_DK features at a time (layout
//                 [k / 4][row][k % 4]: a wave's operand read is 64 consecutive
//                 doubles); a wave owns 16 B rows and keeps one accumulator
//                 per 16-row A tile in registers across all feature chunks.
//                 Operands A[i = c][k = g], B[k = g][j = c], lane = 16 g + c,
//                 result register r = D[g + 4 r][c].  Epilogue, MODE 0: the
//                 kernel values K[a][j] (linear: the dot; rbf: exp(-gamma
//                 (|a|^2 + |b|^2 - 2 dot))) are stored.  MODE 1: the A rows
//                 are walked SV_TA at a time and out[j] = sum_a w_a K(a, j)
//                 + bias, every lane adding its rows in ascending order and
//                 the four row groups folded in a fixed order.
//   k_svm_select  one block.  Every thread keeps the best of its own strided
//                 positions; a round takes the block's best of I_up (largest
//                 -f, ties to the lower position), marks it, then the best of
//                 I_low (smallest -f) among the unmarked, q / 2 rounds.  The
//                 first reduction, before any mark, gives m(alpha) - M(alpha).
//   k_svm_local   one block loads the q x q block of K and the working set's
//                 state; its first wave then runs SMO with libsvm's
//                 second-order pair selection, two positions per lane, the
//                 block in LDS, alpha / f / y in registers.
//   k_svm_update  one thread per node row: f_j += sum_t K[t][j] dy[t], t
//                 ascending (terms with dy[t] == 0 skipped).
//   k_svm_w       W = -0.5 sum_j (c_j l_j) t_j + sum_j c_j in a fixed tree.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>

#include "dkm_internal.h"

namespace dkm {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int SV_B = 256;                 // threads per block
constexpr int SV_TA = DKM_SVM_QMAX;       // A rows per batch (8 MFMA tiles)
constexpr int SV_NT = SV_TA / 16;
constexpr int SV_TB = 64;                 // B rows per block: 16 per wave
constexpr int SV_DK = 16;                 // features staged per step
constexpr int SV_AG = SV_TA * 4 + 16;     // doubles per 4-feature group of A
constexpr int SV_BG = SV_TB * 4 + 16;
constexpr int SEL_B = 1024;               // threads of k_svm_select
constexpr double SV_TAU = 1e-12;          // libsvm's TAU
static_assert(SV_TA % 16 == 0 && SV_TA == 128, "eight A tiles per batch");
// the local solver's q x q block: 128 KiB of the 160 KiB of LDS
static_assert((size_t)DKM_SVM_QMAX * DKM_SVM_QMAX * sizeof(double) <=
                  150 * 1024, "LDS budget");

}  // namespace

template <class TX>
__global__ void __launch_bounds__(SV_B)
    k_svm_norms(const TX *__restrict__ X, int64_t n, int d, int64_t ldx,
                double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * SV_B + threadIdx.x;
  if (i >= n) return;
  const TX *x = X + i * ldx;
  double s = 0.0;
  for (int t = 0; t < d; ++t) {
    const double v = (double)x[t];
    s = fma(v, v, s);
  }
  out[i] = s;
}

// See the header comment.  aidx / asub: A row a is row aidx[asub[a]] of A
// (asub given; a negative asub[a] is an empty slot) or aidx[a]; an index
// outside [0, an_rows) reads as a row of zeros with norm 0.  bidx: B row j is
// row bidx[j] of B, or row j.
template <class TA, class TB, int MODE>
__global__ void __launch_bounds__(SV_B)
    k_svm_panel(const TA *__restrict__ A, int64_t an_rows, int64_t lda,
                const int32_t *__restrict__ aidx,
                const int32_t *__restrict__ asub, int64_t asub_n, int na,
                const TB *__restrict__ B, int64_t bn_rows, int64_t ldb,
                const int32_t *__restrict__ bidx, int64_t nb, int d,
                const double *__restrict__ anorm,
                const double *__restrict__ bnorm, int rbf, double gamma,
                double *__restrict__ K, int64_t ldk,
                const double *__restrict__ wa, const double *__restrict__ wb,
                double bias, double *__restrict__ out) {
  __shared__ double As[(SV_DK / 4) * SV_AG];
  __shared__ double Bs[(SV_DK / 4) * SV_BG];
  __shared__ double an_s[SV_TA], wt_s[SV_TA];
  __shared__ int64_t ai_s[SV_TA], bj_s[SV_TB];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int c = lane & 15, g = lane >> 4;
  const int64_t jb0 = (int64_t)blockIdx.x * SV_TB;
  const int64_t jb = jb0 + w * 16 + c;

  if (tid < SV_TB) {
    const int64_t j = jb0 + tid;
    int64_t r = -1;
    if (j < nb) {
      r = bidx ? (int64_t)bidx[j] : j;
      if (r < 0 || r >= bn_rows) r = -1;
    }
    bj_s[tid] = r;
  }
  __syncthreads();
  double bn = 0.0;
  if (rbf && bj_s[w * 16 + c] >= 0) bn = bnorm[bj_s[w * 16 + c]];

  double part = 0.0;
  for (int a0 = 0; a0 < na; a0 += SV_TA) {
    const int nab = std::min(SV_TA, na - a0);   // A rows of this batch
    const int nt = (nab + 15) / 16;
    __syncthreads();                            // the previous batch is read
    if (tid < SV_TA) {
      int64_t r = -1;
      if (tid < nab) {
        if (asub) {
          const int64_t p = asub[a0 + tid];
          r = (p >= 0 && p < asub_n) ? (int64_t)aidx[p] : -1;
        } else {
          r = aidx[a0 + tid];
        }
        if (r < 0 || r >= an_rows) r = -1;
      }
      ai_s[tid] = r;
      an_s[tid] = (rbf && r >= 0) ? anorm[r] : 0.0;
      if (MODE == 1) {
        double wv = 0.0;
        if (tid < nab) {
          wv = wa[a0 + tid];
          if (wb) wv = wv * wb[a0 + tid];
        }
        wt_s[tid] = wv;
      }
    }
    f64x4 acc[SV_NT];
#pragma unroll
    for (int t = 0; t < SV_NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};

    for (int k0 = 0; k0 < d; k0 += SV_DK) {
      __syncthreads();                          // ai_s; the last chunk is read
#pragma unroll
      for (int u = 0; u < SV_TA * SV_DK / SV_B; ++u) {
        const int e = tid + SV_B * u, i = e / SV_DK, kk = e % SV_DK;
        double v = 0.0;
        if (i < nt * 16) {
          const int64_t r = ai_s[i];
          if (r >= 0 && k0 + kk < d) v = (double)A[r * lda + k0 + kk];
          As[(kk >> 2) * SV_AG + i * 4 + (kk & 3)] = v;
        }
      }
#pragma unroll
      for (int u = 0; u < SV_TB * SV_DK / SV_B; ++u) {
        const int e = tid + SV_B * u, j = e / SV_DK, kk = e % SV_DK;
        const int64_t r = bj_s[j];
        double v = 0.0;
        if (r >= 0 && k0 + kk < d) v = (double)B[r * ldb + k0 + kk];
        Bs[(kk >> 2) * SV_BG + j * 4 + (kk & 3)] = v;
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < SV_DK / 4; ++ks) {
        const double b = Bs[ks * SV_BG + (w * 16 + c) * 4 + g];
#pragma unroll
        for (int t = 0; t < SV_NT; ++t) {
          if (t < nt) {
            const double a = As[ks * SV_AG + (t * 16 + c) * 4 + g];
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0,
                                                          0);
          }
        }
      }
    }
    if (d <= 0) __syncthreads();                // ai_s, an_s, wt_s

#pragma unroll
    for (int t = 0; t < SV_NT; ++t) {
      if (t < nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ia = t * 16 + g + 4 * r;
          double v = acc[t][r];
          if (rbf) {
            const double d2 = (an_s[ia] + bn) - 2.0 * v;
            v = exp(-gamma * d2);
          }
          if (MODE == 0) {
            if (ia < nab && jb < nb) K[(int64_t)(a0 + ia) * ldk + jb] = v;
          } else {
            if (ia < nab) part = fma(wt_s[ia], v, part);
          }
        }
      }
    }
  }
  if (MODE == 1) {
    const double p0 = __shfl(part, c), p1 = __shfl(part, 16 + c);
    const double p2 = __shfl(part, 32 + c), p3 = __shfl(part, 48 + c);
    const double tot = ((p0 + p1) + p2) + p3;
    if (g == 0 && jb < nb) out[jb] = tot + bias;
  }
}

namespace {

// (value, position): the larger value wins, ties go to the lower position;
// "none" is (-inf, INT_MAX).
__device__ inline void best_of(double &v, int &i, double ov, int oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

__device__ inline void wave_best(double &v, int &i) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(i, off);
    best_of(v, i, ov, oi);
  }
}

__device__ inline bool in_up(double y, double a, double C) {
  return y > 0.0 ? a < C : a > 0.0;
}
__device__ inline bool in_low(double y, double a, double C) {
  return y > 0.0 ? a > 0.0 : a < C;
}

}  // namespace

__global__ void __launch_bounds__(SEL_B)
    k_svm_select(const double *__restrict__ f, const double *__restrict__ alpha,
                 const double *__restrict__ y, int m, double C, int q,
                 int32_t *__restrict__ ws, double *__restrict__ gap,
                 int32_t *__restrict__ mark) {
  __shared__ double sv[SEL_B / WAVE];
  __shared__ int si[SEL_B / WAVE];
  __shared__ double rv;
  __shared__ int ri;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const double ninf = -__builtin_inf();

  // the block's best of (v, i), the same in every thread
  auto block_best = [&](double v, int i, double &bv, int &bi) {
    wave_best(v, i);
    if (lane == 0) {
      sv[w] = v;
      si[w] = i;
    }
    __syncthreads();
    if (w == 0) {
      double v2 = lane < SEL_B / WAVE ? sv[lane] : ninf;
      int i2 = lane < SEL_B / WAVE ? si[lane] : INT_MAX;
      wave_best(v2, i2);
      if (lane == 0) {
        rv = v2;
        ri = i2;
      }
    }
    __syncthreads();
    bv = rv;
    bi = ri;
    __syncthreads();
  };

  double uv, lv;
  int ui, li;
  // this thread's best unmarked positions of I_up (by -f) and I_low (by f)
  auto scan = [&](bool use_mark) {
    uv = ninf;
    lv = ninf;
    ui = INT_MAX;
    li = INT_MAX;
    for (int p = tid; p < m; p += SEL_B) {
      if (use_mark && mark[p]) continue;
      const double fp = f[p], a = alpha[p], yp = y[p];
      if (in_up(yp, a, C)) best_of(uv, ui, -fp, p);
      if (in_low(yp, a, C)) best_of(lv, li, fp, p);
    }
  };

  scan(false);
  double bu, bl;
  int iu, il;
  block_best(uv, ui, bu, iu);
  block_best(lv, li, bl, il);
  if (tid == 0) {
    const bool ok = iu != INT_MAX && il != INT_MAX;
    gap[0] = ok ? bu + bl : ninf;       // m(alpha) - M(alpha)
    gap[1] = bu;                        // m(alpha)
    gap[2] = -bl;                       // M(alpha)
  }
  if (q >= m) {                         // the whole node
    for (int a = tid; a < q; a += SEL_B) ws[a] = a < m ? a : -1;
    return;
  }
  for (int p = tid; p < m; p += SEL_B) mark[p] = 0;
  const int hq = q / 2;
  for (int r = 0; r < hq; ++r) {
    if (r > 0) block_best(uv, ui, bu, iu);
    if (iu != INT_MAX && iu % SEL_B == tid) {
      mark[iu] = 1;
      scan(true);
    }
    if (tid == 0) ws[r] = iu != INT_MAX ? iu : -1;
    block_best(lv, li, bl, il);
    if (il != INT_MAX && il % SEL_B == tid) {
      mark[il] = 1;
      scan(true);
    }
    if (tid == 0) ws[hq + r] = il != INT_MAX ? il : -1;
  }
  if (tid == 0 && (q & 1)) ws[q - 1] = -1;
}

// info[0] = SMO steps taken, info[1] = 1 when the step bound ended the loop.
__global__ void __launch_bounds__(SV_B)
    k_svm_local(const double *__restrict__ K, int64_t ldk,
                const int32_t *__restrict__ ws, int q,
                const double *__restrict__ y, double *__restrict__ alpha,
                const double *__restrict__ f, int m, double C, double eps,
                int max_inner, double *__restrict__ dy,
                int32_t *__restrict__ info) {
  extern __shared__ double Kb[];          // q x q
  const int tid = threadIdx.x;
  for (int e = tid; e < q * q; e += SV_B) {
    const int i = e / q, j = e % q;
    const int pi = ws[i], pj = ws[j];
    Kb[e] = (pi >= 0 && pi < m && pj >= 0 && pj < m)
                ? K[(int64_t)i * ldk + pj] : 0.0;
  }
  __syncthreads();
  if (tid >= WAVE) return;
  const int lane = tid;
  const double ninf = -__builtin_inf();

  // positions t = lane and lane + 64 of the working set
  int pos[2];
  bool ok[2];
  double a[2], a0[2], fv[2], yv[2], kd[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int t = lane + 64 * e;
    pos[e] = t < q ? ws[t] : -1;
    ok[e] = pos[e] >= 0 && pos[e] < m;
    a[e] = ok[e] ? alpha[pos[e]] : 0.0;
    fv[e] = ok[e] ? f[pos[e]] : 0.0;
    yv[e] = ok[e] ? y[pos[e]] : 0.0;
    kd[e] = ok[e] ? Kb[t * q + t] : 0.0;
    a0[e] = a[e];
  }
  // the value that working-set position t holds, in every lane
  auto fetch = [&](const double (&v)[2], int t) {
    const double s = (t >> 6) ? v[1] : v[0];
    return __shfl(s, t & 63);
  };

  int it = 0, capped = 1;
  for (; it < max_inner; ++it) {
    // i: the most violating of I_up
    double gv = ninf;
    int i = INT_MAX;
#pragma unroll
    for (int e = 0; e < 2; ++e)
      if (ok[e] && in_up(yv[e], a[e], C)) best_of(gv, i, -fv[e], lane + 64 * e);
    wave_best(gv, i);
    if (i == INT_MAX) {
      capped = 0;
      break;
    }
    const double kii = Kb[i * q + i];
    // j: the largest second-order gain among I_low below i's level
    double g2 = ninf, ov = ninf;
    int j = INT_MAX;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int t = lane + 64 * e;
      if (ok[e] && in_low(yv[e], a[e], C)) {
        g2 = fv[e] > g2 ? fv[e] : g2;
        const double gd = gv + fv[e];
        if (gd > 0.0) {
          double quad = (kii + kd[e]) - 2.0 * Kb[i * q + t];
          if (!(quad > 0.0)) quad = SV_TAU;
          best_of(ov, j, gd * gd / quad, t);
        }
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double o = __shfl_xor(g2, off);
      g2 = o > g2 ? o : g2;
    }
    wave_best(ov, j);
    if (!(gv + g2 >= eps) || j == INT_MAX) {
      capped = 0;
      break;
    }
    // libsvm's two-variable update (Solver::Solve), Ci = Cj = C
    const double yi = fetch(yv, i), yj = fetch(yv, j);
    const double Gi = yi * fetch(fv, i), Gj = yj * fetch(fv, j);
    const double oai = fetch(a, i), oaj = fetch(a, j);
    double ai = oai, aj = oaj;
    double quad = (kii + Kb[j * q + j]) - 2.0 * Kb[i * q + j];
    if (!(quad > 0.0)) quad = SV_TAU;
    if (yi != yj) {
      const double delta = (-Gi - Gj) / quad;
      const double diff = ai - aj;
      ai = ai + delta;
      aj = aj + delta;
      if (diff > 0.0) {
        if (aj < 0.0) {
          aj = 0.0;
          ai = diff;
        }
      } else {
        if (ai < 0.0) {
          ai = 0.0;
          aj = -diff;
        }
      }
      if (diff > 0.0) {                 // diff > Ci - Cj = 0
        if (ai > C) {
          ai = C;
          aj = C - diff;
        }
      } else {
        if (aj > C) {
          aj = C;
          ai = C + diff;
        }
      }
    } else {
      const double delta = (Gi - Gj) / quad;
      const double sum = ai + aj;
      ai = ai - delta;
      aj = aj + delta;
      if (sum > C) {
        if (ai > C) {
          ai = C;
          aj = sum - C;
        }
      } else {
        if (aj < 0.0) {
          aj = 0.0;
          ai = sum;
        }
      }
      if (sum > C) {
        if (aj > C) {
          aj = C;
          ai = sum - C;
        }
      } else {
        if (ai < 0.0) {
          ai = 0.0;
          aj = sum;
        }
      }
    }
    ai = fmin(fmax(ai, 0.0), C);
    aj = fmin(fmax(aj, 0.0), C);
    const double ci = yi * (ai - oai), cj = yj * (aj - oaj);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int t = lane + 64 * e;
      if (t == i) a[e] = ai;
      if (t == j) a[e] = aj;
      if (ok[e]) {
        fv[e] = fma(Kb[i * q + t], ci, fv[e]);
        fv[e] = fma(Kb[j * q + t], cj, fv[e]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int t = lane + 64 * e;
    if (t < q) dy[t] = ok[e] ? yv[e] * (a[e] - a0[e]) : 0.0;
    if (ok[e]) alpha[pos[e]] = a[e];
  }
  if (lane == 0) {
    info[0] = it;
    info[1] = capped;
  }
}

__global__ void __launch_bounds__(SV_B)
    k_svm_update(const double *__restrict__ K, int64_t ldk, int q,
                 const double *__restrict__ dy, double *__restrict__ f,
                 int64_t m) {
  __shared__ double dys[DKM_SVM_QMAX];
  if ((int)threadIdx.x < q) dys[threadIdx.x] = dy[threadIdx.x];
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * SV_B + threadIdx.x;
  if (j >= m) return;
  double s = f[j];
  for (int t = 0; t < q; ++t) {
    const double v = dys[t];
    if (v != 0.0) s = fma(K[(int64_t)t * ldk + j], v, s);
  }
  f[j] = s;
}

// W = -0.5 sum_j (c_j l_j) t_j + sum_j c_j: thread t folds j = t, t + SV_B,
// ...; a tree over the threads then.
__global__ void __launch_bounds__(SV_B)
    k_svm_w(const double *__restrict__ coef, const double *__restrict__ lab,
            const double *__restrict__ tv, int64_t ns,
            double *__restrict__ W) {
  __shared__ double sm[2][SV_B];
  double s = 0.0, cs = 0.0;
  for (int64_t j = threadIdx.x; j < ns; j += SV_B) {
    s = fma(coef[j] * lab[j], tv[j], s);
    cs = cs + coef[j];
  }
  sm[0][threadIdx.x] = s;
  sm[1][threadIdx.x] = cs;
  __syncthreads();
  for (int h = SV_B / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      sm[0][threadIdx.x] = sm[0][threadIdx.x] + sm[0][threadIdx.x + h];
      sm[1][threadIdx.x] = sm[1][threadIdx.x] + sm[1][threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) W[0] = -0.5 * sm[0][0] + sm[1][0];
}

namespace {

bool kernel_ok(int kernel, double gamma, const double *n1, const double *n2) {
  if (kernel == DKM_SVM_LINEAR) return true;
  return kernel == DKM_SVM_RBF && gamma == gamma && n1 && n2;
}

template <class TX>
int svm_norms(const TX *X, int64_t n, int64_t d, int64_t ldx, double *out,
              hipStream_t s) {
  if (n < 0 || n > INT32_MAX || d < 1 || d > INT32_MAX || ldx < d ||
      (n > 0 && (!X || !out)))
    return fail(DKM_E_ARG, "svm norms: bad arguments");
  if (n == 0) return 0;
  k_svm_norms<TX><<<(unsigned)((n + SV_B - 1) / SV_B), SV_B, 0, s>>>(
      X, n, (int)d, ldx, out);
  return check_launch("svm norms");
}

template <class TX>
int svm_rows(const TX *X, int64_t n, int64_t d, int64_t ldx,
             const int32_t *rows, int64_t m, const int32_t *ws, int64_t q,
             const double *norms, int kernel, double gamma, double *K,
             int64_t ldk, hipStream_t s) {
  if (n < 1 || n > INT32_MAX || d < 1 || d > INT32_MAX || ldx < d || !X ||
      !rows || m < 1 || m > INT32_MAX || !ws || q < 1 || q > DKM_SVM_QMAX ||
      !K || ldk < m || !kernel_ok(kernel, gamma, norms, norms))
    return fail(DKM_E_ARG, "svm rows: bad arguments");
  k_svm_panel<TX, TX, 0><<<(unsigned)((m + SV_TB - 1) / SV_TB), SV_B, 0, s>>>(
      X, n, ldx, rows, ws, m, (int)q, X, n, ldx, rows, m, (int)d, norms, norms,
      kernel == DKM_SVM_RBF, gamma, K, ldk, nullptr, nullptr, 0.0, nullptr);
  return check_launch("svm rows");
}

// out[j] = sum_s wa[s] (wb ? wb[s] : 1) K(x_sv[s], b_j) + bias
template <class TX, class TQ>
int svm_sum(const TX *X, int64_t n, int64_t ldx, const int32_t *sv,
            int64_t ns, const TQ *Q, int64_t qn, int64_t ldq,
            const int32_t *qidx, int64_t nq, int64_t d, const double *wa,
            const double *wb, double bias, const double *xnorm,
            const double *qnorm, int kernel, double gamma, double *out,
            hipStream_t s) {
  k_svm_panel<TX, TQ, 1><<<(unsigned)((nq + SV_TB - 1) / SV_TB), SV_B, 0, s>>>(
      X, n, ldx, sv, nullptr, 0, (int)ns, Q, qn, ldq, qidx, nq, (int)d, xnorm,
      qnorm, kernel == DKM_SVM_RBF, gamma, nullptr, 0, wa, wb, bias, out);
  return check_launch("svm decision");
}

template <class TQ>
int svm_decision(const TQ *Q, int64_t nq, int64_t d, int64_t ldq,
                 const void *X, int x_f32, int64_t n, int64_t ldx,
                 const int32_t *sv, int64_t ns, const double *coef, double b,
                 const double *qnorm, const double *xnorm, int kernel,
                 double gamma, double *out, hipStream_t s) {
  if (nq < 0 || nq > INT32_MAX || d < 1 || d > INT32_MAX || ldq < d ||
      ldx < d || n < 1 || n > INT32_MAX || !X || ns < 1 || ns > INT32_MAX ||
      !sv || !coef || (nq > 0 && (!Q || !out)) ||
      !kernel_ok(kernel, gamma, qnorm, xnorm))
    return fail(DKM_E_ARG, "svm decision: bad arguments");
  if (nq == 0) return 0;
  if (x_f32)
    return svm_sum<float, TQ>((const float *)X, n, ldx, sv, ns, Q, nq, ldq,
                              nullptr, nq, d, coef, nullptr, b, xnorm, qnorm,
                              kernel, gamma, out, s);
  return svm_sum<double, TQ>((const double *)X, n, ldx, sv, ns, Q, nq, ldq,
                             nullptr, nq, d, coef, nullptr, b, xnorm, qnorm,
                             kernel, gamma, out, s);
}

}  // namespace

}  // namespace dkm

using namespace dkm;

extern "C" {

int dkm_svm_norms_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                      double *out, void *stream) {
  return svm_norms<double>(X, n, d, ldx, out, (hipStream_t)stream);
}

int dkm_svm_norms_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                      double *out, void *stream) {
  return svm_norms<float>(X, n, d, ldx, out, (hipStream_t)stream);
}

int dkm_svm_rows_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                     const int32_t *rows, int64_t m, const int32_t *ws,
                     int64_t q, const double *norms, int kernel, double gamma,
                     double *K, int64_t ldk, void *stream) {
  return svm_rows<double>(X, n, d, ldx, rows, m, ws, q, norms, kernel, gamma,
                          K, ldk, (hipStream_t)stream);
}

int dkm_svm_rows_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                     const int32_t *rows, int64_t m, const int32_t *ws,
                     int64_t q, const double *norms, int kernel, double gamma,
                     double *K, int64_t ldk, void *stream) {
  return svm_rows<float>(X, n, d, ldx, rows, m, ws, q, norms, kernel, gamma,
                         K, ldk, (hipStream_t)stream);
}

int dkm_svm_select(const double *f, const double *alpha, const double *y,
                   int64_t m, double C, int64_t q, int32_t *ws, double *gap,
                   int32_t *mark, void *stream) {
  if (!f || !alpha || !y || m < 1 || m > INT32_MAX || !(C > 0.0) || q < 2 ||
      q > DKM_SVM_QMAX || !ws || !gap || !mark)
    return fail(DKM_E_ARG, "svm select: bad arguments");
  k_svm_select<<<1, SEL_B, 0, (hipStream_t)stream>>>(f, alpha, y, (int)m, C,
                                                     (int)q, ws, gap, mark);
  return check_launch("svm select");
}

int dkm_svm_local(const double *K, int64_t ldk, const int32_t *ws, int64_t q,
                  const double *y, double *alpha, const double *f, int64_t m,
                  double C, double eps, int64_t max_inner, double *dy,
                  int32_t *info, void *stream) {
  if (!K || !ws || q < 2 || q > DKM_SVM_QMAX || !y || !alpha || !f || m < 1 ||
      m > INT32_MAX || ldk < m || !(C > 0.0) || !(eps > 0.0) ||
      max_inner < 0 || max_inner > INT32_MAX || !dy || !info)
    return fail(DKM_E_ARG, "svm local: bad arguments");
  const size_t lds = (size_t)q * q * sizeof(double);
  if (hipFuncSetAttribute((const void *)k_svm_local,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return fail(DKM_E_LAUNCH, "svm local: LDS attribute");
  k_svm_local<<<1, SV_B, lds, (hipStream_t)stream>>>(
      K, ldk, ws, (int)q, y, alpha, f, (int)m, C, eps, (int)max_inner, dy,
      info);
  return check_launch("svm local");
}

int dkm_svm_update(const double *K, int64_t ldk, int64_t q, const double *dy,
                   double *f, int64_t m, void *stream) {
  if (!K || q < 1 || q > DKM_SVM_QMAX || !dy || !f || m < 1 ||
      m > INT32_MAX || ldk < m)
    return fail(DKM_E_ARG, "svm update: bad arguments");
  k_svm_update<<<(unsigned)((m + SV_B - 1) / SV_B), SV_B, 0,
                 (hipStream_t)stream>>>(K, ldk, (int)q, dy, f, m);
  return check_launch("svm update");
}

int dkm_svm_decision_f64(const double *Q, int64_t nq, int64_t d, int64_t ldq,
                         const void *X, int x_f32, int64_t n, int64_t ldx,
                         const int32_t *sv, int64_t ns, const double *coef,
                         double b, const double *qnorm, const double *xnorm,
                         int kernel, double gamma, double *out, void *stream) {
  return svm_decision<double>(Q, nq, d, ldq, X, x_f32, n, ldx, sv, ns, coef,
                              b, qnorm, xnorm, kernel, gamma, out,
                              (hipStream_t)stream);
}

int dkm_svm_decision_f32(const float *Q, int64_t nq, int64_t d, int64_t ldq,
                         const void *X, int x_f32, int64_t n, int64_t ldx,
                         const int32_t *sv, int64_t ns, const double *coef,
                         double b, const double *qnorm, const double *xnorm,
                         int kernel, double gamma, double *out, void *stream) {
  return svm_decision<float>(Q, nq, d, ldq, X, x_f32, n, ldx, sv, ns, coef, b,
                             qnorm, xnorm, kernel, gamma, out,
                             (hipStream_t)stream);
}

int dkm_svm_w(const void *X, int x_f32, int64_t n, int64_t d, int64_t ldx,
              const int32_t *sv, int64_t ns, const double *coef,
              const double *lab, const double *xnorm, int kernel, double gamma,
              double *tmp, double *W, void *stream) {
  if (!X || n < 1 || n > INT32_MAX || d < 1 || d > INT32_MAX || ldx < d ||
      !sv || ns < 1 || ns > INT32_MAX || !coef || !lab || !tmp || !W ||
      !kernel_ok(kernel, gamma, xnorm, xnorm))
    return fail(DKM_E_ARG, "svm w: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  // the reference's own rbf evaluates to exp(+gamma |x_i - x_j|^2)
  int r;
  if (x_f32)
    r = svm_sum<float, float>((const float *)X, n, ldx, sv, ns,
                              (const float *)X, n, ldx, sv, ns, d, coef, lab,
                              0.0, xnorm, xnorm, kernel, -gamma, tmp, s);
  else
    r = svm_sum<double, double>((const double *)X, n, ldx, sv, ns,
                                (const double *)X, n, ldx, sv, ns, d, coef,
                                lab, 0.0, xnorm, xnorm, kernel, -gamma, tmp, s);
  if (r) return r;
  k_svm_w<<<1, SV_B, 0, s>>>(coef, lab, tmp, ns, W);
  return check_launch("svm w");
}

}  // extern "C"

// Code-object preload (dkm_preload): see dkm_ordered.hip.
namespace dkm {
DKM_TU_FLAGS(svm, 0)
__global__ void k_tu_svm() {}
int preload_svm() {
  hipFuncAttributes a;
  const bool ok = hipFuncGetAttributes(&a, (const void *)k_tu_svm) == hipSuccess;
  return ok ? 0 : 1;
}
}  // namespace dkm
