// dkm_logreg.hip -- logistic regression on the resident dense samples
// (DESIGN.md 3.27): one evaluation of the multinomial (or binomial) loss and
// its gradient, or the logits / probabilities / labels, in ONE read of X.
// All arithmetic is fp64 on v_mfma_f64_16x16x4_f64; fp32 rows are widened in
// the loads.  No fast-math, no floating-point atomic, no grid-wide barrier:
// every cross-block sum is block partials added in a fixed order and every
// grid is a function of the shapes only, so the same input gives the same
// bits from run to run.
//
// Operands of the f64 MFMA (lane l, c = l & 15, g = l >> 4): A[m = c][k = g],
// B[k = g][n = c], result register r = D[g + 4 r][c].  Everything staged in
// LDS has the layout [k / 4][m or n][k % 4] (dkm_pca.hip's), a group of four
// k padded by 8 doubles.
//
//   k_logreg_eval   a block of four waves owns a row chunk and walks it in
//                   tiles of R rows, R = 64, 32, 16 for d <= 64, 128, 256 (the
//                   size class SC).  The tile is staged ONCE, as
//                   T[f / 4][row][f % 4], and serves both products; W^T is
//                   staged once per block as Ws[f / 4][class][f % 4].  The
//                   next tile's rows (and labels) are loaded into registers
//                   before the current tile's MFMAs and stored after them.
//     phase 1 (k = feature): Z^T = W X^T.  Wave w takes the 16 rows
//                   w % (R / 16) and the share w / (R / 16) of the feature
//                   groups (R < 64: the waves split k, so that none idles),
//                   and writes its logits to the panel Zp[share][row / 4]
//                   [class][row % 4].
//     softmax:      256 / R threads per row, each with every (256 / R)-th
//                   class in registers: the shares are added in order, then
//                   the intercept; the maximum and the sum go over the row's
//                   threads by xor shuffles.  Stable forms: exp(z - max),
//                   loss = max + log(sum) - z_y; one column: exp(-|z|),
//                   log1p.  The residual p - onehot(y) overwrites Zp[0] in
//                   place (the same thread, the same address); rows past the
//                   chunk give exact zeros.  Each thread keeps a running loss
//                   and the running sums of its residuals: the intercept's
//                   gradient never goes through the MFMA.
//     phase 2 (k = row): G += R^T X, classes x features, in registers for the
//                   whole chunk.  A reads the residual panel (64 consecutive
//                   doubles), B the same tile T with rows as k: a wave's read
//                   is four pieces of 16 consecutive doubles, 8 doubles apart
//                   modulo the banks.  The waves split the 16-feature tiles;
//                   with one or two of them (d <= 32) they also split the
//                   rows of the tile, and each share goes to a partial of its
//                   own.
//                   Predict mode stops after the softmax and writes logits,
//                   probabilities and the first-maximum index.
//   k_logreg_final  folds the partials in a fixed order (16 slices of the
//                   partials, then the slices in order) into [loss | G].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "dkm_internal.h"

namespace dkm {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int LR_B = 256;              // threads per block: four waves
constexpr int LR_ROWS = 512;           // rows of a chunk, at least
constexpr int LR_MAXC = 4096;          // chunks, at most
constexpr int LR_PAD = 8;              // doubles after a group of four k
constexpr int LR_LOSS = 0, LR_PREDICT = 1;
static_assert(LR_B == 4 * WAVE, "four waves");
static_assert(DKM_LOGREG_MAX_D == 64 << 2, "three size classes");

__device__ inline f64x4 lr_mfma(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// The plan: a function of (d, classes) only.
struct LrPlan {
  int sc, R, FT, KQ, CP, GS, WG, ZS, KS, FP;
  int64_t PS;
  size_t lds;
};

__host__ __device__ inline int lr_ks(int FT) { return FT == 1 ? 4 : FT == 2 ? 2 : 1; }

LrPlan lr_plan(int64_t d, int64_t classes) {
  LrPlan p;
  p.sc = d <= 64 ? 0 : d <= 128 ? 1 : 2;
  p.R = 64 >> p.sc;
  p.FT = (int)((d + 15) / 16);
  p.KQ = 4 * p.FT;
  p.CP = classes <= 16 ? 16 : 32;
  p.GS = 4 * p.R + LR_PAD;
  p.WG = 4 * p.CP + LR_PAD;
  p.ZS = (p.R / 4) * p.WG;
  p.KS = lr_ks(p.FT);
  p.FP = 16 * p.FT;
  p.PS = (int64_t)p.CP * p.FP + 2 * p.CP;
  p.lds = sizeof(double) * ((size_t)p.KQ * p.GS + (size_t)p.KQ * p.WG +
                            (size_t)(64 / p.R) * p.ZS + p.CP);
  return p;
}

bool lr_shape_ok(int64_t n, int64_t d, int64_t ldx, int64_t classes) {
  return n >= 1 && d >= 1 && d <= DKM_LOGREG_MAX_D && ldx >= d &&
         classes >= 1 && classes <= DKM_LOGREG_MAX_CLASSES &&
         n < (INT64_MAX / 16) / ldx;
}

int64_t lr_chunks(int64_t n) {
  return std::max<int64_t>(
      1, std::min<int64_t>((n + LR_ROWS - 1) / LR_ROWS, LR_MAXC));
}

// rows of a chunk: whole tiles of every size class
__host__ __device__ inline int64_t lr_chunk_rows(int64_t n, int64_t nrc) {
  return ((n + nrc - 1) / nrc + 63) / 64 * 64;
}

size_t lr_ws_bytes(int64_t n, const LrPlan &p) {
  return (size_t)round_up(lr_chunks(n) * p.KS * p.PS * 8, 256);
}

}  // namespace

// MODE LR_LOSS: part[(rc KS + ks) PS + class FP + f] = the chunk's (and row
// share's) sum of residual[class] x[f]; in the partial of share 0 also
// [CP FP + class] = the sum of residual[class] and [CP FP + CP] = the loss.
// MODE LR_PREDICT: logits / proba (n x C) and labels, each unless NULL.
template <class TX, int NT, int SC, int MODE>
__global__ void __launch_bounds__(LR_B, 2)   // two blocks per CU: 256 VGPRs
    k_logreg_eval(const TX *__restrict__ X, int64_t n, int d, int64_t ldx,
                  const int32_t *__restrict__ y, const double *__restrict__ W,
                  int C, int fi, int64_t nrc, double *__restrict__ part,
                  double *__restrict__ logits, double *__restrict__ proba,
                  int32_t *__restrict__ labels) {
  constexpr int R = 64 >> SC;          // rows of a tile
  constexpr int NF = 1 << SC;          // feature tiles of a wave, at most
  constexpr int CP = 16 * NT;          // padded logit columns
  constexpr int GS = 4 * R + LR_PAD;   // doubles per feature group of T
  constexpr int WG = 4 * CP + LR_PAD;  // ... of Ws, and per row group of Zp
  constexpr int ZS = (R / 4) * WG;     // one logit panel
  constexpr int NKP = 64 / R;          // feature shares of phase 1
  constexpr int RS = R / 16;           // 16-row pieces of a tile
  constexpr int TPR = LR_B / R;        // softmax threads per row
  constexpr int JJ = CP / TPR;         // classes per softmax thread
  extern __shared__ double lr_sm[];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int c = lane & 15, g = lane >> 4;
  const int FT = (d + 15) >> 4, KQ = 4 * FT, wld = d + fi;
  double *T = lr_sm;
  double *Ws = T + KQ * GS;
  double *Zp = Ws + KQ * WG;
  double *bias = Zp + NKP * ZS;
  const int64_t rc = blockIdx.x;
  const int64_t per = lr_chunk_rows(n, nrc);
  const int64_t row0 = std::min(n, rc * per), row1 = std::min(n, row0 + per);
  const int ns = (int)((row1 - row0 + R - 1) / R);

  // W^T and the intercepts, once per block; zeros past C and d
  for (int e = tid; e < CP * 4 * KQ; e += LR_B) {
    const int cls = e / (4 * KQ), f = e - cls * 4 * KQ;
    Ws[(f >> 2) * WG + cls * 4 + (f & 3)] =
        cls < C && f < d ? W[(int64_t)cls * wld + f] : 0.0;
  }
  if (tid < CP) bias[tid] = fi && tid < C ? W[(int64_t)tid * wld + d] : 0.0;

  // staging: LW = the power of two >= max(d, 16) lanes along a row, 256 / LW
  // rows per pass, NP <= 16 passes per tile
  int lws = 4;
  while ((1 << lws) < d) ++lws;
  const int sf = tid & ((1 << lws) - 1), sr = tid >> lws;
  const int rpp = LR_B >> lws, NP = (R << lws) >> 8;
  const bool fok = sf < d, fst = sf < 4 * KQ;
  // softmax: row rl of the tile, classes sub + TPR jj
  const int rl = tid / TPR, sub = tid & (TPR - 1);
  const int zoff = (rl >> 2) * WG + (rl & 3);
  TX raw[16];
  int32_t ynext = -1;
  auto load = [&](int s) {
    const int64_t base = row0 + (int64_t)s * R;
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (u < NP) {
        const int64_t row = base + sr + rpp * u;
        raw[u] = fok && row < row1 ? X[row * ldx + sf] : (TX)0;
      }
    if (MODE == LR_LOSS) ynext = base + rl < row1 ? y[base + rl] : -1;
  };
  auto store = [&]() {
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (u < NP && fst)
        T[(sf >> 2) * GS + (sr + rpp * u) * 4 + (sf & 3)] = (double)raw[u];
  };

  // phase 1: the 16 rows rs of the tile, the share kp of the feature groups
  const int rs = w & (RS - 1), kp = w / RS;
  const int KQ1 = (d + 3) >> 2, kper = (KQ1 + NKP - 1) / NKP;
  const int q0 = std::min(KQ1, kp * kper), q1 = std::min(KQ1, q0 + kper);
  // phase 2: the feature tiles fslot + WF i, the share ks of the tile's rows
  const int KS = lr_ks(FT), WF = 4 / KS;
  const int fslot = w & (WF - 1), ks = w / WF;
  const int p0 = ks * ((R / 4) / KS), p1 = p0 + (R / 4) / KS;
  int ftc[NF];
#pragma unroll
  for (int i = 0; i < NF; ++i) ftc[i] = std::min(fslot + WF * i, FT - 1);
  f64x4 G[NF][NT];
#pragma unroll
  for (int i = 0; i < NF; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t) G[i][t] = f64x4{0.0, 0.0, 0.0, 0.0};
  double loss = 0.0, bsum[JJ];
#pragma unroll
  for (int jj = 0; jj < JJ; ++jj) bsum[jj] = 0.0;

  if (ns > 0) {
    load(0);
    store();
  }
  __syncthreads();
  for (int s = 0; s < ns; ++s) {
    const int32_t yv = ynext;
    const int64_t row = row0 + (int64_t)s * R + rl;
    const bool live = row < row1;
    const bool more = s + 1 < ns;
    if (more) load(s + 1);

    {
      f64x4 acc[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
      for (int q = q0; q < q1; ++q) {
        const double b = T[q * GS + (16 * rs + c) * 4 + g];
#pragma unroll
        for (int t = 0; t < NT; ++t)
          acc[t] = lr_mfma(Ws[q * WG + (16 * t + c) * 4 + g], b, acc[t]);
      }
      double *zp = Zp + kp * ZS + (4 * rs + (c >> 2)) * WG + (c & 3);
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) zp[(g + 4 * r + 16 * t) * 4] = acc[t][r];
    }
    __syncthreads();

    {
      double z[JJ], res[JJ];
#pragma unroll
      for (int jj = 0; jj < JJ; ++jj) {
        const int j = sub + TPR * jj;
        double v = Zp[zoff + j * 4];
#pragma unroll
        for (int k = 1; k < NKP; ++k) v = v + Zp[k * ZS + zoff + j * 4];
        z[jj] = v + bias[j];
        res[jj] = 0.0;
      }
      if (C == 1) {
        if (sub == 0) {
          const double zz = z[0], e = exp(-fabs(zz)), den = 1.0 + e;
          const double p = zz >= 0.0 ? 1.0 / den : e / den;
          if (MODE == LR_LOSS) {
            if (live) {
              res[0] = p - (double)yv;
              loss = loss + ((yv ? fmax(-zz, 0.0) : fmax(zz, 0.0)) + log1p(e));
            }
          } else if (live) {
            if (logits) logits[row] = zz;
            if (proba) proba[row] = p;
            if (labels) labels[row] = zz > 0.0 ? 1 : 0;
          }
        }
      } else {
        double m = -INFINITY;
        int am = INT_MAX;
#pragma unroll
        for (int jj = 0; jj < JJ; ++jj) {
          const int j = sub + TPR * jj;
          if (j < C) {
            if (z[jj] > m) am = j;     // first index of the lane's maximum
            m = fmax(m, z[jj]);
          }
        }
        if (MODE == LR_PREDICT) {
          double bv = m;
#pragma unroll
          for (int o = TPR / 2; o >= 1; o >>= 1) {
            const double ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(am, o);
            if (ov > bv || (ov == bv && oi < am)) {
              bv = ov;
              am = oi;
            }
          }
        }
#pragma unroll
        for (int o = TPR / 2; o >= 1; o >>= 1) m = fmax(m, __shfl_xor(m, o));
        double e[JJ], sum = 0.0;
#pragma unroll
        for (int jj = 0; jj < JJ; ++jj) {
          e[jj] = sub + TPR * jj < C ? exp(z[jj] - m) : 0.0;
          sum = sum + e[jj];
        }
#pragma unroll
        for (int o = TPR / 2; o >= 1; o >>= 1) sum = sum + __shfl_xor(sum, o);
        if (MODE == LR_LOSS) {
          if (live) {
            if (sub == 0) loss = loss + (m + log(sum));
#pragma unroll
            for (int jj = 0; jj < JJ; ++jj) {
              const int j = sub + TPR * jj;
              if (j < C) res[jj] = e[jj] / sum - (j == yv ? 1.0 : 0.0);
              if (j == yv) loss = loss - z[jj];
            }
          }
        } else if (live) {
#pragma unroll
          for (int jj = 0; jj < JJ; ++jj) {
            const int j = sub + TPR * jj;
            if (j < C) {
              if (logits) logits[row * C + j] = z[jj];
              if (proba) proba[row * C + j] = e[jj] / sum;
            }
          }
          if (labels && sub == 0) labels[row] = am == INT_MAX ? 0 : am;
        }
      }
      if (MODE == LR_LOSS) {
#pragma unroll
        for (int jj = 0; jj < JJ; ++jj) {
          Zp[zoff + (sub + TPR * jj) * 4] = res[jj];
          bsum[jj] = bsum[jj] + res[jj];
        }
      }
    }
    __syncthreads();

    if (MODE == LR_LOSS) {
      for (int q = p0; q < p1; ++q) {
        double a[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) a[t] = Zp[q * WG + (16 * t + c) * 4 + g];
#pragma unroll
        for (int i = 0; i < NF; ++i) {
          const double b =
              T[(4 * ftc[i] + (c >> 2)) * GS + (4 * q + g) * 4 + (c & 3)];
#pragma unroll
          for (int t = 0; t < NT; ++t) G[i][t] = lr_mfma(a[t], b, G[i][t]);
        }
      }
      __syncthreads();
    }
    if (more) store();
    __syncthreads();
  }

  if (MODE == LR_LOSS) {
    const int FP = 16 * FT;
    const int64_t PS = (int64_t)CP * FP + 2 * CP;
    double *o = part + (rc * KS + ks) * PS;
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const int ft = fslot + WF * i, f = 16 * ft + c;
      if (ft < FT && f < d) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int cls = g + 4 * r + 16 * t;
            if (cls < C) o[cls * FP + f] = G[i][t][r];
          }
      }
    }
    // the loss and the intercept's gradient: the threads' sums in order
    // (T and Zp are free: the loop's last barrier)
    T[tid] = loss;
#pragma unroll
    for (int jj = 0; jj < JJ; ++jj) Zp[rl * CP + sub + TPR * jj] = bsum[jj];
    __syncthreads();
    double *o0 = part + rc * KS * PS + (int64_t)CP * FP;
    if (tid < CP) {
      double v = 0.0;
      for (int i = 0; i < R; ++i) v = v + Zp[i * CP + tid];
      o0[tid] = v;
    } else if (tid == CP) {
      double v = 0.0;
      for (int i = 0; i < LR_B; ++i) v = v + T[i];
      o0[CP] = v;
    }
  }
}

// out[0] = the loss, out[1 + class wld + f] = G.  Thread (slice s = tid / 16,
// element tid % 16) folds partials s, s + 16, ...; the slices are then added
// in order by the threads of slice 0.
__global__ void __launch_bounds__(LR_B)
    k_logreg_final(const double *__restrict__ part, int64_t nrc, int KS,
                   int64_t PS, int CP, int FP, int C, int d, int fi,
                   double *__restrict__ out) {
  __shared__ double sm[LR_B];
  const int wld = d + fi;
  const int e = (int)blockIdx.x * 16 + (threadIdx.x & 15);
  const bool ok = e < 1 + C * wld;
  // element e: `cnt` values, `step` apart, from `off`
  int64_t cnt = nrc, step = KS * PS, off = (int64_t)CP * FP + CP;
  if (ok && e > 0) {
    const int cls = (e - 1) / wld, f = (e - 1) - cls * wld;
    if (f < d) {
      cnt = nrc * KS;
      step = PS;
      off = (int64_t)cls * FP + f;
    } else {
      off = (int64_t)CP * FP + cls;
    }
  }
  const int s = threadIdx.x >> 4;
  double v = 0.0;
  if (ok)
    for (int64_t p = s; p < cnt; p += 16) v = v + part[p * step + off];
  sm[threadIdx.x] = v;
  __syncthreads();
  if (s == 0 && ok) {
    for (int i = 1; i < 16; ++i) v = v + sm[i * 16 + threadIdx.x];
    out[e] = v;
  }
}

namespace {

template <class TX, int NT, int SC, int MODE>
int lr_launch(const LrPlan &p, const TX *X, int64_t n, int64_t d, int64_t ldx,
              const int32_t *y, const double *W, int64_t C, int fi,
              double *part, double *logits, double *proba, int32_t *labels,
              hipStream_t s) {
  auto kf = k_logreg_eval<TX, NT, SC, MODE>;
  if (hipFuncSetAttribute((const void *)kf,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)p.lds) != hipSuccess)
    return fail(DKM_E_LAUNCH, "logreg: LDS attribute");
  const int64_t nrc = lr_chunks(n);
  kf<<<(unsigned)nrc, LR_B, p.lds, s>>>(X, n, (int)d, ldx, y, W, (int)C, fi,
                                        nrc, part, logits, proba, labels);
  return check_launch("logreg eval");
}

template <class TX, int MODE>
int lr_dispatch(const LrPlan &p, const TX *X, int64_t n, int64_t d,
                int64_t ldx, const int32_t *y, const double *W, int64_t C,
                int fi, double *part, double *logits, double *proba,
                int32_t *labels, hipStream_t s) {
#define LR_CASE(NT, SC)                                                     \
  if (p.CP == 16 * NT && p.sc == SC)                                        \
    return lr_launch<TX, NT, SC, MODE>(p, X, n, d, ldx, y, W, C, fi, part,  \
                                       logits, proba, labels, s);
  LR_CASE(1, 0) LR_CASE(1, 1) LR_CASE(1, 2)
  LR_CASE(2, 0) LR_CASE(2, 1) LR_CASE(2, 2)
#undef LR_CASE
  return fail(DKM_E_ARG, "logreg: no kernel for the shape");
}

template <class TX>
int lr_lossgrad(const TX *X, int64_t n, int64_t d, int64_t ldx,
                const int32_t *y, const double *W, int64_t C, int fi,
                void *ws, size_t ws_b, double *out, hipStream_t s) {
  if (!lr_shape_ok(n, d, ldx, C) || !X || !y || !W || !out)
    return fail(DKM_E_ARG, "logreg lossgrad: bad arguments");
  const LrPlan p = lr_plan(d, C);
  if (!ws || ws_b < lr_ws_bytes(n, p))
    return fail(DKM_E_WORKSPACE, "logreg lossgrad: workspace too small");
  fi = fi ? 1 : 0;
  if (int r = lr_dispatch<TX, LR_LOSS>(p, X, n, d, ldx, y, W, C, fi,
                                       (double *)ws, nullptr, nullptr,
                                       nullptr, s))
    return r;
  const int64_t ne = 1 + C * (d + fi);
  k_logreg_final<<<(unsigned)((ne + 15) / 16), LR_B, 0, s>>>(
      (const double *)ws, lr_chunks(n), p.KS, p.PS, p.CP, p.FP, (int)C, (int)d,
      fi, out);
  return check_launch("logreg lossgrad: final sum");
}

template <class TX>
int lr_predict(const TX *X, int64_t n, int64_t d, int64_t ldx, const double *W,
               int64_t C, int fi, double *logits, double *proba,
               int32_t *labels, hipStream_t s) {
  if (!lr_shape_ok(n, d, ldx, C) || !X || !W ||
      (!logits && !proba && !labels) || n >= (INT64_MAX / 16) / C)
    return fail(DKM_E_ARG, "logreg predict: bad arguments");
  return lr_dispatch<TX, LR_PREDICT>(lr_plan(d, C), X, n, d, ldx, nullptr, W,
                                     C, fi ? 1 : 0, nullptr, logits, proba,
                                     labels, s);
}

}  // namespace

}  // namespace dkm

using namespace dkm;

extern "C" {

size_t dkm_logreg_workspace_bytes(int64_t n, int64_t d, int64_t classes) {
  if (!lr_shape_ok(n, d, d, classes)) return 0;
  return lr_ws_bytes(n, lr_plan(d, classes));
}

int dkm_logreg_lossgrad_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                            const int32_t *y, const double *W, int64_t classes,
                            int fit_intercept, void *ws, size_t ws_bytes,
                            double *out, void *stream) {
  return lr_lossgrad<double>(X, n, d, ldx, y, W, classes, fit_intercept, ws,
                             ws_bytes, out, (hipStream_t)stream);
}

int dkm_logreg_lossgrad_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                            const int32_t *y, const double *W, int64_t classes,
                            int fit_intercept, void *ws, size_t ws_bytes,
                            double *out, void *stream) {
  return lr_lossgrad<float>(X, n, d, ldx, y, W, classes, fit_intercept, ws,
                            ws_bytes, out, (hipStream_t)stream);
}

int dkm_logreg_predict_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                           const double *W, int64_t classes, int fit_intercept,
                           double *logits, double *proba, int32_t *labels,
                           void *stream) {
  return lr_predict<double>(X, n, d, ldx, W, classes, fit_intercept, logits,
                            proba, labels, (hipStream_t)stream);
}

int dkm_logreg_predict_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                           const double *W, int64_t classes, int fit_intercept,
                           double *logits, double *proba, int32_t *labels,
                           void *stream) {
  return lr_predict<float>(X, n, d, ldx, W, classes, fit_intercept, logits,
                           proba, labels, (hipStream_t)stream);
}

}  // extern "C"

// Code-object preload (dkm_preload): see dkm_ordered.hip.
namespace dkm {
DKM_TU_FLAGS(logreg, 0)
__global__ void k_tu_logreg() {}
int preload_logreg() {
  hipFuncAttributes a;
  const bool ok =
      hipFuncGetAttributes(&a, (const void *)k_tu_logreg) == hipSuccess;
  return ok ? 0 : 1;
}
}  // namespace dkm
