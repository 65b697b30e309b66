// dkm_kpp.hip -- k-means++ (D^2) seeding on the resident dense samples:
// sklearn's greedy rule.  One round draws L trial rows from
// the running minimum distances `mind`, scores all of them in ONE read of X
// and commits the trial that lowers the potential most:
//
//   k_kpp_sample   targets u_l * pot  ->  L rows by a two-level search over
//                  cumsum(mind) (1024-row segment sums, then the segment),
//                  and the rows gathered, widened, into the (L, d) table
//   k_kpp_eval     D_l[i] = sum_j (x_ij - c_lj)^2 for every row and trial,
//                  into the trial-major dc[L][ldc]; per block and trial the
//                  sum of min(mind[i], D_l[i])
//   k_kpp_choose   block partials summed in a fixed order, first minimum
//   k_kpp_commit   mind <- fmin(mind, dc[best]), one sum per segment
//
// The rounds are enqueued back to back: the row numbers, the potential and
// the winner stay on the device, nothing is read back inside the loop.
//
// Why no MFMA.  (x - c)^2 is not a product of matrices; expanding it into
// |x|^2 + |c|^2 - 2 x.c would make it one, but a chosen row must then score
// exactly 0 against itself and every term must be non-negative, and neither
// survives the cancellation.  At L <= 32 a pass moves 8 d bytes per row for
// about 3 L d flops, below the machine's flop-to-byte balance on the vector
// ALU already: the design target is the HBM stream of X.
//
// k_kpp_eval.  A group of G lanes (the smallest power of two >= d, at most
// 64) owns R rows at a time; lane g holds features g, g + G, ... so a wave's
// load is contiguous (rows r NG + q, q the group: consecutive groups read
// consecutive rows).  The trial table is staged in LDS in chunks of at most
// 512 features (32 trials: 128 KiB); lane g reads trial element j = g + G t,
// consecutive lanes consecutive doubles, equal g the same address: every LDS
// read is conflict-free or a broadcast, and feeds R fused multiply-adds.
// Buckets of LB = 4, 8, 16, 32 trials keep R x LB accumulators at 32 .. 64.
// The G partial sums are folded by a transposing butterfly: at level s a lane
// keeps one half of its values and sends the other to lane ^ (1 << s), so a
// fold costs M shuffles in all instead of M log2 G, and the M results end up
// spread over the group's lanes, which store them and add min(mind, D) to
// their own running sums in ascending row order.  The order of every sum is a
// function of (n, d, L) only: the same input gives the same bits.
// A feature count above one chunk takes the chunks in the outer loop and adds
// each chunk's partial distance to dc from the same lane (+ 16 L bytes per
// row and chunk against 4096 of X).
//
// No floating-point atomic, no grid-wide barrier, every loop bound known at
// launch (the searches have fixed trip counts: a NaN target ends at row
// n - 1).  Compiled without fast-math, -ffp-contract=off; the fma() below is
// written out.
#include <hip/hip_runtime.h>

#include <climits>

#include "dkm_internal.h"

namespace dkm {

namespace {

constexpr int KP_B = 256;      // threads of k_kpp_eval and k_kpp_commit
constexpr int KP_CH = 512;     // features per LDS chunk of the trial table
constexpr int KP_SEG = 1024;   // rows per segment of mind (bsum)
constexpr int KP_MAXB = 1024;  // blocks of k_kpp_eval at most
constexpr int KP_SB = 1024;    // threads of k_kpp_choose and k_kpp_sample
static_assert(DKM_KPP_MAX_TRIALS * 32 <= KP_SB, "k_kpp_choose: 32 lanes per trial");
static_assert((size_t)DKM_KPP_MAX_TRIALS * KP_CH * sizeof(double) <=
                  160 * 1024, "the trial chunks fit LDS");

constexpr int kp_log2(int v) { return v <= 1 ? 0 : 1 + kp_log2(v >> 1); }

// the rows per group of a trial bucket
constexpr int kp_rows(int lb) { return lb <= 8 ? 8 : 64 / lb; }
inline int kp_bucket(int64_t L) { return L <= 4 ? 4 : L <= 8 ? 8 : L <= 16 ? 16 : 32; }
inline int kp_lg(int64_t d) {
  int lg = 0;
  while (lg < 6 && ((int64_t)1 << lg) < d) ++lg;
  return lg;
}

struct KppGrid {
  int lg;           // log2 of the lanes per row
  int64_t tpb;      // row tiles per block
  int64_t blocks;
  size_t lds;
};

KppGrid kp_grid(int64_t n, int64_t d, int64_t L) {
  KppGrid g;
  g.lg = kp_lg(d);
  const int lb = kp_bucket(L);
  const int64_t tile = (int64_t)(KP_B >> g.lg) * kp_rows(lb);
  const int64_t tiles = (n + tile - 1) / tile;
  g.tpb = (tiles + KP_MAXB - 1) / KP_MAXB;
  g.blocks = (tiles + g.tpb - 1) / g.tpb;
  const int64_t G = (int64_t)1 << g.lg;
  int64_t cw = d < KP_CH ? (d + G - 1) / G * G : KP_CH;
  if (cw < KP_B) cw = KP_B;   // the block tree of the potentials: LB x KP_B
  g.lds = (size_t)lb * cw * sizeof(double);
  return g;
}

bool kp_shape_ok(int64_t n, int64_t d, int64_t L) {
  return n >= 1 && n <= INT32_MAX && d >= 1 && d <= INT32_MAX && L >= 1 &&
         L <= DKM_KPP_MAX_TRIALS;
}

}  // namespace

// One level of the transposing fold: of its CUR values a lane keeps the half
// its bit S of g selects and adds the partner's copy of that half.  With one
// value left the levels are plain butterflies.  v[0 .. M >> min(lg, log2 M))
// then hold entries (bit s of g) << (log2 M - 1 - s) | i of the group's sums.
template <int CUR, int S, int M>
__device__ __forceinline__ void kpp_fold(double (&v)[M], int g, int lg) {
  if constexpr (S < 6) {
    if (S < lg) {
      if constexpr (CUR >= 2) {
        constexpr int H = CUR / 2;
        const bool hi = (g >> S) & 1;
#pragma unroll
        for (int i = 0; i < H; ++i) {
          const double send = hi ? v[i] : v[i + H];
          const double keep = hi ? v[i + H] : v[i];
          v[i] = keep + __shfl_xor(send, 1 << S, WAVE);
        }
        kpp_fold<H, S + 1, M>(v, g, lg);
      } else {
        v[0] = v[0] + __shfl_xor(v[0], 1 << S, WAVE);
        kpp_fold<1, S + 1, M>(v, g, lg);
      }
    }
  }
}

// dc[l][row] <- |x_row - trial_l|^2, partial[block][l] <- the block's sum of
// min(mind[row], dc[l][row]) (of dc[l][row] when mind is NULL).
template <class TX, int LB, int R>
__global__ __launch_bounds__(KP_B) void k_kpp_eval(
    const TX *__restrict__ X, int64_t n, int d, int64_t ldx,
    const double *__restrict__ T, int L, const double *__restrict__ mind,
    double *__restrict__ dc, int64_t ldc, double *__restrict__ partial,
    int lg, int64_t tpb) {
  constexpr int M = LB * R;
  constexpr int LM = kp_log2(M), LR = kp_log2(R);
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const int G = 1 << lg, g = tid & (G - 1), q = tid >> lg, NG = KP_B >> lg;
  const int64_t tile = (int64_t)NG * R;
  // the entries (trial l = e / R, row slot r = e % R) this lane holds after
  // the fold: e = ehi | i, i < cnt; with more lanes than entries the first
  // copy stores
  const int lf = lg < LM ? lg : LM;
  int ehi = 0;
  for (int s = 0; s < lf; ++s) ehi |= ((g >> s) & 1) << (LM - 1 - s);
  const int cnt = M >> lf;
  const bool owner = (g >> lf) == 0;
  double pl[LB];
#pragma unroll
  for (int j = 0; j < LB; ++j) pl[j] = 0.0;

  const int nch = (d + KP_CH - 1) / KP_CH;
  for (int ch = 0; ch < nch; ++ch) {
    const int c0 = ch * KP_CH;
    const int cw = d - c0 < KP_CH ? d - c0 : KP_CH;
    const int cwp = ((cw + G - 1) >> lg) << lg;
    const bool last = ch == nch - 1;
    __syncthreads();
    for (int i = tid; i < LB * cwp; i += KP_B) {
      const int l = i / cwp, j = i - l * cwp;
      lds[i] = (l < L && j < cw) ? T[(int64_t)l * d + c0 + j] : 0.0;
    }
    __syncthreads();
    const int nt = cwp >> lg;
    for (int64_t tl = 0; tl < tpb; ++tl) {
      const int64_t tbase = ((int64_t)blockIdx.x * tpb + tl) * tile;
      if (tbase >= n) break;
      double v[M];
#pragma unroll
      for (int i = 0; i < M; ++i) v[i] = 0.0;
      for (int t = 0; t < nt; ++t) {
        const int j = g + (t << lg);
        double x[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int64_t row = tbase + (int64_t)r * NG + q;
          x[r] = (row < n && j < cw) ? (double)X[row * ldx + c0 + j] : 0.0;
        }
#pragma unroll
        for (int l = 0; l < LB; ++l) {
          const double c = lds[l * cwp + j];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const double df = x[r] - c;
            v[l * R + r] = fma(df, df, v[l * R + r]);
          }
        }
      }
      kpp_fold<M, 0, M>(v, g, lg);
      if (owner) {
#pragma unroll
        for (int i = 0; i < M; ++i) {
          if (i < cnt) {
            const int e = ehi | i;
            const int l = e >> LR, r = e & (R - 1);
            const int64_t row = tbase + (int64_t)r * NG + q;
            if (l < L && row < n) {
              double *p = dc + (int64_t)l * ldc + row;
              double val = v[i];
              if (ch > 0) val = *p + val;
              *p = val;
              if (last)
                pl[i >> LR] = pl[i >> LR] + (mind ? fmin(mind[row], val) : val);
            }
          }
        }
      }
    }
  }

  // the block's potentials: one column per thread, then a fixed tree
  __syncthreads();
  for (int i = tid; i < LB * KP_B; i += KP_B) lds[i] = 0.0;
  __syncthreads();
  if (owner) {
    const int l0 = ehi >> LR;
    const int nl = (cnt >> LR) > 1 ? (cnt >> LR) : 1;
#pragma unroll
    for (int j = 0; j < LB; ++j)
      if (j < nl) lds[(l0 + j) * KP_B + tid] = pl[j];
  }
  for (int s = KP_B / 2; s >= 1; s >>= 1) {
    __syncthreads();
    for (int i = tid; i < LB * s; i += KP_B) {
      const int l = i / s, t = i - l * s;
      lds[l * KP_B + t] = lds[l * KP_B + t] + lds[l * KP_B + t + s];
    }
  }
  __syncthreads();
  if (tid < L) partial[(int64_t)blockIdx.x * L + tid] = lds[tid * KP_B];
}

// The trial with the first minimum of the summed block partials.
__global__ __launch_bounds__(KP_SB) void k_kpp_choose(
    const double *__restrict__ partial, int64_t nb, int L,
    const int32_t *__restrict__ rows, double *__restrict__ pot,
    int32_t *__restrict__ best, int64_t *__restrict__ index_out) {
  __shared__ double sm[DKM_KPP_MAX_TRIALS][33];
  const int l = threadIdx.x >> 5, j = threadIdx.x & 31;
  double s = 0.0;
  if (l < L)
    for (int64_t b = j; b < nb; b += 32) s = s + partial[b * L + l];
  sm[l][j] = s;
  __syncthreads();
  for (int h = 16; h >= 1; h >>= 1) {
    if (j < h) sm[l][j] = sm[l][j] + sm[l][j + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    int bi = 0;
    double bp = sm[0][0];
    for (int i = 1; i < L; ++i)
      if (sm[i][0] < bp) {
        bp = sm[i][0];
        bi = i;
      }
    pot[0] = bp;
    best[0] = bi;
    index_out[0] = rows[bi];
  }
}

// mind <- fmin(mind, dc[best]) (first: dc[best]) over one 1024-row segment,
// bsum[segment] <- the segment's sum of the new mind.
__global__ __launch_bounds__(KP_B) void k_kpp_commit(
    int64_t n, const double *__restrict__ dc, int64_t ldc,
    const int32_t *__restrict__ best, int first, double *__restrict__ mind,
    double *__restrict__ bsum) {
  __shared__ double sm[KP_B];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * KP_SEG;
  const double *col = dc + (int64_t)best[0] * ldc;
  double s[KP_SEG / KP_B];
#pragma unroll
  for (int u = 0; u < KP_SEG / KP_B; ++u) {
    const int64_t i = base + u * KP_B + tid;
    double m = 0.0;
    if (i < n) {
      m = col[i];
      if (!first) m = fmin(mind[i], m);
      mind[i] = m;
    }
    s[u] = m;
  }
  sm[tid] = (s[0] + s[1]) + (s[2] + s[3]);
  for (int h = KP_B / 2; h >= 1; h >>= 1) {
    __syncthreads();
    if (tid < h) sm[tid] = sm[tid] + sm[tid + h];
  }
  if (tid == 0) bsum[blockIdx.x] = sm[0];
}

// rows[l] <- min(searchsorted(cumsum(mind), u[l] * pot, 'left'), n - 1) and
// T[l] <- that row, widened.  One block: a scan of the segment sums into
// bscan, then a wave per target.
template <class TX>
__global__ __launch_bounds__(KP_SB) void k_kpp_sample(
    const TX *__restrict__ X, int64_t n, int d, int64_t ldx,
    const double *__restrict__ mind, const double *__restrict__ bsum,
    double *__restrict__ bscan, int64_t nseg, const double *__restrict__ pot,
    const double *__restrict__ u, int L, int32_t *__restrict__ rows,
    double *__restrict__ T) {
  __shared__ double tot[KP_SB];
  const int tid = threadIdx.x;
  // inclusive scan of bsum: a run of consecutive segments per thread, a
  // Kogge-Stone scan of the runs' totals, the runs again
  const int64_t per = (nseg + KP_SB - 1) / KP_SB;
  int64_t a = (int64_t)tid * per;
  if (a > nseg) a = nseg;
  const int64_t b = a + per < nseg ? a + per : nseg;
  double s = 0.0;
  for (int64_t i = a; i < b; ++i) s = s + bsum[i];
  tot[tid] = s;
  __syncthreads();
  for (int o = 1; o < KP_SB; o <<= 1) {
    const double t = tid >= o ? tot[tid - o] : 0.0;
    __syncthreads();
    if (tid >= o) tot[tid] = tot[tid] + t;
    __syncthreads();
  }
  double run = tid ? tot[tid - 1] : 0.0;
  for (int64_t i = a; i < b; ++i) {
    run = run + bsum[i];
    bscan[i] = run;
  }
  __syncthreads();

  const int lane = tid & 63;
  for (int w = tid >> 6; w < L; w += KP_SB / WAVE) {
    const double target = u[w] * pot[0];
    // the first segment whose inclusive prefix reaches the target
    int64_t lo = 0, hi = nseg;
    for (int it = 0; it < 32; ++it) {
      if (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (bscan[mid] >= target)
          hi = mid;
        else
          lo = mid + 1;
      }
    }
    int64_t row = n - 1;
    if (lo < nseg) {
      const int64_t r0 = lo * KP_SEG;
      double base = lo ? bscan[lo - 1] : 0.0;
      int found = -1;
      for (int p = 0; p < KP_SEG / WAVE; ++p) {
        const int64_t i = r0 + p * WAVE + lane;
        double incl = i < n ? mind[i] : 0.0;
  #pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
          const double t = __shfl_up(incl, o, WAVE);
          if (lane >= o) incl = incl + t;
        }
        const double val = base + incl;
        const unsigned long long m = __ballot(i < n && val >= target);
        if (found < 0 && m) found = p * WAVE + __ffsll((long long)m) - 1;
        base = __shfl(val, WAVE - 1, WAVE);
      }
      row = found >= 0 ? r0 + found : r0 + KP_SEG - 1;
      if (row > n - 1) row = n - 1;
    }
    if (lane == 0) rows[w] = (int32_t)row;
    for (int j = lane; j < d; j += WAVE)
      T[(int64_t)w * d + j] = (double)X[row * ldx + j];
  }
}

namespace {

template <class TX, int LB>
int kpp_eval_launch(const TX *X, int64_t n, int64_t d, int64_t ldx,
                    const double *T, int64_t L, const double *mind,
                    double *dc, int64_t ldc, double *partial,
                    const KppGrid &g, hipStream_t s) {
  auto kern = k_kpp_eval<TX, LB, kp_rows(LB)>;
  if (hipFuncSetAttribute((const void *)kern,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)g.lds) != hipSuccess)
    return fail(DKM_E_LAUNCH, "kpp eval: LDS attribute");
  kern<<<(unsigned)g.blocks, KP_B, g.lds, s>>>(X, n, (int)d, ldx, T, (int)L,
                                                mind, dc, ldc, partial, g.lg,
                                                g.tpb);
  return check_launch("kpp eval");
}

template <class TX>
int kpp_eval(const TX *X, int64_t n, int64_t d, int64_t ldx, const double *T,
             int64_t L, const double *mind, double *dc, int64_t ldc,
             double *partial, hipStream_t s) {
  if (!kp_shape_ok(n, d, L) || ldx < d || ldc < n || !X || !T || !dc ||
      !partial)
    return fail(DKM_E_ARG, "kpp eval: bad arguments");
  const KppGrid g = kp_grid(n, d, L);
  switch (kp_bucket(L)) {
    case 4:
      return kpp_eval_launch<TX, 4>(X, n, d, ldx, T, L, mind, dc, ldc,
                                    partial, g, s);
    case 8:
      return kpp_eval_launch<TX, 8>(X, n, d, ldx, T, L, mind, dc, ldc,
                                    partial, g, s);
    case 16:
      return kpp_eval_launch<TX, 16>(X, n, d, ldx, T, L, mind, dc, ldc,
                                     partial, g, s);
    default:
      return kpp_eval_launch<TX, 32>(X, n, d, ldx, T, L, mind, dc, ldc,
                                     partial, g, s);
  }
}

template <class TX>
int kpp_sample(const TX *X, int64_t n, int64_t d, int64_t ldx,
               const double *mind, const double *bsum, double *bscan,
               const double *pot, const double *u, int64_t L, int32_t *rows,
               double *T, hipStream_t s) {
  if (!kp_shape_ok(n, d, L) || ldx < d || !X || !mind || !bsum || !bscan ||
      !pot || !u || !rows || !T)
    return fail(DKM_E_ARG, "kpp sample: bad arguments");
  const int64_t nseg = (n + KP_SEG - 1) / KP_SEG;
  k_kpp_sample<TX><<<1, KP_SB, 0, s>>>(X, n, (int)d, ldx, mind, bsum, bscan,
                                       nseg, pot, u, (int)L, rows, T);
  return check_launch("kpp sample");
}

}  // namespace

}  // namespace dkm

using namespace dkm;

extern "C" {

size_t dkm_kpp_workspace_bytes(int64_t n, int64_t d, int64_t L) {
  if (!kp_shape_ok(n, d, L)) return 0;
  const int64_t nseg = (n + KP_SEG - 1) / KP_SEG;
  const int64_t nb1 = kp_grid(n, d, 1).blocks, nbl = kp_grid(n, d, L).blocks;
  // dc, mind, bsum + bscan, partial, the trial table, the rows, the scalars
  return (size_t)(L * n + n + 2 * nseg + (nb1 > nbl ? nb1 : nbl) * L + L * d) *
             sizeof(double) +
         (size_t)L * sizeof(int32_t) + 256;
}

int64_t dkm_kpp_blocks(int64_t n, int64_t d, int64_t L) {
  return kp_shape_ok(n, d, L) ? kp_grid(n, d, L).blocks : 0;
}

int dkm_kpp_eval_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                     const double *trials, int64_t L, const double *mind,
                     double *dc, int64_t ldc, double *partial, void *stream) {
  return kpp_eval<double>(X, n, d, ldx, trials, L, mind, dc, ldc, partial,
                          (hipStream_t)stream);
}

int dkm_kpp_eval_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                     const double *trials, int64_t L, const double *mind,
                     double *dc, int64_t ldc, double *partial, void *stream) {
  return kpp_eval<float>(X, n, d, ldx, trials, L, mind, dc, ldc, partial,
                         (hipStream_t)stream);
}

int dkm_kpp_commit(int64_t n, int64_t L, const double *dc, int64_t ldc,
                   const double *partial, int64_t nblocks, const int32_t *rows,
                   int first, double *mind, double *bsum, double *pot,
                   int32_t *best, int64_t *index_out, void *stream) {
  if (n < 1 || n > INT32_MAX || L < 1 || L > DKM_KPP_MAX_TRIALS || !dc ||
      ldc < n || !partial || nblocks < 1 || !rows || !mind || !bsum || !pot ||
      !best || !index_out)
    return fail(DKM_E_ARG, "kpp commit: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  k_kpp_choose<<<1, KP_SB, 0, s>>>(partial, nblocks, (int)L, rows, pot, best,
                                   index_out);
  if (int r = check_launch("kpp choose")) return r;
  k_kpp_commit<<<(unsigned)((n + KP_SEG - 1) / KP_SEG), KP_B, 0, s>>>(
      n, dc, ldc, best, first, mind, bsum);
  return check_launch("kpp commit");
}

int dkm_kpp_sample_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                       const double *mind, const double *bsum, double *bscan,
                       const double *pot, const double *u, int64_t L,
                       int32_t *rows, double *trials, void *stream) {
  return kpp_sample<double>(X, n, d, ldx, mind, bsum, bscan, pot, u, L, rows,
                            trials, (hipStream_t)stream);
}

int dkm_kpp_sample_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                       const double *mind, const double *bsum, double *bscan,
                       const double *pot, const double *u, int64_t L,
                       int32_t *rows, double *trials, void *stream) {
  return kpp_sample<float>(X, n, d, ldx, mind, bsum, bscan, pot, u, L, rows,
                           trials, (hipStream_t)stream);
}

}  // extern "C"

// Code-object preload (dkm_preload): see dkm_ordered.hip.
namespace dkm {
DKM_TU_FLAGS(kpp, 0)
__global__ void k_tu_kpp() {}
int preload_kpp() {
  hipFuncAttributes a;
  const bool ok = hipFuncGetAttributes(&a, (const void *)k_tu_kpp) == hipSuccess;
  return ok ? 0 : 1;
}
}  // namespace dkm
