// dkm_rfr.hip -- the kernels of RandomForestRegressor: exact CART on fp64
// targets with the variance-reduction proxy -(SL^2 / |L| + SR^2 / |R|), the
// regression sibling of dkm_rf.hip.  The ranks, the sorted orders, the member
// lists segmented by node, dkm_rf_best and dkm_rf_partition are the
// classifier's; what is here is the split search over running fp64 sums, the
// node statistics and the prediction.  No floating-point atomic, no grid-wide
// barrier.
//
//   k_rfr_split_lds     one workgroup per (node, feature) pair whose node has
//                       at most DKM_RFR_LDS_MAX members.  A key is 64 bits:
//                       rank << b | j, j the position in the node's segment
//                       and 2^b the padded size.  Gather, bitonic sort in LDS,
//                       then rfr_chunk over the whole node; an entry's target
//                       is y[members[start + j]] (weight 1: the members are
//                       listed with their multiplicity).
//   k_rfr_split_stream  one workgroup per pair walks the feature's sorted
//                       order RFR_B entries at a time and compacts the node's
//                       entries (rank, multiplicity, target) into an LDS
//                       buffer of RFR_CH + RFR_B entries in order.  Whenever
//                       more than RFR_CH are there, the first RFR_CH are
//                       scored (the one after them is known, so is the rank
//                       that follows every scored entry) and the rest, at
//                       least one, moves to the front.  The left sum and the
//                       left weight are carried in LDS.  Chunks are therefore
//                       RFR_CH entries each but the last, wherever the node's
//                       entries lie in the order.
//   rfr_chunk           m entries, thread t owns the run [t L, (t + 1) L),
//                       L = ceil(m / RFR_B).
//                       Pass 1: p_t = ((0 + w y) + w y) + ... over the run in
//                       order, with the weights' integer sum.
//                       Scan: within a wave the inclusive Hillis-Steele scan
//                       I <- shfl_up(I, o) + I for o = 1, 2, 4 .. 32; E_t is
//                       I of the lane below (0 for lane 0).  The waves' totals
//                       W_v = I of lane 63 are added in wave order from 0:
//                       O_w = ((0 + W_0) + W_1) + ... + W_{w-1}.
//                       Pass 2: SL starts at carry + (O_w + E_t) and takes the
//                       run's w y one by one; at a run end (the next entry's
//                       rank differs, or the node's last position) the score
//                       is -(SL SL / ll + SR SR / rl), SR = S - SL, every
//                       operation rounded on its own; "<=" keeps the last
//                       minimum.
//                       After the chunk: carry <- carry + O_{RFR_W}.
//                       The association is a function of (size, regime) only
//                       (and of the multiplicities, which in the streamed
//                       regime fold equal samples into one entry w y, in the
//                       LDS regime into w entries y): the same input gives the
//                       same bits from run to run.  The two regimes agree
//                       where every sum is exact (integer-valued targets),
//                       not in general.
//   k_rfr_node_stats    one workgroup per node: {sum, min, max} of its
//                       members' targets.  Thread t adds the entries t,
//                       t + RFR_SB, .. in order; the partials are then halved
//                       in LDS, slot t taking slot t + o for o = RFR_SB / 2,
//                       .. 1.
//   k_rfr_predict       one row per thread walks every tree; the leaf values
//                       are added in tree order and divided by the trees.
//
// RFR_B, RFR_CH, RFR_SB and DKM_RFR_LDS_MAX are not tuned: they are the
// classifier's numbers (256 threads, a 2048-entry buffer) and the largest
// power of two that fits; nobody has measured another choice on gfx950.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "dkm_internal.h"

namespace dkm {

namespace {

constexpr int RFR_B = 256;                   // threads of the split kernels
constexpr int RFR_W = RFR_B / WAVE;
constexpr int RFR_CH = 2048;                 // entries scored per streamed chunk
constexpr int RFR_SB = 256;                  // threads of k_rfr_node_stats
constexpr uint64_t RFR_PAD = ~0ull;
// most pairs / nodes of a launch: 4 * index stays an int
constexpr int64_t RFR_MAX_LIST = 1 << 28;
static_assert(RFR_CH >= 2 * RFR_B, "the moved tail never overlaps itself");
static_assert((DKM_RFR_LDS_MAX & (DKM_RFR_LDS_MAX - 1)) == 0, "power of two");
// rank (24 bits) above the position bits in one 64-bit key
static_assert(DKM_RF_MAX_SAMPLES <= (1 << 24) && DKM_RFR_LDS_MAX <= (1 << 30),
              "key");

struct Best {
  double score;
  int pos, lo, hi;
};

// the block's common small state
struct Shared {
  double carry_s;                      // target sum left of the chunk
  int32_t carry_w;                     // weight left of the chunk
  double ws[RFR_W];                    // the waves' run sums
  int32_t ww[RFR_W];
  int32_t wsum[RFR_W];                 // the compaction's counts
  double rs[RFR_B];
  int32_t rp[RFR_B];
};
// the largest power of two whose 64-bit keys fit next to Shared in 160 KiB
static_assert(DKM_RFR_LDS_MAX * 8 + sizeof(Shared) <= 160 * 1024 &&
                  2 * DKM_RFR_LDS_MAX * 8 > 160 * 1024, "LDS budget");
static_assert((RFR_CH + RFR_B) * 16 + sizeof(Shared) <= 64 * 1024,
              "the streamed buffer is static LDS");

__device__ inline int lane_id() { return threadIdx.x & (WAVE - 1); }

// the sorted node in LDS: entry j is key >> b, its target one gather away
struct LdsSrc {
  const uint64_t *keys;
  const int32_t *mem;                  // the node's segment
  const double *y;
  int b;
  __device__ int rank(int j) const { return (int)(keys[j] >> b); }
  __device__ int weight(int) const { return 1; }
  __device__ double target(int j) const {
    return y[mem[(int)(keys[j] & ((1ull << b) - 1ull))]];
  }
};

// the streamed buffer
struct BufSrc {
  const int32_t *rk, *wt;
  const double *yv;
  __device__ int rank(int j) const { return rk[j]; }
  __device__ int weight(int j) const { return wt[j]; }
  __device__ double target(int j) const { return yv[j]; }
};

// See the header comment.  Entries [0, avail) in rank order; [0, m) are
// scored, m <= avail.  An entry at avail - 1 has no known successor: it is a
// run end (the callers let that happen at the node's last position only).
// All threads call this.
template <class Src>
__device__ void rfr_chunk(const Src &src, int m, int avail, int size, double S,
                          Shared &sh, Best &best) {
  const int t = threadIdx.x, lane = lane_id(), w = t >> 6;
  const int L = (m + RFR_B - 1) / RFR_B;
  const int j0 = min(t * L, m), j1 = min(j0 + L, m);
  double is = 0.0;
  int iw = 0;
  for (int j = j0; j < j1; ++j) {
    const int wt = src.weight(j);
    is += (double)wt * src.target(j);
    iw += wt;
  }
  for (int o = 1; o < WAVE; o <<= 1) {
    const double vs = __shfl_up(is, o);
    const int vw = __shfl_up(iw, o);
    if (lane >= o) {
      is = vs + is;
      iw = vw + iw;
    }
  }
  double es = __shfl_up(is, 1);
  int ew = __shfl_up(iw, 1);
  if (lane == 0) {
    es = 0.0;
    ew = 0;
  }
  if (lane == WAVE - 1) {
    sh.ws[w] = is;
    sh.ww[w] = iw;
  }
  __syncthreads();
  double os = 0.0, ts = 0.0;
  int ow = 0, tw = 0;
  for (int v = 0; v < RFR_W; ++v) {
    if (v == w) {
      os = ts;
      ow = tw;
    }
    ts += sh.ws[v];
    tw += sh.ww[v];
  }
  double SL = sh.carry_s + (os + es);
  int ll = sh.carry_w + (ow + ew);
  for (int j = j0; j < j1; ++j) {
    const int r = src.rank(j), wt = src.weight(j);
    SL += (double)wt * src.target(j);
    ll += wt;
    const bool known = j + 1 < avail;
    const int nr = known ? src.rank(j + 1) : r;
    if (!known || nr != r) {
      const double SR = S - SL;
      const int rl = ll == size ? 1 : size - ll;
      const double a = SL * SL / (double)ll, b = SR * SR / (double)rl;
      const double s = -(a + b);
      if (s <= best.score) {
        best.score = s;
        best.pos = ll - 1;
        best.lo = r;
        best.hi = nr;
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    sh.carry_s += ts;
    sh.carry_w += tw;
  }
  __syncthreads();
}

// the block's (score, pos): smallest score, then largest pos; the owner of
// the winning position writes the pair's result (dkm_rf.hip's rf_finish)
__device__ void rfr_finish(const Best &best, int size, Shared &sh,
                           double *score, int32_t *cut) {
  const int t = threadIdx.x;
  sh.rs[t] = best.score;
  sh.rp[t] = best.pos;
  __syncthreads();
  for (int o = RFR_B / 2; o > 0; o >>= 1) {
    if (t < o) {
      const double a = sh.rs[t], b = sh.rs[t + o];
      const int pa = sh.rp[t], pb = sh.rp[t + o];
      if (b < a || (b == a && pb > pa)) {
        sh.rs[t] = b;
        sh.rp[t] = pb;
      }
    }
    __syncthreads();
  }
  const int win = sh.rp[0];
  if (win < 0) {                       // nothing was scored: no cut
    if (t == 0) {
      *score = DBL_MAX;
      cut[0] = size - 1;
      cut[1] = cut[2] = 0;
    }
  } else if (best.pos == win) {
    *score = best.score;
    cut[0] = best.pos;
    cut[1] = best.lo;
    cut[2] = best.hi;
  }
}

__device__ inline void rfr_begin(Shared &sh, Best &best) {
  if (threadIdx.x == 0) {
    sh.carry_s = 0.0;
    sh.carry_w = 0;
  }
  best.score = DBL_MAX;
  best.pos = -1;
  best.lo = best.hi = 0;
}

// does the LDS regime take a node of `size` members?
__device__ inline bool rfr_is_lds(int size, int mode) {
  return mode == DKM_RF_LDS ||
         (mode == DKM_RF_AUTO && size <= DKM_RFR_LDS_MAX);
}

}  // namespace

// nodes[i] = {tree, start, size, id}; pairs[p] = {node, feature}; nsum[i]:
// the node's target sum
__global__ void __launch_bounds__(RFR_B)
    k_rfr_split_lds(const int32_t *__restrict__ rank, int64_t n,
                    const double *__restrict__ y,
                    const int32_t *__restrict__ members,
                    const int32_t *__restrict__ nodes,
                    const double *__restrict__ nsum,
                    const int32_t *__restrict__ pairs, int mode, int pmax,
                    double *__restrict__ score, int32_t *__restrict__ cut) {
  extern __shared__ uint64_t rfr_dyn[];
  __shared__ Shared sh;
  const int p = blockIdx.x, t = threadIdx.x;
  const int node = pairs[2 * p], f = pairs[2 * p + 1];
  const int tree = nodes[4 * node], start = nodes[4 * node + 1];
  const int size = nodes[4 * node + 2];
  if (!rfr_is_lds(size, mode)) return;
  int P = 1, b = 0;
  while (P < size) {
    P <<= 1;
    ++b;
  }
  if (P > pmax) return;                      // larger than the launch's LDS
  uint64_t *keys = rfr_dyn;
  Best best;
  rfr_begin(sh, best);
  const int32_t *mem = members + (int64_t)tree * n + start;
  const int32_t *rk = rank + (int64_t)f * n;
  for (int j = t; j < P; j += RFR_B)
    keys[j] = j < size ? ((uint64_t)(uint32_t)rk[mem[j]] << b) | (uint64_t)j
                       : RFR_PAD;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < P; i += RFR_B) {
        const int x = i ^ j;
        if (x > i) {
          const uint64_t a = keys[i], c = keys[x];
          const bool up = (i & k) == 0;
          if ((a > c) == up) {
            keys[i] = c;
            keys[x] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  const LdsSrc src{keys, mem, y, b};
  rfr_chunk(src, size, size, size, nsum[node], sh, best);
  rfr_finish(best, size, sh, score + p, cut + 3 * (int64_t)p);
}

__global__ void __launch_bounds__(RFR_B)
    k_rfr_split_stream(const int32_t *__restrict__ rank,
                       const int32_t *__restrict__ order, int64_t n,
                       const double *__restrict__ y,
                       const int32_t *__restrict__ node_of,
                       const int32_t *__restrict__ weight,
                       const int32_t *__restrict__ nodes,
                       const double *__restrict__ nsum,
                       const int32_t *__restrict__ pairs, int mode,
                       double *__restrict__ score, int32_t *__restrict__ cut) {
  __shared__ Shared sh;
  __shared__ double yv[RFR_CH + RFR_B];
  __shared__ int32_t rkb[RFR_CH + RFR_B];
  __shared__ int32_t wtb[RFR_CH + RFR_B];
  const int p = blockIdx.x, t = threadIdx.x, lane = lane_id(), w = t >> 6;
  const int node = pairs[2 * p], f = pairs[2 * p + 1];
  const int tree = nodes[4 * node], size = nodes[4 * node + 2];
  const int id = nodes[4 * node + 3];
  if (rfr_is_lds(size, mode)) return;
  Best best;
  rfr_begin(sh, best);
  const double S = nsum[node];
  const int32_t *ord = order + (int64_t)f * n, *rk = rank + (int64_t)f * n;
  const int32_t *nof = node_of + (int64_t)tree * n;
  const int32_t *wgt = weight + (int64_t)tree * n;
  const BufSrc src{rkb, wtb, yv};
  int m = 0;                                 // entries in the buffer (uniform)
  __syncthreads();
  for (int64_t base = 0; base < n; base += RFR_B) {
    const int64_t i = base + t;
    int s = -1;
    if (i < n) {
      s = ord[i];
      if (nof[s] != id) s = -1;
    }
    const unsigned long long bal = __ballot(s >= 0);
    if (lane == 0) sh.wsum[w] = __popcll(bal);
    __syncthreads();
    int off = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
    for (int v = 0; v < RFR_W; ++v) {
      const int c = sh.wsum[v];
      if (v < w) off += c;
      total += c;
    }
    if (s >= 0) {                            // m <= RFR_CH here
      rkb[m + off] = rk[s];
      wtb[m + off] = wgt[s];
      yv[m + off] = y[s];
    }
    m += total;
    __syncthreads();
    if (m > RFR_CH) {
      rfr_chunk(src, RFR_CH, m, size, S, sh, best);
      const int rest = m - RFR_CH;           // 1 .. RFR_B
      if (t < rest) {
        rkb[t] = rkb[RFR_CH + t];
        wtb[t] = wtb[RFR_CH + t];
        yv[t] = yv[RFR_CH + t];
      }
      m = rest;
      __syncthreads();
    }
  }
  if (m > 0) rfr_chunk(src, m, m, size, S, sh, best);
  rfr_finish(best, size, sh, score + p, cut + 3 * (int64_t)p);
}

// stats[i] = {sum, min, max}; an empty node gives {0, +inf, -inf}
__global__ void __launch_bounds__(RFR_SB)
    k_rfr_node_stats(const double *__restrict__ y, int64_t n,
                     const int32_t *__restrict__ members,
                     const int32_t *__restrict__ nodes,
                     double *__restrict__ stats) {
  __shared__ double ss[RFR_SB], smin[RFR_SB], smax[RFR_SB];
  const int i = blockIdx.x, t = threadIdx.x;
  const int tree = nodes[4 * i], start = nodes[4 * i + 1];
  const int size = nodes[4 * i + 2];
  const int32_t *mem = members + (int64_t)tree * n + start;
  double s = 0.0, lo = HUGE_VAL, hi = -HUGE_VAL;
  for (int j = t; j < size; j += RFR_SB) {
    const double v = y[mem[j]];
    s += v;
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  ss[t] = s;
  smin[t] = lo;
  smax[t] = hi;
  __syncthreads();
  for (int o = RFR_SB / 2; o > 0; o >>= 1) {
    if (t < o) {
      ss[t] = ss[t] + ss[t + o];
      smin[t] = smin[t + o] < smin[t] ? smin[t + o] : smin[t];
      smax[t] = smax[t + o] > smax[t] ? smax[t + o] : smax[t];
    }
    __syncthreads();
  }
  if (t == 0) {
    stats[3 * (int64_t)i] = ss[0];
    stats[3 * (int64_t)i + 1] = smin[0];
    stats[3 * (int64_t)i + 2] = smax[0];
  }
}

// feature[v] < 0: a leaf, child[2 v] its leaf number
template <class TX>
__global__ void __launch_bounds__(RFR_B)
    k_rfr_predict(const TX *__restrict__ X, int64_t n, int64_t ldx,
                  const int32_t *__restrict__ roots, int T,
                  const int32_t *__restrict__ feature,
                  const double *__restrict__ value,
                  const int32_t *__restrict__ child,
                  const double *__restrict__ leaf, double *__restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * RFR_B + threadIdx.x;
  if (r >= n) return;
  const TX *x = X + r * ldx;
  double acc = 0.0;
  for (int tr = 0; tr < T; ++tr) {
    int v = roots[tr];
    while (feature[v] >= 0)
      v = child[2 * v + ((double)x[feature[v]] <= value[v] ? 0 : 1)];
    acc += leaf[child[2 * v]];
  }
  out[r] = acc / (double)T;
}

namespace {

template <class TX>
int rfr_predict(const TX *X, int64_t n, int64_t d, int64_t ldx,
                const int32_t *roots, int64_t T, const int32_t *feature,
                const double *value, const int32_t *child, const double *leaf,
                double *out, hipStream_t s) {
  if (n < 0 || n > INT32_MAX || d < 1 || ldx < d || T < 1 || T > INT32_MAX ||
      !roots || !feature || !value || !child || !leaf ||
      (n > 0 && (!X || !out)))
    return fail(DKM_E_ARG, "rfr predict: bad arguments");
  if (n == 0) return 0;
  k_rfr_predict<TX><<<(unsigned)((n + RFR_B - 1) / RFR_B), RFR_B, 0, s>>>(
      X, n, ldx, roots, (int)T, feature, value, child, leaf, out);
  return check_launch("rfr predict");
}

}  // namespace

}  // namespace dkm

using namespace dkm;

extern "C" {

int dkm_rfr_split(const int32_t *rank, const int32_t *order, int64_t n,
                  const double *y, const int32_t *members,
                  const int32_t *node_of, const int32_t *weight,
                  const int32_t *nodes, const double *nsum,
                  const int32_t *pairs, int64_t n_pairs, int64_t max_size,
                  int mode, double *score, int32_t *cut, void *stream) {
  if (!rank || !order || n < 1 || n >= DKM_RF_MAX_SAMPLES || !y || !members ||
      !node_of || !weight || !nodes || !nsum || !pairs || n_pairs < 0 ||
      n_pairs > RFR_MAX_LIST || max_size < 1 || max_size > n ||
      mode < DKM_RF_AUTO || mode > DKM_RF_STREAM ||
      (n_pairs > 0 && (!score || !cut)) ||
      (mode == DKM_RF_LDS && max_size > DKM_RFR_LDS_MAX))
    return fail(DKM_E_ARG, "rfr split: bad arguments");
  if (n_pairs == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (mode != DKM_RF_STREAM) {
    int64_t P = 1;
    const int64_t top = max_size < DKM_RFR_LDS_MAX ? max_size : DKM_RFR_LDS_MAX;
    while (P < top) P <<= 1;
    const size_t lds = (size_t)P * 8;
    if (hipFuncSetAttribute((const void *)k_rfr_split_lds,
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
      return fail(DKM_E_LAUNCH, "rfr split: LDS attribute");
    k_rfr_split_lds<<<(unsigned)n_pairs, RFR_B, lds, s>>>(
        rank, n, y, members, nodes, nsum, pairs, mode, (int)P, score, cut);
    const int r = check_launch("rfr split lds");
    if (r) return r;
  }
  if (mode == DKM_RF_STREAM ||
      (mode == DKM_RF_AUTO && max_size > DKM_RFR_LDS_MAX)) {
    k_rfr_split_stream<<<(unsigned)n_pairs, RFR_B, 0, s>>>(
        rank, order, n, y, node_of, weight, nodes, nsum, pairs, mode, score,
        cut);
    return check_launch("rfr split stream");
  }
  return 0;
}

int dkm_rfr_node_stats(const double *y, int64_t n, const int32_t *members,
                       const int32_t *nodes, int64_t n_nodes, double *stats,
                       void *stream) {
  if (!y || n < 1 || n >= DKM_RF_MAX_SAMPLES || !members || !nodes ||
      n_nodes < 1 || n_nodes > RFR_MAX_LIST || !stats)
    return fail(DKM_E_ARG, "rfr node stats: bad arguments");
  k_rfr_node_stats<<<(unsigned)n_nodes, RFR_SB, 0, (hipStream_t)stream>>>(
      y, n, members, nodes, stats);
  return check_launch("rfr node stats");
}

int dkm_rfr_predict_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                        const int32_t *roots, int64_t T,
                        const int32_t *feature, const double *value,
                        const int32_t *child, const double *leaf, double *out,
                        void *stream) {
  return rfr_predict<double>(X, n, d, ldx, roots, T, feature, value, child,
                             leaf, out, (hipStream_t)stream);
}

int dkm_rfr_predict_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                        const int32_t *roots, int64_t T,
                        const int32_t *feature, const double *value,
                        const int32_t *child, const double *leaf, double *out,
                        void *stream) {
  return rfr_predict<float>(X, n, d, ldx, roots, T, feature, value, child,
                            leaf, out, (hipStream_t)stream);
}

}  // extern "C"

// Code-object preload (dkm_preload): see dkm_ordered.hip.
namespace dkm {
DKM_TU_FLAGS(rfr, 0)
__global__ void k_tu_rfr() {}
int preload_rfr() {
  hipFuncAttributes a;
  const bool ok = hipFuncGetAttributes(&a, (const void *)k_tu_rfr) == hipSuccess;
  return ok ? 0 : 1;
}
}  // namespace dkm
