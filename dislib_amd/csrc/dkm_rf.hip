// dkm_rf.hip -- the kernels of RandomForestClassifier (exact CART with the
// Gini proxy of the reference's dislib/classification/rf/test_split.py).
// Growth is integer work on the per-feature dense ranks of the samples: no
// floating-point sample is read after the preparation.  A tree's members are
// kept expanded (a sample drawn w times by the bootstrap is listed w times),
// segmented by node; node_of names every sample's node for the regime that
// walks the global sorted order.  No floating-point atomic, no grid-wide
// barrier; the integer sums are exact, so the same input gives the same bits
// from run to run, and both regimes give the same bits as each other.
//
// A key is rank << RF_CB | class (rank < 2^24, class < 32).
//
//   k_rf_split_lds     one workgroup per (node, feature) pair whose node has at
//                      most DKM_RF_LDS_MAX members: gather the keys, bitonic
//                      sort in LDS (padded to a power of two), then rf_chunk.
//   k_rf_split_stream  one workgroup per pair walks the feature's sorted order
//                      RF_B entries at a time, compacts the node's entries
//                      (key, multiplicity) into an LDS buffer in order and runs
//                      rf_chunk on the buffer whenever it fills, all but its
//                      last entry: that one moves to the front, so the rank that
//                      follows an entry is always known.  Class counters and
//                      the left size are carried in LDS.
//   rf_chunk           thread t owns a run of consecutive entries.  It counts
//                      its run's classes into column t of cnt[class][thread];
//                      a wave per class scans the columns (4 entries per lane,
//                      shuffles across lanes); the thread then replays its run,
//                      its column being the left counts L_c, and keeps sum L_c^2
//                      and sum R_c^2 up to date in int64.  At a run end (the
//                      next entry's rank differs, or the node's last position)
//                      the score is -(lw / ll + rw / rl) in fp64 as the
//                      reference forms it; "<=" keeps the last minimum.
//   k_rf_best          one thread per node: the first strictly smallest score
//                      over its pairs in draw order.
//   k_rf_partition     one workgroup per node: stable two-way partition of its
//                      segment by rank <= rank_lo with ballot scans, node_of of
//                      the children, the left child's class counts (integer
//                      LDS atomics).  A node without a cut is copied.
//   k_rf_predict       one row per thread walks every tree.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "dkm_internal.h"

namespace dkm {

namespace {

constexpr int RF_B = 256;                    // threads of the split kernels
constexpr int RF_W = RF_B / WAVE;
constexpr int RF_CB = 5;                     // class bits of a key
constexpr int RF_CH = 2048;                  // entries of the streaming buffer
constexpr int RF_PB = 1024;                  // threads of k_rf_partition
constexpr uint32_t RF_PAD = 0xffffffffu;
// most pairs / nodes of a launch: 4 * index stays an int
constexpr int64_t RF_MAX_LIST = 1 << 28;
static_assert((1 << RF_CB) == DKM_RF_MAX_CLASSES, "class bits");
static_assert(((int64_t)DKM_RF_MAX_SAMPLES << RF_CB) <= (1ll << 31), "key");
static_assert((DKM_RF_LDS_MAX & (DKM_RF_LDS_MAX - 1)) == 0, "power of two");
// keys + uint16 counters + the reduction's scratch within 160 KiB
static_assert(DKM_RF_LDS_MAX * 4 + DKM_RF_MAX_CLASSES * RF_B * 2 + 8192 <=
                  160 * 1024, "LDS budget");
static_assert(RF_CH >= 2 * RF_B, "a tile always fits the buffer");

struct Best {
  double score;
  int pos, lo, hi;
};

// the block's common small state
struct Shared {
  int32_t tot[DKM_RF_MAX_CLASSES];     // the node's class counts
  int32_t carry[DKM_RF_MAX_CLASSES];   // counts left of the chunk
  int32_t ctot[DKM_RF_MAX_CLASSES];    // the chunk's counts
  double rs[RF_B];
  int32_t rp[RF_B];
  int32_t wsum[RF_W];
};

__device__ inline int lane_id() { return threadIdx.x & (WAVE - 1); }

// See the header comment.  keys[0 .. avail): entries in rank order, wts their
// multiplicities (nullptr: 1); entries [0, m) are scored, m <= avail.  An
// entry at avail - 1 has no known successor: it is a run end (the caller lets
// that happen at the node's last position only).  All threads call this.
template <class CT>
__device__ void rf_chunk(const uint32_t *keys, const int32_t *wts, int m,
                         int avail, int C, int size, Shared &sh, CT *cnt,
                         Best &best) {
  const int t = threadIdx.x, lane = lane_id(), w = t >> 6;
  const int L = (m + RF_B - 1) / RF_B;
  const int j0 = min(t * L, m), j1 = min(j0 + L, m);
  for (int c = 0; c < C; ++c) cnt[c * RF_B + t] = 0;
  for (int j = j0; j < j1; ++j) {
    const int c = keys[j] & (DKM_RF_MAX_CLASSES - 1);
    cnt[c * RF_B + t] += (CT)(wts ? wts[j] : 1);
  }
  __syncthreads();
  for (int c = w; c < C; c += RF_W) {
    CT *p = cnt + c * RF_B + lane * 4;
    const int a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3];
    const int s = a0 + a1 + a2 + a3;
    int incl = s;
    for (int o = 1; o < WAVE; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    const int ex = incl - s;
    p[0] = (CT)ex;
    p[1] = (CT)(ex + a0);
    p[2] = (CT)(ex + a0 + a1);
    p[3] = (CT)(ex + a0 + a1 + a2);
    if (lane == WAVE - 1) sh.ctot[c] = incl;
  }
  __syncthreads();
  if (j0 < j1) {
    int64_t lw = 0, rw = 0;
    int ll = 0;
    for (int c = 0; c < C; ++c) {
      const int64_t l = sh.carry[c] + (int)cnt[c * RF_B + t];
      const int64_t r = sh.tot[c] - l;
      lw += l * l;
      rw += r * r;
      ll += (int)l;
    }
    for (int j = j0; j < j1; ++j) {
      const uint32_t key = keys[j];
      const int c = key & (DKM_RF_MAX_CLASSES - 1);
      const int64_t wt = wts ? wts[j] : 1;
      const int lc = (int)cnt[c * RF_B + t];
      const int64_t l = sh.carry[c] + lc, r = sh.tot[c] - l;
      lw += wt * (2 * l + wt);
      rw -= wt * (2 * r - wt);
      ll += (int)wt;
      cnt[c * RF_B + t] = (CT)(lc + (int)wt);
      const bool known = j + 1 < avail;
      const uint32_t nxt = known ? keys[j + 1] : 0u;
      if (!known || (nxt >> RF_CB) != (key >> RF_CB)) {
        const int rl = ll == size ? 1 : size - ll;
        const double s = -((double)lw / (double)ll + (double)rw / (double)rl);
        if (s <= best.score) {
          best.score = s;
          best.pos = ll - 1;
          best.lo = (int)(key >> RF_CB);
          best.hi = known ? (int)(nxt >> RF_CB) : best.lo;
        }
      }
    }
  }
  __syncthreads();
  if (t < C) sh.carry[t] += sh.ctot[t];
  __syncthreads();
}

// the block's (score, pos): smallest score, then largest pos; the owner of
// the winning position writes the pair's result
__device__ void rf_finish(const Best &best, int size, Shared &sh,
                          double *score, int32_t *cut) {
  const int t = threadIdx.x;
  sh.rs[t] = best.score;
  sh.rp[t] = best.pos;
  __syncthreads();
  for (int o = RF_B / 2; o > 0; o >>= 1) {
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

__device__ inline void rf_begin(Shared &sh, const int32_t *ncounts, int C,
                                Best &best) {
  if (threadIdx.x < DKM_RF_MAX_CLASSES) {
    sh.tot[threadIdx.x] = (int)threadIdx.x < C ? ncounts[threadIdx.x] : 0;
    sh.carry[threadIdx.x] = 0;
  }
  best.score = DBL_MAX;
  best.pos = -1;
  best.lo = best.hi = 0;
}

// does the LDS regime take a node of `size` members?
__device__ inline bool rf_is_lds(int size, int mode) {
  return mode == DKM_RF_LDS || (mode == DKM_RF_AUTO && size <= DKM_RF_LDS_MAX);
}

}  // namespace

// nodes[i] = {tree, start, size, id}; pairs[p] = {node, feature}
__global__ void __launch_bounds__(RF_B)
    k_rf_split_lds(const int32_t *__restrict__ rank, int64_t n,
                   const int32_t *__restrict__ y, int C,
                   const int32_t *__restrict__ members,
                   const int32_t *__restrict__ nodes,
                   const int32_t *__restrict__ ncounts,
                   const int32_t *__restrict__ pairs, int mode, int pmax,
                   double *__restrict__ score, int32_t *__restrict__ cut) {
  extern __shared__ uint32_t rf_dyn[];
  __shared__ Shared sh;
  const int p = blockIdx.x, t = threadIdx.x;
  const int node = pairs[2 * p], f = pairs[2 * p + 1];
  const int tree = nodes[4 * node], start = nodes[4 * node + 1];
  const int size = nodes[4 * node + 2];
  if (!rf_is_lds(size, mode)) return;
  int P = 1;
  while (P < size) P <<= 1;
  if (P > pmax) return;                      // larger than the launch's LDS
  uint32_t *keys = rf_dyn;
  uint16_t *cnt = (uint16_t *)(rf_dyn + P);
  Best best;
  rf_begin(sh, ncounts + (int64_t)node * C, C, best);
  const int32_t *mem = members + (int64_t)tree * n + start;
  const int32_t *rk = rank + (int64_t)f * n;
  for (int j = t; j < P; j += RF_B) {
    uint32_t key = RF_PAD;
    if (j < size) {
      const int s = mem[j];
      key = ((uint32_t)rk[s] << RF_CB) | (uint32_t)y[s];
    }
    keys[j] = key;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < P; i += RF_B) {
        const int x = i ^ j;
        if (x > i) {
          const uint32_t a = keys[i], b = keys[x];
          const bool up = (i & k) == 0;
          if ((a > b) == up) {
            keys[i] = b;
            keys[x] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  rf_chunk<uint16_t>(keys, nullptr, size, size, C, size, sh, cnt, best);
  rf_finish(best, size, sh, score + p, cut + 3 * (int64_t)p);
}

__global__ void __launch_bounds__(RF_B)
    k_rf_split_stream(const int32_t *__restrict__ rank,
                      const int32_t *__restrict__ order, int64_t n,
                      const int32_t *__restrict__ y, int C,
                      const int32_t *__restrict__ node_of,
                      const int32_t *__restrict__ weight,
                      const int32_t *__restrict__ nodes,
                      const int32_t *__restrict__ ncounts,
                      const int32_t *__restrict__ pairs, int mode,
                      double *__restrict__ score, int32_t *__restrict__ cut) {
  __shared__ Shared sh;
  __shared__ uint32_t keys[RF_CH];
  __shared__ int32_t wts[RF_CH];
  __shared__ uint32_t cnt[DKM_RF_MAX_CLASSES * RF_B];
  const int p = blockIdx.x, t = threadIdx.x, lane = lane_id(), w = t >> 6;
  const int node = pairs[2 * p], f = pairs[2 * p + 1];
  const int tree = nodes[4 * node], size = nodes[4 * node + 2];
  const int id = nodes[4 * node + 3];
  if (rf_is_lds(size, mode)) return;
  Best best;
  rf_begin(sh, ncounts + (int64_t)node * C, C, best);
  const int32_t *ord = order + (int64_t)f * n, *rk = rank + (int64_t)f * n;
  const int32_t *nof = node_of + (int64_t)tree * n;
  const int32_t *wgt = weight + (int64_t)tree * n;
  int m = 0;                                 // entries in the buffer (uniform)
  __syncthreads();
  for (int64_t base = 0; base < n; base += RF_B) {
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
    for (int v = 0; v < RF_W; ++v) {
      const int c = sh.wsum[v];
      if (v < w) off += c;
      total += c;
    }
    if (s >= 0) {
      keys[m + off] = ((uint32_t)rk[s] << RF_CB) | (uint32_t)y[s];
      wts[m + off] = wgt[s];
    }
    m += total;
    __syncthreads();
    if (m > RF_CH - RF_B) {                  // the next tile might not fit
      rf_chunk<uint32_t>(keys, wts, m - 1, m, C, size, sh, cnt, best);
      if (t == 0) {
        keys[0] = keys[m - 1];
        wts[0] = wts[m - 1];
      }
      m = 1;
      __syncthreads();
    }
  }
  if (m > 0) rf_chunk<uint32_t>(keys, wts, m, m, C, size, sh, cnt, best);
  rf_finish(best, size, sh, score + p, cut + 3 * (int64_t)p);
}

// pspan[i] = {first pair, pairs} of node i; best[i] = {feature, rank_lo,
// rank_hi, left size}, feature -1 when the best pair has no valid cut
__global__ void k_rf_best(const int32_t *__restrict__ nodes,
                          const int32_t *__restrict__ pspan,
                          const int32_t *__restrict__ pairs,
                          const double *__restrict__ score,
                          const int32_t *__restrict__ cut, int n_nodes,
                          int32_t *__restrict__ best) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes) return;
  const int p0 = pspan[2 * i], np = pspan[2 * i + 1];
  double bs = DBL_MAX;
  int bp = -1;
  for (int p = p0; p < p0 + np; ++p)
    if (score[p] < bs) {
      bs = score[p];
      bp = p;
    }
  const int size = nodes[4 * i + 2];
  int32_t *o = best + 4 * (int64_t)i;
  if (bp < 0 || cut[3 * (int64_t)bp] == size - 1) {
    o[0] = -1;
    o[1] = o[2] = o[3] = 0;
  } else {
    o[0] = pairs[2 * bp + 1];
    o[1] = cut[3 * (int64_t)bp + 1];
    o[2] = cut[3 * (int64_t)bp + 2];
    o[3] = cut[3 * (int64_t)bp] + 1;
  }
}

__global__ void __launch_bounds__(RF_PB)
    k_rf_partition(const int32_t *__restrict__ rank, int64_t n,
                   const int32_t *__restrict__ y, int C,
                   const int32_t *__restrict__ nodes,
                   const int32_t *__restrict__ best,
                   const int32_t *__restrict__ members_in,
                   int32_t *__restrict__ members_out,
                   int32_t *__restrict__ node_of,
                   int32_t *__restrict__ lcounts) {
  __shared__ int32_t lc[DKM_RF_MAX_CLASSES];
  __shared__ int32_t wsum[RF_PB / WAVE];
  const int i = blockIdx.x, t = threadIdx.x, lane = lane_id(), w = t >> 6;
  const int tree = nodes[4 * i], start = nodes[4 * i + 1];
  const int size = nodes[4 * i + 2], id = nodes[4 * i + 3];
  const int f = best[4 * (int64_t)i], lo = best[4 * (int64_t)i + 1];
  const int nleft = best[4 * (int64_t)i + 3];
  const int32_t *in = members_in + (int64_t)tree * n + start;
  int32_t *out = members_out + (int64_t)tree * n + start;
  if (t < DKM_RF_MAX_CLASSES) lc[t] = 0;
  if (f < 0) {
    for (int j = t; j < size; j += RF_PB) out[j] = in[j];
    if (t < C) lcounts[(int64_t)i * C + t] = 0;
    return;
  }
  const int32_t *rk = rank + (int64_t)f * n;
  int32_t *nof = node_of + (int64_t)tree * n;
  int lbase = 0;                             // left members so far (uniform)
  __syncthreads();
  for (int j0 = 0; j0 < size; j0 += RF_PB) {
    const int j = j0 + t;
    int s = -1;
    bool left = false;
    if (j < size) {
      s = in[j];
      left = rk[s] <= lo;
    }
    const unsigned long long bal = __ballot(left);
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int off = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
    for (int v = 0; v < RF_PB / WAVE; ++v) {
      const int c = wsum[v];
      if (v < w) off += c;
      total += c;
    }
    if (s >= 0) {
      // entries before j: j in all, lbase + off of them left
      const int dst = left ? lbase + off : nleft + (j - (lbase + off));
      if (dst < size) out[dst] = s;
      nof[s] = left ? id : id + 1;
      if (left) atomicAdd(&lc[y[s]], 1);
    }
    lbase += total;
    __syncthreads();
  }
  if (t < C) lcounts[(int64_t)i * C + t] = lc[t];
}

// (The probabilities accumulate in the row's own global slots and the hard
// vote compares all pairs of trees, O(T^2) per row: sized for tens of trees.)
// feature[v] < 0: a leaf, child[2 v] its leaf number.  proba[r][c] <- the
// mean over the trees of frequencies / size, labels[r] <- the first argmax
// of the sums (soft) or the class with most votes, ties to the class voted
// first (hard; votes[r][tree] holds every tree's mode).
template <class TX>
__global__ void __launch_bounds__(RF_B)
    k_rf_predict(const TX *__restrict__ X, int64_t n, int64_t ldx,
                 const int32_t *__restrict__ roots, int T,
                 const int32_t *__restrict__ feature,
                 const double *__restrict__ value,
                 const int32_t *__restrict__ child,
                 const int32_t *__restrict__ freq,
                 const int32_t *__restrict__ lsize,
                 const int32_t *__restrict__ lmode, int C, int hard,
                 double *__restrict__ proba, int32_t *__restrict__ votes,
                 int32_t *__restrict__ labels) {
  const int64_t r = (int64_t)blockIdx.x * RF_B + threadIdx.x;
  if (r >= n) return;
  const TX *x = X + r * ldx;
  double *pr = proba + r * C;
  for (int c = 0; c < C; ++c) pr[c] = 0.0;
  for (int tr = 0; tr < T; ++tr) {
    int v = roots[tr];
    while (feature[v] >= 0)
      v = child[2 * v + ((double)x[feature[v]] <= value[v] ? 0 : 1)];
    const int leaf = child[2 * v];
    const double sz = (double)lsize[leaf];
    for (int c = 0; c < C; ++c)
      pr[c] += (double)freq[(int64_t)leaf * C + c] / sz;
    if (hard) votes[r * T + tr] = lmode[leaf];
  }
  int lab = 0;
  if (hard) {
    int bestn = 0;
    for (int a = 0; a < T; ++a) {
      const int ca = votes[r * T + a];
      int cn = 0;
      for (int b = 0; b < T; ++b) cn += votes[r * T + b] == ca;
      if (cn > bestn) {
        bestn = cn;
        lab = ca;
      }
    }
  } else {
    for (int c = 1; c < C; ++c)
      if (pr[c] > pr[lab]) lab = c;
  }
  labels[r] = lab;
  for (int c = 0; c < C; ++c) pr[c] = pr[c] / (double)T;
}

namespace {

template <class TX>
int rf_predict(const TX *X, int64_t n, int64_t d, int64_t ldx,
               const int32_t *roots, int64_t T, const int32_t *feature,
               const double *value, const int32_t *child, const int32_t *freq,
               const int32_t *lsize, const int32_t *lmode, int64_t C, int hard,
               double *proba, int32_t *votes, int32_t *labels, hipStream_t s) {
  if (n < 0 || n > INT32_MAX || d < 1 || ldx < d || T < 1 || T > INT32_MAX ||
      !roots || !feature || !value || !child || !freq || !lsize || !lmode ||
      C < 1 || C > DKM_RF_MAX_CLASSES || (hard && !votes) ||
      (n > 0 && (!X || !proba || !labels)))
    return fail(DKM_E_ARG, "rf predict: bad arguments");
  if (n == 0) return 0;
  k_rf_predict<TX><<<(unsigned)((n + RF_B - 1) / RF_B), RF_B, 0, s>>>(
      X, n, ldx, roots, (int)T, feature, value, child, freq, lsize, lmode,
      (int)C, hard, proba, votes, labels);
  return check_launch("rf predict");
}

}  // namespace

}  // namespace dkm

using namespace dkm;

extern "C" {

int dkm_rf_split(const int32_t *rank, const int32_t *order, int64_t n,
                 const int32_t *y, int64_t C, const int32_t *members,
                 const int32_t *node_of, const int32_t *weight,
                 const int32_t *nodes, const int32_t *ncounts,
                 const int32_t *pairs, int64_t n_pairs, int64_t max_size,
                 int mode, double *score, int32_t *cut, void *stream) {
  if (!rank || !order || n < 1 || n >= DKM_RF_MAX_SAMPLES || !y || C < 1 ||
      C > DKM_RF_MAX_CLASSES || !members || !node_of || !weight || !nodes ||
      !ncounts || !pairs || n_pairs < 0 || n_pairs > RF_MAX_LIST ||
      max_size < 1 || max_size > n || mode < DKM_RF_AUTO ||
      mode > DKM_RF_STREAM || (n_pairs > 0 && (!score || !cut)) ||
      (mode == DKM_RF_LDS && max_size > DKM_RF_LDS_MAX))
    return fail(DKM_E_ARG, "rf split: bad arguments");
  if (n_pairs == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (mode != DKM_RF_STREAM) {
    int64_t P = 1;
    const int64_t top = max_size < DKM_RF_LDS_MAX ? max_size : DKM_RF_LDS_MAX;
    while (P < top) P <<= 1;
    const size_t lds = (size_t)P * 4 + (size_t)C * RF_B * 2;
    if (hipFuncSetAttribute((const void *)k_rf_split_lds,
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
      return fail(DKM_E_LAUNCH, "rf split: LDS attribute");
    k_rf_split_lds<<<(unsigned)n_pairs, RF_B, lds, s>>>(
        rank, n, y, (int)C, members, nodes, ncounts, pairs, mode, (int)P, score,
        cut);
    const int r = check_launch("rf split lds");
    if (r) return r;
  }
  if (mode == DKM_RF_STREAM ||
      (mode == DKM_RF_AUTO && max_size > DKM_RF_LDS_MAX)) {
    k_rf_split_stream<<<(unsigned)n_pairs, RF_B, 0, s>>>(
        rank, order, n, y, (int)C, node_of, weight, nodes, ncounts, pairs,
        mode, score, cut);
    return check_launch("rf split stream");
  }
  return 0;
}

int dkm_rf_best(const int32_t *nodes, const int32_t *pspan,
                const int32_t *pairs, const double *score, const int32_t *cut,
                int64_t n_nodes, int32_t *best, void *stream) {
  if (!nodes || !pspan || !pairs || !score || !cut || n_nodes < 1 ||
      n_nodes > RF_MAX_LIST || !best)
    return fail(DKM_E_ARG, "rf best: bad arguments");
  k_rf_best<<<(unsigned)((n_nodes + RF_B - 1) / RF_B), RF_B, 0,
              (hipStream_t)stream>>>(nodes, pspan, pairs, score, cut,
                                     (int)n_nodes, best);
  return check_launch("rf best");
}

int dkm_rf_partition(const int32_t *rank, int64_t n, const int32_t *y,
                     int64_t C, const int32_t *nodes, const int32_t *best,
                     int64_t n_nodes, const int32_t *members_in,
                     int32_t *members_out, int32_t *node_of, int32_t *lcounts,
                     void *stream) {
  if (!rank || n < 1 || n >= DKM_RF_MAX_SAMPLES || !y || C < 1 ||
      C > DKM_RF_MAX_CLASSES || !nodes || !best || n_nodes < 1 ||
      n_nodes > RF_MAX_LIST || !members_in || !members_out ||
      members_in == members_out || !node_of || !lcounts)
    return fail(DKM_E_ARG, "rf partition: bad arguments");
  k_rf_partition<<<(unsigned)n_nodes, RF_PB, 0, (hipStream_t)stream>>>(
      rank, n, y, (int)C, nodes, best, members_in, members_out, node_of,
      lcounts);
  return check_launch("rf partition");
}

int dkm_rf_predict_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                       const int32_t *roots, int64_t T, const int32_t *feature,
                       const double *value, const int32_t *child,
                       const int32_t *freq, const int32_t *lsize,
                       const int32_t *lmode, int64_t C, int hard,
                       double *proba, int32_t *votes, int32_t *labels,
                       void *stream) {
  return rf_predict<double>(X, n, d, ldx, roots, T, feature, value, child,
                            freq, lsize, lmode, C, hard, proba, votes, labels,
                            (hipStream_t)stream);
}

int dkm_rf_predict_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                       const int32_t *roots, int64_t T, const int32_t *feature,
                       const double *value, const int32_t *child,
                       const int32_t *freq, const int32_t *lsize,
                       const int32_t *lmode, int64_t C, int hard,
                       double *proba, int32_t *votes, int32_t *labels,
                       void *stream) {
  return rf_predict<float>(X, n, d, ldx, roots, T, feature, value, child, freq,
                           lsize, lmode, C, hard, proba, votes, labels,
                           (hipStream_t)stream);
}

}  // extern "C"

// Code-object preload (dkm_preload): see dkm_ordered.hip.
namespace dkm {
DKM_TU_FLAGS(rf, 0)
__global__ void k_tu_rf() {}
int preload_rf() {
  hipFuncAttributes a;
  const bool ok = hipFuncGetAttributes(&a, (const void *)k_tu_rf) == hipSuccess;
  return ok ? 0 : 1;
}
}  // namespace dkm
