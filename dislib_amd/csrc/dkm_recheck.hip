// dkm_recheck.hip -- the samples a screen leaves undecided: k_recheck_list
// (the screens' per-wave lists), k_recheck_wave, k_recheck_lane and
// k_recheck_exact (the label scan).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "dkm_dense.h"
#include "dkm_screen.h"

namespace dkm {

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One undecided sample per lane (k_recheck_list and k_recheck_lane).
// Stage 1 re-screens in fp32 VALU (x in VGPRs, fp32 centres `cl` of row
// stride dp and |c|^2 `cnl`, in LDS or global memory) -- the P_F32
// arithmetic and bound, ~2^-24 instead of bf16x3's ~2^-16 -- and keeps the
// label when the best two scores are 2B apart.  Otherwise stage 2 runs the
// reference arithmetic on the candidates only (score <= best + 2B: the
// reference winner is always among them, and every other centre is
// strictly farther after sqrt).  Writes lab_out[i] and moves
// the row between the accumulators as amode says (prev = previous label).
// STAGE1_ONLY: return false (writing nothing) when stage 1 cannot decide,
// so the caller can batch the rare stage-2 samples into full waves.
// BND (a bounds call): a row stage 1 decides also gets its
// (ub, lb) under this call's centres, from the two best fp32 scores over all
// k centres (settle_bounds below), and is counted in nset; a row that goes on
// to stage 2 is not written: it keeps the screen's (+inf, 0).
template <bool UP>
__device__ __forceinline__ float f32_outward(double v) {  // v >= 0
  float f = (float)v;
  if (UP) {
    if ((double)f < v) f = __uint_as_float(__float_as_uint(f) + 1u);
  } else {
    if ((double)f > v) f = __uint_as_float(__float_as_uint(f) - 1u);
  }
  return f;
}
// Every fp32 score is within B / 2 of |c|^2 - 2 x.c under the fp64 centres
// (screen_bound<P_F32> is twice the rigorous bound, the rounding of the
// centres to c32 / cn32 included: DESIGN.md 3.14), and xx, the fp32 fma chain
// of d <= 32 squares of fl32(x), within 35 x 2^-24 < 2^-18.8 of |x|^2.  So
// u^2 = xx (1 + 2^-18) + b1 + B and l^2 = xx (1 - 2^-18) + b2 - B bound the
// squared distances with B / 2 + 2^-19.3 xx to spare; they and the roots are
// evaluated in fp64 (roundings of 2^-53: nothing against that spare), and
// the roots are rounded outwards to fp32 once.
__device__ __forceinline__ void settle_bounds(float xx, float b1, float b2,
                                              float B, float *ub, float *lb) {
  const double u2 = fma((double)xx, 1.0 + 0x1.0p-18, (double)b1 + (double)B);
  const double l2 = fma((double)xx, 1.0 - 0x1.0p-18, (double)b2 - (double)B);
  *ub = f32_outward<true>(sqrt(fmax(u2, 0.0)));
  *lb = f32_outward<false>(sqrt(fmax(l2, 0.0)));
}
template <int MAXD, bool VEC, class TX, bool STAGE1_ONLY = false,
          bool BND = false>
__device__ __forceinline__ bool resolve_lane(
    const TX *__restrict__ X, int64_t ldx, int d, int k, int64_t i, int prev,
    const float *cl, const float *cnl, int dp, float cm, const double *ct64,
    int32_t *lab_out, int amode, const AccTarget &at, RcBnd rb = RcBnd{},
    unsigned *nset = nullptr) {
  const TX *xr = X + i * ldx;
  float xf[MAXD];
  float xx = 0.f;
#pragma unroll
  for (int b = 0; b < MAXD / 8; ++b) {
    double o[8];
    if (8 * b < d) {
      load8<VEC>(xr, 8 * b, d, o);
    } else {
#pragma unroll
      for (int m = 0; m < 8; ++m) o[m] = 0.0;
    }
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      xf[8 * b + m] = (float)o[m];
      xx = fmaf(xf[8 * b + m], xf[8 * b + m], xx);
    }
  }
  // fp32 score of centre jc: fma chain over features (padding adds 0 * 0).
  // cl / cnl are the workspace's global fp32 centres, read through the
  // constant address space: jc is wave-uniform, so the rows arrive by scalar
  // loads into SGPRs (an LDS broadcast of the same row costs the full LDS
  // return bandwidth, twice the VALU time of the fma chain).
  typedef const __attribute__((address_space(4))) float cfloat;
  typedef const __attribute__((address_space(4))) f32x4 cf32x4;
  cfloat *clc = (cfloat *)cl;
  cfloat *cnc = (cfloat *)cnl;
  // full rows (dp == MAXD): no per-chunk branch, so the row's scalar loads
  // issue together (one wait instead of one per 4 features)
  const bool full = dp == MAXD;
  auto score = [&](int jc) {
    cfloat *cr = clc + (int64_t)jc * dp;
    float dot = 0.f;
    if (full) {
#pragma unroll
      for (int t4 = 0; t4 < MAXD / 4; ++t4) {
        const f32x4 c4 = *(cf32x4 *)(cr + 4 * t4);
        dot = fmaf(xf[4 * t4 + 0], c4.x, dot);
        dot = fmaf(xf[4 * t4 + 1], c4.y, dot);
        dot = fmaf(xf[4 * t4 + 2], c4.z, dot);
        dot = fmaf(xf[4 * t4 + 3], c4.w, dot);
      }
    } else {
#pragma unroll
      for (int t4 = 0; t4 < MAXD / 4; ++t4) {
        if (4 * t4 < dp) {
          const f32x4 c4 = *(cf32x4 *)(cr + 4 * t4);
          dot = fmaf(xf[4 * t4 + 0], c4.x, dot);
          dot = fmaf(xf[4 * t4 + 1], c4.y, dot);
          dot = fmaf(xf[4 * t4 + 2], c4.z, dot);
          dot = fmaf(xf[4 * t4 + 3], c4.w, dot);
        }
      }
    }
    return fmaf(-2.f, dot, cnc[jc]);
  };
  float b1 = INFINITY, b2 = INFINITY;
  int i1 = 0;
#pragma unroll 4
  for (int jc = 0; jc < k; ++jc) {
    const float sc = score(jc);
    i1 = sc < b1 ? jc : i1;
    b2 = __builtin_amdgcn_fmed3f(b1, b2, sc);
    b1 = fminf(b1, sc);
  }
  const float xn = sqrtf(xx) * (1.0f + (d + 4) * 0x1.0p-24f);
  const float B = screen_bound<P_F32>(d, xn, cm, false);
  const bool sane = (xn < 1e18f) && (xn * cm < 1e30f) && (b1 < 1e30f);
  int bi = i1;
  if (!(sane && b2 - b1 > 2.0f * B)) {
    if constexpr (STAGE1_ONLY) return false;
    const float lim = b1 + 2.0f * B;
    double best = INFINITY;
    bi = -1;
#pragma unroll 1
    for (int jc = 0; jc < k; ++jc) {
      if (sane && !(score(jc) <= lim)) continue;
      const SqDiffT<TX> f{xr, ct64 + jc, ct_ld(k)};
      const double dist = argmin_key(sqrt(pw_leaf(f, 0, d)));
      if (dist < best || bi < 0) {
        best = dist;
        bi = jc;
      }
    }
  } else if constexpr (BND) {
    // decided by stage 1: the label is i1 and b2 the least score of every
    // other centre (the scan was over all k)
    if (b2 < 1e30f) {
      settle_bounds(xx, b1, b2, B, rb.ub + i, rb.lb + i);
      *nset += 1u;
    }
  }
  lab_out[i] = bi;
  if (!(amode & AM_ON)) return true;
  const bool delta = amode & AM_DELTA;
  if (delta && bi == prev) return true;
  const bool sub = delta && prev >= 0;
  for (int t = 0; t < d; ++t) {
    const double x = ld_x(xr + t);
    at.add(bi, t, x);
    if (sub) at.add(prev, t, -x);
  }
  at.count(bi, 1.0);
  if (sub) at.count(prev, -1.0);
  return true;
}

// Exact re-check of the samples the screen left undecided (lab_out < 0,
// encoding the previous label as -(prev + 2)).  Waves scan 64 labels at a
// time (coalesced, no shared counter).
//   k_recheck_lane (d <= 128, fp32 centres fit in LDS): each wave compacts
//     its undecided samples into an LDS list and resolves them 64 at a time,
//     lane = sample.  Stage 1 re-screens in fp32 VALU (x in VGPRs, centres
//     broadcast from LDS) -- the P_F32 arithmetic and bound, ~2^-24 instead
//     of bf16x3's ~2^-16 -- and keeps the label when the best two scores are
//     2B apart.  Otherwise stage 2 runs the reference arithmetic on the
//     candidates only (score <= best + 2B: the reference winner is always
//     among them, and every other centre is strictly farther after sqrt,
//     DESIGN.md 3.1).
//   k_recheck_exact (any d, k): wave per sample, lanes over centres, the
//     reference arithmetic on every centre.
template <class TX>
__device__ __forceinline__ void recheck_accumulate(int amode,
                                                   const AccTarget &at,
                                                   const TX *xr, int d,
                                                   int bi, int prev,
                                                   int lane) {
  if (!(amode & AM_ON)) return;
  const bool delta = amode & AM_DELTA;
  if (delta && bi == prev) return;
  const bool sub = delta && prev >= 0;
  for (int t = lane; t < d; t += 64) {
    const double x = ld_x(xr + t);
    at.add(bi, t, x);
    if (sub) at.add(prev, t, -x);
  }
  if (lane == 0) {
    at.count(bi, 1.0);
    if (sub) at.count(prev, -1.0);
  }
}

__device__ __forceinline__ void recheck_finish_count(
    unsigned long long mine, unsigned long long *blk_count, const WsView &v) {
  if ((threadIdx.x & 63) == 0 && mine)
    __hip_atomic_fetch_add(blk_count, mine, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
  if (threadIdx.x == 0 && *blk_count)
    atomicAdd((unsigned long long *)&v.hdr->rechecked_total, *blk_count);
}

// BND kernels: the rows that got bounds, per block and then in the header
__device__ __forceinline__ void recheck_finish_settled(
    unsigned nset, unsigned long long *blk_settled, const WsView &v) {
  if (nset)
    __hip_atomic_fetch_add(blk_settled, (unsigned long long)nset,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
  if (threadIdx.x == 0 && *blk_settled)
    atomicAdd((unsigned long long *)&v.hdr->bnd_settled, *blk_settled);
}

// resolve_lane's two stages for ONE sample i with the whole wave: lanes
// over centres (jc = lane, lane + 64, ...), the same fp32 scores and bound
// (stage 1), then the reference arithmetic on the centres within the bound
// (stage 2; every centre when the scores are not sane), reduced over the
// wave by (distance, index).  The re-check list's stage-2 samples go here:
// lane per sample, a sample with many candidates (a near-tie among many
// centres) held its whole wave for k sequential exact distances.
template <int MAXD, class TX>
__device__ __forceinline__ void resolve_wave(
    const TX *__restrict__ X, int64_t ldx, int d, int k, int64_t i, int prev,
    const float *cl, const float *cnl, int dp, float cm, const double *ct64,
    int32_t *lab_out, int amode, const AccTarget &at) {
  const int lane = threadIdx.x & 63;
  const TX *xr = X + i * ldx;
  float xf[MAXD];
  float xx = 0.f;
#pragma unroll
  for (int t = 0; t < MAXD; ++t) {      // the same fp32 chain as resolve_lane
    xf[t] = t < d ? (float)ld_x(xr + t) : 0.f;
    xx = fmaf(xf[t], xf[t], xx);
  }
  // the centre's fp32 row (dp floats, 16-B aligned) by 16-B loads, all
  // issued before the fma chain (the same chain order as resolve_lane)
  auto score = [&](int jc) {
    const f32x4 *cr = (const f32x4 *)(cl + (int64_t)jc * dp);
    f32x4 c4[MAXD / 4];
#pragma unroll
    for (int t4 = 0; t4 < MAXD / 4; ++t4)
      if (4 * t4 < dp) c4[t4] = cr[t4];
    float dot = 0.f;
#pragma unroll
    for (int t4 = 0; t4 < MAXD / 4; ++t4)
      if (4 * t4 < dp) {
        dot = fmaf(xf[4 * t4 + 0], c4[t4].x, dot);
        dot = fmaf(xf[4 * t4 + 1], c4[t4].y, dot);
        dot = fmaf(xf[4 * t4 + 2], c4[t4].z, dot);
        dot = fmaf(xf[4 * t4 + 3], c4[t4].w, dot);
      }
    return fmaf(-2.f, dot, cnl[jc]);
  };
  float b1 = INFINITY, b2 = INFINITY;
  int i1 = INT32_MAX;
#pragma unroll 2
  for (int jc = lane; jc < k; jc += 64) {
    const float sc = score(jc);
    i1 = sc < b1 ? jc : i1;
    b2 = __builtin_amdgcn_fmed3f(b1, b2, sc);
    b1 = fminf(b1, sc);
  }
  // wave top-2 (NaN scores never win: fminf / med3 drop them, and the sane
  // test below sends such a sample to stage 2 over every centre)
  for (int off = 1; off < 64; off <<= 1) {
    const float o1 = __shfl_xor(b1, off, 64), o2 = __shfl_xor(b2, off, 64);
    const int oi = __shfl_xor(i1, off, 64);
    const bool tk = (o1 < b1) | ((o1 == b1) & (oi < i1));
    b2 = tk ? fminf(b1, o2) : fminf(b2, o1);
    i1 = tk ? oi : i1;
    b1 = tk ? o1 : b1;
  }
  const float xn = sqrtf(xx) * (1.0f + (d + 4) * 0x1.0p-24f);
  const float B = screen_bound<P_F32>(d, xn, cm, false);
  const bool sane = (xn < 1e18f) && (xn * cm < 1e30f) && (b1 < 1e30f);
  int bi = i1;
  if (!(sane && b2 - b1 > 2.0f * B)) {
    const float lim = b1 + 2.0f * B;
    double best = INFINITY;
    bi = INT32_MAX;
    for (int jc = lane; jc < k; jc += 64) {
      if (sane && !(score(jc) <= lim)) continue;
      const SqDiffT<TX> f{xr, ct64 + jc, ct_ld(k)};
      const double dist = argmin_key(sqrt(pw_leaf(f, 0, d)));
      if (dist < best || bi == INT32_MAX) {
        best = dist;
        bi = jc;
      }
    }
    for (int off = 1; off < 64; off <<= 1) {
      const double ob = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      const bool tk = (ob < best) | ((ob == best) & (oi < bi));
      best = tk ? ob : best;
      bi = tk ? oi : bi;
    }
  }
  if (lane == 0) lab_out[i] = bi;
  recheck_accumulate(amode, at, xr, d, bi, prev, lane);
}

constexpr int RL_CAP = 128;  // per-wave list: a full batch + one chunk

static size_t recheck_lane_lds(int64_t, int64_t) {
  return (size_t)(BLOCK / 64) * RL_CAP * 8;
}

// k_recheck_lane and k_recheck_list, and their forms for a bounds call
// (k_recheck_lane_bnd, k_recheck_list_bnd; d <= 32 only)
#define RC_BND 0
#include "dkm_recheck_kernels.inc"
#undef RC_BND
#define RC_BND 1
#include "dkm_recheck_kernels.inc"
#undef RC_BND

// k_recheck_list's stage-2 samples (fp32 stage 1 could not decide them),
// one wave per sample: lanes over centres (resolve_wave), so a sample with
// many candidates no longer holds a lane -- and its wave -- for a walk over
// every centre with one exact distance after another (the 1-4 ms spikes of
// the steady C3 iterations).  Sums by global fp64 atomics (rare samples).
template <int MAXD, class TX>
__global__ void __launch_bounds__(BLOCK)
    k_recheck_wave(const TX *__restrict__ X, int d, int64_t ldx, int k,
                   WsView v, int32_t *__restrict__ lab_out, double *acc,
                   int amode, int64_t base) {
  const uint32_t cap = (uint32_t)std::min<int64_t>(v.nq / 2, INT32_MAX);
  const uint32_t cnt = min(v.hdr->s2count, cap);
  const int64_t wv = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  const int64_t nwv = (int64_t)gridDim.x * (BLOCK / 64);
  if (wv >= cnt) return;
  const int dp = (int)round_up(d, 4);
  const float cm =
      (float)__longlong_as_double((long long)v.hdr->cmax_bits) * 1.000001f;
  const int am = amode & ~AM_INLDS;
  const AccTarget at = acc_target(am, nullptr, acc, k, d);
  const int2 *s2l = (const int2 *)v.smoved;
  for (int64_t r = wv; r < cnt; r += nwv) {
    const int2 it = s2l[r];
    resolve_wave<MAXD, TX>(X, ldx, d, k, base + it.x, it.y, v.c32, v.cn32,
                           dp, cm, v.ct64, lab_out, am, at);
  }
}

template <bool SMALL, class TX>
__global__ void __launch_bounds__(BLOCK)
    k_recheck_exact(const TX *__restrict__ X, int64_t n, int d, int64_t ldx,
                    int k, WsView v, int32_t *__restrict__ lab_out,
                    double *acc, int amode, int64_t base) {
  if (v.hdr->qcount == 0) return;  // the screen resolved everything
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *lds_acc = smem;
  __shared__ unsigned long long blk_count;
  if (threadIdx.x == 0) blk_count = 0;
  if (amode & AM_INLDS) zero_lds_acc(lds_acc, k, d);
  const AccTarget at = acc_target(amode, lds_acc, acc, k, d);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  const int64_t nwv = (int64_t)gridDim.x * (BLOCK / 64);
  unsigned long long mine = 0;
  for (int64_t c0 = base + wv * 64; c0 < n; c0 += nwv * 64) {
    const int64_t li = c0 + lane;
    const int lv = li < n ? lab_out[li] : 0;
    unsigned long long mask = __ballot(lv < 0);
    mine += __popcll(mask);
    while (mask) {
      const int bit = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int64_t i = c0 + bit;
      const int prev = -__shfl(lv, bit, WAVE) - 2;
      const TX *xr = X + i * ldx;
      double best = INFINITY;
      int bi = 0x7fffffff;  // lanes without a centre never win
      for (int jc = lane; jc < k; jc += 64) {
        const SqDiffT<TX> f{xr, v.ct64 + jc, ct_ld(k)};
        const double dist =
            argmin_key(sqrt(SMALL ? pw_leaf(f, 0, d) : pw_sum(f, d)));
        if (dist < best || bi == 0x7fffffff) {
          best = dist;
          bi = jc;
        }
      }
      wave_argmin(best, bi);
      if (lane == 0) lab_out[i] = bi;
      recheck_accumulate(amode, at, xr, d, bi, prev, lane);
    }
  }
  recheck_finish_count(mine, &blk_count, v);
  if (amode & AM_INLDS) flush_lds_acc(lds_acc, acc, k, d);
}

template <int MAXD, bool VEC, class TX>
static void launch_recheck_lane_t(unsigned g, size_t lds, hipStream_t s,
                                  const TX *X, int64_t end, int d,
                                  int64_t ldx, int k, const WsView &v,
                                  int32_t *lab_out, double *acc, int amode,
                                  int64_t base) {
  k_recheck_lane<MAXD, VEC, TX><<<g, BLOCK, lds, s>>>(X, end, d, ldx, k, v,
                                                       lab_out, acc, amode,
                                                       base);
}

template <int MAXD, class TX>
static const void *recheck_lane_fn(bool vec) {
  return vec ? (const void *)k_recheck_lane<MAXD, true, TX>
             : (const void *)k_recheck_lane<MAXD, false, TX>;
}

template <class TX>
int launch_recheck(const TX *X, int64_t end, int d, int64_t ldx, int k,
                   const WsView &v, int32_t *lab_out, double *acc,
                   int acc_kind, bool vec, int64_t base, hipStream_t s,
                   const RcBnd *bnd) {
  const size_t a_bytes = (size_t)lds_acc_len(k, d) * 8;
  const size_t fb = recheck_lane_lds(k, d);
  const bool lane = d <= 128 && fb <= LDS_BUDGET;
  const int maxd = d <= 32 ? 32 : d <= 64 ? 64 : 128;
  if (bnd && !(lane && maxd == 32))
    return fail(DKM_E_ARG, "exact re-check: bounds need d <= 32");
  const size_t fixed = lane ? fb : 0;
  const int amode = acc_mode(acc_kind, fixed + a_bytes <= LDS_BUDGET);
  const size_t lds = fixed + ((amode & AM_INLDS) ? a_bytes : 0);
  const bool small = d <= 128;
  const void *kf =
      bnd     ? (vec ? (const void *)k_recheck_lane_bnd<32, true, TX>
                     : (const void *)k_recheck_lane_bnd<32, false, TX>)
      : !lane ? (small ? (const void *)k_recheck_exact<true, TX>
                       : (const void *)k_recheck_exact<false, TX>)
      : maxd == 32 ? recheck_lane_fn<32, TX>(vec)
      : maxd == 64 ? recheck_lane_fn<64, TX>(vec)
                   : recheck_lane_fn<128, TX>(vec);
  const int per_cu = resident_blocks(kf, BLOCK, lds);
  const int64_t waves = (end - base + 3 + (lane ? 255 : 63)) / (lane ? 256 : 64);
  const unsigned g = (unsigned)std::max<int64_t>(
      1, std::min<int64_t>((int64_t)dev_info().cus * per_cu,
                           (waves + BLOCK / 64 - 1) / (BLOCK / 64)));
  if (bnd) {
    if (vec)
      k_recheck_lane_bnd<32, true, TX><<<g, BLOCK, lds, s>>>(
          X, end, d, ldx, k, v, lab_out, acc, amode, base, *bnd);
    else
      k_recheck_lane_bnd<32, false, TX><<<g, BLOCK, lds, s>>>(
          X, end, d, ldx, k, v, lab_out, acc, amode, base, *bnd);
  } else if (lane) {
#define DKM_RL(M)                                                            \
  (vec ? launch_recheck_lane_t<M, true, TX>(g, lds, s, X, end, d, ldx, k, v, \
                                            lab_out, acc, amode, base)       \
       : launch_recheck_lane_t<M, false, TX>(g, lds, s, X, end, d, ldx, k,   \
                                             v, lab_out, acc, amode, base))
    if (maxd == 32)
      DKM_RL(32);
    else if (maxd == 64)
      DKM_RL(64);
    else
      DKM_RL(128);
#undef DKM_RL
  } else if (small) {
    k_recheck_exact<true, TX><<<g, BLOCK, lds, s>>>(X, end, d, ldx, k, v,
                                                     lab_out, acc, amode, base);
  } else {
    k_recheck_exact<false, TX><<<g, BLOCK, lds, s>>>(X, end, d, ldx, k, v,
                                                      lab_out, acc, amode, base);
  }
  return check_launch("exact re-check");
}

template <int MAXD, bool VEC, class TX>
static int launch_list_t(const TX *X, int d, int64_t ldx, int k,
                         const WsView &v, int32_t *lab_out, double *acc,
                         int amode, int64_t base, int nseg, size_t lds,
                         hipStream_t s, bool wave_all) {
  const void *kf = (const void *)k_recheck_list<MAXD, VEC, TX>;
  const int per_cu = resident_blocks(kf, BLOCK, lds);
  const int64_t units = (int64_t)nseg * (TL_CAP / 64);
  const int64_t g = std::max<int64_t>(
      1, std::min<int64_t>((int64_t)dev_info().cus * per_cu,
                           (units + BLOCK / 64 - 1) / (BLOCK / 64)));
  if (hipMemsetAsync(&v.hdr->s2count, 0, 4, s) != hipSuccess)
    return fail(DKM_E_LAUNCH, "list re-check: counter reset");
  k_recheck_list<MAXD, VEC, TX><<<(unsigned)g, BLOCK, lds, s>>>(
      X, d, ldx, k, v, lab_out, acc, amode, base, nseg, wave_all ? 1 : 0);
  if (int r = check_launch("list re-check")) return r;
  if (!wave_all) return 0;
  k_recheck_wave<MAXD, TX><<<(unsigned)(dev_info().cus * 4), BLOCK, 0, s>>>(
      X, d, ldx, k, v, lab_out, acc, amode, base);
  return check_launch("list re-check (wave per sample)");
}

// launch_list_t for a bounds call: k_recheck_list_bnd, no wave-per-sample form
template <bool VEC, class TX>
static int launch_list_bnd_t(const TX *X, int d, int64_t ldx, int k,
                             const WsView &v, int32_t *lab_out, double *acc,
                             int amode, int64_t base, int nseg, size_t lds,
                             hipStream_t s, const RcBnd &rb) {
  const void *kf = (const void *)k_recheck_list_bnd<32, VEC, TX>;
  const int per_cu = resident_blocks(kf, BLOCK, lds);
  const int64_t units = (int64_t)nseg * (TL_CAP / 64);
  const int64_t g = std::max<int64_t>(
      1, std::min<int64_t>((int64_t)dev_info().cus * per_cu,
                           (units + BLOCK / 64 - 1) / (BLOCK / 64)));
  if (hipMemsetAsync(&v.hdr->s2count, 0, 4, s) != hipSuccess)
    return fail(DKM_E_LAUNCH, "list re-check: counter reset");
  k_recheck_list_bnd<32, VEC, TX><<<(unsigned)g, BLOCK, lds, s>>>(
      X, d, ldx, k, v, lab_out, acc, amode, base, nseg, 0, rb);
  return check_launch("list re-check (bounds)");
}

// Can the listed samples be resolved lane-per-sample (k_recheck_list)?
bool list_ok(int64_t k, int64_t d) {
  return d <= 128 && recheck_lane_lds(k, d) <= LDS_BUDGET;
}

// wave_all: the list is short (a re-screen's leftovers): every sample goes
// to k_recheck_wave (a wave per sample, its latency spread over the chip)
// instead of lane-per-sample stage 1, whose per-wave walk over all k centres
// costs ~1 ms whatever the list's length.
template <class TX>
int launch_list(const TX *X, int d, int64_t ldx, int k, const WsView &v,
                int32_t *lab_out, double *acc, int acc_kind, bool vec,
                int64_t base, int nseg, hipStream_t s, bool wave_all,
                const RcBnd *bnd) {
  const size_t fb = 0;  // centres are read from global (scalar loads)
  const size_t a_bytes = (size_t)lds_acc_len(k, d) * 8;
  const int amode = acc_mode(acc_kind, fb + a_bytes <= LDS_BUDGET);
  const size_t lds = fb + ((amode & AM_INLDS) ? a_bytes : 0);
  const int maxd = d <= 32 ? 32 : d <= 64 ? 64 : 128;
  if (bnd) {
    if (maxd != 32 || wave_all)
      return fail(DKM_E_ARG, "list re-check: bounds need d <= 32");
    return vec ? launch_list_bnd_t<true, TX>(X, d, ldx, k, v, lab_out, acc,
                                             amode, base, nseg, lds, s, *bnd)
               : launch_list_bnd_t<false, TX>(X, d, ldx, k, v, lab_out, acc,
                                              amode, base, nseg, lds, s,
                                              *bnd);
  }
#define DKM_LL(M)                                                            \
  (vec ? launch_list_t<M, true, TX>(X, d, ldx, k, v, lab_out, acc, amode,    \
                                    base, nseg, lds, s, wave_all)            \
       : launch_list_t<M, false, TX>(X, d, ldx, k, v, lab_out, acc, amode,   \
                                     base, nseg, lds, s, wave_all))
  const int r = maxd == 32 ? DKM_LL(32) : maxd == 64 ? DKM_LL(64) : DKM_LL(128);
#undef DKM_LL
  return r;
}

#define DKM_RECHECK_INST(TX)                                                 \
  template int launch_recheck<TX>(const TX *, int64_t, int, int64_t, int,    \
                                  const WsView &, int32_t *, double *, int,  \
                                  bool, int64_t, hipStream_t,                \
                                  const RcBnd *);                            \
  template int launch_list<TX>(const TX *, int, int64_t, int,                \
                               const WsView &, int32_t *, double *, int,     \
                               bool, int64_t, int, hipStream_t, bool,        \
                               const RcBnd *);
DKM_RECHECK_INST(double)
DKM_RECHECK_INST(float)
#undef DKM_RECHECK_INST

}  // namespace dkm

// Code-object preload (dkm_preload): the runtime loads this file's kernels
// on first use of any of them; an attribute query here does it up front.
namespace dkm {
DKM_TU_FLAGS(recheck, 0)
__global__ void k_tu_recheck() {}
int preload_recheck() {
  hipFuncAttributes a;
  const bool ok =
      hipFuncGetAttributes(&a, (const void *)k_tu_recheck) == hipSuccess;
  return ok ? 0 : 1;
}
}  // namespace dkm
