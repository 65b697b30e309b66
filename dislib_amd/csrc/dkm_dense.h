// dkm_dense.h -- what the dense assignment's translation units share
// (internal): block and LDS sizes, the accumulation modes and the LDS
// accumulators, the row loads, and the launchers of dkm_recheck.hip that
// dkm_dense.hip's dispatch calls.
//
// Accumulation (acc = [sums k*d | counts k], fp64):
//   full   every sample adds its row (partial_sum semantics);
//   delta  incremental: labels[] holds the previous assignment; only samples
//          whose label changes add +x to the new and -x to the old cluster
//          (dkm_assign_delta).
// Both go to block-private LDS accumulators (odd row stride, flushed once
// per block) when they fit, else to fp64 global atomics.  Delta in LDS
// matters: in the first iterations most labels move, and global atomics on
// k rows serialise (a 100M x 32, k = 100 delta pass took 650 ms that way).
#pragma once

#include <hip/hip_runtime.h>

#include "dkm_internal.h"

namespace dkm {

constexpr int BLOCK = 256;
constexpr size_t LDS_BUDGET = 80 * 1024;  // per block -> >= 2 blocks / CU
constexpr size_t LDS_PER_CU = 160 * 1024;

// Accumulation mode bits: AM_ON (accumulate at all), AM_DELTA (incremental:
// only label changes move rows), AM_INLDS (block-private LDS accumulators,
// flushed once per block; else fp64 global atomics).
// AM_MLIST (k_screen_w32, with AM_DELTA and without AM_ON): the rows the
// screen moves are listed (v.smoved, count hdr->nmoved; previous labels in
// v.queue[row]) for sorted_sums_moved instead of added in the screen.
enum : int { AM_NONE = 0, AM_ON = 1, AM_DELTA = 2, AM_INLDS = 4,
             AM_MLIST = 8 };
__host__ __device__ __forceinline__ bool am_full(int m) {
  return (m & (AM_ON | AM_DELTA)) == AM_ON;
}

struct DevInfo {
  int cus = 256;
};
// (dkm_dense.hip) the device's CU count; workgroups of `block` threads
// resident per CU
DevInfo dev_info();
int resident_blocks(const void *kf, int block, size_t lds);

template <class TX>
__device__ __forceinline__ double ld_x(const TX *p) {
  return (double)(*p);
}

// LDS accumulators: row stride of an odd number of doubles, so that the
// rows of different clusters start in different banks (a 32-double row is
// exactly one 256-B bank row: unpadded, every cluster's feature t sits in
// the same bank and same-feature adds of different clusters serialise).
__host__ __device__ __forceinline__ int lds_stride(int d) {
  return (d & 1) ? d : d + 1;
}
__host__ __device__ __forceinline__ int64_t lds_acc_len(int64_t k, int d) {
  return k * lds_stride(d) + k;
}

__device__ __forceinline__ void lds_add(double *p, double v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Where one kernel's sums go: LDS rows (odd stride) or the global acc.
struct AccTarget {
  double *rows;
  double *cnt;
  int stride;
  bool lds;
  __device__ __forceinline__ void add(int row, int t, double v) const {
    double *p = rows + (int64_t)row * stride + t;
    if (lds)
      lds_add(p, v);
    else
      atomic_add_f64(p, v);
  }
  __device__ __forceinline__ void count(int row, double v) const {
    if (lds)
      lds_add(cnt + row, v);
    else
      atomic_add_f64(cnt + row, v);
  }
};

__device__ __forceinline__ AccTarget acc_target(int amode, double *lds_acc,
                                                double *acc, int64_t k,
                                                int d) {
  if (amode & AM_INLDS) {
    const int ds = lds_stride(d);
    return AccTarget{lds_acc, lds_acc + k * ds, ds, true};
  }
  return AccTarget{acc, acc + k * d, d, false};
}

__device__ __forceinline__ void zero_lds_acc(double *lds_acc, int64_t k,
                                             int d) {
  const int64_t len = lds_acc_len(k, d);
  for (int64_t e = threadIdx.x; e < len; e += blockDim.x) lds_acc[e] = 0.0;
}

__device__ __forceinline__ void flush_lds_acc(const double *lds_acc,
                                              double *acc, int64_t k, int d) {
  const int ds = lds_stride(d);
  const int64_t kd = k * d;
  for (int64_t e = threadIdx.x; e < kd + k; e += blockDim.x) {
    const double v = e < kd ? lds_acc[(e / d) * ds + (e % d)]
                            : lds_acc[k * ds + (e - kd)];
    if (v != 0.0) atomic_add_f64(acc + e, v);
  }
}

// Eight consecutive features t0..t0+7 of one row, as fp64.  VEC: d % 8 == 0
// and 16-B aligned rows, so the 8 features are in range iff t0 < d.
template <bool VEC, class TX>
__device__ __forceinline__ void load8(const TX *xr, int t0, int d,
                                      double (&o)[8]) {
  if (VEC) {
    if (t0 < d) {
      if constexpr (sizeof(TX) == 8) {
        const double2 *p = (const double2 *)(xr + t0);
        const double2 a = p[0], b = p[1], c = p[2], e = p[3];
        o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
        o[4] = c.x; o[5] = c.y; o[6] = e.x; o[7] = e.y;
      } else {
        const float4 *p = (const float4 *)(xr + t0);
        const float4 a = p[0], b = p[1];
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
        o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
      }
    } else {
#pragma unroll
      for (int m = 0; m < 8; ++m) o[m] = 0.0;
    }
  } else {
#pragma unroll
    for (int m = 0; m < 8; ++m)
      o[m] = (t0 + m < d) ? (double)xr[t0 + m] : 0.0;
  }
}

// acc_kind: 0 = none (predict), 1 = full accumulation, 2 = delta
inline int acc_mode(int acc_kind, bool lds_fits) {
  if (acc_kind == 0) return AM_NONE;
  return AM_ON | (acc_kind == 2 ? AM_DELTA : 0) | (lds_fits ? AM_INLDS : 0);
}

// A bounds call's (ub, lb) arrays as the re-checks take
// them: a row their fp32 stage decides gets its bounds there.
struct RcBnd {
  float *ub, *lb;
};

// dkm_recheck.hip (the <double> / <float> forms are instantiated there).
// bnd: a bounds call (d <= 32, not wave_all); null: no bounds are written.
bool list_ok(int64_t k, int64_t d);
template <class TX>
int launch_list(const TX *X, int d, int64_t ldx, int k, const WsView &v,
                int32_t *lab_out, double *acc, int acc_kind, bool vec,
                int64_t base, int nseg, hipStream_t s, bool wave_all = false,
                const RcBnd *bnd = nullptr);
template <class TX>
int launch_recheck(const TX *X, int64_t end, int d, int64_t ldx, int k,
                   const WsView &v, int32_t *lab_out, double *acc,
                   int acc_kind, bool vec, int64_t base, hipStream_t s,
                   const RcBnd *bnd = nullptr);

}  // namespace dkm
