// dkm_recheck_kernels.inc -- k_recheck_lane and k_recheck_list, included by
// dkm_recheck.hip twice: RC_BND 0 gives the kernels of those names, RC_BND 1
// the _bnd forms of a bounds call (DESIGN.md 3.14), which take the call's
// (ub, lb) arrays and let resolve_lane's stage 1 write the bounds of the rows
// it decides (counted in hdr->bnd_settled).  One text, so that the two forms
// cannot drift apart and the plain kernels' code stays what it was.
#if RC_BND
#define RC_NAME(x) x##_bnd
#define RC_BND_PARAM , RcBnd rb
#else
#define RC_NAME(x) x
#define RC_BND_PARAM
#endif

template <int MAXD, bool VEC, class TX>
__global__ void __launch_bounds__(BLOCK)
    RC_NAME(k_recheck_lane)(const TX *__restrict__ X, int64_t n, int d, int64_t ldx,
                   int k, WsView v, int32_t *__restrict__ lab_out,
                   double *acc, int amode, int64_t base RC_BND_PARAM) {
  if (v.hdr->qcount == 0) return;  // the screen resolved everything
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int dp = (int)round_up(d, 4);  // c32 row stride (dkm_util)
  // (fp32 centres: global, scalar loads in resolve_lane)
  int64_t *lists = (int64_t *)smem;
  double *lds_acc = (double *)(lists + (BLOCK / 64) * RL_CAP);
  __shared__ unsigned long long blk_count;
  if (threadIdx.x == 0) blk_count = 0;
#if RC_BND
  __shared__ unsigned long long blk_settled;
  unsigned nset = 0;
  if (threadIdx.x == 0) blk_settled = 0;
#endif
  if (amode & AM_INLDS) zero_lds_acc(lds_acc, k, d);
  const float cm =
      (float)__longlong_as_double((long long)v.hdr->cmax_bits) * 1.000001f;
  const AccTarget at = acc_target(amode, lds_acc, acc, k, d);
  __syncthreads();

  const int lane = threadIdx.x & 63;
  int64_t *wl = lists + (threadIdx.x >> 6) * RL_CAP;

  auto resolve = [&](int64_t i) {
#if RC_BND
    resolve_lane<MAXD, VEC, TX, false, true>(X, ldx, d, k, i,
                                             -lab_out[i] - 2, v.c32, v.cn32,
                                             dp, cm, v.ct64, lab_out, amode,
                                             at, rb, &nset);
#else
    resolve_lane<MAXD, VEC, TX>(X, ldx, d, k, i, -lab_out[i] - 2, v.c32,
                                v.cn32, dp,
                                cm, v.ct64, lab_out, amode, at);
#endif
  };

  // Scan: 4 labels per lane (int4), 256 per wave step, the next step's
  // labels in flight while this one resolves (a wave's list only holds
  // samples of steps it has already scanned, so the prefetch is never stale).
  // a0 aligns the int4 loads; lanes outside [base, n) read nothing.
  const int64_t wv = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  const int64_t nwv = (int64_t)gridDim.x * (BLOCK / 64);
  const int64_t a0 =
      base - (int64_t)(((uintptr_t)(lab_out + base) >> 2) & 3);
  auto load4 = [&](int64_t c0, int (&o)[4]) {
    const int64_t i0 = c0 + 4 * lane;
    if (i0 >= base && i0 + 3 < n) {
      const int4 q4 = *(const int4 *)(lab_out + i0);
      o[0] = q4.x; o[1] = q4.y; o[2] = q4.z; o[3] = q4.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        o[c] = (i0 + c >= base && i0 + c < n) ? lab_out[i0 + c] : 0;
    }
  };
  unsigned long long mine = 0;
  int cnt = 0;  // wave-uniform list length
  int cur[4] = {0, 0, 0, 0};
  int64_t c0 = a0 + wv * 256;
  if (c0 < n) load4(c0, cur);
  for (; c0 < n; c0 += nwv * 256) {
    int nxt[4] = {0, 0, 0, 0};
    if (c0 + nwv * 256 < n) load4(c0 + nwv * 256, nxt);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const unsigned long long mask = __ballot(cur[c] < 0);
      if (cur[c] < 0)
        wl[cnt + __popcll(mask & ((1ull << lane) - 1))] = c0 + 4 * lane + c;
      const int add = __popcll(mask);
      mine += add;
      cnt += add;
      if (cnt >= 64) {
        wave_lds_sync();
        resolve(wl[lane]);
        const int rem = cnt - 64;
        const int64_t tail = lane < rem ? wl[64 + lane] : 0;
        wave_lds_sync();
        if (lane < rem) wl[lane] = tail;
        cnt = rem;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) cur[c] = nxt[c];
  }
  wave_lds_sync();
  if (lane < cnt) resolve(wl[lane]);
  recheck_finish_count(mine, &blk_count, v);
#if RC_BND
  recheck_finish_settled(nset, &blk_settled, v);
#endif
  if (amode & AM_INLDS) flush_lds_acc(lds_acc, acc, k, d);
}

// The screen's per-wave lists (WsView::tlist/tcount, nseg segments): lane
// per listed sample (resolve_lane), fp32 centres in LDS.  No label scan:
// the work is proportional to the undecided samples only.
template <int MAXD, bool VEC, class TX>
__global__ void __launch_bounds__(BLOCK)
    RC_NAME(k_recheck_list)(const TX *__restrict__ X, int d, int64_t ldx, int k,
                   WsView v, int32_t *__restrict__ lab_out, double *acc,
                   int amode, int64_t base, int nseg, int wave_all
                   RC_BND_PARAM) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int dp = (int)round_up(d, 4);
  // (fp32 centres: global, scalar loads in resolve_lane)
  double *lds_acc = (double *)smem;
  __shared__ unsigned long long blk_count;
  // per wave: samples stage 1 left undecided, resolved 64 at a time (a
  // lone stage-2 lane would otherwise hold its whole wave for a second pass)
  __shared__ int2 dlist[BLOCK / 64][128];
  if (threadIdx.x == 0) blk_count = 0;
#if RC_BND
  __shared__ unsigned long long blk_settled;
  unsigned nset = 0;
  if (threadIdx.x == 0) blk_settled = 0;
#endif
  if (amode & AM_INLDS) zero_lds_acc(lds_acc, k, d);
  const float cm =
      (float)__longlong_as_double((long long)v.hdr->cmax_bits) * 1.000001f;
  const AccTarget at = acc_target(amode, lds_acc, acc, k, d);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  const int64_t nwv = (int64_t)gridDim.x * (BLOCK / 64);
  unsigned long long mine = 0;
  int2 *dl = dlist[threadIdx.x >> 6];
  int dcnt = 0;  // wave-uniform
  auto stage2 = [&](int2 it) {
    resolve_lane<MAXD, VEC, TX>(X, ldx, d, k, base + it.x, it.y, v.c32,
                                v.cn32, dp,
                                cm, v.ct64, lab_out, amode, at);
  };
  // wave_all: the samples go to the global list that k_recheck_wave
  // resolves a wave per sample (v.smoved as (offset, prev) pairs; the
  // per-wave LDS list only takes what overflows it).  Otherwise stage 1 runs
  // here lane per sample and its leftovers are resolved 64 at a time (a long
  // list holds many of them: a wave per sample cost 0.7 ms per C2 iteration)
  int2 *s2l = (int2 *)v.smoved;
  const uint32_t s2cap = (uint32_t)std::min<int64_t>(v.nq / 2, INT32_MAX);
  // (segment, 64-sample batch) pairs dealt round-robin over all waves, batch
  // index major: every resident wave gets work and the segments' row loads
  // overlap across waves.  Wave-uniform loop; empty batches are skipped.
  for (int64_t L = wv; L < (int64_t)nseg * (TL_CAP / 64); L += nwv) {
    const int64_t sg = L % nseg;
    const int t0 = (int)(L / nseg) * 64;
    const int cnt = v.tcount[sg];
    if (t0 == 0) mine += cnt;
    if (t0 >= cnt) continue;
    const int2 *e = v.tlist + sg * TL_CAP;
    {
      int2 it = make_int2(0, 0);
      bool ok = true;
      if (t0 + lane < cnt) {
        it = e[t0 + lane];
        // wave_all (short lists): every sample straight to k_recheck_wave
#if RC_BND
        ok = !wave_all &&
             resolve_lane<MAXD, VEC, TX, true, true>(
                 X, ldx, d, k, base + it.x, it.y, v.c32, v.cn32, dp, cm,
                 v.ct64, lab_out, amode, at, rb, &nset);
#else
        ok = !wave_all &&
             resolve_lane<MAXD, VEC, TX, true>(X, ldx, d, k, base + it.x,
                                               it.y, v.c32, v.cn32, dp, cm,
                                               v.ct64, lab_out, amode, at);
#endif
      }
      unsigned long long m = __ballot(!ok);
      if (m && wave_all) {
        uint32_t pos = 0;
        if (lane == 0) pos = atomicAdd(&v.hdr->s2count, (uint32_t)__popcll(m));
        pos = (uint32_t)__shfl((int)pos, 0, 64);
        const uint32_t p = pos + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (!ok && p < s2cap) s2l[p] = it;
        m = __ballot(!ok && p >= s2cap);   // the rest: this wave, stage 2
        ok = ok || p < s2cap;
      }
      if (!ok) dl[dcnt + __popcll(m & ((1ull << lane) - 1))] = it;
      dcnt += __popcll(m);
      if (dcnt >= 64) {
        wave_lds_sync();
        stage2(dl[lane]);
        const int rem = dcnt - 64;
        const int2 tail = lane < rem ? dl[64 + lane] : make_int2(0, 0);
        wave_lds_sync();
        if (lane < rem) dl[lane] = tail;
        dcnt = rem;
      }
    }
  }
  wave_lds_sync();
  if (lane < dcnt) stage2(dl[lane]);
  recheck_finish_count(mine, &blk_count, v);
#if RC_BND
  recheck_finish_settled(nset, &blk_settled, v);
#endif
  if (amode & AM_INLDS) flush_lds_acc(lds_acc, acc, k, d);
}

#undef RC_NAME
#undef RC_BND_PARAM
