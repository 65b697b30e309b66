// dkm_recheck_kernels.inc -- k_recheck_lane, k_recheck_list and the latter's
// tile form k_recheck_tile (d <= 32), included by
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

// The tile form of k_recheck_list at d <= 32 (not wave_all): the same lists,
// deal, decision rule, bounds and stage 2, but stage 1 scores a wave's 64
// listed rows on the fp32 MFMA instead of lane per row (DESIGN.md 3.14,
// "The re-check's stage 1 on fp32 MFMA tiles").
//   Rows: whole lines per wave instruction, k_screen_w32's list mapping (lane
//     l = row RI i + l / LR, 16-B piece l % LR of half c; element by element
//     when !VEC), converted to fl32 and passed half by half through a 4 KB
//     per-wave LDS transpose (64 rows x 64 B, 16-B pieces XOR-swizzled) into
//     the MFMA B operand: lane (q, j) holds features 8q + m, m < 8, of rows
//     16b + j, b < 4.  |x|^2 is summed by the loading lanes.
//   The next batch's row loads are issued before this one is scored (stage 1
//     keeps no fp64 row), and the batch after that has its list entries in
//     flight.  Non-empty batches are found 64 deal slots at a time (lane per
//     slot, one tcount load each).
//   Scores: -2 c32 in A-fragment order and cn32 staged in LDS once per block;
//     each chain starts from |c|^2 and takes the 8 k-slices {m, 8 + m, 16 + m,
//     24 + m} in turn.  Lane (q, j) sees centres 16 cb + 4q + i of row 16b + j
//     and keeps a top-2 per b; two xor steps merge the four q, and row
//     l = 16b + j is lane l's own b = q.
#if !RC_BND
constexpr int RT_SCR = 4096 + 256;  // per wave: half-tile transpose, |x|^2
static size_t recheck_tile_lds(int64_t k) {
  return (size_t)(kpad16(k) / 16) * (2048 + 64) + (size_t)(BLOCK / 64) * RT_SCR;
}
#endif

template <bool VEC, class TX>
__global__ void __launch_bounds__(BLOCK)
    __attribute__((amdgpu_waves_per_eu(2)))  // two blocks per CU
    RC_NAME(k_recheck_tile)(const TX *__restrict__ X, int d, int64_t ldx, int k,
                   WsView v, int32_t *__restrict__ lab_out, double *acc,
                   int amode, int64_t base, int nseg RC_BND_PARAM) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int dp = (int)round_up(d, 4);
  const int nkb = (int)(kpad16(k) / 16);
  float *frag = (float *)smem;              // nkb x 2 KB, A-fragment order
  float *cn = frag + (int64_t)nkb * 512;    // nkb x 16
  char *scr0 = (char *)(cn + nkb * 16);
  double *lds_acc = (double *)(scr0 + (BLOCK / 64) * RT_SCR);
  __shared__ unsigned long long blk_count;
  __shared__ int2 dlist[BLOCK / 64][128];
  if (threadIdx.x == 0) blk_count = 0;
#if RC_BND
  __shared__ unsigned long long blk_settled;
  unsigned nset = 0;
  if (threadIdx.x == 0) blk_settled = 0;
#endif
  // lane l of block cb: centre 16 cb + (l & 15), features 8 (l >> 4) + m
  for (int e = threadIdx.x; e < nkb * 512; e += BLOCK) {
    const int cb = e >> 9, l = (e >> 3) & 63, m = e & 7;
    const int c = cb * 16 + (l & 15), t = 8 * (l >> 4) + m;
    frag[e] = (c < k && t < d) ? -2.0f * v.c32[(int64_t)c * dp + t] : 0.f;
  }
  for (int e = threadIdx.x; e < nkb * 16; e += BLOCK)
    cn[e] = e < k ? v.cn32[e] : INFINITY;  // padding centres never score
  if (amode & AM_INLDS) zero_lds_acc(lds_acc, k, d);
  const float cm =
      (float)__longlong_as_double((long long)v.hdr->cmax_bits) * 1.000001f;
  const AccTarget at = acc_target(amode, lds_acc, acc, k, d);
  __syncthreads();
  const int lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
  const int wid = threadIdx.x >> 6;
  const int64_t wv = (int64_t)blockIdx.x * (BLOCK / 64) + wid;
  const int64_t nwv = (int64_t)gridDim.x * (BLOCK / 64);
  char *scr = scr0 + wid * RT_SCR;
  float *s_xx = (float *)(scr + 4096);
  unsigned long long mine = 0;  // per lane here: summed over the wave below
  int2 *dl = dlist[wid];
  int dcnt = 0;  // wave-uniform
  auto stage2 = [&](int2 it) {
    resolve_lane<32, VEC, TX>(X, ldx, d, k, base + it.x, it.y, v.c32, v.cn32,
                              dp, cm, v.ct64, lab_out, amode, at);
  };

  // (segment, 64-sample batch) pairs dealt round-robin over all waves, batch
  // index major, as k_recheck_list deals them; the non-empty ones of 64 slots
  // at a time (lane per slot)
  const int64_t total = (int64_t)nseg * (TL_CAP / 64);
  int64_t L0 = wv - 64 * nwv;
  unsigned long long pend = 0;
  int gcnt = 0;
  auto next_list = [&](int2 &it) -> bool {  // the next batch's entries
    while (!pend) {
      L0 += 64 * nwv;
      if (L0 >= total) return false;
      const int64_t Ll = L0 + lane * nwv;
      int lt0 = 0;
      gcnt = 0;
      if (Ll < total) {
        lt0 = (int)(Ll / nseg) * 64;
        gcnt = v.tcount[Ll % nseg];
        if (lt0 == 0) mine += gcnt;
      }
      pend = __ballot(lt0 < gcnt);
    }
    const int bit = __ffsll((long long)pend) - 1;
    pend &= pend - 1;
    const int64_t L = L0 + bit * nwv;
    const int64_t sg = L % nseg;
    const int t0 = (int)(L / nseg) * 64;
    const int cnt = __shfl(gcnt, bit, 64);
    it = t0 + lane < cnt ? v.tlist[sg * TL_CAP + t0 + lane]
                         : make_int2(-1, 0);  // x < 0: no row
    return true;
  };

  constexpr int EPL = 16 / (int)sizeof(TX);  // elements per 16-B piece
  constexpr int LR = 16 / EPL;                // lanes per half row (8 | 4)
  constexpr int RI = 64 / LR;                 // rows per instruction
  constexpr int IC = 64 / RI;                 // instructions per half
  typedef TX txv __attribute__((ext_vector_type(EPL)));
  txv raw[2][IC];
  const int lrow = lane / LR, lpos = lane % LR;
  auto load_rows = [&](int itx) {
#pragma unroll
    for (int i = 0; i < IC; ++i) {
      const int ro = __shfl(itx, RI * i + lrow, 64);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        raw[c][i] = txv{};
        // only the pieces that hold features (past d a piece could leave X)
        const int t0 = 16 * c + EPL * lpos;
        if (ro < 0 || t0 >= d) continue;
        const TX *p = X + (base + ro) * ldx + t0;
        if (VEC) {
          raw[c][i] = *(const txv *)p;
        } else {
#pragma unroll
          for (int e = 0; e < EPL; ++e)
            if (t0 + e < d) raw[c][i][e] = p[e];
        }
      }
    }
  };
  auto tx_addr = [](int row, int piece) {  // 16-B piece of a 64-B half row
    return 64 * row + 16 * (piece ^ ((row >> 1) & 3));
  };

  int2 itA = make_int2(-1, 0), itB = make_int2(-1, 0);
  bool haveA = next_list(itA);
  bool haveB = haveA && next_list(itB);
  if (haveA) load_rows(itA.x);
  while (haveA) {
    // ---- fl32, |x|^2, and the transpose into the B operand ----
    float xf[4][8];
    float xp[IC];
#pragma unroll
    for (int i = 0; i < IC; ++i) xp[i] = 0.f;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      wave_lds_sync();  // the previous readers of the transpose are done
#pragma unroll
      for (int i = 0; i < IC; ++i) {
        const int row = RI * i + lrow;
        float f[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          f[e] = (float)raw[c][i][e];
          xp[i] = fmaf(f[e], f[e], xp[i]);
        }
        if constexpr (EPL == 2)
          *(f32x2 *)(scr + tx_addr(row, lpos >> 1) + 8 * (lpos & 1)) =
              f32x2{f[0], f[1]};
        else
          *(f32x4 *)(scr + tx_addr(row, lpos)) = f32x4{f[0], f[1], f[2], f[3]};
      }
      wave_lds_sync();
      if ((q >> 1) == c) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int row = 16 * b + j;
          const f32x4 lo = *(const f32x4 *)(scr + tx_addr(row, 2 * (q & 1)));
          const f32x4 hi =
              *(const f32x4 *)(scr + tx_addr(row, 2 * (q & 1) + 1));
          xf[b][0] = lo.x; xf[b][1] = lo.y; xf[b][2] = lo.z; xf[b][3] = lo.w;
          xf[b][4] = hi.x; xf[b][5] = hi.y; xf[b][6] = hi.z; xf[b][7] = hi.w;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < IC; ++i) {
#pragma unroll
      for (int m = 1; m < LR; m <<= 1) xp[i] += __shfl_xor(xp[i], m, 64);
      if (lpos == 0) s_xx[RI * i + lrow] = xp[i];
    }
    wave_lds_sync();
    const float xx = s_xx[lane];
    // ---- the next batch's rows stream in while this one is scored ----
    if (haveB) load_rows(itB.x);
    int2 itC = make_int2(-1, 0);
    const bool haveC = haveB && next_list(itC);

    float r1[4], r2[4];
    int ri[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      r1[b] = INFINITY;
      r2[b] = INFINITY;
      ri[b] = 0;
    }
    for (int cb = 0; cb < nkb; ++cb) {
      const f32x4 c4 = *(const f32x4 *)(cn + cb * 16 + 4 * q);
      const float *blk = frag + cb * 512 + lane * 8;
      const f32x4 a0 = *(const f32x4 *)blk, a1 = *(const f32x4 *)(blk + 4);
      const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      f32x4 accv[4];
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          accv[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              a[m], xf[b][m], m == 0 ? c4 : accv[b], 0, 0, 0);
      const int jc0 = cb * 16 + 4 * q;
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float sc = accv[b][i];
          ri[b] = sc < r1[b] ? jc0 + i : ri[b];
          r2[b] = __builtin_amdgcn_fmed3f(r1[b], r2[b], sc);
          r1[b] = fminf(r1[b], sc);
        }
    }
    // the four q of a row: top-2 of the union (a tie keeps the lower index;
    // a tied row is never decided below)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int off = 16; off < 64; off <<= 1) {
        const float o1 = __shfl_xor(r1[b], off, 64);
        const float o2 = __shfl_xor(r2[b], off, 64);
        const int oi = __shfl_xor(ri[b], off, 64);
        const bool tk = (o1 < r1[b]) | ((o1 == r1[b]) & (oi < ri[b]));
        r2[b] = tk ? fminf(r1[b], o2) : fminf(r2[b], o1);
        ri[b] = tk ? oi : ri[b];
        r1[b] = tk ? o1 : r1[b];
      }
    const float b1 = q == 0 ? r1[0] : q == 1 ? r1[1] : q == 2 ? r1[2] : r1[3];
    const float b2 = q == 0 ? r2[0] : q == 1 ? r2[1] : q == 2 ? r2[2] : r2[3];
    const int i1 = q == 0 ? ri[0] : q == 1 ? ri[1] : q == 2 ? ri[2] : ri[3];

    // ---- lane = row: resolve_lane's decision rule, bounds and sums ----
    const int2 it = itA;
    const float xn = sqrtf(xx) * (1.0f + (d + 4) * 0x1.0p-24f);
    const float B = screen_bound<P_F32>(d, xn, cm, false);
    const bool sane = (xn < 1e18f) && (xn * cm < 1e30f) && (b1 < 1e30f);
    const bool decided = it.x >= 0 && sane && b2 - b1 > 2.0f * B;
    if (decided) {
      const int64_t i = base + it.x;
#if RC_BND
      if (b2 < 1e30f) {
        settle_bounds(xx, b1, b2, B, rb.ub + i, rb.lb + i);
        nset += 1u;
      }
#endif
      lab_out[i] = i1;
      const bool delta = amode & AM_DELTA;
      if ((amode & AM_ON) && !(delta && i1 == it.y)) {
        const bool sub = delta && it.y >= 0;
        const TX *xr = X + i * ldx;
        for (int t = 0; t < d; ++t) {
          const double x = ld_x(xr + t);
          at.add(i1, t, x);
          if (sub) at.add(it.y, t, -x);
        }
        at.count(i1, 1.0);
        if (sub) at.count(it.y, -1.0);
      }
    }
    const bool left = it.x >= 0 && !decided;
    const unsigned long long m = __ballot(left);
    if (left) dl[dcnt + __popcll(m & ((1ull << lane) - 1))] = it;
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
    itA = itB;
    itB = itC;
    haveA = haveB;
    haveB = haveC;
  }
  wave_lds_sync();
  if (lane < dcnt) stage2(dl[lane]);
#pragma unroll
  for (int off = 32; off; off >>= 1)
    mine += (unsigned long long)__shfl_xor((long long)mine, off, 64);
  recheck_finish_count(mine, &blk_count, v);
#if RC_BND
  recheck_finish_settled(nset, &blk_settled, v);
#endif
  if (amode & AM_INLDS) flush_lds_acc(lds_acc, acc, k, d);
}

#undef RC_NAME
#undef RC_BND_PARAM
