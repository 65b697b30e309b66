// dkm_fft.hip -- one-dimensional complex FFT in fp64 (dislib.fft): Stockham
// auto-sort passes of radix 16 / 8 / 4 / 2 with the points of a block in
// registers and LDS, on interleaved complex128 in global memory.
//
// A block of 256 threads owns FFT_PTS = 4096 points: T = 4096 / L transforms
// of length L.  Every thread holds 16 points in registers, as 16 / R
// butterflies of radix R.  With Ns the product of the radices already done,
// butterfly j of a transform (j < L / R, k = j mod Ns) is
//     v[q] = in[j + q L / R] * w^(q k),   w = exp(-2 pi i / (Ns R)),
//     V = DFT_R(v),
//     out[(j / Ns) Ns R + k + q Ns] = V[q],                    q = 0 .. R - 1,
// so the finished digits stay fastest and no bit-reversal pass is needed.
// The first pass has Ns = 1: no twiddles.  The first pass reads global memory
// into registers and the last writes global memory from them; between two
// passes the points go through LDS: load all 16 points, barrier, butterfly,
// store all 16, barrier (one buffer, so a pass may not overwrite what another
// thread has not loaded yet).  A small radix 2^(lg L mod 4) comes first, then
// radix 16 only: 4096 = 16^3 takes three passes and two exchanges.
//
// Three kernels share the pass code:
//   k_fft_lds<PLAIN>   T contiguous transforms, L = n <= 4096.
//   k_fft_cols         one outer pass of radix r <= 256 of a length-nn piece
//                      seen as (r, M = nn / r): a block takes a tile of
//                      T = 4096 / r adjacent inner positions (16 at r = 256)
//                      by all r points, so its lanes run along the inner
//                      index in global memory (t fastest: runs of T complex
//                      values), transforms the T columns, multiplies result
//                      k1 of inner position p by exp(-2 pi i p k1 / nn) and
//                      writes it back to row k1 of the same view.  Row k1 is
//                      then a contiguous piece of length M whose transform
//                      gives the outputs k1 + r k'.
//   k_fft_lds<STRIDED> the last step of n > 4096: the contiguous pieces of
//                      length L = n / P, P = r1 r2.  Piece (k1, k2) lies at
//                      (k1 r2 + k2) L and holds the outputs
//                      k1 + r1 k2 + P k3; a block takes the T pieces
//                      k1 .. k1 + T - 1 of one k2 and its last pass runs its
//                      lanes along k1 (t fastest), so that a store covers T
//                      adjacent outputs every P.
//
// LDS: real and imaginary parts in two double arrays, point i of the block
// (i = t L + index) at pad(i) = i + (i >> 5).  The LDS serves an 8-byte
// access of 32 lanes per step from 32 pairs of banks, bank pair = pad(i) mod
// 32.  Loads of a pass take j + q L / R with consecutive j on consecutive
// lanes: 32 aligned consecutive i share i >> 5, so they are 32 different
// pairs.  The stores of the first pass (Ns = 1) take j R + q: a power-of-two
// stride R <= 32, which unpadded would fall into 32 / R pairs; with the pad,
// lane j adds (j R) >> 5 = j / (32 / R), which counts up once the multiples
// of R wrap around mod 32: 32 different pairs.  Stores with Ns >= 32 are
// runs of 32 again.  What stays is a store with 1 < Ns < 32 (the pass after
// a first pass of radix Ns): runs of Ns lanes R Ns apart, where two runs can
// meet in one pair (2 lanes per pair at worst); the t-fastest loads and
// stores of k_fft_cols and of the STRIDED last pass have stride L and meet
// in up to 8 lanes per pair.  The measured counter is in DESIGN.md 3.22.
//
// No atomics anywhere: the same input gives the same bits.
#include <algorithm>
#include <cmath>

#include "dkm_internal.h"

namespace dkm {

namespace {

constexpr int FFT_B = 256;              // threads per block
constexpr int FFT_LG_PTS = 12;          // lg of the points per block
constexpr int FFT_PTS = 1 << FFT_LG_PTS;
constexpr int FFT_LDS = FFT_PTS + (FFT_PTS >> 5);   // doubles per array
constexpr size_t FFT_LDS_BYTES = (size_t)FFT_LDS * 2 * sizeof(double);
constexpr int FFT_MAX_LG = 28;

enum { FFT_PLAIN = 0, FFT_STRIDED = 1, FFT_COLS = 2 };

struct cplx {
  double x, y;
};

__device__ __forceinline__ cplx operator+(cplx a, cplx b) {
  return {a.x + b.x, a.y + b.y};
}
__device__ __forceinline__ cplx operator-(cplx a, cplx b) {
  return {a.x - b.x, a.y - b.y};
}
__device__ __forceinline__ cplx cmul(cplx a, double wr, double wi) {
  return {fma(a.x, wr, -(a.y * wi)), fma(a.x, wi, a.y * wr)};
}

__device__ __forceinline__ int fft_pad(int i) { return i + (i >> 5); }

// z * exp(-2 pi i e / 16), e a constant after unrolling: +-1 and +-i are
// swaps and signs, the odd eighths one multiply per part
__device__ __forceinline__ cplx mul_w16(cplx z, int e) {
  constexpr double C = 0.92387953251128675613;   // cos(pi / 8)
  constexpr double S = 0.38268343236508977173;   // sin(pi / 8)
  constexpr double H = 0.70710678118654752440;   // sqrt(1 / 2)
  switch (e & 15) {
    case 0: return z;
    case 1: return cmul(z, C, -S);
    case 2: return {H * (z.x + z.y), H * (z.y - z.x)};
    case 3: return cmul(z, S, -C);
    case 4: return {z.y, -z.x};
    case 5: return cmul(z, -S, -C);
    case 6: return {H * (z.y - z.x), -(H * (z.x + z.y))};
    case 7: return cmul(z, -C, -S);
    case 8: return {-z.x, -z.y};
    case 9: return cmul(z, -C, S);
    case 10: return {-(H * (z.x + z.y)), H * (z.x - z.y)};
    case 11: return cmul(z, -S, C);
    case 12: return {-z.y, z.x};
    case 13: return cmul(z, S, C);
    case 14: return {H * (z.x - z.y), H * (z.x + z.y)};
    default: return cmul(z, C, S);
  }
}

__device__ __forceinline__ void bf2(cplx &a, cplx &b) {
  const cplx t = a;
  a = t + b;
  b = t - b;
}

// DFT_4 in place, outputs in natural order
__device__ __forceinline__ void bf4(cplx &a, cplx &b, cplx &c, cplx &d) {
  const cplx t0 = a + c, t1 = a - c, t2 = b + d, u = b - d;
  const cplx t3 = {u.y, -u.x};          // (b - d) * -i
  a = t0 + t2;
  b = t1 + t3;
  c = t0 - t2;
  d = t1 - t3;
}

// DFT_R of v[0 .. R) in place.  R = 4 B is done as B-point transforms over
// v[a + 4 b], the twiddles exp(-2 pi i a c / R), then 4-point transforms
// over a: output q = c + B d is left in v[4 c + d] (fft_slot).
template <int R>
__device__ __forceinline__ void bfly(cplx *v) {
  if (R == 2) {
    bf2(v[0], v[1]);
  } else if (R == 4) {
    bf4(v[0], v[1], v[2], v[3]);
  } else if (R == 8) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      bf2(v[a], v[a + 4]);
      v[a + 4] = mul_w16(v[a + 4], 2 * a);
    }
    bf4(v[0], v[1], v[2], v[3]);
    bf4(v[4], v[5], v[6], v[7]);
  } else if (R == 16) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      bf4(v[a], v[a + 4], v[a + 8], v[a + 12]);
#pragma unroll
      for (int c = 1; c < 4; ++c) v[a + 4 * c] = mul_w16(v[a + 4 * c], a * c);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      bf4(v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);
  }
}

// the register of output q after bfly<R>
template <int R>
__device__ __forceinline__ constexpr int fft_slot(int q) {
  return R == 8 ? 4 * (q & 1) + (q >> 1)
                : R == 16 ? 4 * (q & 3) + (q >> 2) : q;
}

// What a block works on: T = 4096 >> lgL transforms of length 1 << lgL,
// element i of transform t at in[t in_ts + i in_es], result k at
// out[t out_ts + k out_es]; only transforms t < tvalid exist.
struct FftBlock {
  const double2 *in;
  double2 *out;
  int64_t in_ts, in_es, out_ts, out_es;
  const double2 *tw;   // exp(-2 pi i k / n), k < n = 1 << lgn
  int lgn, lgL, tvalid;
  // FFT_COLS: result k of transform t is multiplied by tw[(pos0 + t) k << ows]
  int64_t pos0;
  int ows;
};

// One pass of radix R = 1 << LGR over the block's points; lgNs: lg of the
// product of the radices before it.
template <int LGR, bool FIRST, int MODE>
__device__ __forceinline__ void fft_pass(const FftBlock &a, double *sre,
                                         double *sim, int lgNs) {
  constexpr int R = 1 << LGR, NBF = 16 / R;
  const int lgL = a.lgL, lgT = FFT_LG_PTS - lgL, lgJ = lgL - LGR;
  const bool last = lgNs + LGR == lgL;
  // lanes along the transforms where global memory is contiguous in t
  const bool tfast = (FIRST && MODE == FFT_COLS) || (last && MODE != FFT_PLAIN);
  cplx v[16];
  int tt[NBF], jj[NBF];
#pragma unroll
  for (int u = 0; u < NBF; ++u) {
    const int b = threadIdx.x + FFT_B * u;
    const int t = tfast ? b & ((1 << lgT) - 1) : b >> lgJ;
    const int j = tfast ? b >> lgT : b & ((1 << lgJ) - 1);
    tt[u] = t;
    jj[u] = j;
    if (t >= a.tvalid) continue;
    const int k = j & ((1 << lgNs) - 1);
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int i = j + (q << lgJ);
      cplx x;
      if (FIRST) {
        const double2 g = a.in[t * a.in_ts + i * a.in_es];
        x = {g.x, g.y};
      } else {
        const int p = fft_pad((t << lgL) + i);
        x = {sre[p], sim[p]};
        if (q > 0) {
          const double2 w = a.tw[(int64_t)(q * k) << (a.lgn - lgNs - LGR)];
          x = cmul(x, w.x, w.y);
        }
      }
      v[u * R + q] = x;
    }
  }
  if (!FIRST) __syncthreads();   // every load is done before any store
#pragma unroll
  for (int u = 0; u < NBF; ++u) {
    const int t = tt[u], j = jj[u];
    if (t >= a.tvalid) continue;
    bfly<R>(v + u * R);
    const int k = j & ((1 << lgNs) - 1);
    const int j0 = ((j >> lgNs) << (lgNs + LGR)) + k;
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int o = j0 + (q << lgNs);
      cplx y = v[u * R + fft_slot<R>(q)];
      if (last) {
        if (MODE == FFT_COLS) {
          const double2 w = a.tw[((a.pos0 + t) * o) << a.ows];
          y = cmul(y, w.x, w.y);
        }
        a.out[t * a.out_ts + o * a.out_es] = make_double2(y.x, y.y);
      } else {
        const int p = fft_pad((t << lgL) + o);
        sre[p] = y.x;
        sim[p] = y.y;
      }
    }
  }
  if (!last) __syncthreads();
}

template <int MODE>
__device__ __forceinline__ void fft_block(const FftBlock &a) {
  extern __shared__ double fft_lds[];
  double *sre = fft_lds, *sim = fft_lds + FFT_LDS;
  int lgNs = a.lgL & 3;
  switch (lgNs) {
    case 1: fft_pass<1, true, MODE>(a, sre, sim, 0); break;
    case 2: fft_pass<2, true, MODE>(a, sre, sim, 0); break;
    case 3: fft_pass<3, true, MODE>(a, sre, sim, 0); break;
    default:
      fft_pass<4, true, MODE>(a, sre, sim, 0);
      lgNs = 4;
  }
  for (; lgNs < a.lgL; lgNs += 4) fft_pass<4, false, MODE>(a, sre, sim, lgNs);
}

// PLAIN: G contiguous transforms of length L <= 4096, T per block.
// STRIDED: per input of length n, P = 1 << lgP pieces of length L; block
// (b, l0 / T) takes the pieces of the outputs l0 .. l0 + T - 1 mod P, where
// l = k1 + (k2 << lgr1) lies at piece (k1 << lgr2) + k2.
template <int MODE>
__global__ __launch_bounds__(FFT_B) void k_fft_lds(
    const double2 *in, double2 *out, const double2 *tw, int lgn, int lgL,
    int64_t G, int lgr1, int lgr2) {
  FftBlock a;
  const int lgT = FFT_LG_PTS - lgL;
  const int64_t L = (int64_t)1 << lgL;
  a.tw = tw;
  a.lgn = lgn;
  a.lgL = lgL;
  a.pos0 = 0;
  a.ows = 0;
  if (MODE == FFT_PLAIN) {
    const int64_t g0 = (int64_t)blockIdx.x << lgT;
    a.in = in + g0 * L;
    a.out = out + g0 * L;
    a.in_ts = a.out_ts = L;
    a.in_es = a.out_es = 1;
    a.tvalid = (int)min((int64_t)1 << lgT, G - g0);
  } else {
    const int lgP = lgr1 + lgr2, lgBP = lgP - lgT;   // blocks per input
    const int64_t b = blockIdx.x >> lgBP;
    const int64_t l0 = (blockIdx.x & (((int64_t)1 << lgBP) - 1)) << lgT;
    const int64_t k2 = l0 >> lgr1, k1 = l0 & (((int64_t)1 << lgr1) - 1);
    a.in = in + (b << lgn) + (((k1 << lgr2) + k2) << lgL);
    a.in_ts = L << lgr2;
    a.in_es = 1;
    a.out = out + (b << lgn) + l0;
    a.out_ts = 1;
    a.out_es = (int64_t)1 << lgP;
    a.tvalid = 1 << lgT;
  }
  fft_block<MODE>(a);
}

// One outer pass of radix r = 1 << lgr over pieces of length nn = 1 << lgnn
// (consecutive in memory): block (g, tile) takes the inner positions
// tile T .. tile T + T - 1 of piece g, T = 4096 >> lgr.
__global__ __launch_bounds__(FFT_B) void k_fft_cols(
    const double2 *in, double2 *out, const double2 *tw, int lgn, int lgnn,
    int lgr) {
  FftBlock a;
  const int lgT = FFT_LG_PTS - lgr, lgM = lgnn - lgr, lgTiles = lgM - lgT;
  const int64_t g = blockIdx.x >> lgTiles;
  const int64_t tile = blockIdx.x & (((int64_t)1 << lgTiles) - 1);
  const int64_t base = (g << lgnn) + (tile << lgT);
  a.in = in + base;
  a.out = out + base;
  a.in_ts = a.out_ts = 1;
  a.in_es = a.out_es = (int64_t)1 << lgM;
  a.tw = tw;
  a.lgn = lgn;
  a.lgL = lgr;
  a.tvalid = 1 << lgT;
  a.pos0 = tile << lgT;
  a.ows = lgn - lgnn;
  fft_block<FFT_COLS>(a);
}

int ilog2(int64_t n) {
  int e = 0;
  while (((int64_t)1 << e) < n) ++e;
  return e;
}

bool fft_shape_ok(int64_t n, int64_t batch) {
  return n >= 1 && (n & (n - 1)) == 0 && n <= ((int64_t)1 << FFT_MAX_LG) &&
         batch >= 1 && batch <= INT64_MAX / 16 / n &&
         (n * batch + FFT_PTS - 1) / FFT_PTS <= INT32_MAX;
}

// The plan (fft_plan of _device.py): lg of the outer radices r1, r2 (0 =
// no such pass) and of the length L the LDS kernel transforms.
struct FftPlan {
  int lgr1, lgr2, lgL;
};

FftPlan fft_plan(int lgn) {
  if (lgn <= 12) return {0, 0, lgn};
  if (lgn <= 20) {
    const int lgr = std::min(8, lgn - 8);
    return {lgr, 0, lgn - lgr};
  }
  const int lgL = std::max(8, lgn - 16);
  return {8, lgn - lgL - 8, lgL};
}

size_t fft_ws_bytes(int64_t n, int64_t batch) {
  return n > FFT_PTS ? (size_t)round_up(n * batch * 16, 256) : 256;
}

template <class K>
int fft_lds_attr(K kernel) {
  return hipFuncSetAttribute((const void *)kernel,
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)FFT_LDS_BYTES) == hipSuccess
             ? 0
             : 1;
}

}  // namespace

}  // namespace dkm

using namespace dkm;

extern "C" {

size_t dkm_fft_workspace_bytes(int64_t n, int64_t batch) {
  if (!fft_shape_ok(n, batch)) return 0;
  return fft_ws_bytes(n, batch);
}

int dkm_fft_twiddles(int64_t n, double *out) {
  if (n < 1 || (n & (n - 1)) || n > ((int64_t)1 << FFT_MAX_LG) || !out)
    return fail(DKM_E_ARG, "fft twiddles: bad arguments");
  auto put = [&](int64_t k, long double re, long double im) {
    out[2 * k] = (double)re;
    out[2 * k + 1] = (double)im;
  };
  if (n < 8) {                                // powers of -i only
    static const double q[4][2] = {{1, 0}, {0, -1}, {-1, 0}, {0, 1}};
    for (int64_t k = 0; k < n; ++k) put(k, q[k * (4 / n)][0], q[k * (4 / n)][1]);
    return 0;
  }
  // the first octant in long double, rounded once; the others by symmetry
  const long double step = 2.0L * 3.14159265358979323846264338327950288L /
                           (long double)n;
  for (int64_t k = 0; k <= n / 8; ++k) {
    const long double c = cosl(step * (long double)k);
    const long double s = sinl(step * (long double)k);
    put(k, c, -s);
    put(n / 4 - k, s, -c);
    put(n / 4 + k, -s, -c);
    put(n / 2 - k, -c, -s);
    put(n / 2 + k, -c, s);
    put(3 * n / 4 - k, -s, c);
    put(3 * n / 4 + k, s, c);
    if (k > 0) put(n - k, c, s);
  }
  put(0, 1, 0);
  put(n / 4, 0, -1);
  put(n / 2, -1, 0);
  put(3 * n / 4, 0, 1);
  return 0;
}

int dkm_fft_z(const void *in, void *out, int64_t n, int64_t batch,
              const void *twiddles, void *ws, size_t ws_bytes, void *stream) {
  if (!fft_shape_ok(n, batch) || !in || !out || in == out ||
      (n > 1 && !twiddles) || ((uintptr_t)in | (uintptr_t)out |
                               (uintptr_t)twiddles | (uintptr_t)ws) % 16)
    return fail(DKM_E_ARG, "fft: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  if (n == 1) {
    if (hipMemcpyAsync(out, in, (size_t)batch * 16, hipMemcpyDeviceToDevice,
                       s) != hipSuccess)
      return fail(DKM_E_LAUNCH, "fft: copy");
    return 0;
  }
  if (n > FFT_PTS && (!ws || ws == in || ws == out ||
                      ws_bytes < fft_ws_bytes(n, batch)))
    return fail(DKM_E_WORKSPACE, "fft: workspace too small");
  if (fft_lds_attr(k_fft_lds<FFT_PLAIN>) || fft_lds_attr(k_fft_lds<FFT_STRIDED>) ||
      fft_lds_attr(k_fft_cols))
    return fail(DKM_E_LAUNCH, "fft: LDS attribute");
  const int lgn = ilog2(n);
  const FftPlan p = fft_plan(lgn);
  const double2 *x = (const double2 *)in, *tw = (const double2 *)twiddles;
  double2 *y = (double2 *)out, *w = (double2 *)ws;
  const unsigned nblk = (unsigned)((n * batch + FFT_PTS - 1) / FFT_PTS);
  if (!p.lgr1) {
    const int lgT = FFT_LG_PTS - p.lgL;
    const int64_t nb = (batch + ((int64_t)1 << lgT) - 1) >> lgT;
    k_fft_lds<FFT_PLAIN><<<(unsigned)nb, FFT_B, FFT_LDS_BYTES, s>>>(
        x, y, tw, lgn, p.lgL, batch, 0, 0);
    return check_launch("fft");
  }
  // the outer passes end in the workspace, the LDS pass in the output
  const double2 *src = x;
  if (p.lgr2) {
    k_fft_cols<<<nblk, FFT_B, FFT_LDS_BYTES, s>>>(src, y, tw, lgn, lgn,
                                                  p.lgr1);
    if (int r = check_launch("fft: first outer pass")) return r;
    k_fft_cols<<<nblk, FFT_B, FFT_LDS_BYTES, s>>>(y, w, tw, lgn,
                                                  lgn - p.lgr1, p.lgr2);
    if (int r = check_launch("fft: second outer pass")) return r;
  } else {
    k_fft_cols<<<nblk, FFT_B, FFT_LDS_BYTES, s>>>(src, w, tw, lgn, lgn,
                                                  p.lgr1);
    if (int r = check_launch("fft: outer pass")) return r;
  }
  k_fft_lds<FFT_STRIDED><<<nblk, FFT_B, FFT_LDS_BYTES, s>>>(
      w, y, tw, lgn, p.lgL, 0, p.lgr1, p.lgr2);
  return check_launch("fft: LDS pass");
}

}  // extern "C"

// Code-object preload (dkm_preload): see dkm_ordered.hip.
namespace dkm {
DKM_TU_FLAGS(fft, 0)
__global__ void k_tu_fft() {}
int preload_fft() {
  hipFuncAttributes a;
  const bool ok = hipFuncGetAttributes(&a, (const void *)k_tu_fft) == hipSuccess;
  return ok ? 0 : 1;
}
}  // namespace dkm
