"""``screen_bound<P_F32>`` against the fp32 MFMA's accumulation order (DESIGN.md
3.14, "The re-check's stage 1 on fp32 MFMA tiles"); numpy only, no GPU.

``k_recheck_tile`` scores a row with ``v_mfma_f32_16x16x4_f32``: the chain
starts from cn32 = fl32(|c|^2) and takes eight k-slices in turn, slice m
holding the products of features {m, 8 + m, 16 + m, 24 + m} of x32 = fl32(x)
and -2 c32 = -2 fl32(c).  Two models of a slice are emulated here, and the
derivation covers both: four fused multiply-adds one after the other, and the
four exact products added to the accumulator with one rounding.  Either way
the score must lie within B / 2 of s = |c|^2 - 2 x.c (true fp64 x and c, long
double arithmetic), B = ``bound_f32(|x|, max |c|, d)``: the kernel's own B is
never smaller (its |x| and cmax are inflated).

Rows and centres are adversarial for a summation bound: magnitudes 1e-3 to
1e3 drawn per feature, pairs of features whose products cancel exactly in
x.c, centres parallel and antiparallel to the row (|x.c| = |x| |c|), and rows
that are a centre up to the last fp32 bits (s ~ -|c|^2 from terms of size
|c|^2).
"""
import numpy as np
import pytest

LD = np.longdouble
F = np.float32


def bound_f32(xn, cm, d):
    """``screen_bound<P_F32>(d, xn, cm, false)`` in fp64."""
    rel = (d + 6.0) * 2.0 ** -24
    s = xn + cm
    mag = 2.0 * xn * cm + cm * cm
    b = 2.0 * rel * mag + 16.0 * 2.0 ** -52 * s * s + \
        (8.0 * d) * 2.0 ** -120 * (s + 1.0)
    return b * 1.0001


def _fl32(v):
    """Long double -> fp32, one rounding (long double holds the exact sum of
    an fp32 accumulator and an fp32 x fp32 product unless their exponents are
    more than 16 apart, where the second rounding moves the result by at most
    2^-40 ulp: nothing against B)."""
    return np.asarray(v, dtype=LD).astype(F)


def mfma_scores(x, C, fused):
    """(n, k) fp32 scores in the MFMA's order.  x (n, d) and C (k, d) fp64,
    d <= 32, zero padded to 32 features as the kernel pads."""
    n, d = x.shape
    k = C.shape[0]
    x32 = np.zeros((n, 32), F)
    x32[:, :d] = x.astype(F)
    a32 = np.zeros((k, 32), F)
    a32[:, :d] = F(-2.0) * C.astype(F)                 # exact scaling
    cn32 = np.einsum("ij,ij->i", C, C).astype(F)       # fp64 sum, one rounding
    acc = np.broadcast_to(cn32[None, :], (n, k)).astype(F)
    for m in range(8):
        ts = [m, 8 + m, 16 + m, 24 + m]
        if fused:
            tot = acc.astype(LD)
            for t in ts:
                tot = tot + x32[:, t, None].astype(LD) * a32[None, :, t].astype(LD)
            acc = _fl32(tot)
        else:
            for t in ts:
                acc = _fl32(acc.astype(LD) + x32[:, t, None].astype(LD) *
                            a32[None, :, t].astype(LD))
    return acc


def true_scores(x, C):
    xl, Cl = x.astype(LD), C.astype(LD)
    return (Cl * Cl).sum(1)[None, :] - 2 * (xl[:, None, :] * Cl[None, :, :]).sum(2)


def _mags(rs, shape):
    return 10.0 ** rs.uniform(-3, 3, shape) * rs.choice([-1.0, 1.0], shape)


def _cases(d):
    rs = np.random.RandomState(100 + d)
    n, k = 96, 48
    x = _mags(rs, (n, d))
    C = _mags(rs, (k, d))
    # cancelling pairs: features 2i, 2i + 1 with equal x and opposite c
    for i in range(0, 16):
        for t in range(0, d - 1, 2):
            x[i, t + 1] = x[i, t]
            C[i, t + 1] = -C[i, t]
    # parallel / antiparallel centres, and rows that are nearly a centre
    for i in range(16, 32):
        C[i] = x[i] * (1.0 if i % 2 else -1.0) * 10.0 ** rs.uniform(-2, 2)
    for i in range(32, 48):
        x[i] = C[i] * (1.0 + rs.uniform(-1, 1, d) * 2.0 ** -22)
    # one large feature against many small ones
    x[48:64] = 10.0 ** rs.uniform(-3, -2, (16, d))
    x[48:64, d // 2] = 1e3
    return x, C


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("d", [1, 3, 8, 17, 31, 32])
def test_mfma_order_within_half_B(d, fused):
    x, C = _cases(d)
    s_hat = mfma_scores(x, C, fused).astype(LD)
    s = true_scores(x, C)
    xn = np.sqrt(np.einsum("ij,ij->i", x, x))
    cm = np.sqrt(np.einsum("ij,ij->i", C, C)).max()
    B = bound_f32(xn, cm, d)
    err = np.abs(s_hat - s).max(axis=1).astype(np.float64)
    worst = float((err / (0.5 * B)).max())
    print("d=%d fused=%s: worst |s^ - s| / (B / 2) = %.3f" % (d, fused, worst))
    assert np.all(err <= 0.5 * B), worst
    # the bound is not vacuous: the scores do carry fp32 rounding
    assert err.max() > 0.0
