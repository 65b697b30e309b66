"""Host reference for the per-row k-means bounds; numpy only.

The Lloyd loop for d <= 32 keeps, per row, ``ub`` >= the distance to the row's
own centre and ``lb`` <= the distance to every other centre, and skips every
row with ``ub < lb``.  This module holds what the tests compare those fp32
arrays with:

* ``exact_distances``: the true distances, in long double;
* ``check_valid``: the invariant itself (a violation is a wrong label waiting
  to happen);
* ``screen_slack`` / ``check_screen_tight``: how far a bound the screen has
  just written may lie from the truth (a model of ``bound_consts<bf16x3>``,
  ``bound2_fast`` and the ``BND`` block of ``k_screen_w32``);
* ``pass_model`` / ``check_pass_tight``: how far the bounds pass
  (``k_drift``, ``k_bounds_pass``) may move a bound;
* ``drift_f32`` / ``pass_f32``: the bounds pass in numpy fp32, bit for bit,
  which tells the rows it left active from the rows it settled.

Every constant below is derived from the kernels' formulas in the docstring
that uses it; none is fitted to what a kernel returns.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LD = np.longdouble
# the reference's own rounding: long double (2^-64), d <= 32 squares, one
# root: below 2^-58 relative; 2^-40 leaves a wide margin and still lies far
# below the fp32 ulp (2^-24) by which a wrong bound would be off
REF_EPS = LD(2.0) ** -40
F32_TINY = 2.0 ** -149        # the least positive fp32 (subnormal)
_TINY = np.finfo(LD).tiny


def _chunks(n, size):
    return [(lo, min(n, lo + size)) for lo in range(0, n, size)]


def exact_distances(x, C, chunk=1024):
    """(n, k) distances ``sqrt(sum((x - c)^2))`` in long double.

    ``x``: the samples exactly as the device stores them (fp64, or fp32
    values, which widen exactly); ``C``: the fp64 centres.  Differences,
    squares and the sum over the d features are all long double; rows are
    done ``chunk`` at a time (a few threads: numpy releases the GIL).  A row
    or a centre with a non-finite value gives inf / nan there; the checks
    leave such rows out."""
    x = np.asarray(x)
    C = np.asarray(C, dtype=np.float64)
    n, d = x.shape
    k = C.shape[0]
    assert C.shape[1] == d
    out = np.empty((n, k), dtype=LD)
    Cl = C.astype(LD).T.copy()          # (d, k)

    def run(span):
        lo, hi = span
        xl = x[lo:hi].astype(LD)
        acc = np.zeros((hi - lo, k), dtype=LD)
        with np.errstate(invalid="ignore", over="ignore"):
            for t in range(d):
                df = xl[:, t, None] - Cl[t][None, :]
                df *= df
                acc += df
            np.sqrt(acc, out=out[lo:hi])

    spans = _chunks(n, chunk)
    workers = max(1, min(8, os.cpu_count() or 1, len(spans)))
    if workers == 1:
        for s in spans:
            run(s)
    else:
        with ThreadPoolExecutor(workers) as ex:
            list(ex.map(run, spans))
    return out


def own_other(D, labels):
    """(distance to the row's own centre, least distance to any other), long
    double; nan / inf pass through (np.min propagates nan)."""
    n = D.shape[0]
    idx = np.arange(n)
    labels = np.asarray(labels, dtype=np.int64)
    own = D[idx, labels].copy()
    Dm = D.copy()
    Dm[idx, labels] = np.inf
    with np.errstate(invalid="ignore"):
        other = Dm.min(axis=1)
    return own, other


def _worst(mask, score):
    """Index of the masked row with the largest score."""
    rows = np.flatnonzero(mask)
    return int(rows[np.argmax(np.asarray(score, dtype=np.float64)[rows])])


def check_valid(ub, lb, labels, D, what=""):
    """Raise AssertionError unless, for every row i whose distances are all
    finite,

        ub[i] >= D[i, label] (1 - 2^-40)
        lb[i] <= min_{j != label} D[i, j] (1 + 2^-40)
        lb[i] >= 0, and neither bound is NaN.

    The 2^-40 is the reference's rounding (REF_EPS), not a tolerance for the
    kernel, whose bounds are conservative by design.  The message names the
    worst offender: row, label, bound and distance.  With fewer than two
    centres, or no rows, nothing is checked."""
    D = np.asarray(D)
    n, k = D.shape
    if n == 0 or k < 2:
        return
    ub = np.asarray(ub)[:n]
    lb = np.asarray(lb)[:n]
    labels = np.asarray(labels, dtype=np.int64)[:n]
    assert np.all((labels >= 0) & (labels < k)), "%s: label out of range" % what
    own, other = own_other(D, labels)
    fin = np.isfinite(D).all(axis=1)
    ubl, lbl = ub.astype(LD), lb.astype(LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        bad_nan = fin & (np.isnan(ub) | np.isnan(lb))
        bad_neg = fin & (lb < 0)
        bad_ub = fin & (ubl < own * (1 - REF_EPS))
        bad_lb = fin & (lbl > other * (1 + REF_EPS))
        if bad_nan.any():
            i = int(np.flatnonzero(bad_nan)[0])
            kind = "NaN bound"
        elif bad_neg.any():
            i = _worst(bad_neg, -lb.astype(np.float64))
            kind = "negative lb"
        elif bad_ub.any():
            i = _worst(bad_ub, (own - ubl) / np.maximum(own, _TINY))
            kind = "ub below the distance to the own centre"
        elif bad_lb.any():
            i = _worst(bad_lb, (lbl - other) / np.maximum(lbl, _TINY))
            kind = "lb above the distance to another centre"
        else:
            return
    raise AssertionError(
        "%s: %s: row %d label %d ub %r own distance %s lb %r nearest other "
        "%s (%d NaN, %d negative, %d ub, %d lb violations of %d rows)"
        % (what, kind, i, int(labels[i]), float(ub[i]), own[i], float(lb[i]),
           other[i], int(bad_nan.sum()), int(bad_neg.sum()),
           int(bad_ub.sum()), int(bad_lb.sum()), n))


# ---------------------------------------------------------------------------
# the screen's bounds
# ---------------------------------------------------------------------------
def centre_norm_max(C):
    """``cm`` as ``k_prepare`` and ``k_screen_w32`` derive it: the largest
    centre norm (the root of the sequential fp64 sum of squares) times
    1.000001."""
    C = np.asarray(C, dtype=np.float64)
    n2 = np.zeros(C.shape[0])
    for t in range(C.shape[1]):
        n2 = n2 + C[:, t] * C[:, t]
    return float(np.sqrt(n2.max())) * 1.000001


def bound2(xn, cm, d):
    """``bound2_fast`` with ``bound_consts<bf16x3>``, in fp64: the screen's
    2B for a row of norm ``xn`` (packed scores)."""
    rel = 3.1 * 2.0 ** -16 + (3.0 * d + 6.0) * 2.0 ** -23
    k_mag = 2.0 * (2.0 * rel + 2.0 ** -16) * 1.0001
    k_s2 = 2.0 * 16.0 * 2.0 ** -52 * 1.0001
    k_s1 = 2.0 * (8.0 * d) * 2.0 ** -120 * 1.0001
    s = xn + cm
    return k_mag * (2.0 * xn * cm + cm * cm) + k_s2 * s * s + k_s1 * (s + 1.0)


def screen_slack(x, C, d, f32):
    """Per row, in fp64: what the square of a bound that ``k_screen_w32`` has
    just written may differ from the true squared distance by,

        slack = 2^-15 |x|^2 + 1.1 B2(x),
        B2(x) = k_mag (2 xn cm + cm^2) + k_s2 s^2 + k_s1 (s + 1),  s = xn + cm,

    xn = |x| (not below the kernel's floor 2^-50), cm = ``centre_norm_max``.
    ``check_screen_tight`` then holds

        ub^2 <= (D_own^2 + slack) (1 + 2^-19)
        lb^2 >= (D_other^2 - slack) (1 - 2^-19), floored at 0.

    ``f32`` says that the samples are fp32 (``x`` must then be the fp32
    array: its values widen exactly); else ``x`` is the stored fp64.

    Where the numbers come from.  The kernel writes, all in fp32,

        u2 = xx (1 + 2^-16) + (r1 + 0.505 B2k),  ub = sqrt(u2) (1 + 2^-21)
        l2 = xx (1 - 2^-16) + (so - 0.505 B2k),  lb = sqrt(l2) (1 - 2^-21)

    with B2k its own fp32 ``bound2_fast``, r1 the label's score and so the
    least score of the other centres.

    * The score's own error: |score - (|c|^2 - 2 x.c)| <= B = B2k / 2 (the
      screen's claim; the labels rest on it).  So r1 + 0.505 B2k <= s_own +
      1.005 B2k and so - 0.505 B2k >= s_other - 1.005 B2k: 0.5 of the 1.005
      is the score's error, 0.505 = 0.5 x 1.01 the kernel's own safety factor.
    * xx is the fp32 sum of d <= 32 squares of fl32(x): within 35 x 2^-24 <
      2^-18.9 of |x|^2.  With the kernel's 2^-16: |x|^2 (2^-16 + 2^-18.9 +
      2^-34.9) < 2^-15.8 |x|^2.  The model's 2^-15 is the doubled 2^-16; it
      leaves 2^-16.2 |x|^2 unused.
    * The fp32 evaluation: three roundings (0.505 B2k, the sum with the
      score, the fma), each at most 2^-24 of |x|^2, |score| or B2k.  |score|
      <= mag = 2 xn cm + cm^2 and B2k >= k_mag mag >= 14.4 x 2^-16 mag, so
      they sum to below 3 x 2^-24 |x|^2 + 0.0008 B2k.
    * B2k against this fp64 B2: the kernel's xn is v_sqrt (1 ulp) of xx times
      1 + (d + 8) 2^-24, at most xn (1 + 2^-18); its cm is the fp64 value
      rounded to fp32 times 1.000001f; the polynomial costs a few ulp.  B2k
      <= B2 (1 + 2^-17).
      Together: 1.005 (1 + 2^-17) + 0.0008 < 1.006 of B2; the model grants
      1.1.
    * The roots: v_sqrt within 1 ulp, the factor 1 +- 2^-21 and one rounding
      of the product: ub <= sqrt(u2) (1 + 2^-21 + 2^-22.4), so ub^2 <= u2 (1 +
      2^-19); the same downwards for lb.
    """
    x = np.asarray(x)
    assert (x.dtype == np.float32) == bool(f32), (x.dtype, f32)
    assert x.shape[1] == d
    xw = x.astype(np.float64)
    x2 = np.einsum("ij,ij->i", xw, xw)
    xn = np.maximum(np.sqrt(x2), 2.0 ** -50)
    return 2.0 ** -15 * x2 + 1.1 * bound2(xn, centre_norm_max(C), d)


def check_screen_tight(ub, lb, labels, D, slack, rows, what=""):
    """The rows ``rows`` (a boolean mask) had their bounds written by this
    call's screen.  Those it decided (finite ``ub``) must lie within
    ``screen_slack`` of the truth; and a row whose two nearest centres are
    clearly apart, D_other^2 - D_own^2 > 2 slack, must have been decided: the
    screen decides when its two best scores differ by more than B2k, the
    scores are within B2k / 2 of the truth, and 2 slack >= 2.2 B2 > 2 B2k.
    (Without this second clause a screen that left every row to the re-check,
    (+inf, 0), would be valid and vacuously tight.)"""
    n = D.shape[0]
    ub = np.asarray(ub)[:n].astype(np.float64)
    lb = np.asarray(lb)[:n].astype(np.float64)
    own, other = own_other(D, labels)
    own2 = (own * own).astype(np.float64)
    oth2 = (other * other).astype(np.float64)
    rows = np.asarray(rows, dtype=bool) & np.isfinite(own2) & \
        np.isfinite(oth2)
    decided = rows & np.isfinite(ub)
    clear = rows & (oth2 - own2 > 2.0 * slack)
    miss = clear & ~decided
    if miss.any():
        i = _worst(miss, (oth2 - own2) / slack)
        raise AssertionError(
            "%s: screened row %d (label %d) left undecided: D_own^2 %r "
            "D_other^2 %r slack %r (%d such rows)"
            % (what, i, int(labels[i]), own2[i], oth2[i], slack[i],
               int(miss.sum())))
    f = 2.0 ** -19
    ub_max = np.sqrt((own2 + slack) * (1 + f))
    lb_min = np.sqrt(np.maximum(oth2 - slack, 0.0) * (1 - f))
    _tight(ub, lb, ub_max, lb_min, decided, labels, what + ": screen")
    return int(decided.sum())


def _tight(ub, lb, ub_max, lb_min, rows, labels, what):
    with np.errstate(invalid="ignore"):
        bad_u = rows & ~(ub <= ub_max)
        bad_l = rows & ~(lb >= lb_min)
    if bad_u.any():
        with np.errstate(invalid="ignore", divide="ignore"):
            i = _worst(bad_u, np.where(np.isfinite(ub), ub / ub_max, np.inf))
        raise AssertionError(
            "%s: ub looser than the model: row %d label %d ub %r limit %r "
            "(%d rows)" % (what, i, int(labels[i]), float(ub[i]),
                           float(ub_max[i]), int(bad_u.sum())))
    if bad_l.any():
        i = _worst(bad_l, lb_min - lb)
        raise AssertionError(
            "%s: lb looser than the model: row %d label %d lb %r limit %r "
            "(%d rows)" % (what, i, int(labels[i]), float(lb[i]),
                           float(lb_min[i]), int(bad_l.sum())))


# ---------------------------------------------------------------------------
# the bounds pass
# ---------------------------------------------------------------------------
def drift_exact(C_prev, C):
    """Per-centre drift ||c - c_prev|| in fp64."""
    df = np.asarray(C, dtype=np.float64) - np.asarray(C_prev, dtype=np.float64)
    return np.sqrt(np.einsum("ij,ij->i", df, df))


def _others(delta):
    """Per centre: the largest drift of any OTHER centre (k_drift's largest,
    or its second largest for the first centre that drifted most)."""
    k = delta.shape[0]
    im = int(np.argmax(delta))           # the first index of the maximum
    d1 = delta[im]
    d2 = np.max(np.delete(delta, im)) if k > 1 else delta.dtype.type(0)
    out = np.full(k, d1, dtype=delta.dtype)
    out[im] = d2
    return out


def pass_model(ub0, lb0, labels, C_prev, C):
    """(ub_max, lb_min, ub_min, lb_max): the limits within which
    ``k_bounds_pass`` must leave the bounds ``ub0`` / ``lb0`` of rows it
    settles, in fp64.  It may not charge less than the drift (ub_new >= ub0 +
    delta_label, lb_new <= max(lb0 - delta_other, 0)), and not much more:

        ub_new <= (ub0 + delta_label (1 + 2^-20) + 2^-149) (1 + 2^-21)
        lb_new >= max(lb0 - delta_other (1 + 2^-20) - 2^-149, 0) (1 - 2^-21)

    delta: the exact drift per centre; delta_other: the largest drift, or the
    second largest for rows of the centre that drifted most.

    The kernel's factors are 2^-40 on the fp64 drift, its round-up to fp32
    (at most 2^-23 relative, or one subnormal step 2^-149: the added
    constant), the fp32 add (2^-24), the documented 1 +- 2^-22 and the
    rounding of that product (2^-24): 1 + 2^-22.9 on the drift and 1 +
    2^-21.6 on the sum.  The model doubles the 2^-22 to 2^-21 and grants the
    drift 2^-20."""
    ub0 = np.asarray(ub0).astype(np.float64)
    lb0 = np.asarray(lb0).astype(np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    delta = drift_exact(C_prev, C)
    up = delta * (1 + 2.0 ** -20) + F32_TINY
    down = _others(delta) * (1 + 2.0 ** -20) + F32_TINY
    ub_max = (ub0 + up[labels]) * (1 + 2.0 ** -21)
    lb_min = np.maximum(lb0 - down[labels], 0.0) * (1 - 2.0 ** -21)
    # the other side: every rounding of the pass goes away from the other
    # bound, so it charges at least the drift itself (this module's fp64
    # delta is within 2^-50 of the true one: 2^-45 is taken off)
    low = 1 - 2.0 ** -45
    ub_min = ub0 + delta[labels] * low
    lb_max = np.maximum(lb0 - _others(delta)[labels] * low, 0.0)
    return ub_max, lb_min, ub_min, lb_max


def check_pass_tight(ub, lb, limits, rows, labels, what=""):
    """The rows ``rows`` (mask) were settled by the bounds pass: their new
    bounds lie within ``limits`` = ``pass_model(...)``."""
    n = limits[0].shape[0]
    ub = np.asarray(ub)[:n].astype(np.float64)
    lb = np.asarray(lb)[:n].astype(np.float64)
    rows = np.asarray(rows, dtype=bool)
    _tight(ub, lb, limits[0], limits[1], rows, labels, what + ": bounds pass")
    with np.errstate(invalid="ignore"):
        bad = rows & (~(ub >= limits[2]) | ~(lb <= limits[3]))
    if bad.any():
        with np.errstate(invalid="ignore"):
            i = _worst(bad, np.fmax(limits[2] - ub, lb - limits[3]))
        raise AssertionError(
            "%s: bounds pass charged less than the drift: row %d label %d "
            "ub %r (at least %r) lb %r (at most %r) (%d rows)"
            % (what, i, int(labels[i]), float(ub[i]), float(limits[2][i]),
               float(lb[i]), float(limits[3][i]), int(bad.sum())))


def _f32_up(v):
    """fp64 -> fp32, rounded towards +inf."""
    v = np.asarray(v, dtype=np.float64)
    f = v.astype(np.float32)
    low = f.astype(np.float64) < v
    return np.where(low, np.nextafter(f, np.float32(np.inf)), f).astype(
        np.float32)


def drift_f32(C_prev, C):
    """``k_drift``'s fp32 drifts as (least, greatest) possible arrays: the
    kernel sums the squares with fma in fp64 (its root is within 2^-48 of
    this module's) and multiplies by 1 + 2^-40 before it rounds up.  The two
    arrays differ only where that 2^-48 straddles an fp32 step."""
    delta = drift_exact(C_prev, C)
    return (_f32_up(delta * (1 + 2.0 ** -40) * (1 - 2.0 ** -47)),
            _f32_up(delta * (1 + 2.0 ** -40) * (1 + 2.0 ** -47)))


def pass_f32(ub0, lb0, labels, drift):
    """``k_bounds_pass`` in numpy fp32, operation for operation:
    u = (u + drift[label]) (1 + 2^-22), l = max(l - down, 0) (1 - 2^-22),
    down = the largest drift, or the second largest for rows of the (first)
    centre that drifted most; a drift that is not finite makes every u
    +inf.  Returns (u, l, active = !(u < l))."""
    f = np.float32
    ub0 = np.asarray(ub0, dtype=f)
    lb0 = np.asarray(lb0, dtype=f)
    labels = np.asarray(labels, dtype=np.int64)
    drift = np.asarray(drift, dtype=f)
    with np.errstate(invalid="ignore", over="ignore"):
        u = ((ub0 + drift[labels]).astype(f) * f(1.0 + 2.0 ** -22)).astype(f)
        if not np.all(drift < np.inf):
            u = np.full_like(u, np.inf)
        low = (lb0 - _others(drift)[labels]).astype(f)
        l = (np.fmax(low, f(0)) * f(1.0 - 2.0 ** -22)).astype(f)
        active = ~(u < l)
    return u, l, active
