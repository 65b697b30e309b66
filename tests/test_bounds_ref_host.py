"""The host reference of the per-row bounds checks itself (no GPU):
``tests/bounds_ref.py`` must accept bounds that follow the kernels' documented
formulas and reject bounds that are wrong by one fp32 ulp, or vacuous, before
``tests/test_gpu_bounds_exact.py`` holds the device's arrays against it."""
import numpy as np
import pytest

from tests import bounds_ref as br

F = np.float32
LD = np.longdouble


def _down(v):
    """long double -> fp32, rounded towards -inf."""
    f = np.asarray(v, dtype=LD).astype(F)
    high = f.astype(LD) > v
    return np.where(high, np.nextafter(f, F(-np.inf)), f).astype(F)


def _up(v):
    f = np.asarray(v, dtype=LD).astype(F)
    low = f.astype(LD) < v
    return np.where(low, np.nextafter(f, F(np.inf)), f).astype(F)


def _case(n, d, k, seed, spread=8.0):
    rng = np.random.RandomState(seed)
    C = rng.uniform(-spread, spread, (k, d))
    lab = rng.randint(0, k, n)
    x = C[lab] + rng.standard_normal((n, d))
    return x, C


def test_exact_distances_against_a_float128_loop():
    x, C = _case(7, 4, 3, 0)
    x[2] = C[1]                       # a row equal to a centre
    x[5] *= 1e-3
    D = br.exact_distances(x, C, chunk=3)
    assert D.dtype == LD and D.shape == (7, 3)
    for i in range(7):
        for j in range(3):
            a = LD(0)
            for t in range(4):
                df = LD(x[i, t]) - LD(C[j, t])
                a += df * df
            assert D[i, j] == np.sqrt(a), (i, j)
    assert D[2, 1] == 0
    # fp32 samples are used as stored, widened
    x32 = x.astype(F)
    assert np.array_equal(br.exact_distances(x32, C),
                          br.exact_distances(x32.astype(np.float64), C))
    # non-finite rows give inf / nan and nothing else changes
    xb = x.copy()
    xb[0, 1] = np.inf
    xb[3, 0] = np.nan
    Db = br.exact_distances(xb, C)
    assert np.all(np.isinf(Db[0])) and np.all(np.isnan(Db[3]))
    keep = [1, 2, 4, 5, 6]
    assert np.array_equal(Db[keep], D[keep])


def _truth(n=300, d=8, k=9, seed=1):
    x, C = _case(n, d, k, seed)
    D = br.exact_distances(x, C)
    lab = np.argmin(D, axis=1)
    own, other = br.own_other(D, lab)
    return x, C, D, lab, _up(own), _down(other)


def test_check_valid_accepts_the_truth():
    x, C, D, lab, ub, lb = _truth()
    br.check_valid(ub, lb, lab, D)
    br.check_valid(np.full_like(ub, np.inf), np.zeros_like(lb), lab, D)
    # a row equal to its centre: ub = 0 is valid
    x[4] = C[lab[4]]
    D = br.exact_distances(x, C)
    ub[4] = 0
    br.check_valid(ub, lb, lab, D)
    # k = 1: nothing to check, whatever the arrays hold
    br.check_valid(ub * 0 - 1, lb * np.nan, lab * 0, D[:, :1])
    # a non-finite row is left out
    xb = x.copy()
    xb[7, 0] = np.nan
    ub[7], lb[7] = np.nan, -1
    br.check_valid(ub, lb, lab, br.exact_distances(xb, C))


@pytest.mark.parametrize("kind", ["ub", "lb", "nan_ub", "nan_lb", "neg"])
def test_check_valid_rejects_one_ulp(kind):
    x, C, D, lab, ub, lb = _truth()
    row = 123
    if kind == "ub":
        ub[row] = np.nextafter(ub[row], F(-np.inf))
    elif kind == "lb":
        lb[row] = np.nextafter(lb[row], F(np.inf))
    elif kind == "nan_ub":
        ub[row] = np.nan
    elif kind == "nan_lb":
        lb[row] = np.nan
    else:
        lb[row] = -F(2.0) ** -149
    with pytest.raises(AssertionError, match="row %d label %d" %
                       (row, lab[row])):
        br.check_valid(ub, lb, lab, D, kind)


# ---------------------------------------------------------------------------
# the screen's bounds, by the documented formulas in numpy fp32
# ---------------------------------------------------------------------------
def _bound2_f32(xx, cm, d):
    """bound_consts<bf16x3> and bound2_fast, operation for operation in fp32
    (np.sqrt for v_sqrt_f32: the 4 ulp the kernel allows cover either)."""
    rel = F(3.1) * F(2.0 ** -16) + (F(3.0) * F(d) + F(6.0)) * F(2.0 ** -23)
    k_mag = F(2.0) * (F(2.0) * rel + F(2.0 ** -16)) * F(1.0001)
    k_s2 = F(2.0) * F(16.0) * F(2.0 ** -52) * F(1.0001)
    k_s1 = F(2.0) * (F(8.0) * F(d)) * F(2.0 ** -120) * F(1.0001)
    xn = np.sqrt(np.clip(xx, F(2.0 ** -100), None)) * \
        (F(1.0) + F(d + 8) * F(2.0 ** -24))
    s = xn + cm
    mag = xn * (F(2.0) * cm) + cm * cm
    b = k_mag * mag
    b = (k_s2 * s) * s + b
    return (k_s1 * (s + F(1.0)) + b).astype(F)


def _screen_f32(x, C, lab, rng):
    """(ub, lb, decided) as the BND block of k_screen_w32 computes them from
    scores that are off by up to +-B."""
    n, d = x.shape
    xf = x.astype(F)
    xx = np.zeros(n, F)
    for t in range(d):
        xx = xf[:, t] * xf[:, t] + xx
    cn = np.sqrt(np.max(np.einsum("ij,ij->i", C, C)))
    cm = F(cn) * F(1.000001)
    B2 = _bound2_f32(xx, cm, d)
    s = np.einsum("ij,ij->i", C, C)[None, :] - 2.0 * x @ C.T
    s = s + rng.uniform(-0.499, 0.499, s.shape) * B2[:, None]
    s = s.astype(F)
    idx = np.arange(n)
    r1 = s[idx, lab]
    so = s.copy()
    so[idx, lab] = np.inf
    so = so.min(axis=1)
    Bs = F(0.505) * B2
    u2 = (xx.astype(np.float64) * (1 + 2.0 ** -16) + (r1 + Bs)).astype(F)
    l2 = (xx.astype(np.float64) * (1 - 2.0 ** -16) + (so - Bs)).astype(F)
    ub = np.sqrt(np.maximum(u2, F(0))) * F(1 + 2.0 ** -21)
    lb = np.sqrt(np.maximum(l2, F(0))) * F(1 - 2.0 ** -21)
    decided = (so - r1 > B2) & (r1 <= so)
    ub = np.where(decided, ub, F(np.inf)).astype(F)
    lb = np.where(decided, lb, F(0)).astype(F)
    return ub, lb, decided


@pytest.mark.parametrize("f32", [False, True])
def test_screen_slack_accepts_the_documented_formulas(f32):
    n, d, k = 1000, 32, 20
    x, C = _case(n, d, k, 2, spread=10.0)
    if f32:
        x = x.astype(F)
    rng = np.random.RandomState(5)
    D = br.exact_distances(x, C)
    lab = np.argmin(D, axis=1)
    ub, lb, decided = _screen_f32(x.astype(np.float64), C, lab, rng)
    assert decided.sum() > 0.9 * n
    br.check_valid(ub, lb, lab, D)
    slack = br.screen_slack(x, C, d, f32)
    rows = np.ones(n, bool)
    assert br.check_screen_tight(ub, lb, lab, D, slack, rows) == decided.sum()
    # vacuous: a clearly separated row left undecided
    own, other = br.own_other(D, lab)
    gap = (other * other - own * own).astype(np.float64)
    i = int(np.argmax(gap / slack))
    assert gap[i] > 2 * slack[i] and decided[i]
    u2, l2 = ub.copy(), lb.copy()
    u2[i] = np.inf
    with pytest.raises(AssertionError, match="row %d " % i):
        br.check_screen_tight(u2, lb, lab, D, slack, rows)
    # ... unless the screen did not write it
    rows[i] = False
    br.check_screen_tight(u2, lb, lab, D, slack, rows)
    rows[i] = True
    # vacuous: lb = 0 on a decided row; ub far too large
    l2[i] = 0
    with pytest.raises(AssertionError, match="lb looser.*row %d " % i):
        br.check_screen_tight(ub, l2, lab, D, slack, rows)
    u2 = ub.copy()
    u2[i] = F(np.sqrt(float(own[i]) ** 2 + 4 * slack[i]))
    with pytest.raises(AssertionError, match="ub looser.*row %d " % i):
        br.check_screen_tight(u2, lb, lab, D, slack, rows)
    # the wrong dtype for the claimed storage is refused
    with pytest.raises(AssertionError):
        br.screen_slack(x, C, d, not f32)


def test_bound2_matches_the_fp32_evaluation():
    """The fp64 B2 of the model against the kernel's fp32 arithmetic: the
    docstring of screen_slack grants 1 + 2^-17."""
    rng = np.random.RandomState(3)
    for d in (1, 8, 17, 32):
        xx = (rng.uniform(0, 40, 200) ** 2).astype(F)
        cn = rng.uniform(0.1, 60)
        b32 = _bound2_f32(xx, F(cn) * F(1.000001), d).astype(np.float64)
        xn = np.sqrt(xx.astype(np.float64))
        b64 = br.bound2(np.maximum(xn, 2.0 ** -50), cn * 1.000001, d)
        assert np.all(b32 <= b64 * (1 + 2.0 ** -17))
        assert np.all(b32 >= b64 * (1 - 2.0 ** -17))


# ---------------------------------------------------------------------------
# the bounds pass
# ---------------------------------------------------------------------------
def _pass_case(seed=7, n=1000, k=12, d=5):
    rng = np.random.RandomState(seed)
    Cp = rng.uniform(-5, 5, (k, d))
    C = Cp + rng.standard_normal((k, d)) * rng.uniform(0, 0.3, (k, 1))
    C[4] = Cp[4]                                  # one centre at rest
    lab = rng.randint(0, k, n)
    ub0 = rng.uniform(0, 3, n).astype(F)
    lb0 = rng.uniform(0, 6, n).astype(F)
    ub0[:5] = np.inf                              # re-check rows: (+inf, 0)
    lb0[:5] = 0
    return Cp, C, lab, ub0, lb0


def test_pass_model_accepts_the_documented_formulas():
    Cp, C, lab, ub0, lb0 = _pass_case()
    lo, hi = br.drift_f32(Cp, C)
    delta = br.drift_exact(Cp, C)
    assert np.all(lo.astype(np.float64) >= delta) and np.all(hi >= lo)
    assert lo[4] == 0 and hi[4] == 0
    lim = br.pass_model(ub0, lb0, lab, Cp, C)
    rows = np.ones(lab.shape[0], bool)
    for dr in (lo, hi):
        u, l, act = br.pass_f32(ub0, lb0, lab, dr)
        assert act[:5].all() and 0 < act.sum() < act.size
        br.check_pass_tight(u, l, lim, rows, lab)
        assert np.all(u[5:] >= ub0[5:]) and np.all(l <= lb0)
    # the centre that drifted most is charged the second largest drift
    im = int(np.argmax(delta))
    second = np.sort(delta)[-2]
    r = np.flatnonzero((lab == im) & (lb0 > 1))[0]
    assert abs((lb0[r] - l[r]) - second) < 1e-5 * second + 1e-6
    r = np.flatnonzero((lab != im) & (lb0 > 1))[0]
    assert abs((lb0[r] - l[r]) - delta[im]) < 1e-5 * delta[im] + 1e-6
    # no drift: only the 2^-22 factors
    u, l, _ = br.pass_f32(ub0, lb0, lab, np.zeros_like(lo))
    br.check_pass_tight(u, l, br.pass_model(ub0, lb0, lab, C, C), rows, lab)


def test_pass_model_rejects_loose_and_vacuous_bounds():
    Cp, C, lab, ub0, lb0 = _pass_case()
    lim = br.pass_model(ub0, lb0, lab, Cp, C)
    u, l, _ = br.pass_f32(ub0, lb0, lab, br.drift_f32(Cp, C)[1])
    rows = np.ones(lab.shape[0], bool)
    delta = br.drift_exact(Cp, C)
    im = int(np.argmax(delta))
    # a row of the centre that drifted most, charged the largest drift
    r = int(np.flatnonzero((lab == im) & (lb0 > 2))[0])
    bad = l.copy()
    bad[r] = F((lb0[r] - F(delta[im])) * F(1 - 2.0 ** -22))
    with pytest.raises(AssertionError, match="lb looser.*row %d " % r):
        br.check_pass_tight(u, bad, lim, rows, lab)
    # a row charged the largest drift instead of its own centre's
    r = int(np.flatnonzero(lab == 4)[0])
    bad = u.copy()
    bad[r] = F(ub0[r] + delta[im])
    with pytest.raises(AssertionError, match="ub looser.*row %d " % r):
        br.check_pass_tight(bad, l, lim, rows, lab)
    # charged less than the drift: the drift rounded down, the own add lost
    r = int(np.flatnonzero((lab == 2) & np.isfinite(ub0))[0])
    bad = u.copy()
    bad[r] = ub0[r]
    with pytest.raises(AssertionError, match="less than the drift: row %d "
                       % r):
        br.check_pass_tight(bad, l, lim, rows, lab)
    r = int(np.flatnonzero((lab == 2) & (lb0 > 2))[0])
    bad = l.copy()
    bad[r] = np.nextafter(F(lb0[r] - F(br._others(delta)[2])), F(np.inf))
    with pytest.raises(AssertionError, match="less than the drift: row %d "
                       % r):
        br.check_pass_tight(u, bad, lim, rows, lab)
    # vacuous
    r = int(np.flatnonzero(lim[1] > 0)[0])
    bad = l.copy()
    bad[r] = 0
    with pytest.raises(AssertionError, match="lb looser.*row %d " % r):
        br.check_pass_tight(u, bad, lim, rows, lab)
    bad = u.copy()
    bad[r] = np.inf
    with pytest.raises(AssertionError, match="ub looser.*row %d " % r):
        br.check_pass_tight(bad, l, lim, rows, lab)
    rows[r] = False                     # not a row of the pass: not held
    br.check_pass_tight(bad, l, lim, rows, lab)


def test_pass_f32_non_finite_drift_makes_every_row_active():
    Cp, C, lab, ub0, lb0 = _pass_case()
    dr = br.drift_f32(Cp, C)[0]
    dr[3] = np.inf
    u, l, act = br.pass_f32(ub0, lb0, lab, dr)
    assert np.all(np.isinf(u)) and act.all() and np.all(l >= 0)
