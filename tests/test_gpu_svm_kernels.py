"""GPU tests of the CascadeSVM entries of the C ABI (dkm_svm.hip), called one
by one, entry by entry against a longdouble restatement with running error
bounds.

``dkm_svm_rows_*``: node sizes m around the 16-row MFMA tile and the 64-row
block (1, 2, 15, 16, 17, 63, 64, 65, 257), feature counts d around the 4-wide
MFMA step and the 16-feature staging chunk (1, 3, 4, 5, 16, 17, 64, 65, 129),
``ldx = d + 3`` with NaN padding, fp32 rows, ``rows[]`` shuffled and sparse
inside an X whose other rows are NaN (a read of one would show in K), working
sets with q > m, q = m and q < m.  The bound is ``(d + 8) u`` per dot product
(u = 2^-53; the MFMA's sum of d products, and the norms' fma chains), carried
through ``exp``'s condition number for rbf.

``dkm_svm_select``: the rule restated in numpy, with ties, blocks of more
than one trip per thread, q >= m.  ``dkm_svm_update``: the fma chain.
``dkm_svm_decision_*`` / ``dkm_svm_w``: nq in {1, 17, 130} against n_SV in
{1, 16, 33} and one n_SV past a 128-row batch.

The solver (select, rows, local, update driven by
``dislib_amd.classification.csvm.solve_node``) is checked from the returned
alpha alone, with tolerances that follow from the stopping rule ``m(alpha) -
M(alpha) < 1e-3``: ``0 <= alpha <= C`` exactly; ``|sum y alpha| <= m C u``
(a step moves two entries by the same amount, each rounded once at a
magnitude below C); the gap recomputed in longdouble ``<= 1e-3`` plus the
gradient's running error bound; the dual objective at most
``f* + 1e-3 C m / 2`` with f* sklearn's at ``tol=1e-10`` (a feasible point
with gap eps is within eps times the sum of the positive slacks of the
optimum, by convexity).  Duplicate rows with opposite labels and an all-bound
solution terminate.  Two runs give identical bytes.
"""
import ctypes

import numpy as np
import pytest

from dislib_amd import _lib

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
GAMMA = 0.07
MS = [1, 2, 15, 16, 17, 63, 64, 65, 257]
DS = [1, 3, 4, 5, 16, 17, 64, 65, 129]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _so():
    return _lib.lib()


def _problem(m, d, dtype, seed):
    """(X buffer on the device with ldx = d + 3 and NaN everywhere a kernel
    must not read, the node's rows, the node's samples as fp64)."""
    rng = np.random.default_rng(seed)
    n = 3 * m + 5
    rows = rng.permutation(n)[:m].astype(np.int32)
    buf = np.full((n, d + 3), np.nan, dtype=dtype)
    xs = rng.standard_normal((m, d)).astype(dtype)
    buf[rows, :d] = xs
    return _dev(buf), rows, xs.astype(np.float64)


def _norms(X, d, dtype):
    so = _so()
    out = torch.empty(X.shape[0], dtype=torch.float64, device="cuda")
    fn = so.dkm_svm_norms_f32 if dtype == np.float32 else so.dkm_svm_norms_f64
    _lib.check(fn(_p(X), X.shape[0], d, X.stride(0), _p(out), _stream()),
               "norms")
    return out


def _kernel_ref(a, b, d, rbf, gamma=GAMMA):
    """(K in longdouble, its error bound) for fp64 rows a, b."""
    al, bl = a.astype(LD), b.astype(LD)
    dot = al @ bl.T
    mag = np.abs(al) @ np.abs(bl).T
    e_dot = (d + 8) * U * mag
    if not rbf:
        return dot, e_dot + 2 * U * np.abs(dot)
    an, bn = (al * al).sum(1), (bl * bl).sum(1)
    d2 = an[:, None] + bn[None, :] - 2 * dot
    z = -LD(gamma) * d2
    e_z = abs(gamma) * ((d + 8) * U * (an[:, None] + bn[None, :]) +
                        2 * e_dot + 4 * U * (an[:, None] + bn[None, :] +
                                             2 * np.abs(dot))) + \
        2 * U * np.abs(z)
    k = np.exp(z)
    return k, k * (np.expm1(e_z) + 4 * U)


def _rows(X, d, dtype, rows, ws, q, norms, rbf, gamma=GAMMA):
    so = _so()
    m = len(rows)
    K = torch.full((q, m + 2), 7.0, dtype=torch.float64, device="cuda")
    fn = so.dkm_svm_rows_f32 if dtype == np.float32 else so.dkm_svm_rows_f64
    rows_d, ws_d = _dev(rows), _dev(ws)     # named: alive during the call
    _lib.check(fn(_p(X), X.shape[0], d, X.stride(0), _p(rows_d), m,
                  _p(ws_d), q, _p(norms),
                  _lib.SVM_RBF if rbf else _lib.SVM_LINEAR, gamma, _p(K),
                  m + 2, _stream()), "rows")
    return K.cpu().numpy()


def _check_rows(m, d, dtype, seed):
    X, rows, xs = _problem(m, d, dtype, seed)
    norms = _norms(X, d, dtype)
    rng = np.random.default_rng(seed + 1)
    sets = []
    if m + 3 <= _lib.SVM_QMAX:                       # q > m
        sets.append(np.concatenate([np.arange(m), [-1, -1, -1]]))
    if m <= _lib.SVM_QMAX:                           # q = m
        sets.append(rng.permutation(m))
    if m > 16:                                       # q < m
        q = 16 if m <= 128 else _lib.SVM_QMAX
        sets.append(rng.permutation(m)[:q])
    for ws in sets:
        ws = ws.astype(np.int32)
        q = len(ws)
        ok = ws >= 0
        for rbf in (False, True):
            K = _rows(X, d, dtype, rows, ws, q, norms, rbf)
            assert np.all(K[:, m:] == 7.0)           # ldk is honoured
            ref, bound = _kernel_ref(xs[ws[ok]], xs, d, rbf)
            err = np.abs(K[ok, :m].astype(LD) - ref)
            assert np.all(err <= bound), (m, d, q, rbf, float(err.max()))


@pytest.mark.parametrize("dtype", [np.float64, np.float32],
                         ids=["f64", "f32"])
@pytest.mark.parametrize("m", MS)
def test_rows_every_node_size(m, dtype):
    _check_rows(m, DS[MS.index(m)], dtype, 100 + m)


@pytest.mark.parametrize("dtype", [np.float64, np.float32],
                         ids=["f64", "f32"])
@pytest.mark.parametrize("d", DS)
def test_rows_every_feature_count(d, dtype):
    _check_rows(65, d, dtype, 200 + d)


def test_rows_are_symmetric_and_repeatable():
    X, rows, xs = _problem(65, 17, np.float64, 5)
    norms = _norms(X, 17, np.float64)
    ws = np.arange(65, dtype=np.int32)
    a = _rows(X, 17, np.float64, rows, ws, 65, norms, True)
    b = _rows(X, 17, np.float64, rows, ws, 65, norms, True)
    assert a.tobytes() == b.tobytes()
    assert np.array_equal(a[:, :65], a[:, :65].T)


# ---------------------------------------------------------------------------
def _select_ref(f, alpha, y, c, q):
    m = len(f)
    up = ((y > 0) & (alpha < c)) | ((y < 0) & (alpha > 0))
    low = ((y > 0) & (alpha > 0)) | ((y < 0) & (alpha < c))
    gap = (np.max(-f[up]) - np.min(-f[low])) if up.any() and low.any() \
        else -np.inf
    if q >= m:
        return np.concatenate([np.arange(m), -np.ones(q - m)]), gap
    taken = np.zeros(m, dtype=bool)
    ws = -np.ones(q)
    for r in range(q // 2):
        for s, (mask, key) in enumerate(((up, -f), (low, f))):
            cand = np.flatnonzero(mask & ~taken)
            if len(cand):
                best = cand[np.argmax(key[cand])]    # first of the ties
                taken[best] = True
                ws[s * (q // 2) + r] = best
    return ws, gap


@pytest.mark.parametrize("m,q", [(2, 2), (5, 8), (17, 16), (257, 128),
                                 (2500, 128), (40, 15), (6, 4)])
def test_select(m, q):
    so = _so()
    rng = np.random.default_rng(m * 7 + q)
    c = 2.0
    y = rng.choice([-1.0, 1.0], m)
    alpha = rng.choice([0.0, c, 0.5, 1.25], m)
    f = np.round(rng.standard_normal(m), 1)          # many ties
    if m == 6:                                       # I_up runs out
        y[:] = 1.0
        alpha[:] = [c, c, c, c, 0.5, c]
    ws = torch.full((q + 1,), 99, dtype=torch.int32, device="cuda")
    gap = torch.empty(3, dtype=torch.float64, device="cuda")
    mark = torch.empty(m, dtype=torch.int32, device="cuda")
    fd, ad, yd = _dev(f), _dev(alpha), _dev(y)
    _lib.check(so.dkm_svm_select(_p(fd), _p(ad), _p(yd), m, c, q, _p(ws),
                                 _p(gap), _p(mark), _stream()), "select")
    ref_ws, ref_gap = _select_ref(f, alpha, y, c, q)
    got = ws.cpu().numpy()
    assert got[q] == 99
    assert np.array_equal(got[:q], ref_ws.astype(np.int32))
    g = gap.cpu().numpy()
    assert g[0] == ref_gap and (not np.isfinite(ref_gap) or
                                g[0] == g[1] - g[2])


@pytest.mark.parametrize("m", [1, 255, 256, 257, 700])
def test_update(m):
    so = _so()
    rng = np.random.default_rng(m)
    q = 37
    K = rng.standard_normal((q, m + 3))
    dy = rng.standard_normal(q)
    dy[::3] = 0.0
    f = rng.standard_normal(m + 1)
    fd, Kd, dyd = _dev(f), _dev(K), _dev(dy)
    _lib.check(so.dkm_svm_update(_p(Kd), m + 3, q, _p(dyd), _p(fd), m,
                                 _stream()), "update")
    got = fd.cpu().numpy()
    assert got[m] == f[m]
    ref = f[:m].astype(LD) + dy.astype(LD) @ K[:, :m].astype(LD)
    mag = np.abs(f[:m]) + np.abs(dy) @ np.abs(K[:, :m])
    assert np.all(np.abs(got[:m] - ref) <= (q + 2) * U * mag)


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("x32", [False, True], ids=["x64", "x32"])
@pytest.mark.parametrize("ns", [1, 16, 33, 300])
def test_decision(ns, x32):
    so = _so()
    d = 17
    xt = np.float32 if x32 else np.float64
    X, sv, xs = _problem(ns, d, xt, 300 + ns)
    xnorm = _norms(X, d, xt)
    rng = np.random.default_rng(ns)
    coef = rng.standard_normal(ns)
    b = 0.375
    sv_d, coef_d = _dev(sv), _dev(coef)
    for nq, q32 in ((1, False), (17, True), (130, False)):
        qt = np.float32 if q32 else np.float64
        qbuf = np.full((nq, d + 3), np.nan, dtype=qt)
        qs = rng.standard_normal((nq, d)).astype(qt)
        qbuf[:, :d] = qs
        Q = _dev(qbuf)
        qnorm = _norms(Q, d, qt)
        fn = so.dkm_svm_decision_f32 if q32 else so.dkm_svm_decision_f64
        for rbf in (False, True):
            outs = []
            for _ in range(2):
                out = torch.full((nq + 1,), 7.0, dtype=torch.float64,
                                 device="cuda")
                _lib.check(fn(_p(Q), nq, d, d + 3, _p(X), int(x32),
                              X.shape[0], X.stride(0), _p(sv_d), ns,
                              _p(coef_d), b, _p(qnorm), _p(xnorm),
                              int(rbf), GAMMA, _p(out), _stream()),
                           "decision")
                outs.append(out.cpu().numpy())
            assert outs[0].tobytes() == outs[1].tobytes()
            assert outs[0][nq] == 7.0
            k, kb = _kernel_ref(qs.astype(np.float64), xs, d, rbf)
            ref = k @ coef.astype(LD) + b
            mag = np.abs(k) @ np.abs(coef)
            bound = kb @ np.abs(coef) + (ns + 3) * U * (mag + abs(b))
            err = np.abs(outs[0][:nq] - ref)
            assert np.all(err <= bound), (ns, nq, rbf, float(err.max()))


@pytest.mark.parametrize("ns,rbf", [(1, True), (33, False), (33, True),
                                    (300, True)])
def test_w(ns, rbf):
    so = _so()
    d = 5
    X, sv, xs = _problem(ns, d, np.float64, 400 + ns)
    xnorm = _norms(X, d, np.float64)
    rng = np.random.default_rng(ns)
    coef = rng.standard_normal(ns)
    lab = rng.choice([-1.0, 1.0, 2.0], ns)
    sv_d, coef_d, lab_d = _dev(sv), _dev(coef), _dev(lab)
    ws = []
    for _ in range(2):
        tmp = torch.empty(ns, dtype=torch.float64, device="cuda")
        w = torch.empty(1, dtype=torch.float64, device="cuda")
        _lib.check(so.dkm_svm_w(_p(X), 0, X.shape[0], d, X.stride(0),
                                _p(sv_d), ns, _p(coef_d),
                                _p(lab_d), _p(xnorm), int(rbf), GAMMA,
                                _p(tmp), _p(w), _stream()), "w")
        ws.append(w.cpu().numpy())
    assert ws[0].tobytes() == ws[1].tobytes()
    k, kb = _kernel_ref(xs, xs, d, rbf, gamma=-GAMMA)
    cl = (coef * lab).astype(LD)
    ref = -0.5 * (cl @ k @ cl) + coef.astype(LD).sum()
    mag = 0.5 * (np.abs(cl) @ np.abs(k) @ np.abs(cl)) + np.abs(coef).sum()
    bound = 0.5 * (np.abs(cl) @ kb @ np.abs(cl)) + (2 * ns + 16) * U * mag
    assert abs(ws[0][0] - ref) <= bound


# ---------------------------------------------------------------------------
def _solve(x, y, c, rbf, q=None, dtype=np.float64):
    from dislib_amd.classification import csvm
    so = _so()
    X = _dev(x.astype(dtype))
    rows = _dev(np.arange(len(y), dtype=np.int32))
    xnorm = csvm.norms(so, X, dtype == np.float32) if rbf else None
    stats = {}
    alpha, f = csvm.solve_node(so, X, dtype == np.float32, rows, _dev(y),
                               xnorm, int(rbf), GAMMA, c, q=q, stats=stats)
    return alpha.cpu().numpy(), f.cpu().numpy(), stats


def _contract(x, y, c, rbf, alpha):
    m = len(y)
    assert np.all(alpha >= 0.0) and np.all(alpha <= c)
    assert abs(np.sum((y * alpha).astype(LD))) <= m * c * U
    k, kb = _kernel_ref(x, x, x.shape[1], rbf)
    ya = (y * alpha).astype(LD)
    f = k @ ya - y
    ferr = kb @ np.abs(ya)
    up = ((y > 0) & (alpha < c)) | ((y < 0) & (alpha > 0))
    low = ((y > 0) & (alpha > 0)) | ((y < 0) & (alpha < c))
    if up.any() and low.any():
        gap = np.max(-f[up]) - np.min(-f[low])
        assert gap <= 1e-3 + 2 * ferr.max(), float(gap)
    return float(0.5 * (ya @ k @ ya) - alpha.astype(LD).sum())


@pytest.mark.parametrize("rbf", [False, True], ids=["linear", "rbf"])
@pytest.mark.parametrize("m,q", [(60, None), (61, None), (200, None),
                                 (200, 16)])
def test_solver_contract(m, q, rbf):
    from sklearn.svm import SVC
    rng = np.random.default_rng(m)
    x = rng.standard_normal((m, 5))
    y = np.where(x[:, 0] + 0.5 * rng.standard_normal(m) > 0, 1.0, -1.0)
    c = 1.5
    alpha, f, stats = _solve(x, y, c, rbf, q)
    obj = _contract(x, y, c, rbf, alpha)
    ref = SVC(C=c, kernel="rbf" if rbf else "linear", gamma=GAMMA,
              tol=1e-10).fit(x, y)
    star = np.zeros(m)
    star[ref.support_] = np.abs(ref.dual_coef_[0])
    k, _ = _kernel_ref(x, x, 5, rbf)
    ys = (y * star).astype(LD)
    fstar = float(0.5 * (ys @ k @ ys) - star.astype(LD).sum())
    assert obj <= fstar + 1e-3 * c * m / 2
    again, f2, _ = _solve(x, y, c, rbf, q)
    assert alpha.tobytes() == again.tobytes() and f.tobytes() == f2.tobytes()


def test_duplicate_rows_with_opposite_labels_terminate():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((20, 3))
    x = np.concatenate([x, x[:6]])
    y = np.concatenate([np.where(x[:20, 0] > 0, 1.0, -1.0),
                        -np.where(x[:6, 0] > 0, 1.0, -1.0)])
    for rbf in (False, True):
        alpha, _, stats = _solve(x, y, 1.0, rbf)
        _contract(x, y, 1.0, rbf, alpha)
        # of two copies with opposite labels at least one ends at C
        assert np.all(np.maximum(alpha[20:], alpha[:6]) == 1.0)


def test_all_bound_solution_terminates():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((40, 4))
    y = np.where(np.arange(40) % 2 == 0, 1.0, -1.0)
    c = 1e-6
    alpha, _, _ = _solve(x, y, c, False)
    _contract(x, y, c, False, alpha)
    assert np.all(alpha == c)
