"""CPU tests of ALS: the numpy statement of its semantics (tests/als_ref.py)
against the reference's own output (tests/golden/als_ref.npz), the measured
tolerances, ``Dataset.transpose`` and the estimator's host-side surface."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import als_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "als_ref.npz"))
CASES = sorted({k.split("__")[0] for k in G.files})


def _inputs(name):
    sub, n_f, lam, tol, max_iter, check, seed = G[name + "__meta"]
    stored = np.nonzero(G[name + "__r_stored"])
    r = sp.csr_matrix((G[name + "__r"][stored], stored),
                      shape=G[name + "__r"].shape)
    test = sp.csr_matrix(G[name + "__test"]) \
        if name + "__test" in G.files else None
    return r, int(sub), test, (int(n_f), float(lam), float(tol),
                               int(max_iter), bool(check), int(seed))


@pytest.fixture(scope="module")
def ref_results():
    """als_ref of every golden case, computed once."""
    out = {}
    for name in CASES:
        r, sub, test, args = _inputs(name)
        out[name] = ref.als_ref(r, -(-r.shape[0] // sub), *args, test=test)
    return out


def test_golden_has_every_case():
    assert CASES == ["doc", "holes_f8_s4", "m_f100_s1", "m_f32_s4",
                     "m_f32_s4_maxiter", "m_f32_s4_test", "m_f8_s1",
                     "m_f8_s1_test", "m_f8_s4", "m_f8_s4_long",
                     "m_f8_s4_noconv"]
    r = _inputs("holes_f8_s4")[0]
    assert (r.data == 0).sum() == 2                       # stored zeros
    assert (np.diff(r.indptr) == 0).any()                 # an empty item
    assert (np.bincount(r.indices, minlength=40) == 0).any()   # ... user
    assert not bool(G["m_f32_s4_maxiter__converged"])
    assert int(G["m_f32_s4_maxiter__n_iter"]) == 4
    assert int(G["m_f8_s4_noconv__n_iter"]) == 3
    assert len(G["m_f8_s4_noconv__rmses"]) == 0


@pytest.mark.parametrize("name", CASES)
def test_ref_stops_where_the_reference_stops(name, ref_results):
    res = ref_results[name]
    assert res.n_iter == int(G[name + "__n_iter"])
    assert res.converged == bool(G[name + "__converged"])
    assert res.users.dtype == np.float32 == res.items.dtype
    assert len(res.rmses) == len(G[name + "__rmses"])


def test_measured_gaps_and_tolerances(ref_results):
    """The largest gaps to the reference are what tests/als_ref.py records
    (rounded up, by less than 5 %), and the tolerances are 4 times those."""
    factor_gap = rmse_gap = 0.0
    for name in CASES:
        res = ref_results[name]
        for got, key in ((res.users, "__users"), (res.items, "__items")):
            want = G[name + key]
            factor_gap = max(factor_gap,
                             np.abs(got - want).max() / np.abs(want).max())
        if len(res.rmses):
            rmse_gap = max(rmse_gap, np.abs(np.array(res.rmses) -
                                            G[name + "__rmses"]).max())
    print("factor gap %.4g rmse gap %.4g" % (factor_gap, rmse_gap))
    assert 0.95 * ref.MEASURED_FACTOR_GAP < factor_gap <= \
        ref.MEASURED_FACTOR_GAP
    assert 0.95 * ref.MEASURED_RMSE_GAP < rmse_gap <= ref.MEASURED_RMSE_GAP
    assert ref.T_FACTORS == 4 * ref.MEASURED_FACTOR_GAP
    assert ref.T_RMSE == 4 * ref.MEASURED_RMSE_GAP
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for v in (ref.MEASURED_FACTOR_GAP, ref.MEASURED_RMSE_GAP, ref.T_FACTORS,
              ref.T_RMSE):
        assert "%.3g" % v in design, v


def test_docstring_case_predictions(ref_results):
    res = ref_results["doc"]
    p = ref.predict_user(res.users, res.items, 0)
    assert 2.75 < p[0] < 3.25 and p[1] < 1 and p[2] > 4.5
    assert np.allclose(p, [3.10, 0.54, 4.78], atol=0.01)


@pytest.mark.parametrize("name", ["doc", "m_f8_s4", "holes_f8_s4"])
def test_dataset_transpose_equals_the_reference(name):
    from dislib_amd.data import load_data
    r, sub, _, _ = _inputs(name)
    ds = load_data(x=r, subset_size=sub)
    dt = ds.transpose()
    assert len(dt) == len(ds) and dt.sparse
    assert dt.n_features == r.shape[0]
    for i, s in enumerate(dt):
        want = G["%s__t%d" % (name, i)]
        assert s.samples.shape == want.shape
        assert np.array_equal(s.samples.toarray(), want)
    assert "%s__t%d" % (name, len(dt)) not in G.files
    bounds = ref.transpose_bounds(r.shape[1], len(ds))
    assert [s.samples.shape[0] for s in dt] == [b - a for a, b in bounds]


def test_dataset_transpose_n_subsets_and_dense():
    from dislib_amd.data import load_data
    x = np.arange(35.0).reshape(5, 7)
    dt = load_data(x, subset_size=2).transpose(n_subsets=3)
    assert [s.samples.shape for s in dt] == [(2, 5), (2, 5), (3, 5)]
    assert np.array_equal(np.vstack([s.samples for s in dt]), x.T)
    assert dt.n_features == 5 and not dt.sparse
    dt = load_data(sp.csr_matrix(x), subset_size=5).transpose()
    assert len(dt) == 1 and np.array_equal(dt[0].samples.toarray(), x.T)


def test_import_and_constructor_attributes():
    import dislib_amd
    from dislib_amd.recommendation import ALS
    est = ALS()
    assert (est._seed, est._n_f, est._lambda, est._tol, est._max_iter,
            est._verbose, est._arity, est._check_convergence) == (
                None, 100, 0.065, 1e-4, 100, False, 5, True)
    assert est.converged is False and est.users is None and \
        est.items is None and est.n_iter == 0
    est = ALS(666, 8, 0.1, 0.01, 7, 3, False, True, device="cuda:0")
    assert (est._seed, est._n_f, est._lambda, est._tol, est._max_iter,
            est._arity, est._check_convergence, est._verbose) == (
                666, 8, 0.1, 0.01, 7, 3, False, True)
    with pytest.raises(TypeError):
        ALS(666, 8, 0.1, 0.01, 7, 3, False, True, "cuda:0")
    pkg = dislib_amd.install_as_dislib()
    from dislib.recommendation import ALS as aliased
    assert aliased is ALS and pkg.recommendation.ALS is ALS


def _boom(*a, **k):
    raise AssertionError("the GPU library was touched")


def _ratings_dataset():
    from dislib_amd.data import load_data
    return load_data(x=_inputs("doc")[0], subset_size=1)


def test_dense_is_refused_before_any_gpu_use(monkeypatch):
    from dislib_amd import _lib
    from dislib_amd.data import load_data
    from dislib_amd.recommendation import ALS
    monkeypatch.setattr(_lib, "lib", _boom)
    with pytest.raises(ValueError, match="sparse"):
        ALS().fit(load_data(np.ones((6, 3)), subset_size=2))


def test_distributed_world_is_refused(monkeypatch):
    from dislib_amd import _lib, _shard
    from dislib_amd.recommendation import ALS
    monkeypatch.setattr(_lib, "lib", _boom)
    monkeypatch.setattr(_shard, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="one rank"):
        ALS().fit(_ratings_dataset())


def test_n_f_above_the_limit_is_refused(monkeypatch):
    from dislib_amd import _lib
    from dislib_amd.recommendation import ALS
    monkeypatch.setattr(_lib, "lib", _boom)
    with pytest.raises(NotImplementedError, match="limited to 128"):
        ALS(n_f=129).fit(_ratings_dataset())


def test_predict_user_quirk():
    """``user_id > users.shape[1]`` compares with the number of factors."""
    from dislib_amd.recommendation import ALS
    est = ALS()
    with pytest.raises(Exception, match="not trained"):
        est.predict_user(0)
    est.users = np.arange(12, dtype=np.float32).reshape(6, 2)
    est.items = np.ones((3, 2), dtype=np.float32)
    assert np.array_equal(est.predict_user(2), [9, 9, 9])   # 2 == n_f: kept
    nan = est.predict_user(3)                    # a user that does exist
    assert nan.shape == (2,) and np.isnan(nan).all()   # items.shape[1] long
    assert np.array_equal(est.predict_user(2),
                          ref.predict_user(est.users, est.items, 2))


def test_abi_constants_agree():
    from dislib_amd import _lib
    src = open(os.path.join(ROOT, "include", "dkm.h")).read()
    consts = dict(re.findall(r"#define (DKM_\w+) (\d+)", src))
    assert int(consts["DKM_ABI_VERSION"]) == _lib.ABI_VERSION == 9
    assert int(consts["DKM_ALS_MAX_NF"]) == _lib.ALS_MAX_NF == 128
    assert int(consts["DKM_ALS_CHUNK"]) == _lib.ALS_CHUNK
    so = _lib.load()
    assert so.dkm_als_workspace_bytes(1000, 100) >= 16 * 1000
    assert so.dkm_als_workspace_bytes(0, 1) > 0
    for bad in ((-1, 8), (2 ** 31, 8), (10, 0), (10, 129)):
        assert so.dkm_als_workspace_bytes(*bad) == 0


# --------------------------------------------------------------------------
# The longdouble yardstick of the kernel tests (tests/als_ref.py, 2nd half)
# --------------------------------------------------------------------------
LD, U = ref.LD, ref.U


def test_longdouble_is_wider_than_fp64():
    assert np.finfo(LD).eps <= 2.0 ** -63


@pytest.mark.parametrize("n", [1, 2, 17, 128])
def test_solve_ld_agrees_with_fp64_solve_when_well_conditioned(n):
    """Within 8 n cond u of np.linalg.solve, whose own forward error that
    is; solve_ld's is 2^-11 of it."""
    rng = np.random.default_rng(n)
    for trial in range(3):
        b = rng.uniform(-1, 1, (n + 3 + trial, n))
        a = b.T.dot(b) + 0.5 * np.eye(n)
        v = rng.uniform(-5, 5, n)
        y, y64 = ref.solve_ld(a, v), np.linalg.solve(a, v)
        assert y.dtype == LD
        bound = 8 * n * np.linalg.cond(a) * U * np.abs(y64).max()
        assert (np.abs((y - y64).astype(np.float64)) <= bound).all()


@pytest.mark.parametrize("n_f", ref.COND_NF)
def test_conditioning_inputs_keep_the_bound_a_check(n_f):
    """The small-lambda family: n_c = 1, 2, n_f - 1, n_f, n_f + 1, the
    bound's conditioning term at most 2^-12 for every row, and solve_ld's
    residual below the fp64 solve's."""
    for dtype in (np.float64, np.float32):
        m, x = ref.conditioning_case(n_f, dtype)
        assert x.dtype == dtype and x.min() < -0.9 and x.max() > 0.9
        assert list(np.diff(m.indptr)) == [1, 2, n_f - 1, n_f, n_f + 1]
        rows = ref.update_rows(m, x, ref.COND_LAMBDA)
        worst = 0.0
        for i, (y, cond) in enumerate(rows):
            assert 8 * n_f * cond * U <= 2.0 ** -12, (i, cond)
            assert cond <= 1 + n_f / ref.COND_LAMBDA
            worst = max(worst, cond)
            idx, r = ref.used_entries(m, i, x.shape[0])
            a, v = ref.normal_equations(idx, r, x, ref.COND_LAMBDA, LD)
            a64, v64 = ref.normal_equations(idx, r, x, ref.COND_LAMBDA)
            y64 = np.linalg.solve(a64, v64)
            res = np.abs(a.dot(y) - v).max()
            res64 = np.abs(a.dot(y64.astype(LD)) - v).max()
            assert np.isfinite(float(res64)) and res <= res64, (i, res, res64)
        assert worst > 1e6                   # ... and it is ill-conditioned
        print("n_f %d %s: largest cond %.3g" % (n_f, np.dtype(dtype).name,
                                                worst))


def test_update_rows_entry_rule():
    """Used iff data != 0 and 0 <= index < n_cols; duplicates stay apart in
    the Gram sum and in n_c; no entry gives zeros."""
    x = np.random.default_rng(3).uniform(-1, 1, (6, 4))
    m = ref.Csr.from_rows([([1, 7, -1, 3], [2.0, 9.0, 9.0, 0.0]),   # one
                           ([5, 6, -2], [1.0, 2.0, 3.0]),           # none
                           ([], []),
                           ([2, 2, 4], [1.5, -0.5, 3.0]),           # twice
                           ([4, 2, 2], [3.0, -0.5, 1.5])], 5)
    rows = ref.update_rows(m, x, 0.1, 5)
    a = np.outer(x[1], x[1]) + 0.1 * np.eye(4)
    assert np.allclose(rows[0][0].astype(float), np.linalg.solve(a, 2 * x[1]),
                       rtol=1e-12, atol=0)
    for i in (1, 2):
        assert np.array_equal(rows[i][0], np.zeros(4)) and rows[i][1] == 0.0
    a = 2 * np.outer(x[2], x[2]) + np.outer(x[4], x[4]) + 0.3 * np.eye(4)
    want = np.linalg.solve(a, x[2] + 3 * x[4])
    assert np.allclose(rows[3][0].astype(float), want, rtol=1e-12, atol=0)
    assert np.allclose(rows[4][0].astype(float), want, rtol=1e-12, atol=0)
    summed = np.linalg.solve(a - np.outer(x[2], x[2]) - 0.1 * np.eye(4),
                             x[2] + 3 * x[4])
    assert not np.allclose(want, summed, rtol=1e-3)
    # with the bound at x.shape[0] = 6, column 5 of row 1 comes in
    assert ref.update_rows(m, x, 0.1)[1][1] > 0


@pytest.mark.parametrize("name", CASES)
def test_longdouble_restatement_reproduces_update(name, ref_results):
    """update_rows against als_ref.update on the goldens' inputs (the last
    items half-step of the fit, and the first users half-step from the fp64
    initial items with their NaN means): within the fp32 store and the fp64
    solve's own forward bound."""
    r, sub, test, args = _inputs(name)
    res = ref_results[name]
    r_i = sp.csr_matrix(r, dtype=np.float64)
    r_u = sp.csr_matrix(r_i.T)
    r_u.sort_indices()
    n_f, lam, seed = args[0], args[1], args[5]
    for m, x in ((r_i, res.users), (r_u, ref.initial_items(r_i, n_f, seed))):
        y32 = ref.update(m, x, lam)
        if m is r_i:
            assert np.array_equal(y32, res.items)
        rows = ref.update_rows(m, x, lam)
        assert len(rows) == m.shape[0]
        for i, (y, cond) in enumerate(rows):
            err = np.abs((y32[i].astype(LD) - y).astype(np.float64))
            assert (err <= ref.update_bound(y, cond, n_f)).all(), i
        # the fp64 flavour is als_ref.update before the store
        rows64 = ref.update_rows(m, x, lam, dtype=np.float64)
        assert np.array_equal(
            np.array([y for y, _ in rows64]).astype(np.float32), y32)


@pytest.mark.parametrize("name", CASES)
def test_longdouble_restatement_reproduces_sse(name, ref_results):
    """sse_ld against als_ref.sse on the goldens: the count exactly, the sum
    within the derived bound at numpy's depth (the square's own rounding,
    any order inside a row, the chain over the rows)."""
    r, sub, test, args = _inputs(name)
    res = ref_results[name]
    r_u = sp.csr_matrix(sp.csr_matrix(r, dtype=np.float64).T)
    r_u.sort_indices()
    n = r_u.shape[0]
    for a, b in ((0, n), (n // 3, n - 1), (2, 2)):
        s64, c64 = ref.sse(r_u, res.users, res.items, a, b, a)
        depth = 1 + int(np.diff(r_u.indptr).max()) + (b - a)
        s, c, bound = ref.sse_ld(r_u, res.users, res.items, a, b, a,
                                 depth=depth)
        assert c == c64
        assert abs(float(LD(s64) - s)) <= bound, (a, b)
        assert bound <= 1e-12 * float(s) or s == 0


def test_sse_ld_and_row_means_ld_rules():
    users = np.array([[1.0, 2.0], [0.5, -1.0]], dtype=np.float32)
    items = np.array([[1.0, 1.0], [2.0, 0.0], [np.nan, np.nan]],
                     dtype=np.float32)
    m = ref.Csr.from_rows([([0, 1, 2, -1], [5.0, 0.0, 1.0, 1.0]),
                           ([1, 1], [2.0, -1.0]), ([], []), ([0], [0.0])], 3)
    s, c, bound = ref.sse_ld(m, users, items, 0, 2, 0, n_items=2)
    # (5 - 3)^2 + (2 - 1)^2 + (-1 - 1)^2: the NaN item and column -1 dropped
    assert (float(s), c) == (9.0, 3) and 0 < bound < 1e-13
    assert ref.sse_ld(m, users, items, 1, 2, 0, n_items=2)[:2] == (9.0, 2)
    assert ref.sse_ld(m, users, items, 2, 2, 0)[:2] == (0.0, 0)
    assert ref.sse_depth(129, 257) == 3 + 6 + 2 + 8
    means = ref.row_means_ld(m)
    assert means.dtype == LD
    assert np.array_equal(means[[0, 1, 3]].astype(float), [1.75, 0.5, 0.0])
    assert np.isnan(means[2])
    assert np.array_equal(ref.row_means_bound(m),
                          [(4 / 64 + 8) * U * 7 / 4, (2 / 64 + 8) * U * 3 / 2,
                           0.0, 0.0])
