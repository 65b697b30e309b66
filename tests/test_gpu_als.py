"""GPU tests of ``dislib_amd.recommendation.ALS`` (dkm_als.hip): every golden
case of the reference (tests/golden/als_ref.npz) through ``fit``."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests import als_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "als_ref.npz"))
CASES = sorted({k.split("__")[0] for k in G.files})


def _inputs(name):
    """(items x users CSR with the stored zeros, subset_size, test or None,
    constructor arguments) of a golden case."""
    sub, n_f, lam, tol, max_iter, check, seed = G[name + "__meta"]
    stored = np.nonzero(G[name + "__r_stored"])
    r = sp.csr_matrix((G[name + "__r"][stored], stored),
                      shape=G[name + "__r"].shape)
    test = sp.csr_matrix(G[name + "__test"]) \
        if name + "__test" in G.files else None
    kw = dict(n_f=int(n_f), lambda_=float(lam), tol=float(tol),
              max_iter=int(max_iter), check_convergence=bool(check),
              random_state=int(seed))
    return r, int(sub), test, kw


def _fit(name):
    from dislib_amd.data import load_data
    from dislib_amd.recommendation import ALS
    r, sub, test, kw = _inputs(name)
    est = ALS(**kw)
    out = est.fit(load_data(x=r, subset_size=sub), test=test)
    return est, out


@pytest.fixture(scope="module")
def fits():
    return {name: _fit(name) for name in CASES}


@pytest.mark.parametrize("name", CASES)
def test_fit_equals_reference(name, fits):
    est, (users, items) = fits[name]
    assert users is est.users and items is est.items
    assert est.users.dtype == np.float32 == est.items.dtype
    assert est.n_iter == int(G[name + "__n_iter"])
    assert est.converged == bool(G[name + "__converged"])
    for got, key in ((est.users, "__users"), (est.items, "__items")):
        want = G[name + key]
        assert got.shape == want.shape
        gap = np.abs(got - want).max() / np.abs(want).max()
        print(name, key, "gap %.3g (T %.3g)" % (gap, ref.T_FACTORS))
        assert gap <= ref.T_FACTORS
    want = G[name + "__rmses"]
    assert len(est.rmse_) == len(want)
    if len(want):
        gap = np.abs(np.array(est.rmse_) - want).max()
        print(name, "rmse gap %.3g (T %.3g)" % (gap, ref.T_RMSE))
        assert gap <= ref.T_RMSE


def test_fit_equals_the_restatement(fits):
    """The kernels against the numpy statement of the same arithmetic: a few
    float32 ulp per iteration, far inside the tolerance to the reference."""
    for name in ("doc", "holes_f8_s4", "m_f100_s1"):
        r, sub, test, kw = _inputs(name)
        want = ref.als_ref(r, -(-r.shape[0] // sub), kw["n_f"],
                           kw["lambda_"], kw["tol"], kw["max_iter"],
                           kw["check_convergence"], kw["random_state"], test)
        est = fits[name][0]
        assert est.n_iter == want.n_iter and est.converged == want.converged
        for got, w in ((est.users, want.users), (est.items, want.items)):
            assert np.abs(got - w).max() <= 1e-4 * np.abs(w).max()
        assert np.abs(np.array(est.rmse_) - want.rmses).max() <= 1e-5


def test_docstring_case_predictions(fits):
    """The three inequalities of the reference's test_predict."""
    predictions = fits["doc"][0].predict_user(user_id=0)
    assert 2.75 < predictions[0] < 3.25
    assert predictions[1] < 1
    assert predictions[2] > 4.5


def test_two_fits_are_byte_identical(fits):
    for name in ("m_f32_s4_test", "holes_f8_s4"):
        est, _ = _fit(name)
        first = fits[name][0]
        assert est.users.tobytes() == first.users.tobytes()
        assert est.items.tobytes() == first.items.tobytes()
        assert est.rmse_ == first.rmse_ and est.n_iter == first.n_iter


def test_n_f_above_the_limit_raises():
    from dislib_amd import _lib
    from dislib_amd.data import load_data
    from dislib_amd.recommendation import ALS
    r, sub, _, _ = _inputs("doc")
    with pytest.raises(NotImplementedError, match=str(_lib.ALS_MAX_NF)):
        ALS(n_f=_lib.ALS_MAX_NF + 1).fit(load_data(x=r, subset_size=sub))
