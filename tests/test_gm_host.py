"""CPU tests of the GaussianMixture reference side: the numpy restatement
(tests/gm_ref.py) in fp64 and in longdouble against the goldens (the
reference's own output), the conditions every golden input meets, and the
parts of ``dislib_amd.cluster.GaussianMixture`` that need no GPU."""
import hashlib

import numpy as np
import pytest
from numpy.random.mtrand import RandomState

from dislib_amd.cluster import GaussianMixture
from tests import gm_ref as gr
from tests.conftest import load_golden

PARAMS = ("weights", "means", "covariances", "precisions_cholesky")
ATTRS = ("weights_", "means_", "covariances_", "precisions_cholesky_")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def close(got, want, tol):
    """Within ``tol`` relative to the array's max magnitude."""
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got).astype(np.float64)
    return got.shape == want.shape and \
        np.abs(got - want).max() <= tol * np.abs(want).max()


def keep(g, key="gap"):
    """Rows whose labels are compared: top-two gap of at least GAP."""
    return g[key] >= gr.GAP


_FITS = {}


def fitted(name, dt):
    """One restated fit per (case, arithmetic), shared by the tests."""
    if (name, dt) not in _FITS:
        inp = gr.inputs(name)
        m = gr.RefGM(dt=dt, **inp["kw"])
        blocks = gr.split(inp["x"], inp["sizes"])
        m.fit(blocks)
        lab = m.predict(blocks)
        plab = m.predict(gr.split(inp["x_test"], inp["test_sizes"]))
        _FITS[name, dt] = m, lab, plab
    return _FITS[name, dt]


@pytest.mark.parametrize("name", gr.CASES)
def test_golden_inputs_meet_their_conditions(name):
    g, inp = load_golden(name), gr.inputs(name)
    assert sha(inp["x"]) == str(g["x_sha"])
    assert sha(inp["x_test"]) == str(g["x_test_sha"])
    assert list(g["sizes"]) == inp["sizes"]
    if name not in gr.NO_CHOL:
        assert len(set(inp["sizes"])) > 1           # uneven Subsets
    tol = inp["kw"].get("tol", 1e-3)
    assert np.abs(g["trace"] - tol).min() >= 1e-6
    for key in ("gap", "gap_test"):
        assert (g[key] < gr.GAP).mean() <= 0.005
    if name not in gr.NO_CHOL:
        assert g["cond"] <= 1e3
    assert g["cond"] == gr.max_cond(g["covariances"])


def test_golden_cases_cover_what_they_are_for():
    assert load_golden("gm_a")["n_iter"] == 5
    assert load_golden("gm_b")["n_iter"] > 20
    assert load_golden("gm_c")["n_iter"] > 2
    e = load_golden("gm_e")
    assert e["n_iter"] == 0 and not e["converged"] and len(e["trace"]) == 3
    assert load_golden("gm_g")["n_iter"] > 5
    assert gr.inputs("gm_c")["x"].dtype == np.float32
    assert all(np.issubdtype(gr.inputs(n)["x"].dtype, np.integer)
               for n in ("gm_f1", "gm_f2"))


@pytest.mark.parametrize("dt", [np.float64, np.longdouble],
                         ids=["fp64", "longdouble"])
@pytest.mark.parametrize("name", gr.CASES)
def test_restatement_equals_the_golden(name, dt):
    g = load_golden(name)
    m, lab, plab = fitted(name, dt)
    assert m.n_iter == g["n_iter"] and m.converged_ == g["converged"]
    assert np.array_equal(lab[keep(g)], g["labels"][keep(g)])
    kt = keep(g, "gap_test")
    assert np.array_equal(plab[kt], g["predict_labels"][kt])
    for p, a in zip(PARAMS, ATTRS):
        if p == "precisions_cholesky" and name in gr.NO_CHOL:
            assert close(getattr(m, a), g[p], 1e-10 * float(g["cond"]))
        else:
            assert close(getattr(m, a), g[p], 1e-10), p
    assert abs(float(m.lower_bound_) - g["lower_bound"]) <= \
        1e-10 * abs(g["lower_bound"])
    assert np.allclose(m.trace, g["trace"], rtol=1e-6, atol=1e-12)
    if "kmeans_centers" in g:
        assert np.array_equal(m.kmeans_centers, g["kmeans_centers"])


def test_single_steps_agree_between_the_arithmetics():
    inp = gr.inputs("gm_b")
    g = load_golden("gm_b")
    x = inp["x"][:300]
    a = gr.estep(x, g["weights"], g["means"], g["precisions_cholesky"])
    b = gr.estep(x, g["weights"], g["means"], g["precisions_cholesky"],
                 np.longdouble)
    assert close(a["resp"], b["resp"], 1e-12)
    assert close(a["lse"], b["lse"], 1e-13)
    for u, v in zip(gr.mstep(x, a["resp"]),
                    gr.mstep(x, a["resp"], dt=np.longdouble)):
        assert close(u, v, 1e-11)


# ---------------------------------------------------------------------------
# the class, without a GPU
# ---------------------------------------------------------------------------
def test_init_params():
    """test_gm.py:16-44, plus the private names the reference keeps."""
    weights_init = np.array([0.4, 0.6])
    means_init = np.array([[0, 0], [2, 3]])
    random_state = RandomState(666)
    gm = GaussianMixture(n_components=2, covariance_type='diag', tol=1e-4,
                         reg_covar=1e-5, max_iter=3, init_params='random',
                         weights_init=weights_init, means_init=means_init,
                         precisions_init='todo', random_state=random_state)
    expected = (2, 'diag', 1e-4, 1e-5, 3, 'random', weights_init, means_init,
                'todo', random_state)
    real = (gm.n_components, gm.covariance_type, gm.tol, gm.reg_covar,
            gm.max_iter, gm.init_params, gm.weights_init, gm.means_init,
            gm.precisions_init, gm.random_state)
    assert expected == real
    d = GaussianMixture()
    assert (d.n_components, d.covariance_type, d.tol, d.reg_covar, d.max_iter,
            d.init_params, d._arity, d._verbose, d.random_state) == \
        (1, 'full', 1e-3, 1e-6, 100, 'kmeans', 50, False, None)
    assert GaussianMixture(arity=7, verbose=True)._arity == 7
    with pytest.raises(TypeError):
        GaussianMixture(1, 'full', 1e-3, 1e-6, 100, 'kmeans', None, None,
                        None, 50, False, None, "cuda:0")   # keyword-only


@pytest.mark.parametrize("kw,match", [
    (dict(n_components=0), "n_components"), (dict(tol=-0.1), "tol"),
    (dict(max_iter=0), "max_iter"), (dict(reg_covar=-0.1), "reg_covar"),
    (dict(covariance_type=''), "covariance_type")])
def test_validation_errors(kw, match):
    """test_gm.py:116-154: raised before anything touches the device."""
    from dislib_amd.data import load_data
    ds = load_data(np.array([[0, 0], [0, 1], [1, 0]]), subset_size=10)
    with pytest.raises(ValueError, match="Invalid value for '%s'" % match):
        GaussianMixture(**kw).fit(ds)


@pytest.mark.parametrize("ct", ['tied', 'diag', 'spherical'])
def test_unimplemented_covariance_types(ct):
    from dislib_amd.data import load_data
    ds = load_data(np.array([[0., 0], [0, 1], [1, 0]]), subset_size=10)
    with pytest.raises(NotImplementedError, match=ct):
        GaussianMixture(covariance_type=ct).fit(ds)


def test_sparse_is_refused_and_predict_needs_a_fit():
    import scipy.sparse as sp
    from sklearn.exceptions import NotFittedError

    from dislib_amd.data import Dataset, Subset, load_data
    ds = Dataset(n_features=3, sparse=True)
    ds.append(Subset(sp.csr_matrix(np.eye(3))))
    with pytest.raises(NotImplementedError, match="dense"):
        GaussianMixture().fit(ds)
    with pytest.raises(NotFittedError):
        GaussianMixture().predict(load_data(np.eye(3), subset_size=3))


def test_install_as_dislib_exports_the_class():
    import dislib_amd
    dislib_amd.install_as_dislib()
    from dislib.cluster import GaussianMixture as G
    assert G is GaussianMixture
