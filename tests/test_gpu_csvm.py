"""GPU tests of ``dislib_amd.classification.CascadeSVM`` against every golden
case of ``csvm_ref.npz`` (the reference run three times, see
``tests/golden/gen_golden_csvm.py``) under the acceptance rules of
``csvm_ref.check_against_golden``, plus ``score``, the duplicate rows, the
toy tests of the reference's ``tests/test_csvm.py`` and the refusals."""
import numpy as np
import pytest

from dislib_amd.classification import CascadeSVM
from dislib_amd.data import Dataset, Subset, load_data
from tests import csvm_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _dataset(x, y, sizes):
    ds = Dataset(n_features=x.shape[1])
    off = 0
    for s in sizes:
        ds.append(Subset(x[off:off + s], y[off:off + s]))
        off += s
    return ds


_FITS = {}


def _fit(name):
    """The fit of a golden case, shared among the tests."""
    if name not in _FITS:
        g = ref.case(name)
        ds = _dataset(g["x"], g["y"], g["sizes"])
        ds._device_data()
        dd, p = ds._device, ds._device.X.data_ptr()
        est = CascadeSVM(**g["kw"])
        est.fit(ds)
        # the resident image is the one uploaded before the fit
        assert ds._device_data() is dd and dd.X.data_ptr() == p
        _FITS[name] = (g, est)
    return _FITS[name]


@pytest.mark.parametrize("name", ref.case_names())
def test_against_golden(name):
    g, est = _fit(name)
    probe = load_data(g["probe"], subset_size=64)
    est.decision_function(probe)
    dec = probe.labels.astype(np.float64)
    assert dec.dtype == np.float64 and probe[0].labels.dtype == np.float64
    est.predict(probe)
    pred = probe.labels
    print(name, "iterations", est.iterations, "converged", est.converged,
          "W", est.w_, "dec err", np.abs(dec - g["dec"]).max(),
          "n_sv", len(est._clf.support_))
    ref.check_against_golden(g, est.iterations, est.converged, est.w_, dec,
                             pred, est._clf.support_)
    clf = est._clf
    assert list(clf.classes_) == sorted(set(g["y"].tolist()))
    assert clf.dual_coef_.shape == (1, len(clf.support_))
    assert clf.n_support_.sum() == len(clf.support_)
    assert np.array_equal(clf.support_vectors_,
                          g["x"][clf.support_].astype(np.float64))
    ypm = np.where(g["y"][clf.support_] == clf.classes_[1], 1.0, -1.0)
    assert np.all(np.sign(clf.dual_coef_[0]) == ypm)
    assert np.array_equal(pred, clf.classes_[(dec > 0).astype(int)])


def test_score_is_the_recomputed_accuracy():
    g, est = _fit("rbf_auto")
    rng = np.random.default_rng(0)
    truth = rng.choice(np.unique(g["y"]), len(g["probe"]))
    probe = load_data(g["probe"], subset_size=64, y=truth)
    acc = est.score(probe)
    assert np.array_equal(probe.labels, truth)
    est.predict(probe)
    assert acc == np.mean(probe.labels == truth)


def test_two_fits_are_byte_identical():
    g = ref.case("lin_b0")
    out = []
    for _ in range(2):
        est = CascadeSVM(**g["kw"])
        est.fit(_dataset(g["x"], g["y"], g["sizes"]))
        out.append((est._clf.dual_coef_.tobytes(),
                    est._clf.intercept_.tobytes(), np.array(est.w_).tobytes(),
                    est._clf.support_.tobytes()))
    assert out[0] == out[1]


def test_duplicates():
    g, est = _fit("duplicates")
    assert est._clf.support_vectors_.shape[0] == 6
    assert len(set(est._clf.support_.tolist())) == 6


def _toy(points, **kw):
    ds = Dataset(n_features=2)
    p1, p2, p3, p4 = points
    ds.append(Subset(np.array([p1, p4]), np.array([0, 1])))
    ds.append(Subset(np.array([p3, p2]), np.array([1, 0])))
    est = CascadeSVM(cascade_arity=3, max_iter=10, tol=1e-4, c=2, gamma=0.1,
                     random_state=666, verbose=False, **kw)
    est.fit(ds)
    return est


def test_toy_predict():
    pts = [1, 2], [2, 1], [-1, -2], [-2, -1]
    est = _toy(pts, kernel="linear", check_convergence=False)
    test_set = load_data(x=np.array(list(pts) + [[1, 1], [-1, -1]]),
                         subset_size=2)
    est.predict(test_set)
    l1, l2, l3, l4, l5, l6 = test_set.labels
    assert l1 == l2 == l5 == 0
    assert l3 == l4 == l6 == 1


def test_toy_score():
    pts = [1, 2], [2, 1], [-1, -2], [-2, -1]
    est = _toy(pts, kernel="rbf", check_convergence=True)
    test_set = load_data(x=np.array(pts), subset_size=2,
                         y=np.array([0, 0, 1, 1]))
    assert est.score(test_set) == 1.0


def test_toy_decision_function():
    pts = [0, 2], [0, 1], [0, -2], [0, -1]
    est = _toy(pts, kernel="rbf", check_convergence=False)
    test_set = load_data(x=np.array(pts), subset_size=2)
    est.decision_function(test_set)
    d1, d2, d3, d4 = test_set.labels
    assert np.isclose(abs(d1) - abs(d3), 0)
    assert np.isclose(abs(d2) - abs(d4), 0)
    test_set = load_data(x=np.array([[1, 0], [-1, 0]]), subset_size=1)
    est.decision_function(test_set)
    d5, d6 = test_set.labels
    assert np.isclose(d5, 0)
    assert np.isclose(d6, 0)


def test_refusals():
    import scipy.sparse as sp
    x = np.arange(12.0).reshape(6, 2)
    with pytest.raises(NotImplementedError):
        CascadeSVM().fit(load_data(sp.csr_matrix(x), 3, y=np.arange(6) % 2))
    with pytest.raises(ValueError, match="binary"):
        CascadeSVM().fit(load_data(x, 3, y=np.arange(6) % 3))
    with pytest.raises(ValueError, match="greater than one"):
        CascadeSVM().fit(load_data(x, 3, y=np.array([0, 0, 0, 1, 0, 1])))
