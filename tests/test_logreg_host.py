"""CPU tests of the host-side surface of LogisticRegression: every refusal
that needs no device is raised before the GPU library is touched."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.exceptions import NotFittedError

from dislib_amd import _lib, _shard
from dislib_amd.classification import LogisticRegression
from dislib_amd.data import Dataset, Subset, load_data

X = np.arange(12.0).reshape(6, 2)
Y = np.array([0, 1, 0, 1, 1, 0])


@pytest.fixture
def no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the GPU library was touched")
    monkeypatch.setattr(_lib, "lib", boom)


def _ds(x, y):
    ds = Dataset(n_features=x.shape[1])
    ds.append(Subset(x, labels=y))
    return ds


@pytest.mark.parametrize("ds,kwargs,exc,match", [
    (load_data(sp.random(30, 5, density=0.3, format="csr", random_state=0),
               subset_size=10), {}, NotImplementedError, "dense"),
    (load_data(X, subset_size=3), {}, ValueError, "no labels"),
    (_ds(X, np.zeros((6, 2))), {}, ValueError, "per sample"),
    (_ds(X, Y[:5]), {}, ValueError, "per sample"),
    (_ds(X, np.zeros(6)), {}, ValueError, "at least 2 classes"),
    (_ds(np.zeros((40, 2)), np.arange(40) % 33), {}, ValueError,
     "at most 32 classes"),
    (_ds(X, Y), dict(C=0.0), ValueError, "C must be positive"),
    (_ds(X, Y), dict(tol=-1e-9), ValueError, "tol must be"),
    (_ds(X, Y), dict(max_iter=0), ValueError, "max_iter must be"),
    (_ds(np.zeros((6, 257)), Y), {}, ValueError, "at most 256 features"),
    (Dataset(n_features=2), {}, ValueError, "at least 1 sample"),
])
def test_fit_refusals(no_gpu, ds, kwargs, exc, match):
    with pytest.raises(exc, match=match):
        LogisticRegression(**kwargs).fit(ds)


def test_predict_and_world_refusals(no_gpu, monkeypatch):
    ds = _ds(X, Y)
    lr = LogisticRegression()
    calls = (lr.predict, lr.predict_proba, lr.decision_function, lr.score)
    for call in calls:
        with pytest.raises(NotFittedError):
            call(ds)
    lr.coef_, lr.classes_ = np.zeros((1, 3)), np.array([0, 1])
    for call in calls:
        with pytest.raises(ValueError, match="3 features"):
            call(ds)
    monkeypatch.setattr(_shard, "world", lambda: (0, 2))
    for call in (LogisticRegression().fit,) + calls:
        with pytest.raises(NotImplementedError, match="one rank"):
            call(ds)


def test_constructor_and_constants():
    header = open(os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "include", "dkm.h")).read()
    for name, value in (("MAX_D", _lib.LOGREG_MAX_D),
                        ("MAX_CLASSES", _lib.LOGREG_MAX_CLASSES)):
        assert value == int(re.search(r"#define DKM_LOGREG_%s (\d+)" % name,
                                      header).group(1))
    assert _lib.LOGREG_MAX_D >= 256
    assert _lib.LOGREG_MAX_CLASSES == _lib.RF_MAX_CLASSES
    lr = LogisticRegression(0.5, False, 1e-6, 7, device="cuda:0")
    assert (lr.C, lr.fit_intercept, lr.tol, lr.max_iter, lr._device) == \
        (0.5, False, 1e-6, 7, "cuda:0")
    lr = LogisticRegression()
    assert (lr.C, lr.fit_intercept, lr.tol, lr.max_iter) == \
        (1.0, True, 1e-4, 100)
    assert lr.coef_ is None and lr.intercept_ is None and \
        lr.classes_ is None and lr.n_iter_ is None
    with pytest.raises(TypeError):
        LogisticRegression(1.0, True, 1e-4, 100, "cuda:0")
