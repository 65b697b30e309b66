"""CPU tests of the host-side surface of LinearRegression: every refusal that
needs no device is raised before the GPU library is touched."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.exceptions import NotFittedError

import dislib_amd
from dislib_amd import _lib, _shard
from dislib_amd.data import Dataset, Subset, load_data
from dislib_amd.regression import LinearRegression

X = np.arange(12.0).reshape(6, 2)
Y = np.arange(6.0)


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
    (_ds(X, np.array(["a"] * 6)), {}, ValueError, "finite number"),
    (_ds(X, np.array([0, 1, 2, 3, 4, np.inf])), {}, ValueError, "finite"),
    (_ds(X, np.zeros((6, 2))), {}, ValueError, "per sample"),
    (Dataset(n_features=2), {}, ValueError, "at least 1 sample"),
    (_ds(np.zeros((2, 127)), np.zeros(2)), {}, ValueError, "at most 128"),
    (_ds(np.zeros((2, 128)), np.zeros(2)), dict(fit_intercept=False),
     ValueError, "at most 128"),
])
def test_fit_refusals(no_gpu, ds, kwargs, exc, match):
    with pytest.raises(exc, match=match):
        LinearRegression(**kwargs).fit(ds)


def test_predict_and_world_refusals(no_gpu, monkeypatch):
    ds = _ds(X, Y)
    lr = LinearRegression()
    with pytest.raises(NotFittedError):
        lr.predict(ds)
    lr.coef_ = np.zeros(3)
    with pytest.raises(ValueError, match="3 features"):
        lr.predict(ds)
    monkeypatch.setattr(_shard, "world", lambda: (0, 2))
    for call in (LinearRegression().fit, lr.predict):
        with pytest.raises(NotImplementedError, match="one rank"):
            call(ds)


def test_constructor_constant_and_alias():
    header = open(os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "include", "dkm.h")).read()
    assert _lib.TSQR_MAX_W == 128 == int(
        re.search(r"#define DKM_TSQR_MAX_W (\d+)", header).group(1))
    lr = LinearRegression(False, 7, device="cuda:0")
    assert (lr._fit_intercept, lr._arity, lr._device) == (False, 7, "cuda:0")
    lr = LinearRegression()
    assert lr._fit_intercept is True and lr._arity == 50
    assert lr.coef_ is None and lr.intercept_ is None
    with pytest.raises(TypeError):
        LinearRegression(True, 7, "cuda:0")
    dislib_amd.install_as_dislib()
    from dislib.regression import LinearRegression as aliased
    assert aliased is LinearRegression
