"""CPU tests of StandardScaler: the numpy restatement (tests/scaler_ref.py)
equals the reference's goldens s01 .. s07 bit for bit, and the estimator's
host-side contract (constructor, validation, refusals)."""
import hashlib

import numpy as np
import pytest
import scipy.sparse as sp

from dislib_amd.data import Dataset, Subset
from dislib_amd.preprocessing import StandardScaler
from tests import scaler_ref as sr
from tests.conftest import load_golden


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def check_scaled(g, key, y):
    """The scaled matrix against the golden's full copy or its sha256."""
    assert str(y.dtype) == str(g[key + "y_dtype"])
    if key + "y" in g:
        assert same(y, g[key + "y"])
    else:
        assert not np.isnan(y).any()
        assert sha(y) == str(g[key + "y_sha"])


def golden_cases():
    """(golden name, key of the case's arrays, x, Subset sizes, arity)."""
    for name in ("s01", "s02", "s03", "s04", "s05", "s06"):
        for key, x, sizes, arities in sr.inputs(name):
            for arity in arities:
                k = key if len(arities) == 1 else "%sa%d_" % (key, arity)
                yield name, key, k, x, sizes, arity


CASES = list(golden_cases())


@pytest.mark.parametrize("case", CASES,
                         ids=["%s_%sa%d" % (c[0], c[1], c[5]) for c in CASES])
def test_restatement_equals_the_reference(case):
    name, key, k, x, sizes, arity = case
    g = load_golden(name)
    assert sha(x) == str(g[key + "x_sha"])
    assert list(g[key + "sizes"]) == list(sizes)
    blocks = sr.split(x, sizes)
    mean, var = sr.fit(blocks, arity)
    assert same(mean, g[k + "mean"]) and same(var, g[k + "var"])
    check_scaled(g, k, np.concatenate(sr.transform(blocks, mean, var)))


def test_restatement_s07_fp32_data_fp64_statistics():
    g = load_golden("s07")
    (_, x, sizes, _), = sr.inputs("s07")
    mean, var = sr.fit(sr.split(x, sizes), 50)
    assert same(mean, g["mean"]) and same(var, g["var"])
    x32, sizes32 = sr.s07_input()
    assert sha(x32) == str(g["x_sha"]) and x32.dtype == np.float32
    y = np.concatenate(sr.transform(sr.split(x32, sizes32), mean, var))
    assert y.dtype == np.float64
    check_scaled(g, "", y)


def test_goldens_cover_what_they_are_for():
    g = load_golden("s02")
    assert not (np.array_equal(g["a50_mean"], g["a2_mean"]) and
                np.array_equal(g["a50_var"], g["a2_var"]))
    g = load_golden("s05")
    assert np.isnan(g["a_y"][:, 2]).all() and np.isinf(g["a_y"][:, 3]).all()
    assert np.isfinite(g["a_y"][:, [0, 1, 4]]).all()
    assert np.isnan(g["b_y"]).all()
    assert load_golden("s03")["mean"].dtype == np.float32
    assert load_golden("s04")["mean"].dtype == np.float64


def test_constructor_and_validation():
    sc = StandardScaler()
    assert sc._arity == 50 and sc.mean_ is None and sc.var_ is None
    assert StandardScaler(arity=3)._arity == 3
    assert StandardScaler(7, sums="reference")._arity == 7
    with pytest.raises(ValueError, match="sums"):
        StandardScaler(sums="exact")
    with pytest.raises(TypeError):
        StandardScaler(50, "reference")      # keyword-only


def test_transform_before_fit_raises_the_reference_exception():
    ds = Dataset(n_features=2)
    ds.append(Subset(np.ones((3, 2))))
    with pytest.raises(Exception, match="Model has not been initialized."):
        StandardScaler().transform(ds)


@pytest.mark.parametrize("sums", ["fast", "reference"])
def test_sparse_dataset_is_refused(sums):
    ds = Dataset(n_features=4, sparse=True)
    ds.append(Subset(sp.random(5, 4, density=0.5, format="csr",
                               random_state=0)))
    sc = StandardScaler(sums=sums)
    with pytest.raises(NotImplementedError):
        sc.fit(ds)
    sc._mean, sc._var = np.zeros(4), np.ones(4)
    with pytest.raises(NotImplementedError):
        sc.transform(ds)


def test_install_as_dislib_aliases_preprocessing():
    import sys

    import dislib_amd
    names = ("dislib", "dislib.cluster", "dislib.data", "dislib.neighbors",
             "dislib.preprocessing")
    saved = {k: sys.modules.get(k) for k in names}
    try:
        dislib_amd.install_as_dislib()
        from dislib.preprocessing import StandardScaler as S2
        assert S2 is StandardScaler
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
