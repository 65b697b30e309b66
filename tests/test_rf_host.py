"""CPU tests of RandomForestClassifier: the numpy restatement's split rule
against the reference's own ``test_split`` results (``rf_ref.npz``), the
feature draws, the constructor and the refusals that need no GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from dislib_amd import _lib, _shard
from dislib_amd.classification import RandomForestClassifier
from dislib_amd.classification import rf
from dislib_amd.data import Dataset, Subset
from tests import rf_ref
from tests.conftest import load_golden

G = load_golden("rf_ref")
CASES = sorted(k[:-8] for k in G if k.endswith("__values"))


@pytest.mark.parametrize("name", CASES)
def test_split_rule_equals_the_reference(name):
    v, y = G[name + "__values"], G[name + "__y"]
    score, pos, lo, hi = rf_ref.split(v, y, int(G[name + "__meta"][0]))
    assert np.float64(score).tobytes() == G[name + "__score"].tobytes()
    if pos == len(y) - 1:
        assert np.isinf(G[name + "__value"])
        return
    value = rf_ref.threshold(lo, hi)
    assert value == rf.threshold(lo, hi)
    assert lo <= value < hi
    if v.dtype == np.float64:
        assert value == G[name + "__value"]
    else:
        assert value == (np.float64(lo) + np.float64(hi)) / 2


def test_threshold_never_reaches_the_upper_value():
    lo = np.float64(1.0)
    hi = np.nextafter(lo, 2.0)
    assert rf_ref.threshold(lo, hi) == lo and rf.threshold(lo, hi) == lo


def test_feature_draws():
    seeds, nodes = np.array([3, 3, 2 ** 31 - 2]), np.array([0, 7, 123456])
    o = rf.feature_order(seeds, nodes, 13)
    for i in range(3):
        assert np.array_equal(o[i], rf_ref.feature_order(seeds[i], nodes[i],
                                                         13))
        assert sorted(o[i]) == list(range(13))
    assert not np.array_equal(o[0], o[1])


def test_constructor_and_try_features():
    est = RandomForestClassifier()
    assert (est.n_estimators, est.try_features_init, est.max_depth,
            est.distr_depth_init, est.sklearn_max, est.hard_vote) == (
                10, 'sqrt', np.inf, 'auto', 1e8, False)
    assert [rf.resolve_try_features(a, 12) for a in
            ('sqrt', 'third', None, 5)] == [3, 4, 12, 5]
    assert rf.resolve_try_features('third', 2) == 1


def test_refusals_without_a_gpu(monkeypatch):
    x, y = np.random.RandomState(0).rand(40, 3), np.arange(40)
    ds = Dataset(n_features=3, sparse=True)
    ds.append(Subset(sp.csr_matrix(x), y % 2))
    with pytest.raises(NotImplementedError):
        RandomForestClassifier().fit(ds)
    ds = Dataset(n_features=3)
    ds.append(Subset(x, y % 2))
    ds.append(Subset(x))
    with pytest.raises(ValueError, match="labelled"):
        RandomForestClassifier().fit(ds)
    ds = Dataset(n_features=3)
    ds.append(Subset(x, y))
    with pytest.raises(ValueError, match="classes"):
        RandomForestClassifier().fit(ds)
    ds = Dataset(n_features=3)
    ds.append(Subset(x, y % 2))
    monkeypatch.setattr(_lib, "RF_MAX_SAMPLES", 40)
    with pytest.raises(ValueError, match="samples"):
        RandomForestClassifier().fit(ds)
    monkeypatch.setattr(_shard, "active", lambda: True)
    with pytest.raises(NotImplementedError, match="one rank"):
        RandomForestClassifier().fit(ds)
