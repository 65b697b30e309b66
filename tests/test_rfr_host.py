"""CPU tests of RandomForestRegressor: the constructor, the refusals that
need no GPU and the restatement's split rule on hand-checkable vectors."""
import numpy as np
import pytest
import scipy.sparse as sp

from dislib_amd import _lib, _shard
from dislib_amd.data import Dataset, Subset
from dislib_amd.regression import RandomForestRegressor
from tests import rfr_ref

X, Y = np.random.RandomState(0).rand(40, 3), np.arange(40.0)
BAD = np.where(np.arange(40) == 3, np.nan, Y)


def test_constructor_defaults():
    est = RandomForestRegressor()
    assert (est.n_estimators, est.try_features_init, est.max_depth,
            est.distr_depth_init, est.sklearn_max, est.trees, est.times_) == (
                10, 'sqrt', np.inf, 'auto', 1e8, None, None)


@pytest.mark.parametrize("subsets,kw,exc,match", [
    ([(sp.csr_matrix(X), Y)], dict(sparse=True), NotImplementedError, "dense"),
    ([(X, Y)], dict(world=True), NotImplementedError, "one rank"),
    ([(X, Y), (X, None)], {}, ValueError, "no labels"),
    ([], {}, ValueError, "with samples"),
    ([(X, BAD)], {}, ValueError, "finite number"),
    ([(X, np.where(BAD == BAD, Y, np.inf))], {}, ValueError, "finite number"),
    ([(X, Y)], dict(most=40), ValueError, "fewer than"),
    ([(X, Y)], dict(try_features=4), ValueError, "try_features"),
])
def test_refusals_without_a_gpu(monkeypatch, subsets, kw, exc, match):
    ds = Dataset(n_features=3, sparse=kw.get("sparse", False))
    for x, y in subsets:
        ds.append(Subset(x, y))
    monkeypatch.setattr(_shard, "active", lambda: kw.get("world", False))
    monkeypatch.setattr(_lib, "RF_MAX_SAMPLES", kw.get("most", 1 << 24))
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("library touched"))
    with pytest.raises(exc, match=match):
        RandomForestRegressor(try_features=kw.get("try_features",
                                                  'sqrt')).fit(ds)


@pytest.mark.parametrize("v,y,want", [
    # -(SL^2 / ll + SR^2 / rl) after each run; the minimum is at position 1
    ([1, 2, 3, 4], [0, 0, 6, 6], (-(0 / 2 + 144 / 2), 1, 2, 3)),
    # ties in the value: positions 0 and 2 are inside runs
    ([5, 5, 7, 7], [1, 3, 4, 8], (-(16 / 2 + 144 / 2), 1, 5, 7)),
    # a constant feature: only the last position is scored, no cut
    ([2, 2, 2], [1, 2, 6], (-(81 / 3 + 0 / 1), 2, 2, 2)),
    # two equal minima (-(4/1 + 4/2) at 0, -(4/2 + 4/1) at 1): the last wins
    ([1, 2, 3], [2, 0, 2], (-6.0, 1, 2, 3)),
    # unsorted input; -0.0 and 0.0 are one value
    ([0.0, 3, -0.0, 1], [5, 1, 5, 1], (-(100 / 2 + 4 / 2), 1, 0, 1)),
])
def test_split_by_hand(v, y, want):
    got = rfr_ref.split(np.array(v, dtype=np.float64), np.array(y))
    assert tuple(got) == want
