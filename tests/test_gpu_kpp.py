"""GPU tests of ``kmeans_plusplus`` and ``KMeans(init="k-means++")`` against
tests/kpp_ref.py.  Each case first asserts on the restatement a 1e-9 pot margin
of its targets and trial potentials; the device rounds below 4e-13 relative."""
import numpy as np
import pytest

from dislib_amd.cluster import KMeans, kmeans_plusplus
from dislib_amd.cluster import kmeans as kmeans_mod
from dislib_amd.data import Dataset, Subset
from tests import kpp_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# n, d, k, n_local_trials, Subsets, dtype, seed
CASES = [(300, 2, 9, None, 1, np.float64, 0),
         (300, 33, 2, 3, 3, np.float32, 1),
         (2100, 33, 9, None, 3, np.float64, 2),
         (2100, 2, 9, 5, 1, np.float32, 3),
         (300, 2, 1, None, 3, np.float64, 4),
         (40, 2, 40, None, 3, np.float64, 5),
         (300, 33, 9, 1, 1, np.float64, 6)]


def _dataset(x, parts):
    """x as a Dataset of ``parts`` uneven Subsets."""
    cuts = [0] + [len(x) * (i * i + 1) // (parts * parts + 1)
                  for i in range(1, parts)] + [len(x)]
    ds = Dataset(n_features=x.shape[1])
    for a, b in zip(cuts[:-1], cuts[1:]):
        ds.append(Subset(samples=x[a:b]))
    return ds


def _blobs(seed):
    """Six well-separated blobs of 50 rows, away from the unit cube."""
    rng = np.random.default_rng(seed)
    cen = 40.0 + 25.0 * np.arange(6)[:, None] * np.array([1.0, -1.0])
    x = np.repeat(cen, 50, axis=0) + rng.standard_normal((300, 2))
    return x, np.repeat(np.arange(6), 50)


@pytest.mark.parametrize("n,d,k,L,parts,dtype,seed", CASES)
def test_indices_equal_the_restatement(n, d, k, L, parts, dtype, seed):
    x = (3.0 * np.random.default_rng(seed).standard_normal((n, d)) - 2.0
         ).astype(dtype)
    want, margin = kpp_ref.kpp_ref(x.astype(np.float64), k, seed, L)
    assert margin > 1e-9
    centers, idx = kmeans_plusplus(_dataset(x, parts), k, random_state=seed,
                                   n_local_trials=L)
    assert idx.dtype == np.int64 and np.array_equal(idx, want)
    assert centers.dtype == np.float64
    assert np.array_equal(centers, x[want].astype(np.float64))


def test_fewer_distinct_rows_than_k_and_non_finite():
    x = np.tile(np.array([[0.0, 1.0], [2.0, 3.0], [5.0, 5.0]]), (20, 1))
    _, idx = kmeans_plusplus(_dataset(x, 1), 6, random_state=0)
    assert idx.shape == (6,) and ((idx >= 0) & (idx < 60)).all()
    assert len(np.unique(x[idx[:3]], axis=0)) == 3
    x[7, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        kmeans_plusplus(_dataset(x, 1), 3, random_state=0)


def test_kmeans_init_equals_lloyd_from_those_centres(monkeypatch):
    x, _ = _blobs(7)
    want, margin = kpp_ref.kpp_ref(x, 9, 3)
    assert margin > 1e-9
    ds = _dataset(x, 3)
    # sums="reference": the Lloyd sums whose bits repeat from run to run
    km = KMeans(n_clusters=9, random_state=3, max_iter=5, init="k-means++",
                sums="reference")
    km.fit_predict(ds)
    assert np.array_equal(km.init_indices_, want)
    monkeypatch.setattr(kmeans_mod, "_init_centers", lambda *a: x[want].copy())
    ds2 = _dataset(x, 3)
    km2 = KMeans(n_clusters=9, random_state=3, max_iter=5, sums="reference")
    km2.fit_predict(ds2)
    assert km2.init_indices_ is None and km.n_iter == km2.n_iter
    assert np.array_equal(km.centers, km2.centers)
    assert np.array_equal(ds.labels_int32(), ds2.labels_int32())


@pytest.mark.parametrize("seed", [0, 1])
def test_one_initial_centre_in_every_blob(seed):
    x, blob = _blobs(seed)
    want, margin = kpp_ref.kpp_ref(x, 6, seed)
    assert margin > 1e-9 and sorted(blob[want]) == list(range(6))
    _, idx = kmeans_plusplus(_dataset(x, 1), 6, random_state=seed)
    assert sorted(blob[idx]) == list(range(6))
    # the default init: every centre of the unit cube is nearest to one blob
    rand = kmeans_mod._init_centers(2, False, 6, seed)
    near = ((x[None] - rand[:, None]) ** 2).sum(axis=2).argmin(axis=1)
    assert len(set(blob[near])) < 6
