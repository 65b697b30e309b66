"""CPU tests of the host-side surface of k-means++ seeding: every refusal is
raised before the GPU library is touched."""
import numpy as np
import pytest
import scipy.sparse as sp

from dislib_amd import _lib, _shard
from dislib_amd.cluster import KMeans, kmeans_plusplus
from dislib_amd.data import Dataset, load_data


@pytest.fixture
def no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the GPU library was touched")
    monkeypatch.setattr(_lib, "lib", boom)


DENSE = np.arange(12.0).reshape(6, 2)


@pytest.mark.parametrize("kwargs,exc", [
    (dict(n_clusters=0), ValueError),
    (dict(n_clusters=7), ValueError),
    (dict(n_clusters=2, n_local_trials=0), ValueError),
    (dict(n_clusters=2, n_local_trials=_lib.KPP_MAX_TRIALS + 1), ValueError),
    (dict(n_clusters=2, random_state=np.random.RandomState(0)), TypeError),
])
def test_argument_refusals(no_gpu, kwargs, exc):
    with pytest.raises(exc):
        kmeans_plusplus(load_data(DENSE, subset_size=3), **kwargs)


def test_data_refusals(no_gpu, monkeypatch):
    csr = load_data(sp.random(30, 5, density=0.3, format="csr",
                              random_state=0), subset_size=10)
    with pytest.raises(NotImplementedError, match="dense"):
        kmeans_plusplus(csr, 2)
    with pytest.raises(NotImplementedError, match="dense"):
        KMeans(n_clusters=2, init="k-means++").fit(csr)
    with pytest.raises(ValueError, match="empty"):
        kmeans_plusplus(Dataset(n_features=2), 1)
    monkeypatch.setattr(_shard, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="one rank"):
        kmeans_plusplus(load_data(DENSE, subset_size=3), 2)


def test_init_keyword():
    assert _lib.KPP_MAX_TRIALS == 32
    assert KMeans().init_indices_ is None and KMeans()._init == "random"
    assert KMeans(init="k-means++")._init == "k-means++"
    with pytest.raises(ValueError, match="init"):
        KMeans(init="bogus")
    with pytest.raises(TypeError):
        KMeans(8, 10, 1e-4, 50, None, False, "auto", None, "fast", "random")
