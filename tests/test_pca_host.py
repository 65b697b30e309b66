"""CPU tests of the host-side surface of PCA: every refusal that needs no
device is raised before the GPU library is touched."""
import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.exceptions import NotFittedError

import dislib_amd
from dislib_amd import _lib, _shard
from dislib_amd.data import load_data
from dislib_amd.decomposition import PCA

DENSE = np.arange(12.0).reshape(6, 2)


@pytest.fixture
def no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the GPU library was touched")
    monkeypatch.setattr(_lib, "lib", boom)


@pytest.mark.parametrize("x,kwargs,exc", [
    (sp.random(30, 5, density=0.3, format="csr", random_state=0), {},
     NotImplementedError),
    (DENSE[:1], {}, ValueError),
    (np.zeros((2, _lib.PCA_MAX_D + 1)), {}, ValueError),
    (DENSE, dict(n_components=0), ValueError),
    (DENSE, dict(n_components=3), ValueError),
    (DENSE, dict(n_components=1.5), ValueError),
])
def test_fit_refusals(no_gpu, x, kwargs, exc):
    with pytest.raises(exc):
        PCA(**kwargs).fit(load_data(x, subset_size=3))


def test_transform_and_world_refusals(no_gpu, monkeypatch):
    ds = load_data(DENSE, subset_size=4)
    pca = PCA()
    with pytest.raises(NotFittedError):
        pca.transform(ds)
    pca.mean_, pca.components_ = np.zeros(3), np.eye(3)
    with pytest.raises(ValueError, match="3 features"):
        pca.transform(ds)
    monkeypatch.setattr(_shard, "world", lambda: (0, 2))
    for call in (PCA().fit, PCA().fit_transform, pca.transform):
        with pytest.raises(NotImplementedError, match="one rank"):
            call(ds)


def test_constructor_and_alias():
    assert _lib.PCA_MAX_D == 4096
    pca = PCA(3, 7, device="cuda:0")
    assert (pca._n_components, pca._arity, pca._device) == (3, 7, "cuda:0")
    assert PCA()._n_components is None and PCA()._arity == 50
    for a in ("components_", "explained_variance_",
              "explained_variance_ratio_", "mean_"):
        assert getattr(pca, a) is None
    with pytest.raises(TypeError):
        PCA(3, 7, "cuda:0")
    dislib_amd.install_as_dislib()
    from dislib.decomposition import PCA as aliased
    assert aliased is PCA
