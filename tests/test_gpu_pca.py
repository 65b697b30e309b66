"""GPU tests of PCA (dkm_pca.hip, dislib_amd.decomposition) against numpy in
``np.longdouble`` built from the same inputs; u = 2^-53, eps = 2^-52.

Gram kernel: every entry of G against ``sum_r a_ri a_rj`` with
``a = [x - p | 1]`` in longdouble, within the forward bound of a recursively
summed dot product, ``B_ij = (n + 8) u sum_r |a_ri| |a_rj|``.  Projection:
``(d + 8) u sum_f |x_f - m_f| |v_f|``.

Estimator.  With s = column d of G, ``cov = (G[:d,:d] - s s^T / n) / (n - 1)``
on the host carries B through: ``E_ij = (B_ij + (B_id |s_j| + |s_i| B_jd) / n
+ 4 u (|S_ij| + |s_i s_j| / n)) / (n - 1)`` (the four roundings of outer,
divide, subtract, divide).  Eigenvalues move by at most ``||E||_F`` (Weyl) plus
eigh's own ``64 d eps ||C||_F``; eigenvector k by ``(4 ||E||_F + 64 d eps
||C||_F) / gap_k``; ``mean_ = p + s / n`` by ``B_id / n + 4 u (|p| + |s| / n)``.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from dislib_amd import _device
from dislib_amd.cluster import KMeans
from dislib_amd.data import Dataset, Subset
from dislib_amd.decomposition import PCA

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LD = np.longdouble
U, EPS = 2.0 ** -53, 2.0 ** -52
R = _device.PCA_CHUNK_ROWS
DTYPES = [np.float64, np.float32]
# (n, d, padding columns): da across a 16-column tile and a 64-column panel
# (d = 64: the second panel is the ones column alone), three panels; fewer
# rows than an MFMA step / a slab; one chunk, two, more than the 16 slices
GRAM = [(37, d, 3) for d in (1, 15, 16, 63, 64, 130)] + \
       [(n, 15, 3) for n in (1, 3, 17)] + [(3, 130, 0), (R, 5, 0),
                                           (R + 1, 5, 3), (16 * R + 1, 5, 3)]


def _dd(n, d, pad, dtype, rng, loc=0.0):
    """Rows of a wider device matrix (NaN in the padding and past row n)."""
    buf = np.full((n + 2, d + pad), np.nan, dtype=dtype)
    buf[:n, :d] = (rng.standard_normal((n, d)) + loc).astype(dtype)
    X = torch.from_numpy(buf).cuda()[:n, :d]
    dd = SimpleNamespace(X=X, n=n, d=d, dtype=dtype, device=X.device)
    return dd, buf[:n, :d].astype(LD)


def _gram_ref(x, p):
    """(G, B) of the module docstring for longdouble rows x and pivot p."""
    n = x.shape[0]
    a = np.concatenate([x - p.astype(LD), np.ones((n, 1), LD)], axis=1)
    return a.T @ a, (n + 8) * U * (np.abs(a).T @ np.abs(a))


def _cov_ref(x, p):
    """(mean, cov, E, mean bound) in longdouble."""
    n, d = x.shape
    G, B = _gram_ref(x, p)
    s, S = G[:d, d], G[:d, :d]
    ss = np.abs(np.outer(s, s)) / n
    E = (B[:d, :d] + (np.outer(B[:d, d], np.abs(s)) +
                      np.outer(np.abs(s), B[:d, d])) / n +
         4 * U * (np.abs(S) + ss)) / (n - 1)
    mb = B[:d, d] / n + 4 * U * (np.abs(p) + np.abs(s) / n)
    return p + s / n, (S - np.outer(s, s) / n) / (n - 1), E, mb


def _fro(m):
    return float(np.sqrt((m * m).sum()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,pad", GRAM)
def test_gram(n, d, pad, dtype):
    assert [_device.pca_chunks(m, 5) for m in (R, R + 1, 16 * R + 1)] == \
        [1, 2, 17]
    dd, x = _dd(n, d, pad, dtype, np.random.default_rng(100 * n + d))
    p = _device.pca_pivot(dd)
    G = _device.pca_gram(dd, p).cpu().numpy()
    ref, B = _gram_ref(x, p.cpu().numpy())
    assert G[d, d] == n and np.array_equal(G, G.T)
    assert np.all(np.abs(G - ref) <= B), float((np.abs(G - ref) / B).max())
    assert G.tobytes() == _device.pca_gram(dd, p).cpu().numpy().tobytes()


def test_pivot_keeps_the_variances():
    """Mean 1e6, spread 1: without the shift the update of the scatter would
    lose about eight more digits than the bound allows."""
    n, d = 5000, 5
    x = np.random.default_rng(7).standard_normal((n, d)) + 1e6
    ds = Dataset(n_features=d)
    ds.append(Subset(x))
    pca = PCA()
    pca.fit(ds)
    p = _device.pca_pivot(ds._device_data()).cpu().numpy()
    _, cov, E, _ = _cov_ref(x.astype(LD), p)
    lam = np.linalg.eigvalsh(cov.astype(np.float64))[::-1]
    tol = _fro(E) + 64 * d * EPS * _fro(cov)
    assert tol < 1e-9
    assert np.all(np.abs(pca.explained_variance_ - lam) <= tol)


def _signed(v):
    big = np.argmax(np.abs(v), axis=1)
    return v * np.where(v[np.arange(len(v)), big] < 0, -1.0, 1.0)[:, None]


@pytest.mark.parametrize("d,nc,sizes", [
    (3, None, (150, 1, 149)), (3, 1, (7, 293)), (65, None, (100, 300)),
    (65, 1, (399, 1)), (65, 17, (130, 20, 250))])
def test_estimator(d, nc, sizes):
    """X = Z diag(scales) Q^T + offset with Z's sample covariance the identity
    (centred, orthonormalised), so the spectrum is scales^2 = 0.95^k."""
    rng = np.random.default_rng(d)
    n = sum(sizes)
    z = rng.standard_normal((n, d))
    z = np.linalg.qr(z - z.mean(0))[0] * np.sqrt(n - 1)
    q = np.linalg.qr(rng.standard_normal((d, d)))[0]
    x = z * 0.95 ** (np.arange(d) / 2) @ q.T + 10 * rng.standard_normal(d)
    ds = Dataset(n_features=d)
    for a, b in zip(np.cumsum((0,) + sizes[:-1]), np.cumsum(sizes)):
        ds.append(Subset(x[a:b]))
    pca = PCA(n_components=nc)
    pca.fit(ds)
    k = d if nc is None else nc
    p = _device.pca_pivot(ds._device_data()).cpu().numpy()
    mean, cov, E, mb = _cov_ref(x.astype(LD), p)
    cov64 = cov.astype(np.float64)
    lam, vec = np.linalg.eigh(cov64)
    lam, vec = lam[::-1], _signed(vec[:, ::-1].T)
    gap = np.minimum(np.diff(lam, prepend=np.inf) * -1,
                     np.diff(lam, append=-np.inf) * -1)
    assert np.all(gap >= 1e-3 * lam[0])          # a condition on the inputs
    tl = _fro(E) + 64 * d * EPS * _fro(cov)
    tv = (4 * _fro(E) + 64 * d * EPS * _fro(cov)) / gap
    tr = float(np.trace(cov))
    ttr = float(np.trace(E)) + d * U * tr
    assert pca.components_.shape == (k, d) and pca.mean_.shape == (d,)
    assert np.all(np.abs(pca.mean_ - mean) <= mb)
    assert np.all(np.abs(pca.explained_variance_ - lam[:k]) <= tl)
    assert np.all(np.abs(pca.explained_variance_ratio_ - lam[:k] / tr) <=
                  (tl + lam[:k] * ttr / tr) / tr + 4 * U)
    assert np.all(np.linalg.norm(pca.components_ - vec[:k], axis=1) <= tv[:k])
    big = np.argmax(np.abs(pca.components_), axis=1)
    assert np.all(pca.components_[np.arange(k), big] > 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,c", [(d, c) for d in (1, 17, 130)
                                 for c in sorted({1, 16, 17, d})])
def test_project(d, c, dtype):
    rng = np.random.default_rng(10 * d + c)
    mean, V = rng.standard_normal(d), rng.standard_normal((c, d))
    md, Vd = torch.from_numpy(mean).cuda(), torch.from_numpy(V).cuda()
    for n in (1, 63, 64, 65, 200):
        dd, x = _dd(n, d, 0 if d == 17 else 3, dtype, rng, loc=0.5)
        Y = _device.pca_project(dd, md, Vd).cpu().numpy()
        xc = x - mean.astype(LD)
        err = np.abs(Y - xc @ V.T.astype(LD))
        assert Y.shape == (n, c)
        assert np.all(err <= (d + 8) * U * (np.abs(xc) @ np.abs(V.T)))


@pytest.mark.parametrize("on_device", [True, False])
def test_dataset_contract(on_device):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((90, 6)) * np.arange(1, 7)
    xs = torch.from_numpy(x).cuda() if on_device else x
    ds = Dataset(n_features=6)
    for a, b in ((0, 50), (50, 51), (51, 90)):
        ds.append(Subset(xs[a:b], labels=np.arange(a, b)))
    pca = PCA(n_components=2)
    out = pca.fit_transform(ds)
    before = ds._device_data()
    kept = before.X.clone()
    out = pca.transform(ds)
    assert out is not ds and out.n_features == 2
    assert out.subsets_sizes() == ds.subsets_sizes() == [50, 1, 39]
    assert all(o.labels is s.labels for o, s in zip(out, ds))
    assert ds._device_data() is before and torch.equal(before.X, kept)
    assert all(s.samples.shape == (b - a, 6) for s, (a, b) in
               zip(ds, before.subset_slices()))
    img = out._device
    assert img is not None and out._device_data() is img
    assert img.X.dtype == torch.float64 and tuple(img.X.shape) == (90, 2)
    for s, (a, b) in zip(out, img.subset_slices()):
        assert isinstance(s.samples, torch.Tensor if on_device else np.ndarray)
        got = s.samples.cpu().numpy() if on_device else s.samples
        assert np.array_equal(got, img.X[a:b].cpu().numpy())
        if on_device:
            assert s.samples.data_ptr() == img.X[a:b].data_ptr()
    xc, vt = x.astype(LD) - pca.mean_, pca.components_.T.astype(LD)
    assert np.all(np.abs(img.X.cpu().numpy() - xc @ vt) <=
                  (6 + 8) * U * (np.abs(xc) @ np.abs(vt)))
    KMeans(n_clusters=3, random_state=0, max_iter=3).fit(out)
    again = PCA(n_components=2)
    again.fit(ds)
    for a in ("components_", "explained_variance_", "mean_"):
        assert getattr(pca, a).tobytes() == getattr(again, a).tobytes()
