"""GPU tests of ``dislib_amd.cluster.DBSCAN`` (dkm_dbscan.hip): labels and
``n_clusters`` equal tests/dbscan_ref.py element for element, and the
reference's own output (tests/golden/dbscan_ref.npz) where a golden exists.
"""
import os

import numpy as np
import pytest

from tests import dbscan_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden",
                         "dbscan_ref.npz"))
CASES = sorted({k.split("__")[0] for k in G.files})


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _fit(x, eps, ms, subset_size=None, **kw):
    """(labels int64[n], n_clusters, dataset) of a fit on ``x``."""
    from dislib_amd.cluster import DBSCAN
    from dislib_amd.data import load_data
    ds = load_data(x, subset_size=subset_size or max(1, len(x)))
    est = DBSCAN(eps=eps, min_samples=ms, **kw)
    assert est.fit(ds) is None
    assert ds._device_labels() is not None
    lab = ds.labels_int32()
    return lab.astype(np.int64), est.n_clusters, ds


def _check(x, eps, ms, **kw):
    want, ncl = ref.dbscan_ref(x, eps, ms)
    got, n, _ = _fit(x, eps, ms, **kw)
    assert np.array_equal(got, want)
    assert n == ncl
    return want, ncl


_REF = {}


def _golden_ref(name):
    if name not in _REF:
        _, eps, ms = G[name + "__meta"]
        _REF[name] = ref.dbscan_ref(G[name + "__x"], float(eps), int(ms))
    return _REF[name]


@pytest.mark.parametrize("setting", range(5))
@pytest.mark.parametrize("name", CASES)
def test_golden_cases(name, setting):
    sub, eps, ms = G[name + "__meta"]
    nr, mx, *dims = (int(v) for v in G[name + "__settings"][setting])
    dims = [c for c in dims if c >= 0]
    got, ncl, _ = _fit(G[name + "__x"], float(eps), int(ms), int(sub),
                       n_regions=nr, max_samples=None if mx < 0 else mx,
                       dimensions=dims or None)
    want, wncl = _golden_ref(name)
    assert np.array_equal(got, want) and ncl == wncl
    # the reference itself: every setting is its n_regions=1 clustering
    assert np.array_equal(got, G[name + "__labels_s0"])
    assert np.array_equal(
        got, ref.renumber(G["%s__labels_s%d" % (name, setting)]))
    assert ncl == int(G["%s__ncl_s%d" % (name, setting)])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_tile_edges(n):
    x = ref.blobs_noise(3, n_blob=120, n_noise=20)[:n]
    _check(x, 0.3, 3)


def test_ragged_subsets_and_an_empty_one():
    from dislib_amd.cluster import DBSCAN
    from dislib_amd.data import Dataset, Subset
    x = ref.blobs_noise(7)
    want, ncl = ref.dbscan_ref(x, 0.3, 5)
    cuts = [(0, 100), (100, 200), (200, 200), (200, 300), (300, 340)]
    ds = Dataset(n_features=2)
    for a, b in cuts:
        ds.append(Subset(samples=x[a:b]))
    est = DBSCAN(eps=0.3, min_samples=5)
    est.fit_predict(ds)
    assert ds._device_labels() is not None
    assert est.n_clusters == ncl
    for s, (a, b) in zip(ds, cuts):
        lab = np.asarray(s.labels).astype(np.int64)
        assert lab.shape == (b - a,)
        assert np.array_equal(lab, want[a:b])


def test_empty_dataset():
    from dislib_amd.cluster import DBSCAN
    from dislib_amd.data import Dataset, Subset
    ds = Dataset(n_features=3)
    ds.append(Subset(samples=np.zeros((0, 3))))
    ds.append(Subset(samples=np.zeros((0, 3))))
    est = DBSCAN(eps=0.5)
    est.fit(ds)
    assert est.n_clusters == 0
    for s in ds:
        assert np.asarray(s.labels).shape == (0,)


@pytest.mark.parametrize("d,eps", [(10, 1.6), (130, 5.5)])
def test_both_distance_paths(d, eps):
    rng = np.random.default_rng(d)
    c = rng.uniform(-3, 3, (3, d))
    x = c[rng.integers(0, 3, 300)] + 0.3 * rng.standard_normal((300, d))
    want, ncl = _check(x, eps, 5)
    assert ncl >= 1


@pytest.mark.parametrize("ms", [3, 5])
@pytest.mark.parametrize("eps", [1.0, np.nextafter(1.0, 2.0)])
def test_exactly_at_eps(eps, ms):
    """A 12 x 12 integer grid: distance 1 is out at eps = 1 and in one ulp
    above it."""
    g = np.arange(12.0)
    x = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    want, ncl = _check(x, float(eps), ms)
    if eps == 1.0:
        assert ncl == 0 and (want == -1).all()
    elif ms == 3:
        # (ms = 5: only the inner points are core, and every corner's two
        # neighbours are non-core edge points, so the corners are noise)
        assert ncl == 1 and (want == 0).all()


def _chain(n, y, rng):
    x = np.stack([0.9 * np.arange(n), np.full(n, y)], -1)
    return x[rng.permutation(n)]


def test_union_find_one_chain():
    x = _chain(2000, 0.0, np.random.default_rng(0))
    want, ncl = _check(x, 1.0, 2)
    assert ncl == 1 and (want == 0).all()


def test_union_find_two_chains_interleaved():
    rng = np.random.default_rng(1)
    a, b = _chain(2000, 0.0, rng), _chain(2000, 1.5, rng)
    x = np.empty((4000, 2))
    x[0::2], x[1::2] = a, b
    want, ncl = _check(x, 1.0, 2)
    assert ncl == 2
    assert (want[0::2] == 0).all() and (want[1::2] == 1).all()


def test_border_never_bridges():
    """Two 5-point core groups and one point within eps of a core of each:
    two clusters, the point with the nearer core."""
    grp = np.array([[0, 0], [.1, 0], [-.1, 0], [0, .1], [0, -.1]])
    left, right = grp + [0.0, 0.0], grp + [1.5, 0.0]
    # eps = 0.67: the point's neighbours are itself, left's (.1, 0) at 0.64
    # and right's (1.4, 0) at 0.66 -- three, so it is not core; the groups
    # are 1.3 apart
    mid = np.array([[0.74, 0.0]])
    x = np.concatenate([left, mid, right])
    want, ncl = _check(x, 0.67, 5)
    assert ncl == 2
    assert (want[:5] == 0).all() and want[5] == 0 and (want[6:] == 1).all()


@pytest.fixture(scope="module")
def spread():
    """5,000 x 3 blobs spread over many cells."""
    return ref.blobs_noise(5, n_blob=4600, n_noise=400, d=3, centers=12,
                           std=0.3, box=8.0)


def test_prune_on_and_off(spread):
    from dislib_amd import _lib
    from dislib_amd.cluster import dbscan as mod
    x = torch.from_numpy(spread).cuda()
    on, n_on = mod._fit_device(x, 0.35, 5, [0, 1, 2])
    off, n_off = mod._fit_device(x, 0.35, 5, [0, 1, 2],
                                 flags=_lib.DBSCAN_NOPRUNE)
    assert torch.equal(on, off) and int(n_on) == int(n_off)
    want, ncl = ref.dbscan_ref(spread, 0.35, 5)
    assert np.array_equal(on.cpu().numpy().astype(np.int64), want)
    assert int(n_on) == ncl and ncl > 1


def test_prune_data_in_one_cell():
    x = np.random.default_rng(2).uniform(0.0, 0.2, (300, 3))
    _check(x, 0.25, 4)


def test_eps_larger_than_the_extent():
    x = ref.blobs_noise(4, n_blob=260, n_noise=40)
    want, ncl = _check(x, 50.0, 5)
    assert ncl == 1 and (want == 0).all()


@pytest.mark.parametrize("eps", [0.0, -1.0])
def test_eps_not_positive_is_all_noise(eps):
    x = ref.blobs_noise(4, n_blob=100, n_noise=10)
    # (min_samples = 1 would make every lone sample a component of one, which
    # stays: the reference's rule)
    want, ncl = _check(x, eps, 2)
    assert ncl == 0 and (want == -1).all()


def test_fp32_samples():
    x = ref.blobs_noise(9).astype(np.float32)
    _check(x, 0.3, 5, subset_size=100)


def test_strided_rows():
    """Samples that are a column slice of a wider device tensor."""
    from dislib_amd.cluster import DBSCAN
    from dislib_amd.data import load_data
    x = ref.blobs_noise(10, d=3)
    wide = torch.zeros((len(x), 8), dtype=torch.float64, device="cuda")
    wide[:, 2:5] = torch.from_numpy(x).cuda()
    ds = load_data(wide[:, 2:5], subset_size=120)
    est = DBSCAN(eps=0.45, min_samples=5)
    est.fit(ds)
    want, ncl = ref.dbscan_ref(x, 0.45, 5)
    assert np.array_equal(ds.labels_int32().astype(np.int64), want)
    assert est.n_clusters == ncl


def test_determinism():
    from dislib_amd.cluster import dbscan as mod
    x = torch.from_numpy(ref.blobs_noise(7)).cuda()
    runs = [mod._fit_device(x, 0.3, 5, [0, 1])[0] for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def test_memory_is_linear():
    from dislib_amd import _lib
    from dislib_amd.cluster import DBSCAN
    from dislib_amd.data import load_data
    n, d = 20000, 2
    bound = 64 * n + 2 ** 20
    assert 0 < _lib.load().dkm_dbscan_workspace_bytes(n, d) <= bound
    x = torch.from_numpy(ref.blobs_noise(6, n_blob=18000, n_noise=2000,
                                         centers=10, box=10.0)).cuda()
    ds = load_data(x, subset_size=5000)
    ds._device_data()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    est = DBSCAN(eps=0.2, min_samples=5)
    est.fit(ds)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    # an n x n byte matrix alone would be 400 MB
    assert rise < bound + 2 * n * d * 8 + (16 << 20), rise
    assert est.n_clusters >= 1


def test_nan_sample_raises():
    x = ref.blobs_noise(4, n_blob=50, n_noise=5)
    x[17, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        _fit(x, 0.3, 5)
