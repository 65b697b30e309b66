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


    # n = 20,000 is 313 tiles in three partitions of 105: two ballot rounds,
    # the second with 41 of its 64 lanes live.  The prune must not change a
    # label.
    from dislib_amd.cluster import dbscan as mod
    got = ds.labels_int32()
    off, n_off = mod._fit_device(x, 0.2, 5, [0, 1], flags=_lib.DBSCAN_NOPRUNE)
    assert np.array_equal(got, off.cpu().numpy())
    assert est.n_clusters == int(n_off)
    assert int(got.max()) == est.n_clusters - 1 and int(got.min()) == -1


# ---------------------------------------------------------------------------
# Every dispatch edge of dkm_dbscan.hip ("Dispatch edges").

def _device_fit(x, eps, ms, flags=0):
    from dislib_amd.cluster import dbscan as mod
    xd = x if torch.is_tensor(x) else torch.from_numpy(x).cuda()
    lab, ncl = mod._fit_device(xd, eps, ms, list(range(xd.shape[1])),
                               flags=flags)
    return lab.cpu().numpy().astype(np.int64), int(ncl)


def _prune_on_and_off(x, eps, ms, want, ncl):
    from dislib_amd import _lib
    xd = torch.from_numpy(x).cuda()
    for flags in (0, _lib.DBSCAN_NOPRUNE):
        got, n = _device_fit(xd, eps, ms, flags)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (flags, bad[:8], got[bad[:8]], want[bad[:8]])
        assert n == ncl, flags


_PARTS = {}


def _parts(key, make, eps, ms):
    """(x, dbscan_parts(x)) of a seeded dataset, computed once."""
    if key not in _PARTS:
        x = make()
        _PARTS[key] = x, ref.dbscan_parts(x, eps, ms)
    return _PARTS[key]


def _assert_not_degenerate(p):
    """On the reference's output, so no input passes vacuously."""
    assert p.n_clusters >= 2
    assert np.count_nonzero(p.labels == -1) >= 1
    assert np.count_nonzero(~p.core & (p.labels >= 0)) >= 1


# eps = c * sqrt(d): three blobs of std 0.25 (pair distances about
# 0.35 sqrt(d)) plus uniform noise, c fixed where the CPU reference finds
# the blobs, leaves the uniform rows noise and has border rows
BUCKET_EPS = {1: 0.1, 7: 0.25, 8: 0.25, 9: 0.25, 16: 0.25, 17: 0.25,
              32: 0.3, 33: 0.3, 64: 0.3, 65: 0.3, 128: 0.32, 129: 0.32}


@pytest.mark.parametrize("d", sorted(BUCKET_EPS))
def test_every_feature_bucket(d):
    """k_db_pair<8|16|32|64|0> on both sides of every boundary, the last
    also across pw_sum's 128; n = 600 is 10 tiles in two partitions."""
    eps = BUCKET_EPS[d] * np.sqrt(d)
    x, p = _parts(("bucket", d), lambda: ref.blobs_noise(
        d, n_blob=540, n_noise=60, d=d, centers=3, std=0.25), eps, 5)
    assert x.shape == (600, d)
    _assert_not_degenerate(p)
    _prune_on_and_off(x, eps, 5, p.labels, p.n_clusters)


def _beyond_box(kind):
    """600 x 24: three blobs of std 0.25 and 60 uniform rows that differ in
    features 16..23 only ("high": the boxes of features 0..15 see nothing of
    it), the same with features 0..15 all 1.5 ("const": boxes of no extent),
    or that differ in features 0..15 only ("low")."""
    rng = np.random.default_rng(24)
    n, d = 600, 24
    which = rng.integers(0, 3, n)
    x = 0.25 * rng.standard_normal((n, d))
    lo, hi = (0, 16) if kind == "low" else (16, 24)
    c = rng.uniform(-4, 4, (3, hi - lo))
    x[:, lo:hi] += c[which]
    x[540:, lo:hi] = rng.uniform(-5, 5, (60, hi - lo))
    if kind == "const":
        x[:, :16] = 1.5
    return np.ascontiguousarray(x[rng.permutation(n)])


@pytest.mark.parametrize("kind,eps", [("high", 1.4), ("const", 0.7),
                                      ("low", 1.4)])
def test_features_beyond_the_box(kind, eps):
    x, p = _parts(("box", kind), lambda: _beyond_box(kind), eps, 5)
    _assert_not_degenerate(p)
    _prune_on_and_off(x, eps, 5, p.labels, p.n_clusters)


def test_many_clusters_across_scan_chunks():
    """750 clusters whose first rows spread over 5,250 rows: the rank of a
    cluster is carried over six chunks of k_db_scan (12 partitions)."""
    x, want, ncl = ref.islands(1500, 11)
    assert x.shape == (5250, 2) and ncl == 750
    first = np.array([np.flatnonzero(want == c)[0] for c in (0, 749)])
    assert first[0] < 1024 and first[1] >= 4096
    rl, rn = ref.dbscan_ref(x, ref.ISLANDS_EPS, ref.ISLANDS_MS)
    assert np.array_equal(want, rl) and ncl == rn
    xd = torch.from_numpy(x).cuda()
    runs = [_device_fit(xd, ref.ISLANDS_EPS, ref.ISLANDS_MS)
            for _ in range(3)]
    for got, n in runs:
        assert np.array_equal(got, want) and n == ncl
    assert runs[0][0].tobytes() == runs[1][0].tobytes() == \
        runs[2][0].tobytes()


def test_two_ballot_rounds():
    """n = 16,450: 258 tiles, three partitions of 86, so the second round's
    ballot has 22 live lanes."""
    x, want, ncl = ref.islands(4700, 12)
    assert x.shape == (16450, 2) and ncl == 2350
    _prune_on_and_off(x, ref.ISLANDS_EPS, ref.ISLANDS_MS, want, ncl)


@pytest.mark.parametrize("n", [1024, 1025, 3000])
def test_scan_edges_every_row_a_cluster(n):
    """min_samples = 1 and no two rows within eps: every row is a cluster,
    numbered by itself -- the prefix sum at and past one chunk."""
    rng = np.random.default_rng(n)
    g = np.arange(64.0)
    x = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    x = np.ascontiguousarray(x[rng.permutation(len(x))[:n]])
    got, ncl = _device_fit(x, 0.9, 1)         # the nearest rows are 1 apart
    assert np.array_equal(got, np.arange(n)) and ncl == n


def test_union_find_every_pair_unions():
    """4,096 rows within eps of each other, 16 partitions: every thread
    unions with every earlier row at once."""
    x = np.random.default_rng(13).uniform(0.0, 1.0, (4096, 2))
    _prune_on_and_off(x, 2.0, 5, np.zeros(4096, np.int64), 1)


@pytest.mark.parametrize("bridge", [True, False])
def test_union_find_two_cliques(bridge):
    x, want, ncl = ref.two_cliques(2000, bridge, 14)
    assert ncl == (1 if bridge else 2)
    _prune_on_and_off(x, ref.CLIQUES_EPS, ref.CLIQUES_MS, want, ncl)


@pytest.mark.parametrize("ms,one", [(0, True), (1, True), (130, True),
                                    (131, False), (2 ** 40, False)])
def test_min_samples_edges(ms, one):
    """130 rows all within eps: one cluster up to min_samples = n, noise
    beyond (the kernels clamp min_samples to 2^31 - 1)."""
    x = ref.blobs_noise(15, n_blob=110, n_noise=20)
    got, ncl = _device_fit(x, 50.0, ms)
    assert ncl == (1 if one else 0)
    assert (got == (0 if one else -1)).all()


def test_duplicate_rows():
    x = np.concatenate([np.full((200, 2), 0.25), np.full((3, 2), 9.0)])
    want = np.array([0] * 200 + [-1] * 3)
    _prune_on_and_off(x, 0.5, 4, want, 1)
    x = x[np.random.default_rng(16).permutation(203)]
    want = np.where(x[:, 0] < 1.0, 0, -1)
    _prune_on_and_off(x, 0.5, 4, want, 1)


def test_duplicated_border_row():
    """Five copies of a border row that sees one core row of a group of
    nine: 5 + 1 neighbours stay below min_samples = 8, and every copy gets
    that core's label."""
    ring = 0.1 * np.array([[1, 0], [-1, 0], [0, 1], [0, -1], [.7, .7],
                           [-.7, .7], [.7, -.7], [-.7, -.7]])
    far = ring + [5.0, 5.0]
    x = np.concatenate([far, [[5.0, 5.0]], [[0.62, 0.0]] * 2, [[0.0, 0.0]],
                        ring, [[0.62, 0.0]] * 3])
    p = ref.dbscan_parts(x, 0.55, 8)
    copies = np.flatnonzero(x[:, 0] == 0.62)
    assert len(copies) == 5 and not p.core[copies].any()
    assert (p.labels[copies] == 1).all() and p.n_clusters == 2
    assert (p.attach[copies] == 12).all()     # ring's (0.1, 0)
    _prune_on_and_off(x, 0.55, 8, p.labels, p.n_clusters)


def test_nan_sample_raises():
    x = ref.blobs_noise(4, n_blob=50, n_noise=5)
    x[17, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        _fit(x, 0.3, 5)
