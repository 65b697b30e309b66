"""GPU tests of KMeans(sums="reference"): centres bit-identical to the
reference's golden vectors, and the kernels behind it (dkm_ordered_sums_*,
dkm_merge_tree) against numpy's sequential ``np.add.at`` per Subset and the
oracle's ``merge_tree``.

The grouping tile of dkm_ordered.hip is T = 2048 rows (ORD_T): the kernel
tests cut Subsets of T - 1, T, T + 1 and 2 T + 1 rows besides ragged ones
with an empty and a one-row Subset."""
import hashlib

import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.datasets import make_blobs

from oracle import kmeans_oracle as orc
from tests.conftest import load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

T = 2048
LAYOUTS = {
    "ragged": [700, 0, 1, 1300, 50, 2100, 849],          # n = 5000
    "tiles": [T - 1, T, T + 1, 2 * T + 1],
}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _km(**kw):
    from dislib_amd.cluster import KMeans
    return KMeans(sums="reference", **kw)


def _load(x, n, y=None):
    from dislib_amd.data import load_data
    return load_data(x, subset_size=n, y=y)


def _labels(ds):
    return np.asarray(ds.labels.astype(np.int64))


# ---------------------------------------------------------------------------
# the reference's golden fits: centres with ==
# ---------------------------------------------------------------------------
def test_f01_toy_integer_samples():
    from dislib_amd.data import Dataset, Subset
    g = load_golden("f01_toy")
    ds = Dataset(n_features=2)
    ds.append(Subset(np.array([[1, 2], [2, 1]])))
    ds.append(Subset(np.array([[-1, -2], [-2, -1]])))
    km = _km(n_clusters=2, random_state=666)
    km.fit(ds)
    assert np.array_equal(km.centers, g["centers"])
    assert (km.centers == np.array([[1.5, 1.5], [-1.5, -1.5]])).all()
    assert km.n_iter == g["n_iter"]


def test_f03_blobs610():
    g = load_golden("f03_blobs610")
    ds = _load(g["x"], 300)
    km = _km(n_clusters=3, random_state=170)
    km.fit_predict(ds)
    assert np.array_equal(km.centers, g["centers"])
    assert np.array_equal(_labels(ds), g["labels"])
    assert km.n_iter == g["n_iter"]


@pytest.mark.parametrize("name,n,d,blobs,box,rs,sub,k,iters", [
    ("f04_c1mini", 20000, 50, 10, None, 0, 2000, 10, 5),
    ("f05_c2mini", 20000, 32, 100, (-10, 10), 1, 5000, 100, 3),
    ("f06_c3mini", 10000, 64, 50, (-10, 10), 2, 5000, 1000, 2),
])
def test_config_minis(name, n, d, blobs, box, rs, sub, k, iters):
    g = load_golden(name)
    kw = dict(n_samples=n, n_features=d, centers=blobs, random_state=rs)
    if box is not None:
        kw["center_box"] = box
    x, _ = make_blobs(**kw)
    assert hashlib.sha256(x.tobytes()).hexdigest() == str(g["x_sha"])
    ds = _load(x, sub)
    km = _km(n_clusters=k, max_iter=iters, tol=0, random_state=0)
    km.fit_predict(ds)
    assert km.n_iter == g["n_iter"]
    assert np.array_equal(_labels(ds), g["labels"])
    assert np.array_equal(km.centers, g["centers"])


def test_f09_empty_clusters():
    g = load_golden("f09_empty")
    ds = _load(g["x"], 50)
    km = _km(n_clusters=6, max_iter=4, random_state=9)
    km.fit_predict(ds)
    assert np.array_equal(_labels(ds), g["labels"])
    assert np.array_equal(km.centers, g["centers"])
    assert km.n_iter == g["n_iter"]


def test_f10_fp32_chain_and_merge():
    g = load_golden("f10_fp32")
    ds = _load(g["x"], 500)
    km = _km(n_clusters=4, max_iter=5, tol=0, random_state=3)
    km.fit_predict(ds)
    assert np.array_equal(_labels(ds), g["labels"])
    assert np.array_equal(km.centers, g["centers"])
    assert km.n_iter == g["n_iter"]


def test_f11_iteration_rules():
    g = load_golden("f11_iters")
    ds = _load(g["x"], 100)
    km = _km(n_clusters=3, max_iter=0, random_state=11)
    km.fit(ds)
    assert km.n_iter == 1 == g["n_iter_max0"]
    assert np.array_equal(km.centers, g["centers_max0"])
    km = _km(n_clusters=3, max_iter=50, tol=1e-1, random_state=11)
    km.fit(ds)
    assert km.n_iter == g["n_iter_tol"]
    assert np.array_equal(km.centers, g["centers_tol"])
    assert ds.labels is None


@pytest.mark.parametrize("arity", [50, 2])
def test_f13_arity_tree_over_120_subsets(arity):
    g = load_golden("f13_arity")
    ds = _load(g["x"], 50)
    assert len(ds) == 120
    km = _km(n_clusters=6, max_iter=4, tol=0, arity=arity, random_state=13)
    km.fit_predict(ds)
    assert np.array_equal(_labels(ds), g["labels_a%d" % arity])
    assert np.array_equal(km.centers, g["centers_a%d" % arity])
    assert km.n_iter == len(g["trace_a%d" % arity])


def test_f14_preloaded_labels():
    g = load_golden("f14_prelabels")
    ds = _load(g["x"], 100, y=g["y"].copy())
    km = _km(n_clusters=3, random_state=14)
    km.fit_predict(ds)
    lab = ds.labels
    assert str(lab.dtype) == str(g["labels_dtype"])
    assert np.array_equal(lab, g["labels"])
    assert np.array_equal(km.centers, g["centers"])


def test_arity_one_raises_instead_of_looping():
    g = load_golden("f09_empty")
    with pytest.raises(ValueError, match="arity"):
        _km(n_clusters=6, arity=1, random_state=9).fit(_load(g["x"], 50))


# ---------------------------------------------------------------------------
# determinism, and consistency with the default order
# ---------------------------------------------------------------------------
def test_f05_run_to_run_identical_and_close_to_fast():
    from dislib_amd.cluster import KMeans
    x, _ = make_blobs(n_samples=20000, n_features=32, centers=100,
                      center_box=(-10, 10), random_state=1)
    kw = dict(n_clusters=100, max_iter=3, tol=0, random_state=0)
    cen = []
    for _ in range(2):
        km = _km(**kw)
        km.fit(_load(x, 5000))
        cen.append(km.centers.copy())
    assert cen[0].tobytes() == cen[1].tobytes()
    fast = KMeans(sums="fast", **kw)
    fast.fit(_load(x, 5000))
    err = np.max(np.abs(fast.centers - cen[0]) /
                 np.maximum(np.abs(cen[0]), 1.0))
    print("fast vs reference: max rel err %.3g" % err)
    assert err <= 1e-9


# ---------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------
def test_csr_is_not_implemented():
    rng = np.random.default_rng(0)
    xs = sp.random(200, 30, density=0.2, format="csr", random_state=rng)
    with pytest.raises(NotImplementedError, match="dense"):
        _km(n_clusters=4, random_state=0).fit(_load(xs, 50))


def test_partials_beyond_hbm_headroom_raise(monkeypatch):
    from dislib_amd import _device
    g = load_golden("f09_empty")
    ds = _load(g["x"], 50)
    ds._device_data()                   # the upload itself is not capped
    monkeypatch.setattr(_device, "_IMAGE_HEADROOM", 1 << 62)
    with pytest.raises(ValueError, match="GiB.*larger Subsets"):
        _km(n_clusters=6, random_state=9).fit(ds)


# ---------------------------------------------------------------------------
# the kernels against np.add.at per Subset
# ---------------------------------------------------------------------------
def _case_data(layout, d, k, dtype, seed):
    sizes = LAYOUTS[layout]
    n = sum(sizes)
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) *
         10.0 ** rng.uniform(-8, 8, (n, d))).astype(dtype)
    lab = rng.integers(0, k, n).astype(np.int32)
    if dtype == np.float32 and k > 1:
        # the last cluster's rows are fp32 subnormals: a flushed add gives 0
        sub = lab == k - 1
        x[sub] = (rng.standard_normal((int(sub.sum()), d)) *
                  1e-40).astype(np.float32)
    lab[::53] = -1
    lab[7::61] = k
    return sizes, x, lab


def _ref_partials(sizes, x, lab, k, perm=False, rng=None):
    """[(sums (k, d) in x's dtype, counts int64)] per Subset: np.add.at is
    the sequential chain in row order (oracle.partial_sum)."""
    out, lo = [], 0
    for s in sizes:
        rows = np.arange(lo, lo + s)
        if perm:
            rows = rng.permutation(rows)
        rows = rows[(lab[rows] >= 0) & (lab[rows] < k)]
        sums = np.zeros((k, x.shape[1]), dtype=x.dtype)
        np.add.at(sums, lab[rows], x[rows])
        out.append((sums, np.bincount(lab[rows], minlength=k).astype(
            np.int64)))
        lo += s
    return out


CASES = [("ragged", d, k, np.float64) for d in (1, 3, 32, 33, 64, 130)
         for k in (1, 2, 100, 1000)]
CASES += [("ragged", d, k, np.float32) for d, k in
          ((1, 2), (3, 100), (32, 100), (33, 1000), (64, 2), (130, 100))]
CASES += [("tiles", 32, 100, np.float64), ("tiles", 1, 1000, np.float64),
          ("tiles", 33, 2, np.float32), ("tiles", 130, 1, np.float64)]


@pytest.mark.parametrize("layout,d,k,dtype", CASES)
def test_ordered_sums_and_merge_vs_numpy(layout, d, k, dtype):
    from dislib_amd import _device, _shard
    from dislib_amd.data import Dataset, Subset
    sizes, x, lab = _case_data(layout, d, k, dtype, seed=d * 1000 + k)
    n, S = len(x), len(sizes)
    ref = _ref_partials(sizes, x, lab, k)
    # not vacuous: another row order gives other bits on the CPU already
    if n // max(k, 1) > 2:
        other = _ref_partials(sizes, x, lab, k, True,
                              np.random.default_rng(1))
        assert any(not np.array_equal(a[0], b[0])
                   for a, b in zip(ref, other))
        assert all(np.array_equal(a[1], b[1]) for a, b in zip(ref, other))
    if dtype == np.float32 and k > 1:
        tiny = np.concatenate([r[0][k - 1] for r in ref])
        assert np.any((tiny != 0) & (np.abs(tiny) < np.finfo(np.float32).tiny))
    ds = Dataset(n_features=d)
    lo = 0
    for s in sizes:
        ds.append(Subset(x[lo:lo + s]))
        lo += s
    dd = ds._device_data()
    assert dd.dtype == dtype and dd.n == n
    arity = 3
    sched, n_ops, n_slots = _shard.merge_schedule(S, arity)
    with _device.on(dd.device):
        osum = _device.OrderedSums(dd, k, 0, S, sched, n_ops, n_slots)
        labels = torch.from_numpy(lab).to(dd.device)
        acc = torch.full((k * (d + 1),), np.nan, dtype=torch.float64,
                         device=dd.device)
        osum.partials.fill_(np.nan)        # every element must be written
        _device.ordered_sums(dd, labels, osum)
        _device.merge_tree(osum, acc, dtype == np.float32)
        got = osum.partials.cpu().numpy().reshape(S, k * (d + 1))
        order = osum.group_order(n).cpu().numpy()
        root = acc.cpu().numpy()
    for s in range(S):
        assert np.array_equal(got[s, :k * d].reshape(k, d),
                              ref[s][0].astype(np.float64)), s
        assert np.array_equal(got[s, k * d:], ref[s][1].astype(np.float64))
    assert not (np.signbit(got) & (got == 0)).any()   # no -0.0 in a partial
    # stable grouping by (Subset, label), labels outside [0, k) last
    subset = np.repeat(np.arange(S), sizes)
    bins = np.where((lab >= 0) & (lab < k), lab, k)
    assert np.array_equal(order, np.argsort(subset * (k + 1) + bins,
                                            kind="stable"))
    want_s, want_c = orc.merge_tree(ref, arity)
    assert np.array_equal(root[:k * d].reshape(k, d),
                          want_s.astype(np.float64))
    assert np.array_equal(root[k * d:], want_c.astype(np.float64))


def test_group_order_is_the_stable_argsort():
    """Valid labels only: the group order is np.argsort(subset * k + label,
    kind="stable")."""
    from dislib_amd import _device, _shard
    from dislib_amd.data import Dataset, Subset
    sizes, k, d = [T + 1, 3, 0, 2 * T + 5, 64, 65], 37, 2
    n = sum(sizes)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, d))
    lab = rng.integers(0, k, n).astype(np.int32)
    lab[:T + 1] = 4                       # one label over a tile boundary
    ds = Dataset(n_features=d)
    lo = 0
    for s in sizes:
        ds.append(Subset(x[lo:lo + s]))
        lo += s
    dd = ds._device_data()
    with _device.on(dd.device):
        osum = _device.OrderedSums(dd, k, 0, len(sizes),
                                   *_shard.merge_schedule(len(sizes), 50))
        _device.ordered_sums(dd, torch.from_numpy(lab).to(dd.device), osum)
        order = osum.group_order(n).cpu().numpy()
    subset = np.repeat(np.arange(len(sizes)), sizes)
    assert np.array_equal(order, np.argsort(subset * k + lab, kind="stable"))
