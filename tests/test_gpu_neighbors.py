"""GPU parity of the distance-primitive reuse rows, through
the C ABI (dkm_knn_f64, dkm_radius_count_f64 / dkm_radius_fill_f64):

* ``NearestNeighbors.kneighbors`` (reference neighbors/base.py:40-87)
  against the reference's own outputs (tests/golden/neighbors_ref.npz) and
  against the oracle's sequential restatement on larger seeded inputs:
  indices exact; distances bit-exact in sklearn's kd_tree regime (d <= 15,
  n_neighbors < n_fit // 2), within the GEMM expansion's rounding otherwise
  (|d^2 - d_ref^2| <= 1e-13 (|x|^2 + |y|^2)).
* DBSCAN ``_compute_neighbours`` (cluster/dbscan/classes.py:124-141):
  neighbour lists and core flags exact.
"""
import os

import numpy as np
import pytest

from oracle import neighbors_oracle as orc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden",
                         "neighbors_ref.npz"))
KNN = sorted({k.split("__")[0] for k in G.files if k.startswith("kn_")})
DB = sorted({k.split("__")[0] for k in G.files if k.startswith("db_")})


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _knn(xf, xq, sub, kn, subq=None):
    from dislib_amd.data import load_data
    from dislib_amd.neighbors import NearestNeighbors
    nn = NearestNeighbors(n_neighbors=kn)
    nn.fit(load_data(xf, subset_size=sub))
    return nn.kneighbors(load_data(xq, subset_size=subq or sub))


@pytest.mark.parametrize("name", KNN)
def test_kneighbors_reference_golden(name):
    sub, kn = (int(v) for v in G[name + "__meta"])
    xf, xq = G[name + "__xf"], G[name + "__xq"]
    d, i = _knn(xf, xq, sub, kn)
    assert i.dtype == np.int64 and d.dtype == np.float64
    assert np.array_equal(i, G[name + "__ind"])
    ref = G[name + "__dist"]
    if xf.shape[1] <= 15 and kn < sub // 2:
        assert np.array_equal(d, ref)
    else:
        scale2 = (xf ** 2).sum(1).max() + (xq ** 2).sum(1).max()
        assert np.max(np.abs(d ** 2 - ref ** 2)) <= 1e-13 * scale2


@pytest.mark.parametrize("nq,nx,d,kn,seed", [
    (3000, 5000, 3, 5, 0),       # many partitions, small k
    (1000, 20000, 16, 32, 1),    # largest k, d at the 16-register template
    (700, 3000, 70, 8, 2),       # d > 64: query read from memory
    (129, 300, 64, 1, 3),        # ragged last wave, one neighbour
    (64, 257, 9, 17, 4),         # k between templates (K = 32 slots)
    (500, 3000, 5, 33, 5),       # n_neighbors > 32: the two-scan path
    (300, 2000, 12, 100, 6),     # two scans again (passes: kn > 2048)
    (200, 700, 70, 64, 7),       # two scans, d > 64 (query from memory)
    (300, 20000, 5, 1000, 8),    # the two-scan path (32 < kn <= 2048)
    (130, 6144, 70, 2048, 9),    # its largest kn, d > 64
    (64, 1200, 3, 1200, 10),     # kn = nx: every row
])
def test_kneighbors_vs_oracle(nq, nx, d, kn, seed):
    rng = np.random.default_rng(seed)
    xf = rng.standard_normal((nx, d)) * rng.uniform(0.5, 3.0, d)
    xq = rng.standard_normal((nq, d)) * rng.uniform(0.5, 3.0, d)
    # (the reference fits sklearn per Subset: n_neighbors <= subset rows)
    dist, ind = _knn(xf, xq, max(1000, kn), kn, 250)
    od, oi = orc.kneighbors_exact(xf, xq, kn)
    assert np.array_equal(ind, oi)
    assert np.array_equal(dist, od)


def test_kneighbors_two_scan_overflow_falls_back():
    """Fit rows in distance order: the union of the partitions' top-32 lists
    gives a loose threshold, the candidate lists outgrow their cap and the
    call reruns in passes of 32 -- same result."""
    xf = np.arange(60000, dtype=np.float64)[:, None] * np.ones((1, 2))
    xq = np.array([[0.25, 0.0], [3.0, 3.0], [59999.0, 1.0]])
    dist, ind = _knn(xf, xq, 60000, 1000, 3)
    od, oi = orc.kneighbors_exact(xf, xq, 1000)
    assert np.array_equal(ind, oi) and np.array_equal(dist, od)


def test_kneighbors_ties_by_index():
    """Integer grid with duplicate points: equal distances rank by fit
    index (the reference's argsort merge does the same for the first
    occurrences it keeps)."""
    rng = np.random.default_rng(7)
    xf = rng.integers(0, 4, (600, 2)).astype(np.float64)
    xq = rng.integers(0, 4, (100, 2)).astype(np.float64)
    dist, ind = _knn(xf, xq, 600, 12, 100)
    od, oi = orc.kneighbors_exact(xf, xq, 12)
    assert np.array_equal(ind, oi) and np.array_equal(dist, od)


def test_kneighbors_closer_row_after_a_full_tie_group():
    """A full list of equal distances, then a closer row: the displaced
    entries carried down the list keep their index order, so the lowest
    index of the tie group survives (an insertion that only let empty slots
    take ties dropped it: [10, 1, 2, 3] instead of [10, 0, 1, 2])."""
    xf = np.zeros((40, 2))
    xf[:10, 0] = 1.0           # rows 0..9 at distance 1
    xf[10] = 0.0               # row 10 at distance 0
    xf[11:] = 5.0 + np.arange(29)[:, None]
    xq = np.zeros((3, 2))
    dist, ind = _knn(xf, xq, 40, 4, 3)
    assert ind.tolist() == [[10, 0, 1, 2]] * 3
    assert dist.tolist() == [[0.0, 1.0, 1.0, 1.0]] * 3
    od, oi = orc.kneighbors_exact(xf, xq, 4)
    assert np.array_equal(ind, oi)


def test_kneighbors_overflowed_distances_fill_the_list():
    """Fewer finite rows than n_neighbors: rows whose squared distance
    overflows to +inf still fill the list (sklearn returns them too), as
    real fit indices with distance inf, never a sentinel."""
    rng = np.random.default_rng(11)
    xf = rng.standard_normal((40, 3))
    xf[3:] = 1e200 * (1.0 + rng.random((37, 3)))   # (1e200)^2 = inf
    xq = rng.standard_normal((5, 3))
    dist, ind = _knn(xf, xq, 40, 8, 5)
    od, oi = orc.kneighbors_exact(xf[:3], xq, 3)
    assert np.array_equal(ind[:, :3], oi) and np.array_equal(dist[:, :3], od)
    assert np.all(np.isinf(dist[:, 3:]))
    assert np.all((ind[:, 3:] >= 3) & (ind[:, 3:] < 40))
    for row in ind:
        assert len(set(row.tolist())) == 8


def test_sparse_kneighbors_nan_distances_rank_last():
    """Finite data whose squares overflow: r = -2 inf + inf + inf = NaN.
    NaN ranks after +inf (numpy's argpartition / argsort order, which the
    reference's sklearn brute force uses), and such rows fill the list as
    real fit indices, never the INT32_MAX empty-slot sentinel."""
    import scipy.sparse as sp
    fd = np.zeros((6, 3))
    fd[0, 0] = 1e200            # with the query: inf - inf = NaN
    fd[1:, 1] = np.arange(1, 6)
    qd = np.zeros((2, 3))
    qd[:, 0] = 1e200
    mf, mq = sp.csr_matrix(fd), sp.csr_matrix(qd)
    gd, gi = _knn_csr(mf, mq, 6, 6, 2)
    f = (mf.indptr.astype(np.int64), mf.indices, mf.data)
    q = (mq.indptr.astype(np.int64), mq.indices, mq.data)
    od, oi = orc.kneighbors_csr(f, q, 6)
    assert np.array_equal(gi, oi)
    assert np.array_equal(gd, od, equal_nan=True)
    assert gi[:, -1].tolist() == [0, 0] and np.isnan(gd[:, -1]).all()
    assert np.isinf(gd[:, :-1]).all()


def test_kneighbors_return_indices_only_and_device_data():
    from dislib_amd.data import load_data
    from dislib_amd.neighbors import NearestNeighbors
    rng = np.random.default_rng(9)
    x = rng.random((500, 4))
    xt = torch.from_numpy(x).cuda()
    nn = NearestNeighbors(n_neighbors=3)
    nn.fit(load_data(xt, subset_size=100))
    ind = nn.kneighbors(load_data(x, subset_size=100), return_distance=False)
    assert np.array_equal(ind, orc.kneighbors_exact(x, x, 3)[1])


def test_kneighbors_argument_errors():
    from dislib_amd.data import load_data
    from dislib_amd.neighbors import NearestNeighbors
    x = np.random.default_rng(0).random((40, 3))
    nn = NearestNeighbors(n_neighbors=11)
    nn.fit(load_data(x, subset_size=10))
    with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
        nn.kneighbors(load_data(x, subset_size=10))
    with pytest.raises(ValueError, match="n_neighbors > 0"):
        nn.kneighbors(load_data(x, subset_size=10), n_neighbors=0)
    with pytest.raises(TypeError):
        nn.kneighbors(load_data(x, subset_size=10), n_neighbors=2.5)


def _eps_query(x, sub, eps, ms, b, e):
    from dislib_amd.cluster.dbscan import compute_neighbours
    from dislib_amd.data import load_data
    return compute_neighbours(eps, ms, False, b, e,
                              *list(load_data(x, subset_size=sub)))


@pytest.mark.parametrize("name", DB)
def test_epsilon_query_reference_golden(name):
    x = G[name + "__x"]
    sub, eps, ms, b, e = G[name + "__meta"]
    nl, cp = _eps_query(x, int(sub), eps, ms, int(b), int(e))
    off, ref = G[name + "__offsets"], G[name + "__neigh"]
    assert len(nl) == len(off) - 1
    for r, v in enumerate(nl):
        assert np.array_equal(v, ref[off[r]:off[r + 1]]), (name, r)
    assert cp == list(G[name + "__core"])


@pytest.mark.parametrize("n,d,eps,b,e,grid", [
    (3000, 5, 1.0, 100, 2900, False),
    (2000, 64, 11.0, 0, 2000, False),
    (500, 100, 14.0, 30, 480, False),   # d > 64: query read from memory
    (1500, 2, 1.5, 0, 1500, True),      # integer grid: many equal distances
    (6000, 2, 1e9, 0, 3, False),        # lists of 6000 (> LDS sort cap)
    (21000, 2, 1e9, 0, 3, True),        # 6 runs, 3 merge passes, ties
    (800, 2, 2.0, 0, 800, True),        # distances exactly eps (excluded)
    (300, 3, 0.0, 0, 300, True),        # eps = 0: no neighbours at all
    (300, 3, -1.0, 0, 300, False),      # negative eps: none either
])
def test_epsilon_query_vs_oracle(n, d, eps, b, e, grid):
    rng = np.random.default_rng(n + d)
    x = (rng.integers(0, 6, (n, d)).astype(np.float64) if grid
         else rng.standard_normal((n, d)))
    nl, cp = _eps_query(x, 250, eps, 4, b, e)
    onl, ocp = orc.compute_neighbours(eps, 4, b, e, x)
    assert len(nl) == len(onl)
    for r in range(len(nl)):
        assert np.array_equal(nl[r], onl[r]), r
    assert cp == ocp


# --- sparse epsilon query (classes.py:130, sparse=True) --------------------
from tests.test_neighbors_golden import (DBS, assert_same_up_to_ties,  # noqa
                                         sparse_case)


def _eps_query_csr(m, sub, eps, ms, b, e):
    from dislib_amd.cluster.dbscan import compute_neighbours
    from dislib_amd.data import load_data
    return compute_neighbours(eps, ms, True, b, e,
                              *list(load_data(m, subset_size=sub)))


@pytest.mark.parametrize("name", DBS)
def test_sparse_epsilon_query_reference_golden(name):
    import scipy.sparse as sp
    ip, ix, dv, shape, meta, off, ref, core = sparse_case(name)
    sub, eps, ms, b, e = meta
    m = sp.csr_matrix((dv, ix, ip), shape=tuple(shape))
    nl, cp = _eps_query_csr(m, int(sub), eps, ms, int(b), int(e))
    assert len(nl) == len(off) - 1
    for r, v in enumerate(nl):
        assert_same_up_to_ties(v, ref[off[r]:off[r + 1]], ip, ix, dv,
                               int(b) + r, (name, r))
    assert cp == list(core)


@pytest.mark.parametrize("n,d,dens,eps,b,e,kind", [
    (3000, 500, 0.02, 2.0, 100, 2900, "uniform"),   # ~10 nnz per row
    (2000, 8, 0.3, 2.0, 0, 2000, "grid"),           # ties on integer values
    (1200, 100000, 0.0001, 1.2, 0, 1200, "uniform"),  # mostly empty rows
    (5000, 8, 0.5, 1e9, 0, 3, "uniform"),           # lists of 5000 (> LDS)
    (600, 30, 0.2, 0.0, 0, 600, "grid"),            # eps = 0: none
    (600, 30, 0.2, 2.0, 0, 600, "unsorted"),        # unsorted column order
    (400, 20, 0.3, 3.0, 0, 400, "big"),             # 1e200: overflow -> inf
])
def test_sparse_epsilon_query_vs_oracle(n, d, dens, eps, b, e, kind):
    import scipy.sparse as sp
    rng = np.random.default_rng(n + d)
    rvs = {"grid": lambda k: rng.integers(1, 4, k).astype(np.float64),
           "big": lambda k: rng.choice([1.0, -2.0, 1e200], k)}.get(
        kind, lambda k: rng.uniform(-1, 1, k))
    m = sp.random(n, d, density=dens, format="csr", random_state=rng,
                  data_rvs=rvs)
    m.sort_indices()
    ip, ix, dv = m.indptr.astype(np.int64), m.indices, m.data
    if kind == "unsorted":  # same matrix, entries reversed within rows
        perm = np.concatenate([np.arange(ip[i + 1] - 1, ip[i] - 1, -1)
                               for i in range(n)]).astype(np.int64)
        m = sp.csr_matrix((dv[perm], ix[perm], ip), shape=m.shape)
        assert not m.has_sorted_indices
    nl, cp = _eps_query_csr(m, 250, eps, 4, b, e)
    onl, ocp = orc.compute_neighbours_csr(eps, 4, b, e, ip, ix, dv)
    assert len(nl) == len(onl)
    for r in range(len(nl)):
        assert np.array_equal(nl[r], onl[r]), r
    assert cp == ocp
    if kind == "grid" and eps > 0:
        assert sum(len(v) for v in nl) > n  # more than the points themselves


# --- sparse kneighbors (sklearn brute force on CSR Subsets) ---------------
from tests.test_neighbors_golden import (KNS, assert_knn_same_up_to_ties,  # noqa
                                         sp_matrix, sparse_knn_case)


def _knn_csr(mf, mq, sub, kn, subq=None, same=False):
    from dislib_amd.data import load_data
    from dislib_amd.neighbors import NearestNeighbors
    nn = NearestNeighbors(n_neighbors=kn)
    fds = load_data(mf, subset_size=sub)
    nn.fit(fds)
    return nn.kneighbors(fds if same else load_data(mq, subset_size=subq or sub))


@pytest.mark.parametrize("name", KNS)
def test_sparse_kneighbors_reference_golden(name):
    """Distances bit-exact against what the reference returned; indices
    equal up to the order of exactly equal distances."""
    f, q, d, sub, kn, dist, ind = sparse_knn_case(name)
    mf, mq = sp_matrix(f, d), sp_matrix(q, d)
    same = np.array_equal(f[0], q[0]) and np.array_equal(f[2], q[2]) and \
        np.array_equal(f[1], q[1])
    gd, gi = _knn_csr(mf, mq, sub, kn, same=same)
    assert gi.dtype == np.int64
    assert_knn_same_up_to_ties(gd, gi, dist, ind, name)
    f32 = f[2].dtype == np.float32
    assert gd.dtype == (np.float32 if f32 else np.float64)
    od, oi = orc.kneighbors_csr(f, q, kn, f32=f32)
    assert np.array_equal(gi, oi) and np.array_equal(gd, od)


@pytest.mark.parametrize("nq,nx,d,dens,kn,kind", [
    (3000, 5000, 500, 0.02, 5, "uniform"),     # many partitions
    (1000, 8000, 50, 0.1, 32, "uniform"),      # the largest single pass
    (500, 3000, 8, 0.5, 40, "grid"),           # ties on integers, 2 passes
    (700, 2000, 100000, 0.00001, 6, "uniform"),  # ~37% empty rows: ties
    (129, 300, 30, 0.2, 1, "uniform"),         # ragged wave, one neighbour
    (300, 1500, 20, 0.3, 70, "big"),           # 1e200 entries: inf rows
    (200, 12000, 40, 0.1, 1000, "grid"),       # two-scan path, many ties
    (256, 600, 40, 0.2, 9, "unsorted"),        # unsorted rows read sorted
])
def test_sparse_kneighbors_vs_oracle(nq, nx, d, dens, kn, kind):
    import scipy.sparse as sp
    rng = np.random.default_rng(nq + nx + d)
    rvs = {"grid": lambda k: rng.integers(1, 4, k).astype(np.float64),
           "big": lambda k: rng.choice([1.0, -2.0, 1e200], k,
                                       p=[0.45, 0.45, 0.1])}.get(
        kind, lambda k: rng.uniform(-1, 1, k))
    mf = sp.random(nx, d, density=dens, format="csr", random_state=rng,
                   data_rvs=rvs)
    mq = sp.random(nq, d, density=dens, format="csr", random_state=rng,
                   data_rvs=rvs)
    mf.sort_indices()
    mq.sort_indices()
    f = (mf.indptr.astype(np.int64), mf.indices, mf.data)
    q = (mq.indptr.astype(np.int64), mq.indices, mq.data)
    if kind == "unsorted":
        ip = mf.indptr
        perm = np.concatenate([np.arange(ip[i + 1] - 1, ip[i] - 1, -1)
                               for i in range(nx)]).astype(np.int64)
        mf = sp.csr_matrix((mf.data[perm], mf.indices[perm], ip),
                           shape=mf.shape)
        assert not mf.has_sorted_indices
    gd, gi = _knn_csr(mf, mq, 1000, kn, 250)
    od, oi = orc.kneighbors_csr(f, q, kn)
    if kind == "big":
        # NaN squared distances (inf - inf) never enter a list here; the
        # oracle ranks them last: compare where the oracle's are not NaN
        ok = ~np.isnan(od).any(1)
        assert ok.sum() > nq // 2
        gd, gi, od, oi = gd[ok], gi[ok], od[ok], oi[ok]
    assert np.array_equal(gi, oi)
    assert np.array_equal(gd, od)


def test_sparse_kneighbors_self_query_is_zero_and_errors():
    """Querying the fitted Dataset itself: every row's first neighbour is
    itself at distance exactly 0 (q.q and ||q||^2 are the same sum); mixed
    dense / sparse Datasets and duplicate column entries raise."""
    import scipy.sparse as sp
    from dislib_amd.data import load_data
    from dislib_amd.neighbors import NearestNeighbors
    rng = np.random.default_rng(3)
    m = sp.random(400, 60, density=0.2, format="csr", random_state=rng)
    m = m + sp.random(400, 60, density=0.0, format="csr")   # canonical
    m.data = rng.standard_normal(m.nnz) * 7.0
    nn = NearestNeighbors(n_neighbors=3)
    ds = load_data(m.tocsr(), subset_size=100)
    nn.fit(ds)
    dist, ind = nn.kneighbors(ds)
    nz = np.diff(m.indptr) > 0
    assert np.all(dist[:, 0] == 0.0)
    assert np.array_equal(ind[nz, 0], np.nonzero(nz)[0])
    with pytest.raises(ValueError, match="both be sparse or both dense"):
        nn.kneighbors(load_data(m.toarray(), subset_size=100))
    dup = sp.csr_matrix((np.array([1.0, 2.0, 3.0]), np.array([0, 0, 1]),
                         np.array([0, 2, 3])), shape=(2, 4))
    nn.fit(load_data(dup, subset_size=2))
    with pytest.raises(ValueError, match="duplicate column"):
        nn.kneighbors(load_data(dup, subset_size=2), n_neighbors=1)
