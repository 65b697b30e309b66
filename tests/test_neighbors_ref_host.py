"""CPU tests of tests/neighbors_ref.py: the helpers against brute force, the
conditions their generated inputs must meet for the GPU cases to prove
anything, and the host query dkm_knn_plan."""
import ctypes
import math

import numpy as np
import pytest

from dislib_amd import _lib
from oracle import neighbors_oracle as orc
from tests import neighbors_ref as ref


def plan(nq, nx, kn):
    pl, P = ctypes.c_int64(-7), ctypes.c_int32(-7)
    path = _lib.load().dkm_knn_plan(nq, nx, kn, ctypes.byref(pl),
                                    ctypes.byref(P))
    return path, pl.value, P.value


def brute_knn(Q, X, kn, f32=False):
    """Python loops, math.sqrt (float32's for ``f32``), a sort of (r, j)
    tuples."""
    di, ii = [], []
    for q in Q:
        pairs = []
        for j, x in enumerate(X):
            r = 0.0
            for a, b in zip(q, x):
                df = float(a) - float(b)
                r = r + df * df
            pairs.append((r, j))
        pairs.sort()
        di.append([float(np.sqrt(np.float32(r))) if f32 else math.sqrt(r)
                   for r, _ in pairs[:kn]])
        ii.append([j for _, j in pairs[:kn]])
    return np.array(di), np.array(ii)


@pytest.mark.parametrize("make,d,kn", [(ref.normal, 3, 5), (ref.grid, 2, 7),
                                       (ref.mixed, 9, 40), (ref.grid, 1, 40)])
def test_knn_exact_against_brute_force(make, d, kn):
    Q, X = make(1, 6, d), make(2, 40, d)
    dist, ind = ref.knn_exact(Q, X, kn)
    bd, bi = brute_knn(Q, X, kn)
    assert np.array_equal(ind, bi) and np.array_equal(dist, bd)
    r = ref.seq_sq_distances(Q, X)
    assert np.array_equal(np.sqrt(np.sort(r, axis=1)[:, :kn]), dist)


@pytest.mark.parametrize("make,d", [(ref.normal, 3), (ref.grid, 2),
                                    (ref.mixed, 20), (ref.mixed, 136)])
def test_radius_exact_against_brute_force(make, d):
    Q, X = make(3, 5, d), make(4, 60, d)
    # pair by pair (numpy's 1-D norm is a BLAS dot: another arithmetic)
    full = np.array([[np.sqrt(np.add.reduce((q - x) * (q - x))) for x in X]
                     for q in Q])
    eps = float(np.median(full))
    got = ref.radius_exact(Q, X, eps)
    sizes = []
    for q in range(len(Q)):
        pairs = sorted((full[q, j], j) for j in range(len(X))
                       if full[q, j] < eps)
        assert got[q][0].tolist() == [j for _, j in pairs]
        assert got[q][1].tolist() == [v for v, _ in pairs]
        sizes.append(len(pairs))
    assert 0 < sum(sizes) < len(Q) * len(X)
    assert all(len(i) == 0 for i, _ in ref.radius_exact(Q, X, 0.0))
    assert all(len(i) == 60 for i, _ in ref.radius_exact(Q, X, np.inf))
    assert ref.radius_exact(Q, X[:0], 1.0)[0][0].shape == (0,)


def test_radius_exact_is_the_oracles_lists():
    x = ref.grid(5, 80, 2)
    lists, _ = orc.compute_neighbours(2.0, 1, 10, 50, x)
    got = ref.radius_exact(x[10:50], x, 2.0)
    for a, (b, _) in zip(lists, got):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("kind,f32", [("uniform", False), ("grid", False),
                                      ("grid", True), ("uniform", True)])
def test_csr_twins_against_the_dense_form(kind, f32):
    """The CSR helpers return the oracle's lists; on integer values every
    sum is exact, so they must also equal a dense brute force."""
    d = 12
    f = ref.random_csr(6, 50, d, 5, kind, empty=0.2)
    q = ref.random_csr(7, 9, d, 5, kind, empty=0.2)
    if f32:
        f = (f[0], f[1], f[2].astype(np.float32).astype(np.float64))
        q = (q[0], q[1], q[2].astype(np.float32).astype(np.float64))
    dist, ind = ref.knn_csr_exact(q, f, 11, f32)
    od, oi = orc.kneighbors_csr(f, q, 11, f32=f32)
    assert np.array_equal(dist, od) and np.array_equal(ind, oi)
    lists = ref.radius_csr_exact(f, 3, 20, 2.5, f32)
    ol, _ = orc.compute_neighbours_csr(2.5, 1, 3, 23, *f, f32=f32)
    assert len(lists) == 20
    for (i, dv), o in zip(lists, ol):
        assert np.array_equal(i, o)
        assert np.all(np.diff(dv) >= 0) and np.all(dv < 2.5)
    if kind == "grid":
        F, Qd = ref.csr_dense(f, d), ref.csr_dense(q, d)
        bd, bi = brute_knn(Qd, F, 11, f32)
        assert np.array_equal(ind, bi) and np.array_equal(dist, bd)
        for r, (i, dv) in enumerate(lists):
            full = np.sqrt(((F[3 + r] - F) ** 2).sum(1))
            if f32:
                full = np.sqrt(((F[3 + r] - F) ** 2).sum(1).astype(
                    np.float32)).astype(np.float64)
            pairs = sorted((full[j], j) for j in range(50) if full[j] < 2.5)
            assert i.tolist() == [j for _, j in pairs]
            assert dv.tolist() == [v for v, _ in pairs]


def brute_candidates(r, plen, P, kn):
    """two_scan_candidates by sorting tuples."""
    out = []
    for row in r:
        key = [(float("inf"), 1, j) if np.isnan(v) else (float(v), 0, j)
               for j, v in enumerate(row)]
        union = []
        for p in range(P):
            union += sorted(key[p * plen:(p + 1) * plen])[:32]
        union.sort()
        if len(union) < kn:
            out.append(len(row))
            continue
        out.append(sum(1 for k in key if k <= union[kn - 1]))
    return out


@pytest.mark.parametrize("name,nx,plen,P,kn", [
    ("normal", 300, 50, 6, 100),
    ("ties", 300, 50, 6, 100),
    ("short", 70, 17, 5, 40),       # partitions shorter than 32 rows
    ("ragged", 130, 40, 4, 97),     # a last partition of 10 rows
    ("sorted", 300, 50, 6, 100),    # fit rows in distance order: loose
    ("nonfinite", 120, 40, 3, 90),
])
def test_two_scan_candidates_against_brute_force(name, nx, plen, P, kn):
    rng = np.random.default_rng(nx + kn)
    if name == "ties":
        r = rng.integers(0, 5, (4, nx)).astype(np.float64)
    elif name == "sorted":
        r = np.sort(rng.random((4, nx)), axis=1)
    else:
        r = rng.random((4, nx))
    if name == "nonfinite":
        r[:, ::3] = np.inf
        r[:, 1::7] = np.nan
    got = ref.two_scan_candidates(r, plen, P, kn)
    assert got.tolist() == brute_candidates(r, plen, P, kn)
    assert (got >= kn).all() and (got <= nx).all()
    if name == "short":
        assert (got == kn).all()     # the union is every row: exact
    if name == "sorted":
        # the kn-th of the union sits in partition kn // 32: 3 * 50 + 4
        assert (got == 50 * (kn // 32) + kn % 32).all()


def test_rank_keys_order():
    r = np.array([np.nan, np.inf, 1.0, -0.0, 0.0, 5e-324])
    k = ref.rank_keys(r)
    assert k[3] == k[4] == 0
    assert np.argsort(k, kind="stable").tolist() == [3, 4, 5, 2, 1, 0]


def test_plan_matches_the_documented_rule():
    assert plan(0, 5, 1)[0] == 0 and plan(-1, 5, 1)[0] == 0
    assert plan(3, 0, 1)[0] == 0 and plan(3, 5, 0)[0] == 0
    assert plan(3, 5, 6)[0] == 0 and plan(3, 2 ** 31, 1)[0] == 0
    assert plan(3, 5, 6) == (0, -7, -7)          # nothing written
    assert _lib.load().dkm_knn_plan(3, 5, 1, None, None) == 1
    # passes: >= 4096 waves wanted, partitions of >= 256 rows
    assert plan(1, 1, 1) == (1, 1, 1)
    assert plan(65, 255, 32) == (1, 255, 1)
    assert plan(65, 513, 2) == (1, 257, 2)
    assert plan(257, 1030, 5) == (1, 258, 4)
    assert plan(3, 2088, 2081) == (1, 261, 8)
    assert plan(3, 2049, 2049)[0] == 1 and plan(3, 2048, 2048)[0] == 2
    assert plan(3, 33, 32)[0] == 1 and plan(3, 33, 33)[0] == 2
    # two scans: kn / 32 + 1 partitions or more, their first 32 rows
    # holding kn rows between them
    assert plan(65, 33, 33) == (2, 17, 2)
    assert plan(65, 132, 33) == (2, 66, 2)
    assert plan(65, 2048, 2048) == (2, 32, 64)
    assert plan(65, 2047, 2047) == (2, 32, 64)
    assert plan(8193, 70, 33) == (2, 35, 2)
    for nq, nx, kn in [(65, 100, 100), (65, 101, 100), (65, 400, 100),
                       (65, 1000, 1000), (65, 1001, 1000), (65, 4000, 1000),
                       (3, 8500, 2048), (3, 8500, 2000), (65, 64, 64),
                       (65, 65, 64), (65, 256, 64)]:
        path, pl, P = plan(nq, nx, kn)
        assert path == 2 and (P - 1) * pl < nx <= P * pl and P <= 128
        held = sum(min(32, min(nx, (p + 1) * pl) - p * pl) for p in range(P))
        assert held >= kn, (nq, nx, kn)


@pytest.mark.parametrize("kn", [2048, 2000])
@pytest.mark.parametrize("d", [2, 20])
def test_sorted_line_overflows_for_two_queries_of_three(d, kn):
    """The shape of the GPU overflow case, checked here: nx = 8500."""
    nx = 8500
    Q, X = ref.sorted_line(nx, d)
    r = ref.seq_sq_distances(Q, X)
    assert np.all(np.diff(r[0]) > 0) and np.all(np.diff(r[2]) < 0)
    path, pl, P = plan(3, nx, kn)
    assert path == 2
    c = ref.two_scan_candidates(r, pl, P, kn)
    assert c[0] > ref.KB_CAP and c[2] > ref.KB_CAP
    assert kn <= c[1] <= ref.KB_CAP


def test_eps_cases_cover_the_edges():
    assert {c[0] for c in ref.EPS_CASES} == set(ref.EPS_D)
    assert {c[1] for c in ref.EPS_CASES} == {1, 63, 64, 65, 257}
    assert {c[2] for c in ref.EPS_CASES} == {0, 1, 255, 256, 257, 1030}
    assert len(set(ref.EPS_CASES)) == 2 * len(ref.EPS_D)


@pytest.mark.parametrize("d", ref.EPS_D)
def test_mixed_data_shows_the_order_of_summation(d):
    """In the inputs of the GPU epsilon cases numpy's pairwise sum and the
    sequential sum differ in at least one pair, within eps, whenever the two
    orders differ at all (d >= 9; they do at 8 as well, and cannot below);
    and no list is trivially empty or full."""
    differ = 0
    for dd, nq, nx in ref.EPS_CASES:
        if dd != d:
            continue
        Q, X, eps = ref.eps_case(d, nq, nx)
        pair = np.array([orc.vec_matrix_euclid(q, X) for q in Q])
        seq = np.sqrt(ref.seq_sq_distances(Q, X))
        differ += np.count_nonzero((pair != seq) & (pair < eps))
        if d < 8:
            assert np.array_equal(pair, seq)
        if nx >= 255:
            inside = np.count_nonzero(pair < eps)
            assert 0.2 * pair.size < inside < 0.5 * pair.size
    assert (differ >= 1) == (d >= 8)


@pytest.mark.parametrize("d", [1, 20])
def test_band_case(d):
    b = ref.band_case(d)
    assert np.sqrt(b.r) == b.D
    assert b.eps[1] < b.D < b.eps[2]
    if d == 1:
        assert b.D * b.D == b.r
    else:
        assert b.D * b.D > b.r          # r < eps^2, yet sqrt(r) == eps
    for eps, inside in zip(b.eps, b.inside):
        idx, _ = ref.radius_exact(b.Q, b.X, eps)[0]
        assert (b.at in idx.tolist()) == inside
        # within the band on either side of eps^2
        assert abs(b.r - eps * eps) <= eps * eps * 2.0 ** -50


@pytest.mark.parametrize("m", [0, 1, 2, 3, 4095, 4096, 4097, 8192, 8193,
                               12289, 20481])
def test_seg_sort_case_has_lists_of_m_and_5(m):
    Q, X, eps = ref.seg_sort_case(m)
    lists = ref.radius_exact(Q, X, eps)
    assert len(lists[0][0]) == m and len(lists[1][0]) == 5
    if m > 100:
        assert len(np.unique(lists[0][1])) < m // 4     # mostly ties
