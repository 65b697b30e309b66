"""Host references and input generators for tests/test_gpu_neighbors_kernels.py
-- TEST INFRASTRUCTURE ONLY, numpy only.

Thin helpers over oracle/neighbors_oracle.py, whose arithmetic
tests/test_neighbors_golden.py pins to the reference's own outputs; nothing
here restates a distance, it calls the oracle's.  tests/
test_neighbors_ref_host.py holds these helpers to brute force on the CPU.
"""
import types

import numpy as np

from oracle import neighbors_oracle as orc
from oracle.kmeans_oracle import vec_matrix_euclid

KB_CAP = 4096            # candidates per query of the two-scan path
_KEY_NAN = np.uint64(0x7ff8000000000000)


# --------------------------------------------------------------------------
# references
# --------------------------------------------------------------------------
def knn_exact(Q, X, kn):
    """(dist, ind) of ``kneighbors_exact``: sequential sums, ascending
    (distance, index)."""
    with np.errstate(all="ignore"):
        return orc.kneighbors_exact(np.ascontiguousarray(X, np.float64),
                                    np.ascontiguousarray(Q, np.float64), kn)


def seq_sq_distances(Q, X):
    """The (nq, nx) squared sequential distances the kNN kernels rank by:
    the oracle's ``seq_distances`` sums, before its sqrt."""
    Q = np.asarray(Q, np.float64)
    X = np.asarray(X, np.float64)
    r = np.zeros((Q.shape[0], X.shape[0]))
    with np.errstate(all="ignore"):
        for t in range(X.shape[1]):
            df = Q[:, t, None] - X[None, :, t]
            r = r + df * df
    return r


def radius_exact(Q, X, eps):
    """Per query row of Q: (indices int64, distances) of the rows of X with
    ``_vec_matrix_euclid`` distance < eps, ascending (distance, index): the
    arithmetic and order of ``compute_neighbours`` with separate query and
    fit arrays."""
    Q = np.ascontiguousarray(Q, np.float64)
    X = np.ascontiguousarray(X, np.float64)
    out = []
    with np.errstate(all="ignore"):
        for q in Q:
            dist = vec_matrix_euclid(q, X).flatten()
            neigh = np.where(dist < eps)[0]
            neigh = neigh[np.lexsort((neigh, dist[neigh]))]
            out.append((neigh.astype(np.int64), dist[neigh]))
    return out


def knn_csr_exact(q_csr, f_csr, kn, f32=False):
    """``kneighbors_csr`` with the query first, like :func:`knn_exact`."""
    with np.errstate(all="ignore"):
        return orc.kneighbors_csr(f_csr, q_csr, kn, f32=f32)


def radius_csr_exact(csr, q0, nq, eps, f32=False):
    """Per query row q0 .. q0 + nq of the CSR matrix: (indices, distances)
    of ``compute_neighbours_csr``'s lists (its arithmetic: the oracle's
    ``csr_sq_distances``)."""
    indptr, indices, data = csr
    data = np.asarray(data, np.float64)
    out = []
    with np.errstate(all="ignore"):
        lists, _ = orc.compute_neighbours_csr(eps, 1, q0, q0 + nq, indptr,
                                              indices, data, f32=f32)
        for q, neigh in zip(range(q0, q0 + nq), lists):
            r = orc.csr_sq_distances(indptr, indices, data, q)
            dist = np.sqrt(r.astype(np.float32) if f32 else r)
            out.append((neigh.astype(np.int64),
                        dist[neigh].astype(np.float64)))
    return out


def rank_keys(r):
    """Squared distances as the kNN kernels' ranking keys: the bit pattern
    of r >= 0 (-0.0 folded onto +0.0), NaN after +inf."""
    r = np.asarray(r, np.float64)
    keys = (r + 0.0).view(np.uint64).copy()
    keys[np.isnan(r)] = _KEY_NAN
    return keys


def two_scan_candidates(keys, plen, P, kn):
    """What the two-scan path must collect, per query, from the full (nq,
    nx) matrix of squared distances: the partitions [p plen, (p + 1) plen)
    each give their first 32 rows by (r, index); the kn-th smallest (r,
    index) of the union of those is the threshold; the result is the number
    of pairs <= it.  More than ``KB_CAP`` for some query: the call fell back
    to passes of 32."""
    keys = rank_keys(np.atleast_2d(keys))
    nq, nx = keys.shape
    assert (P - 1) * plen < nx <= P * plen
    idx = np.arange(nx)
    out = np.empty(nq, np.int64)
    for q in range(nq):
        union = []
        for p in range(P):
            a, b = p * plen, min(nx, (p + 1) * plen)
            o = np.lexsort((idx[a:b], keys[q, a:b]))[:32]
            union.extend(zip(keys[q, a:b][o].tolist(), (a + o).tolist()))
        union.sort()
        if len(union) < kn:            # an empty slot: every row is below
            out[q] = nx
            continue
        tk, ti = union[kn - 1]
        k = keys[q]
        out[q] = np.count_nonzero((k < tk) | ((k == tk) & (idx <= ti)))
    return out


# --------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------
def mixed(seed, n, d):
    """Rows whose features differ in magnitude by up to 10^6, so that the
    order of summation of a squared distance shows in its bits."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-3, 3, d)


# the epsilon cases of the GPU file: every d twice, the (nq, nx) edges in
# turn, so that each d meets a fit set of 255 rows or more
EPS_D = [1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 63, 64, 65, 127, 128, 129,
         136]
_EPS_NQ = [1, 63, 64, 65, 257]
_EPS_NX = [0, 1, 255, 256, 257, 1030]
EPS_CASES = [(d, _EPS_NQ[(i + s) % 5], _EPS_NX[(i + 3 * s // 2) % 6])
             for i, d in enumerate(EPS_D) for s in (0, 2)]


def eps_case(d, nq, nx):
    """Q, X of mixed magnitude and an eps that takes about a third of the
    pairs (1.0 without pairs)."""
    Q, X = mixed(100 + d, 257, d)[:nq], mixed(200 + d, 1030, d)[:nx]
    if nx == 0:
        return Q, X, 1.0
    dist = np.array([vec_matrix_euclid(q, X) for q in Q])
    return Q, X, float(np.quantile(dist, 0.33)) * (1 + 2.0 ** -30)


def normal(seed, n, d):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)) * rng.uniform(0.5, 3.0, d)


def grid(seed, n, d, hi=4):
    """Integer grid with many duplicate rows: most distances tie."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, hi, (n, d)).astype(np.float64)


def sorted_line(nx, d, seed=0):
    """The overflow case of the two-scan path.  Fit row j = (j, u_j, 0, ...)
    with u_j uniform in [0, 1e6).  Queries 0 and 2 sit 1e13 beyond either
    end of feature 0: (j +- 1e13)^2 moves by 2e13 from one row to the next,
    more than u_j^2 ever does, so the fit rows are in distance order, every
    partition's first 32 are its nearest 32 and the threshold is loose.
    Query 1 sits on the line: u_j^2 (up to 1e12) swamps (j - x)^2 < 1e8, the
    order is scattered over the partitions and the threshold is tight."""
    rng = np.random.default_rng(seed)
    X = np.zeros((nx, d))
    X[:, 0] = np.arange(nx)
    X[:, 1 % d] += rng.uniform(0, 1e6, nx)
    Q = np.zeros((3, d))
    Q[0, 0] = -1e13
    Q[1, 0] = nx // 2
    Q[2, 0] = 1e13
    return Q, X


def random_csr(seed, n, d, max_len, kind="uniform", empty=0.0):
    """(indptr int64, indices int32 sorted, data) with row lengths 0 ..
    max_len; ``empty``: the share of rows forced empty; ``kind`` "grid":
    integer values 1 .. 3 (ties)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, min(max_len, d) + 1, n)
    lens[rng.random(n) < empty] = 0
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    indices = np.concatenate(
        [np.sort(rng.choice(d, k, replace=False)) for k in lens] +
        [np.zeros(0, np.int64)]).astype(np.int32)
    nnz = int(indptr[-1])
    data = (rng.integers(1, 4, nnz).astype(np.float64) if kind == "grid"
            else rng.uniform(-1, 1, nnz))
    return indptr, indices, data


def csr_dense(csr, d):
    indptr, indices, data = csr
    out = np.zeros((len(indptr) - 1, d))
    for i in range(len(indptr) - 1):
        out[i, indices[indptr[i]:indptr[i + 1]]] = \
            data[indptr[i]:indptr[i + 1]]
    return out


def band_case(d, seed=0):
    """One query row and fit rows for the 2^-48 band of the epsilon
    decision.  Row ``at`` has squared distance r and distance D = sqrt(r);
    returns the three eps of the band -- D (the row is excluded: D < D is
    false, although r == D^2 for d = 1 and r < fl(D^2) for the d = 20 row,
    which is searched for that), its lower neighbour (excluded) and its
    upper neighbour (included)."""
    rng = np.random.default_rng(seed)
    q = np.zeros((1, d))
    if d == 1:
        X = np.array([[0.3], [1.1], [2.5], [7.0]])
        at = 1
    else:
        X = rng.standard_normal((400, d))
        at = None
    dist = vec_matrix_euclid(q[0], X).flatten()
    r = dist * 0
    for j in range(len(X)):   # pairwise squares, before the sqrt
        df = q[0] - X[j]
        r[j] = np.add.reduce(df * df)
    assert np.array_equal(np.sqrt(r), dist)
    if at is None:
        # sqrt rounded up: D^2 rounds above r, so r < eps^2 at eps = D and
        # only the sqrt and compare exclude the row
        up = np.flatnonzero(dist * dist > r)
        assert up.size
        at = int(up[0])
    D = dist[at]
    return types.SimpleNamespace(
        Q=q, X=X, at=at, r=r[at], D=D,
        eps=[D, np.nextafter(D, 0.0), np.nextafter(D, np.inf)],
        inside=[False, False, True])


def seg_sort_case(m, seed=0):
    """Two queries; the first has exactly ``m`` rows within eps = 1000 (on a
    2-D integer grid: most distances tie), the second 5 (a cluster 1e6
    away).  Fit rows shuffled."""
    rng = np.random.default_rng(seed + m)
    near = rng.integers(0, 40, (m, 2)).astype(np.float64)
    far = 1e6 + rng.integers(0, 3, (5, 2)).astype(np.float64)
    X = np.vstack([near, far])[rng.permutation(m + 5)]
    Q = np.array([[0.0, 0.0], [1e6, 1e6]])
    return Q, X, 1000.0
