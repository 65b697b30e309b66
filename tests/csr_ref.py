"""Host reference and input generators of the CSR k-means kernel tests
(test_csr_host.py, test_gpu_csr_kernels.py).

Expected values come from the oracle's sklearn-order arithmetic
(``oracle.kmeans_oracle.sparse_distances``) in each row's STORED order; the
samples are never densified (d goes to 65537).  Samples travel as raw CSR
arrays ``(indptr int64, indices int32, data fp64)`` so that unsorted rows
and stored zeros reach the kernels as given; centres are scipy CSR, sparse
in content.

``screen_bound`` / ``classify`` restate the screen's per-sample bound and
its decision test from the header comment of dkm_sparse.hip (not from the
library), with fp64 scores:

  u = 2^-24, w = 2^-53, b = 2^-8, n stored entries, A = ||x|| cmax,
  |s_j| <= cmax^2 + 2 A, M = xx + 2 cmax^2 + 4 A
  B = 2 (2 b (1 + 2^-14) A + (n + 2) u A + n w A + u (2 cmax^2 + 2 A)
         + 4 w M) + 2^-100
  decided  <=>  s1 + B < s2 - B

The kernel's fp32 B is looser than this B by less than 2.2 x (it doubles
the (n + 2) u A term, takes (2 n + 6) w M and rounds up), and its fp32
scores lie within B / 2 of the exact ones, so
  * a row whose exact gap s2 - s1 exceeds 8 B (and whose second distance
    xx + s2 exceeds 8 B, the clamp test) is SURELY DECIDED: the fp32 gap is
    at least 8 B - 2.2 B > 2 x 2.2 B;
  * a row whose best centre has a twin -- another centre with the same
    values on the row's stored columns and the same squared norm -- is
    SURELY UNDECIDED: both walk the same bf16 entries in the same order, so
    their fp32 scores are equal bit for bit and s1 + B < s2 - B is false.
"""
import numpy as np
import scipy.sparse as sp

from oracle import kmeans_oracle as orc

N_SUP = 12          # stored entries per centre on disjoint supports


def raw(m):
    """Raw arrays of a scipy CSR matrix (no sort, no copy of the order)."""
    return (np.asarray(m.indptr, dtype=np.int64),
            np.asarray(m.indices, dtype=np.int32),
            np.asarray(m.data, dtype=np.float64))


def as_csr(indptr, indices, data, d):
    """The scipy view of raw arrays: stored order and stored zeros kept (the
    constructor neither sorts nor prunes)."""
    return sp.csr_matrix((np.asarray(data, dtype=np.float64),
                          np.asarray(indices, dtype=np.int32),
                          np.asarray(indptr, dtype=np.int64)),
                         shape=(len(indptr) - 1, d))


def distances(indptr, indices, data, d, C):
    return orc.sparse_distances(as_csr(indptr, indices, data, d),
                                sp.csr_matrix(C))


def expected(indptr, indices, data, d, C, dist=None):
    """(labels int64[n], sums scipy CSR (k, d), counts int64[k]): the
    oracle's distances with first-index argmin, sums as onehot^T X."""
    k = C.shape[0]
    n = len(indptr) - 1
    if dist is None:
        dist = distances(indptr, indices, data, d, C)
    labels = np.argmin(dist, axis=1).astype(np.int64) if n else \
        np.zeros(0, np.int64)
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    return labels, label_sums(indptr, indices, data, d, k, labels), counts


def _onehot(labels, k, keep):
    rows = np.nonzero(keep)[0]
    return sp.csr_matrix((np.ones(len(rows)), (rows, labels[rows])),
                         shape=(len(labels), k))


def label_sums(indptr, indices, data, d, k, labels, keep=None):
    if keep is None:
        keep = np.ones(len(labels), bool)
    return sp.csr_matrix(
        _onehot(labels, k, keep).T @ as_csr(indptr, indices, data, d))


def expected_delta(indptr, indices, data, d, k, labels, prev):
    """The incremental call's (sums scipy CSR (k, d), counts fp64[k]): +x to
    the new cluster of every row whose label changed, -x from its previous
    one when that lies in [0, k)."""
    labels, prev = np.asarray(labels), np.asarray(prev)
    moved = labels != prev
    old = moved & (prev >= 0) & (prev < k)
    pc = np.where(old, prev, 0)
    sums = label_sums(indptr, indices, data, d, k, labels, moved) - \
        label_sums(indptr, indices, data, d, k, pc, old)
    counts = np.bincount(labels[moved], minlength=k).astype(np.float64) - \
        np.bincount(pc[old], minlength=k).astype(np.float64)
    return sp.csr_matrix(sums), counts


# ---------------------------------------------------------------------------
# the screen's bound, restated from the header comment of dkm_sparse.hip
# ---------------------------------------------------------------------------
def screen_bound(xx, n, cmax):
    u, w, b = 2.0 ** -24, 2.0 ** -53, 2.0 ** -8
    A = np.sqrt(xx) * cmax
    c2 = cmax * cmax
    M = xx + 2 * c2 + 4 * A
    return 2 * (2 * b * (1 + 2.0 ** -14) * A + (n + 2) * u * A + n * w * A +
                u * (2 * c2 + 2 * A) + 4 * w * M) + 2.0 ** -100


def classify(indptr, indices, data, d, C):
    """(surely_decided bool[n], surely_undecided bool[n]) (module
    docstring), from exact fp64 scores s_j = |c_j|^2 - 2 x.c_j."""
    C = sp.csr_matrix(C)
    k = C.shape[0]
    n = len(indptr) - 1
    X = as_csr(indptr, indices, data, d)
    cn = np.asarray(C.multiply(C).sum(axis=1)).ravel()
    cmax = np.sqrt(cn.max())
    s = cn[None, :] - 2.0 * np.asarray((X @ C.T).todense())
    xx = np.asarray(X.multiply(X).sum(axis=1)).ravel()
    B = screen_bound(xx, np.diff(indptr), cmax)
    order = np.argsort(s, axis=1, kind="stable")
    rows = np.arange(n)
    s1 = s[rows, order[:, 0]]
    s2 = s[rows, order[:, 1]] if k > 1 else np.full(n, np.inf)
    decided = (s2 - s1 > 8 * B) & (xx + s2 > 8 * B)
    Cc = C.tocsc()
    undecided = np.zeros(n, bool)
    for i in range(n):
        j1 = order[i, 0]
        near = np.nonzero((s[i] == s1[i]) & (cn == cn[j1]))[0]
        if len(near) < 2:
            continue
        cols = indices[indptr[i]:indptr[i + 1]]
        sub = np.asarray(Cc[:, cols][near].todense()) if len(cols) else \
            np.zeros((len(near), 0))
        own = sub[list(near).index(j1)]
        undecided[i] = (np.all(sub == own, axis=1).sum() >= 2)
    assert not (decided & undecided).any()
    return decided, undecided


# ---------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------
def int_centres(k, d, rng):
    """k centres of integer values of magnitude 2..4 and mixed signs (exact
    in bf16): on pairwise disjoint supports of N_SUP columns spread over
    [0, d) (columns 0 and d - 1 included) where d has room for them, else on
    distinct column pairs.  Returns (scipy CSR, list of supports)."""
    if k * N_SUP <= d:
        cols = rng.permutation(d - 2)[:k * N_SUP - 2] + 1
        cols = rng.permutation(np.concatenate([[0, d - 1], cols]))
        sup = [np.sort(cols[j * N_SUP:(j + 1) * N_SUP]) for j in range(k)]
    else:
        pairs = [(a, b) for a in range(d) for b in range(a + 1, d)]
        assert len(pairs) >= k, "d too small for k distinct column pairs"
        pick = rng.permutation(len(pairs))[:k]
        sup = [np.array(pairs[p]) for p in pick]
    rows = np.concatenate([[j] * len(s) for j, s in enumerate(sup)])
    vals = rng.integers(2, 5, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
    C = sp.csr_matrix((vals, (rows, np.concatenate(sup))), shape=(k, d))
    return C, sup


def _rows_of(C, owners, rng):
    """Row i = g x (centre owners[i] on its support), g = 1 or 2, the
    entries in a shuffled stored order for odd i."""
    indptr, indices, data = [0], [], []
    for i, j in enumerate(owners):
        sl = slice(C.indptr[j], C.indptr[j + 1])
        cols, vals = C.indices[sl], C.data[sl]
        if i % 2:
            o = rng.permutation(len(cols))
            cols, vals = cols[o], vals[o]
        indices.extend(cols)
        data.extend((1.0 + (i // 2) % 2) * vals)
        indptr.append(len(indices))
    return (np.array(indptr, np.int64), np.array(indices, np.int32),
            np.array(data, np.float64))


def own_rows(k, d, n, seed):
    """(indptr, indices, data, C): int_centres and rows that copy centre
    i % k (once or doubled): every centre wins some row (n >= k), every row
    is surely decided."""
    rng = np.random.default_rng(seed)
    C, sup = int_centres(k, d, rng)
    return _rows_of(C, np.arange(n) % k, rng) + (C,)


def twin_rows(k, d, n, seed):
    """(indptr, indices, data, C): every centre j < k // 2 has an exact copy
    at j + ceil(k / 2) and the rows copy those centres, so every row ties
    exactly between a centre and its copy and must take the lower index."""
    assert k >= 2
    rng = np.random.default_rng(seed)
    h = (k + 1) // 2
    base, sup = int_centres(h, d, rng)
    C = sp.vstack([base, base[:k - h]], format="csr")
    return _rows_of(base, np.arange(n) % (k - h), rng) + (C,)


def near_twin_pairs(k, offset):
    """The (low, high = low + offset) centre pairs of near_twin_rows: blocks
    of ``offset`` centres paired with the following block."""
    return [(b + j, b + j + offset) for b in range(0, k, 2 * offset)
            for j in range(offset) if b + j + offset < k]


def near_twin_rows(k, d, n, seed, offset, scale=1.0, descending=False):
    """(indptr, indices, data, C): pairs of centres c, c (1 + r 2^-8) on a
    shared 12-column support (|r| <= 1 per entry, r = 0 for every 8th pair:
    exact ties), the members ``offset`` centres apart (the slice width:
    different slices); rows on 10 of those columns near the pair's midpoint.  The distance
    gaps lie below the bf16 table's rounding.  Unpaired centres sit far
    away on supports of their own."""
    rng = np.random.default_rng(seed)
    pairs = near_twin_pairs(k, offset)
    assert pairs and (k - len(pairs)) * N_SUP <= d
    cols = rng.permutation(d)
    C = sp.lil_matrix((k, d))
    sup = []
    for m, (lo, hi) in enumerate(pairs):
        s = np.sort(cols[m * N_SUP:(m + 1) * N_SUP])
        sup.append(s)
        c = rng.uniform(0.5, 1.0, N_SUP) * rng.choice([-1.0, 1.0], N_SUP)
        r = rng.uniform(-1, 1, N_SUP) * (m % 8 != 7)
        C[lo, s] = c * scale
        C[hi, s] = c * scale * (1 + r * 2.0 ** -8)
    paired = {j for p in pairs for j in p}
    for t, j in enumerate(sorted(set(range(k)) - paired)):
        s = cols[(len(pairs) + t) * N_SUP:(len(pairs) + t + 1) * N_SUP]
        C[j, s] = 40.0 * scale
    C = sp.csr_matrix(C)
    indptr, indices, data = [0], [], []
    for i in range(n):
        m = i % len(pairs)
        c = np.sort(rng.choice(sup[m], 10, replace=False))
        if descending:
            c = c[::-1]
        v = 0.5 * np.asarray((C[pairs[m][0], c] +
                              C[pairs[m][1], c]).todense()).ravel()
        indices.extend(c)
        data.extend(v * (1 + rng.normal(0, 0.003, 10)))
        indptr.append(len(indices))
    return (np.array(indptr, np.int64), np.array(indices, np.int32),
            np.array(data, np.float64), C)


def length_rows(lengths, d, seed, zeros=False):
    """(indptr, indices, data): rows of exactly the given stored lengths at
    sorted distinct random columns, integer values of magnitude 1..3 and
    mixed signs; ``zeros``: every third stored entry is a stored 0.0."""
    rng = np.random.default_rng(seed)
    indptr, indices, data = [0], [], []
    for ln in lengths:
        indices.extend(np.sort(rng.choice(d, ln, replace=False)))
        data.extend(rng.integers(1, 4, ln) * rng.choice([-1.0, 1.0], ln))
        indptr.append(len(indices))
    data = np.array(data, np.float64)
    if zeros:
        data[::3] = 0.0
    return (np.array(indptr, np.int64), np.array(indices, np.int32), data)


def dense_int_centres(k, d, seed):
    """k dense centres of integer values -3..3, except centres 0, k - 1 and
    (k > 3) 2: three entries of magnitude 1, the same squared norm 3, the
    smallest of all -- an empty row ties between them and must take 0."""
    rng = np.random.default_rng(seed)
    C = rng.integers(-3, 4, (k, d)).astype(np.float64)
    for t, j in enumerate([0, k - 1, 2][:min(k, 3)] if k != 3 else [0, 2]):
        C[j] = 0.0
        C[j, [1 + t, d // 2 + t, d - 2 - t]] = [1.0, -1.0, 1.0]
    norms = (C * C).sum(axis=1)
    assert (np.sort(norms)[min(k, 3):] > 3).all()
    return sp.csr_matrix(C)


def bf16_round(x):
    """fp64 -> fp32 -> bf16, round to nearest even, as fp64."""
    bits = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7fff + ((bits >> 16) & 1)) & 0xffff0000
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


def table_scores(indptr, indices, data, d, C):
    """The screen's scores |c_j|^2 - 2 x.c_j with c rounded to bf16 and x to
    fp32, evaluated in fp64 (the kernel's fp32 chain lies within 2^-20
    relative of it on a dozen entries)."""
    C = sp.csr_matrix(C)
    cn = np.asarray(C.multiply(C).sum(axis=1)).ravel()
    Cb = C.copy()
    Cb.data = bf16_round(C.data)
    X = as_csr(indptr, indices,
               np.asarray(data, np.float32).astype(np.float64), d)
    return cn[None, :] - 2.0 * np.asarray((X @ Cb.T).todense())
