"""The semantics of ``dislib_amd.recommendation.ALS`` restated in numpy: the
reference's loop (``dislib/recommendation/als/base.py``) with the normal
equations solved exactly in fp64 and stored as float32, both RMSE rules and
the transpose split.  Checked against the reference's own output
(``tests/golden/als_ref.npz``) by ``tests/test_als_host.py``; the GPU tests
compare the estimator with the same goldens.

The second half of the module is the kernels' yardstick
(``tests/test_gpu_als_kernels.py``): the same operations in
``np.longdouble`` with the kernels' entry rule spelled out (``Csr``,
``solve_ld``, ``update_rows``, ``sse_ld``, ``row_means_ld``), the derived
error bound of the squared error (``sse_bound``) and the inputs of the
conditioning case, which the host test checks before the GPU test uses them.

The reference solves every row with scipy's ``cg`` to a relative residual of
1e-5, so an exact solve differs from it by a gap that is measured, not
derived.  ``MEASURED_*`` are the largest gaps of this restatement over all
goldens (factors: largest entry-wise gap of ``users`` / ``items`` relative
to the matrix's largest entry; RMSE: largest absolute gap over every recorded
iteration); the acceptance tolerances are 4 times those, the margin being
there because ``cg``'s error scales with each row's condition number and the
goldens sample only a few.  ``test_als_host.py`` asserts that the measured
values still are what is written here.
"""
from math import sqrt

import numpy as np
import scipy.sparse as sp

MEASURED_FACTOR_GAP = 2.64e-3   # case m_f8_s4_long (30 iterations), items
MEASURED_RMSE_GAP = 1.20e-4     # case m_f8_s1_test
T_FACTORS = 4 * MEASURED_FACTOR_GAP
T_RMSE = 4 * MEASURED_RMSE_GAP


def transpose_bounds(n_cols, n_subsets):
    """Column ranges of the reference's ``_get_split_i``
    (``data/classes.py:396-413``)."""
    stride = n_cols // n_subsets
    return [(i * stride, n_cols if i == n_subsets - 1 else (i + 1) * stride)
            for i in range(n_subsets)]


def normal_equations(idx, r, x, lambda_, dtype=np.float64):
    """(A, v) of one row in ``dtype`` (fp64, or longdouble formed from the
    fp64 / fp32 inputs): non-zero entries ``r`` at columns ``idx``."""
    xs = np.asarray(x[idx], dtype=dtype)
    a = xs.T.dot(xs) + dtype(lambda_) * len(idx) * np.eye(x.shape[1],
                                                          dtype=dtype)
    return a, xs.T.dot(np.asarray(r, dtype=dtype))


def update(m, x, lambda_):
    """One half-step over the rows of the CSR matrix ``m``: float32."""
    m = sp.csr_matrix(m)
    y = np.zeros((m.shape[0], x.shape[1]), dtype=np.float32)
    for i in range(m.shape[0]):
        sl = slice(m.indptr[i], m.indptr[i + 1])
        idx, r = m.indices[sl], m.data[sl]
        idx, r = idx[r != 0], r[r != 0]
        if len(idx):
            a, v = normal_equations(idx, r, x, lambda_)
            y[i] = np.linalg.solve(a, v)
    return y


def sse(m, users, items, row_begin, row_end, user_offset):
    """(sum of squared errors, count) over the non-zeros of rows
    [row_begin, row_end), ``users`` indexed by row - row_begin +
    user_offset; fp64."""
    m = sp.csr_matrix(m)
    u64, i64 = users.astype(np.float64), items.astype(np.float64)
    s, c = 0.0, 0
    for row in range(row_begin, row_end):
        sl = slice(m.indptr[row], m.indptr[row + 1])
        idx, r = m.indices[sl], m.data[sl]
        idx, r = idx[r != 0], r[r != 0]
        pred = i64[idx].dot(u64[row - row_begin + user_offset])
        s += float(np.sum((r - pred) ** 2))
        c += len(idx)
    return s, c


def rmse(m, users, items, spans=None):
    """All of ``m`` (the test matrix), or the mean over the row ranges
    ``spans`` of each range's RMSE with ``users`` indexed from 0 -- the
    reference's ``_compute_train_rmse``, quirk included."""
    if spans is None:
        spans = [(0, m.shape[0])]
    out = []
    for a, b in spans:
        s, c = sse(m, users, items, a, b, 0)
        out.append(sqrt(s / c))
    return float(np.mean(out))


def initial_items(r_items, n_f, seed):
    """``items`` before the first update (``base.py:151-166``)."""
    m = sp.csr_matrix(r_items)
    if seed:
        np.random.seed(seed)
    items = np.random.rand(m.shape[0], n_f)
    with np.errstate(all="ignore"):
        items[:, 0] = [np.mean(m.data[m.indptr[i]:m.indptr[i + 1]])
                       if m.indptr[i + 1] > m.indptr[i] else np.nan
                       for i in range(m.shape[0])]
    return items


class Result(object):
    pass


def als_ref(r_items, n_subsets, n_f, lambda_=0.065, tol=1e-4, max_iter=100,
            check_convergence=True, seed=None, test=None):
    """The fit on the items x users matrix ``r_items`` that ``n_subsets``
    Subsets hold: ``users``, ``items``, ``n_iter``, ``converged``,
    ``rmses``."""
    r_i = sp.csr_matrix(r_items, dtype=np.float64)
    r_u = sp.csr_matrix(r_i.T)
    r_u.sort_indices()
    items = initial_items(r_i, n_f, seed)
    users = None
    if test is not None:
        r_t, spans = sp.csr_matrix(test, dtype=np.float64), None
    else:
        r_t, spans = r_u, transpose_bounds(r_i.shape[1], n_subsets)
    res = Result()
    res.rmses, res.converged = [], False
    cur, i = np.inf, 0
    while not (i >= max_iter or res.converged):
        last = cur
        users = update(r_u, items, lambda_)
        items = update(r_i, users, lambda_)
        if check_convergence:
            cur = rmse(r_t, users, items, spans)
            res.rmses.append(cur)
            res.converged = abs(last - cur) < tol
        i += 1
    res.users, res.items, res.n_iter = users, items, i
    return res


def predict_user(users, items, user_id):
    if user_id > users.shape[1]:
        return np.full([items.shape[1]], np.nan)
    return users[user_id].dot(items.T)


# --------------------------------------------------------------------------
# The kernels' yardstick: longdouble, with the kernels' entry rule.
# --------------------------------------------------------------------------
LD = np.longdouble
U = 2.0 ** -53                  # unit roundoff of fp64


class Csr(object):
    """A bare CSR triple.  scipy refuses what the kernel tests need to
    store: column indices outside the shape, negative ones, duplicates
    that stay apart."""

    def __init__(self, indptr, indices, data, shape):
        self.indptr = np.asarray(indptr, dtype=np.int64)
        self.indices = np.asarray(indices, dtype=np.int32)
        self.data = np.asarray(data, dtype=np.float64)
        self.shape = tuple(shape)
        assert len(self.indptr) == self.shape[0] + 1
        assert len(self.indices) == len(self.data) == self.indptr[-1]

    @property
    def nnz(self):
        return int(self.indptr[-1])

    @classmethod
    def from_rows(cls, rows, n_cols):
        """``rows``: one (columns, values) pair per row, stored as given."""
        indptr = np.cumsum([0] + [len(c) for c, _ in rows])
        cat = (lambda k: np.concatenate([np.asarray(r[k], dtype=np.float64)
                                         for r in rows]) if rows else [])
        return cls(indptr, cat(0), cat(1), (len(rows), n_cols))


def solve_ld(a, v):
    """y with a y = v for a symmetric positive definite ``a``: a Cholesky
    factorisation (column by column, left-looking) and the two
    substitutions, every operation in longdouble."""
    a = np.asarray(a, dtype=LD)
    n = a.shape[0]
    low = np.zeros((n, n), dtype=LD)
    for j in range(n):
        low[j, j] = np.sqrt(a[j, j] - low[j, :j].dot(low[j, :j]))
        low[j + 1:, j] = (a[j + 1:, j] -
                          low[j + 1:, :j].dot(low[j, :j])) / low[j, j]
    y = np.array(v, dtype=LD)
    for j in range(n):                       # L z = v
        y[j] = y[j] / low[j, j]
        y[j + 1:] -= low[j + 1:, j] * y[j]
    for j in range(n - 1, -1, -1):           # L^T y = z
        y[j] = y[j] / low[j, j]
        y[:j] -= low[j, :j] * y[j]
    return y


def used_entries(m, i, n_cols):
    """(columns, values) of row ``i`` that the kernels use: an entry counts
    iff its value is not 0 and 0 <= column < n_cols.  Nothing is sorted and
    nothing is merged: a column stored twice is two entries."""
    sl = slice(m.indptr[i], m.indptr[i + 1])
    idx, r = np.asarray(m.indices[sl]), np.asarray(m.data[sl])
    keep = (r != 0) & (idx >= 0) & (idx < n_cols)
    return idx[keep], r[keep]


def update_rows(m, x, lambda_, n_cols=None, dtype=LD):
    """One half-step, one row at a time: a list with (y, cond) per row of
    ``m`` (a ``Csr`` or a scipy CSR matrix, read as stored).  y (``dtype``,
    n_f long) solves the row's normal equations over ``used_entries`` --
    duplicates are separate terms of the Gram sum and of n_c -- with
    ``solve_ld`` for longdouble and ``np.linalg.solve`` otherwise; cond is
    the 2-norm condition number of the fp64 matrix.  A row that uses no
    entry gives (zeros, 0.0).  ``n_cols``: the bound on the columns (the
    kernel's ``m``), ``x.shape[0]`` by default."""
    n_cols = x.shape[0] if n_cols is None else n_cols
    out = []
    for i in range(m.shape[0]):
        idx, r = used_entries(m, i, n_cols)
        if len(idx) == 0:
            out.append((np.zeros(x.shape[1], dtype=dtype), 0.0))
            continue
        a, v = normal_equations(idx, r, x, lambda_, dtype)
        y = solve_ld(a, v) if dtype is LD else np.linalg.solve(a, v)
        a64 = a if dtype is np.float64 else \
            normal_equations(idx, r, x, lambda_)[0]
        out.append((y, float(np.linalg.cond(a64))))
    return out


def update_bound(y, cond, n_f):
    """The update kernels' bound on |y_kernel - y|, entry by entry: the fp32
    store and the forward bound of the fp64 Cholesky solve."""
    y = np.abs(np.asarray(y, dtype=np.float64))
    return 2.0 ** -24 * y + 8 * n_f * cond * U * y.max()


def gamma(k):
    """k u / (1 - k u): the relative error of k chained fp64 roundings."""
    return k * U / (1 - k * U)


def sse_depth(max_len, n_rows):
    """Most roundings between one squared difference and ``dkm_als_sse``'s
    sum: one fma per entry of a lane (a lane takes every 64th entry of its
    row), the 6 steps of the wave's butterfly, the final kernel's fold of
    rows t, t + 256, ... in one thread, the 8 steps of its tree."""
    return -(-max_len // 64) + 6 + -(-max(n_rows, 1) // 256) + 8


def sse_ld(m, users, items, row_begin, row_end, user_offset, n_items=None,
           depth=None):
    """(sum, count, bound) of ``dkm_als_sse`` over ``used_entries`` (column
    bound ``n_items``, ``items.shape[0]`` by default) of rows [row_begin,
    row_end): the sum of (r - u . i)^2 in longdouble, the exact count, and
    a running bound on |kernel's sum - sum| that follows the kernel's
    operations (u = 2^-53, nothing measured):

    * dot.  ``fma(u_f, i_f, dot)`` over the n_f factors in order.  The
      product of two fp32 numbers is exact in fp64, so every step is one
      rounded add and the first adds to 0 exactly:
      |dot^ - dot| <= E_dot = gamma(n_f - 1) sum_f |u_f| |i_f|.
    * diff^ = fl(r - dot^), one more rounding of a value within E_dot of
      diff: |diff^ - diff| <= E = (1 + 2 u) E_dot + u |diff|.
    * square.  The fma forms diff^ diff^ exactly:
      |diff^^2 - diff^2| <= 2 |diff| E + E^2.
    * sum.  The terms are >= 0 and each passes through at most ``depth``
      rounded adds (``sse_depth``: lane chain, butterfly, fold, tree), so
      the computed sum is within gamma(depth) sum diff^^2 of their exact
      sum, whatever the tree's shape.

    bound = sum (2 |diff| E + E^2) + gamma(depth) sum (|diff| + E)^2, times
    1 + 2^-10 for this function's own longdouble roundings (the same terms
    with 2^-64 in place of u, a 2^-11th).  ``depth`` overrides the kernel's
    depth for a sum taken in another order."""
    n_items = items.shape[0] if n_items is None else n_items
    n_f = users.shape[1]
    s = e_sq = t_sq = LD(0)
    c, max_len = 0, 0
    for row in range(row_begin, row_end):
        idx, r = used_entries(m, row, n_items)
        max_len = max(max_len, int(m.indptr[row + 1] - m.indptr[row]))
        if len(idx) == 0:
            continue
        u = users[row - row_begin + user_offset].astype(LD)
        it = items[idx].astype(LD)
        diff = np.abs(r.astype(LD) - it.dot(u))
        e = (1 + 2 * U) * gamma(n_f - 1) * np.abs(it).dot(np.abs(u)) + \
            U * diff
        s += np.sum(diff * diff)
        e_sq += np.sum(2 * diff * e + e * e)
        t_sq += np.sum((diff + e) ** 2)
        c += len(idx)
    if depth is None:
        depth = sse_depth(max_len, row_end - row_begin)
    bound = (e_sq + gamma(depth) * t_sq) * (1 + 2.0 ** -10)
    return s, c, float(bound)


def row_means_ld(m):
    """Every row's mean of its stored entries (zeros included) in
    longdouble; NaN for a row that stores none."""
    out = np.full(m.shape[0], np.nan, dtype=LD)
    for i in range(m.shape[0]):
        row = np.asarray(m.data[m.indptr[i]:m.indptr[i + 1]], dtype=LD)
        if len(row):
            out[i] = np.sum(row) / len(row)
    return out


def row_means_bound(m):
    """Bound on |dkm_als_row_means - mean| per row: (len / 64 + 8) u
    sum |data| / len.  A lane adds every 64th entry in a chain (at most
    len / 64 + 1 rounded adds, the first exact), the butterfly adds 6
    roundings and the division one.  With entries of both signs the sum
    cancels, so no bound in ulps of the mean itself can be derived."""
    out = np.zeros(m.shape[0])
    for i in range(m.shape[0]):
        row = np.abs(np.asarray(m.data[m.indptr[i]:m.indptr[i + 1]]))
        if len(row):
            out[i] = (len(row) / 64 + 8) * U * float(np.sum(row)) / len(row)
    return out


COND_LAMBDA = 1e-6
COND_NF = (16, 49, 128)


def conditioning_case(n_f, dtype=np.float64):
    """(m, x) where the Cholesky's accuracy is what is measured, for
    lambda = COND_LAMBDA: factors uniform in [-1, 1), rows with n_c = 1, 2,
    n_f - 1, n_f, n_f + 1 entries (the Gram matrix has rank n_c < n_f in
    the first three), ratings uniform in [-5, 5).  Every |x| < 1 gives
    ||Gram|| <= n_c n_f against lambda n_c on the diagonal, so cond(A) <=
    1 + n_f / lambda and 8 n_f cond(A) u <= 2^-12 up to n_f = 128: the
    update's bound stays a check (``test_als_host.py`` asserts it)."""
    rng = np.random.default_rng(7000 + n_f)
    x = rng.uniform(-1, 1, (n_f + 4, n_f)).astype(dtype)
    rows = []
    for n_c in sorted({1, 2, n_f - 1, n_f, n_f + 1} - {0}):
        cols = rng.choice(x.shape[0], n_c, replace=False)
        rows.append((cols, rng.uniform(-5, 5, n_c)))
    return Csr.from_rows(rows, x.shape[0]), x
