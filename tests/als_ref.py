"""The semantics of ``dislib_amd.recommendation.ALS`` restated in numpy: the
reference's loop (``dislib/recommendation/als/base.py``) with the normal
equations solved exactly in fp64 and stored as float32, both RMSE rules and
the transpose split.  Checked against the reference's own output
(``tests/golden/als_ref.npz``) by ``tests/test_als_host.py``; the GPU tests
compare the estimator with the same goldens.

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


def normal_equations(idx, r, x, lambda_):
    """(A, v) of one row in fp64: non-zero entries ``r`` at columns
    ``idx``."""
    xs = np.asarray(x[idx], dtype=np.float64)
    a = xs.T.dot(xs) + lambda_ * len(idx) * np.eye(x.shape[1])
    return a, xs.T.dot(np.asarray(r, dtype=np.float64))


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
