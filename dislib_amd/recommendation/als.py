"""``ALS`` -- drop-in for ``dislib.recommendation.ALS`` (dislib v0.2.0,
``dislib/recommendation/als/base.py``) on a sparse Dataset that is resident
in HBM.

Same constructor, private attributes, ``converged`` / ``users`` / ``items``,
``fit(dataset, test=None) -> (users, items)`` and ``predict_user`` as the
reference, plus ``n_iter`` (the iterations the last fit ran) and the
keyword-only ``device``.  ``arity`` is stored and has no effect: there is no
merge tree.

What is kept of the reference, line by line:

* Seeding (``base.py:151-159``): ``if self._seed: np.random.seed(seed)``, so
  ``random_state`` 0 and ``None`` do not seed; then ``items =
  np.random.rand(n_m, n_f)`` in fp64 on the host, column 0 replaced by every
  item row's ``np.mean(row.data)`` (``:162-166``; stored zeros count, an item
  that stores nothing gets NaN, which no user gathers).
* One iteration (``:173-174``) updates ``users`` from ``(R^T, items)`` and
  then ``items`` from ``(R, users)``.  For a row with non-zero entries at
  ``idx`` (``:225-242``): ``n_c = len(idx)``, ``A = X[idx]^T X[idx] +
  lambda n_c I``, ``v = X[idx]^T r[idx]``, the result stored as float32 --
  the first users update reads the fp64 initial items, every later update
  float32 factors.  A row without a non-zero entry gives zeros.  Stored
  entries equal to 0 are dropped as ``sparse.find`` drops them, in the
  update and in the RMSE.
* Convergence (``:117-121, 176-190``): with ``check_convergence``,
  ``converged = |last_rmse - rmse| < tol`` starting from ``rmse = inf``; the
  loop ends on ``converged`` or at ``i >= max_iter``.  With ``test`` the RMSE
  runs over the non-zeros of ``test`` (users as rows).  Without it, it is the
  mean over the Subsets of the transposed Dataset of each Subset's own RMSE,
  and each of those indexes ``users`` by the row number *inside the Subset*
  (``_get_rmse(sb, U, I)``, ``:123-126, 246-253``).  That is wrong for every
  Subset but the first; it is what stops the reference's loop, so it is
  reproduced here (``dkm_als_sse`` with ``user_offset = 0``).
* ``predict_user`` (``:210-215``) keeps the ``user_id > users.shape[1]`` test
  (it compares with the number of factors, not of users) and the NaN vector
  of length ``items.shape[1]``.

What differs: the normal equations are solved exactly (Gram matrix and
Cholesky in fp64, rounded to float32 on store) where the reference runs
scipy's ``cg`` to a relative residual of 1e-5, so factors agree with the
reference to a measured tolerance (``tests/als_ref.py``), not bit for bit;
the RMSE's dot products are fp64 (the reference's are float32).  ``lambda_``
must make every row's matrix positive definite (any ``lambda_ > 0`` does).
Duplicate entries of a row are not summed (``sparse.find`` sums them).

Where it runs.  The ratings are ``dataset._device_data(device)``, the CSR
image; torch transposes it on the device (a stable sort of the column
indices); ``dkm_als.hip`` does the item means, both half-steps of every
iteration and the squared error.  Per iteration two doubles per RMSE Subset
come to the host.  Every sum has a fixed order: two fits of the same input
are byte-identical.

Refusals, all before any GPU call: a dense Dataset (``ValueError``), a
``torch.distributed`` world larger than 1 and ``n_f`` above
``dislib_amd._lib.ALS_MAX_NF`` (``NotImplementedError``).
"""
import ctypes
from math import sqrt

import numpy as np

from .. import _lib
from .._device import on, preload, ptr, resolve, stream_ptr, torch
from ..data.classes import _transpose_bounds


class ALS(object):
    """Alternating least squares on MI355X (see the module docstring).

    Parameters match ``dislib.recommendation.ALS``; ``device`` is a
    keyword-only extension.
    """

    def __init__(self, random_state=None, n_f=100, lambda_=0.065,
                 tol=1e-4, max_iter=100, arity=5,
                 check_convergence=True, verbose=False, *, device=None):
        self._seed = random_state
        self._n_f = n_f
        self._lambda = lambda_
        self._tol = tol
        self._max_iter = max_iter
        self._verbose = verbose
        self._arity = arity
        self._check_convergence = check_convergence
        self._device = device
        self.converged = False
        self.users = None
        self.items = None
        self.n_iter = 0
        self.rmse_ = []          # the RMSE after every iteration that took it

    def _has_finished(self, i):
        return i >= self._max_iter or self.converged

    def _has_converged(self, last_rmse, rmse):
        return abs(last_rmse - rmse) < self._tol

    def fit(self, dataset, test=None):
        """Fit the factors to ``dataset`` (every sample = the ratings of one
        item).  ``test``: a sparse matrix with users as rows and items as
        columns to take the convergence RMSE on instead of the training
        data.  Returns ``(users, items)``."""
        import scipy.sparse as sp
        from .. import _shard
        if not dataset.sparse:
            raise ValueError("ALS takes a sparse Dataset (ratings with items "
                             "as samples)")
        if _shard.active():
            raise NotImplementedError(
                "ALS runs on one rank: a torch.distributed world larger "
                "than 1 is not supported")
        n_f = int(self._n_f)
        if n_f > _lib.ALS_MAX_NF:
            raise NotImplementedError(
                "ALS keeps a row's normal equations in LDS: n_f is limited "
                "to %d, got %d" % (_lib.ALS_MAX_NF, n_f))
        if n_f < 1:
            raise ValueError("n_f must be at least 1, got %d" % n_f)
        n_m = int(np.sum(dataset.subsets_sizes())) if len(dataset) else 0
        n_u = int(dataset.n_features)
        bounds = _transpose_bounds(n_u, len(dataset))
        if self._verbose:
            print("Item chunks: %s" % len(dataset))
            print("User chunks: %s" % len(bounds))
        if test is not None:
            test = sp.csr_matrix(test, dtype=np.float64)
            if test.shape[0] > n_u or test.shape[1] > n_m:
                raise ValueError("test has shape %r; users x items is at "
                                 "most (%d, %d)" % (test.shape, n_u, n_m))
        if self._seed:
            np.random.seed(self._seed)
        self.converged = False
        items0 = np.random.rand(n_m, n_f)

        so = _lib.lib()                     # no GPU / no libdkm: raise here
        dd = dataset._device_data(self._device)
        t = torch()
        with on(dd.device):
            preload(dd.device)
            r_i = _Csr(dd.indptr, dd.indices, dd.data, n_m, n_u)
            r_u = csr_transpose(r_i)
            items = t.from_numpy(items0).to(dd.device)
            if n_m:
                items[:, 0] = row_means(so, r_i)
            if test is not None:
                r_t = _Csr(
                    t.from_numpy(test.indptr.astype(np.int64)).to(dd.device),
                    t.from_numpy(test.indices.astype(np.int32)).to(dd.device),
                    t.from_numpy(test.data).to(dd.device), test.shape[0],
                    test.shape[1])
                spans = None
            else:
                r_t, spans = r_u, bounds
            users = None
            self.rmse_ = []
            rmse, i = np.inf, 0
            while not self._has_finished(i):
                last_rmse = rmse
                users = update(so, r_u, items, self._lambda)
                items = update(so, r_i, users, self._lambda)
                if self._check_convergence:
                    rmse = _rmse(so, r_t, users, items, spans)
                    self.rmse_.append(rmse)
                    self.converged = self._has_converged(last_rmse, rmse)
                    if self._verbose:
                        print("%s RMSE: %.3f  [%s]" % (
                            "Train" if spans else "Test", rmse,
                            abs(last_rmse - rmse)))
                i += 1
            self.n_iter = i
            self.users = None if users is None else users.cpu().numpy()
            self.items = items.cpu().numpy()
        return self.users, self.items

    def predict_user(self, user_id):
        """The expected ratings of ``user_id`` for every item; a NaN vector
        when ``user_id > users.shape[1]`` (the reference's test)."""
        if self.users is None or self.items is None:
            raise Exception("Model not trained, call first model.fit()")
        if user_id > self.users.shape[1]:
            return np.full([self.items.shape[1]], np.nan)
        return self.users[user_id].dot(self.items.T)


class _Csr(object):
    """A CSR matrix on the device: indptr int64, indices int32, data fp64."""

    def __init__(self, indptr, indices, data, n_rows, n_cols):
        t = torch()
        self.indptr, self.n_rows, self.n_cols = indptr, int(n_rows), \
            int(n_cols)
        if data.numel() == 0:            # keep valid device pointers
            indices = t.zeros(1, dtype=t.int32, device=indptr.device)
            data = t.zeros(1, dtype=t.float64, device=indptr.device)
        self.indices, self.data = indices, data
        self.nnz = int(indptr.shape[0] and indptr[-1].item())


def csr_transpose(m):
    """The transposed device CSR matrix with sorted indices: scipy's
    ``m.T.tocsr()``, entry for entry (a stable sort by column keeps the rows
    of a column in order; stored zeros stay)."""
    t = torch()
    dev = m.indptr.device
    nnz = m.nnz
    cols = m.indices[:nnz].to(t.int64)
    counts = t.bincount(cols, minlength=m.n_cols)[:m.n_cols] if nnz else \
        t.zeros(m.n_cols, dtype=t.int64, device=dev)
    indptr = t.zeros(m.n_cols + 1, dtype=t.int64, device=dev)
    indptr[1:] = t.cumsum(counts, 0)
    rows = t.repeat_interleave(
        t.arange(m.n_rows, dtype=t.int32, device=dev),
        m.indptr[1:] - m.indptr[:-1], output_size=nnz)
    perm = t.sort(cols, stable=True).indices
    return _Csr(indptr, rows[perm].contiguous(),
                m.data[:nnz][perm].contiguous(), m.n_cols, m.n_rows)


def row_means(so, m):
    """fp64 device vector of every row's ``np.mean(row.data)``."""
    t = torch()
    out = t.empty(m.n_rows, dtype=t.float64, device=m.indptr.device)
    _lib.check(so.dkm_als_row_means(ptr(m.indptr), ptr(m.data), m.n_rows,
                                    ptr(out), stream_ptr()),
               "dkm_als_row_means")
    return out


def update(so, m, X, lambda_):
    """One half-step: the float32 (m.n_rows, n_f) factors of ``m``'s rows
    from the fp64 / fp32 factors ``X`` of its columns."""
    t = torch()
    X = X.contiguous()
    n_f = X.shape[1]
    Y = t.empty((m.n_rows, n_f), dtype=t.float32, device=X.device)
    fn = so.dkm_als_update_f32 if X.dtype == t.float32 else \
        so.dkm_als_update_f64
    _lib.check(fn(ptr(m.indptr), ptr(m.indices), ptr(m.data), m.n_rows,
                  ptr(X), X.shape[0], n_f, X.stride(0), float(lambda_),
                  ptr(Y), stream_ptr()), "dkm_als_update")
    return Y


def sse(so, m, users, items, row_begin, row_end, user_offset):
    """(sum of squared errors, count) over the non-zero entries of rows
    ``[row_begin, row_end)`` of ``m`` as a device fp64 pair."""
    t = torch()
    n_f = users.shape[1]
    nr = row_end - row_begin
    wsb = int(so.dkm_als_workspace_bytes(nr, n_f))
    if wsb == 0:
        raise ValueError("ALS: bad RMSE range [%d, %d)" % (row_begin,
                                                          row_end))
    ws = t.empty(wsb, dtype=t.uint8, device=users.device)
    out = t.empty(2, dtype=t.float64, device=users.device)
    _lib.check(so.dkm_als_sse(
        ptr(m.indptr), ptr(m.indices), ptr(m.data), row_begin, row_end,
        user_offset, ptr(users), users.shape[0], ptr(items), items.shape[0],
        n_f, ctypes.c_void_p(ws.data_ptr()), wsb, ptr(out), stream_ptr()),
        "dkm_als_sse")
    return out


def _rmse(so, m, users, items, spans):
    """The reference's convergence RMSE: over all of ``m`` (``spans`` None:
    the test matrix), or the mean of the RMSEs of the row ranges ``spans``,
    each indexing ``users`` from 0 (``_compute_train_rmse``)."""
    t = torch()
    if spans is None:
        spans = [(0, m.n_rows)]
    parts = t.stack([sse(so, m, users, items, a, b, 0) for a, b in spans])
    rmses = []
    for s, c in parts.cpu().numpy():
        if c == 0:
            raise ValueError("Found array with 0 sample(s) while computing "
                             "the RMSE of a Subset without ratings")
        rmses.append(sqrt(s / c))
    return float(np.mean(rmses))
