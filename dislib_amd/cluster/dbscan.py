"""``DBSCAN`` -- drop-in for ``dislib.cluster.DBSCAN`` (dislib v0.2.0,
``dislib/cluster/dbscan/base.py``) on a Dataset that is resident in HBM, and
the epsilon query it is built on.

``DBSCAN``
----------
Same constructor and private attributes as the reference (``base.py:68-82``,
with its ``n_regions >= 1`` assertion) plus the keyword-only ``device``;
``fit`` / ``fit_predict`` set the Subsets' labels and return ``None``;
``n_clusters`` is the number of clusters found.

The result is exact DBSCAN as the reference computes it with one region
(``_compute_labels``, ``classes.py:162-191``):

* two samples are neighbours when their ``_vec_matrix_euclid`` distance is
  below ``eps`` -- the epsilon query's arithmetic and its ``dist < eps``
  rule, decided as ``dkm_radius_count_f64`` decides it; a sample is its own
  neighbour; ``eps <= 0`` gives no neighbours at all;
* a sample with at least ``min_samples`` neighbours is a core point; two
  core points within ``eps`` are in one component;
* a non-core sample joins the component of its nearest core neighbour only,
  ties going to the smallest (distance, Dataset row): it never links two
  components, and with no core neighbour it is alone.  (The reference's
  ``np.argsort`` leaves the order among exactly equal distances unpinned,
  ``tests/test_neighbors_tie_rule.py``);
* a component of fewer than ``min_samples`` members is noise (``-1``), even
  when it holds a core point (``classes.py:187-189``: a lone core point
  whose border points are all nearer to another core);
* the other components are numbered 0, 1, ... by the smallest Dataset row
  among their members.

``n_regions``, ``dimensions``, ``arrange_data`` and ``max_samples`` are
accepted and stored; they do not change the result.  In the reference they
partition the work over tasks, and its multi-region result is this same
clustering (up to the numbering) except in rare boundary cases, e.g. a sample
that a neighbouring region, seeing only part of its neighbours, takes for
non-core.  Here ``dimensions`` only picks the features of
the cell ordering below.

Where it runs.  The samples are ``dataset._device_data(device)``; fp32 and
integer samples are widened to fp64 (as ``compute_neighbours`` widens them:
numpy's ``vector - matrix`` of the reference stays in fp32 for fp32 samples,
which is not reproduced).  Nothing n rows long comes to the host.  Torch
orders the rows by grid cell of side ``eps`` (a stable sort of one int64 key,
one gather); three calls of ``dkm_dbscan.hip`` then find the core points,
union the core points within ``eps`` of each other (a lock-free union-find)
and keep every non-core row's nearest core, and turn the forest into
labels.  Memory is O(n): no neighbour list and nothing n x n exists, the
distances are recomputed in each pass.  Labels leave as one int32 device
tensor (``Dataset._attach_device_labels``) and materialise when a Subset's
``labels`` are read.  Every result is a function of the input only, so labels
are identical from run to run.

Refusals.  A sparse Dataset and a ``torch.distributed`` world larger than 1
raise ``NotImplementedError``; non-finite samples raise the ``ValueError`` of
``compute_neighbours``' input check.  An empty Dataset and empty Subsets
work (``n_clusters == 0``, empty labels).

``compute_neighbours``
----------------------
Reference: ``_compute_neighbours`` of
``/root/reference/dislib/cluster/dbscan/classes.py:124-141`` -- for every
sample of rows ``[begin_idx, end_idx)`` of the concatenated Subsets, the
indices of all samples whose ``_vec_matrix_euclid`` distance (``:153-154``,
numpy's ``sqrt(add.reduce((x - s)**2))`` in its pairwise order) is below
``epsilon``, ordered by distance, and whether there are at least
``min_samples`` of them.

Here the concatenated samples are uploaded once and ``dkm_radius_count_f64``
/ ``dkm_radius_fill_f64`` compute the same fp64 distances (bit-exact: the
k-means exact arithmetic), select ``dist < epsilon``, and sort each list by
(distance, index).  The reference's ``np.argsort`` gives the same order
except among exactly equal distances, which it may order differently.

Sparse Subsets (``sparse=True``, the reference's ``pairwise_distances``
branch, ``:130``) go through ``dkm_radius_count_csr_f64`` /
``dkm_radius_fill_csr_f64``: sklearn 1.7's fp64 CSR expansion
``sqrt(max(-2 q.x + |q|^2 + |x|^2, 0))`` in its own operation order.  The
concatenated CSR matrix is taken with sorted column indices (a sorted copy
when a Subset's are not; scipy's products then follow the same order).
"""
import ctypes

import numpy as np

from .. import _lib
from .._device import (_is_torch, on, preload, ptr, resolve, stream_ptr,
                       torch)
from .._device import assert_all_finite as _device_assert_finite

# features in the ordering's cell key (63 bits shared among them)
_KEY_DIMS = 16


class DBSCAN:
    """Exact DBSCAN on MI355X (see the module docstring).

    Parameters match ``dislib.cluster.DBSCAN``; ``device`` is a keyword-only
    extension.  fp32 and integer samples are widened to fp64.
    """

    def __init__(self, eps=0.5, min_samples=5, arrange_data=True, n_regions=1,
                 dimensions=None, max_samples=None, *, device=None):
        assert n_regions >= 1, \
            "Number of regions must be greater or equal to 1."

        self._eps = eps
        self._min_samples = min_samples
        self._n_regions = n_regions
        self._dimensions_init = dimensions
        self._dimensions = dimensions
        self._arrange_data = arrange_data
        self._subset_sizes = []
        self._sorting = []
        self._max_samples = max_samples
        self._components = None
        self._device = device
        self._n_clusters = None      # device int32[1] of the last fit

    def fit(self, dataset):
        """Cluster ``dataset`` and set its Subsets' labels."""
        from .. import _shard
        if dataset.sparse:
            raise NotImplementedError(
                "DBSCAN takes dense samples (the epsilon query "
                "compute_neighbours takes sparse Subsets)")
        if _shard.active():
            raise NotImplementedError(
                "DBSCAN runs on one rank: a torch.distributed world larger "
                "than 1 is not supported")
        if self._dimensions_init is None:
            self._dimensions = range(dataset.n_features)
        _lib.lib()                          # no GPU / no libdkm: raise here
        dd = dataset._device_data(self._device)
        with on(dd.device):
            preload(dd.device)
            labels, n_clusters = _fit_device(
                dd.X, float(self._eps), max(0, int(self._min_samples)),
                list(self._dimensions))
        self._n_clusters = n_clusters
        self._components = None
        dataset._attach_device_labels(labels)

    def fit_predict(self, dataset):
        """The same as :meth:`fit` (API standardisation, as the reference)."""
        self.fit(dataset)

    @property
    def n_clusters(self):
        if self._n_clusters is None:
            raise AttributeError("n_clusters: call fit first")
        if self._components is None:
            self._components = list(range(int(self._n_clusters.item())))
        return len(self._components)


def _cell_order(X, eps, dims):
    """The stable order of X's rows by grid cell of side ``eps`` over the
    features ``dims`` (at most _KEY_DIMS of them, first = most significant),
    as an int64 permutation; None when there is nothing to order by.  The
    cell index of a feature is clamped so that all of them fit 63 bits."""
    t = torch()
    n, d = X.shape
    dims = [int(c) for c in dims if 0 <= int(c) < d][:_KEY_DIMS]
    if n < 2 or not dims or not (eps > 0) or eps == float("inf"):
        return None
    bits = 63 // len(dims)
    top = float(2 ** min(bits, 52) - 1)
    cols = X[:, dims]
    cell = t.floor((cols - cols.min(dim=0).values) / eps).clamp_(0.0, top)
    cell = cell.to(t.int64)
    key = t.zeros(n, dtype=t.int64, device=X.device)
    for c in range(len(dims)):
        key = (key << bits) | cell[:, c]
    return t.argsort(key, stable=True)


def _fit_device(X, eps, min_samples, dims, flags=0):
    """(labels int32[n], n_clusters int32[1]) on X's device for the (n, d)
    device matrix ``X``; ``flags``: ``_lib.DBSCAN_NOPRUNE``."""
    t = torch()
    dev = X.device
    n, d = X.shape
    n_clusters = t.zeros(1, dtype=t.int32, device=dev)
    labels = t.empty(n, dtype=t.int32, device=dev)
    if n == 0:
        return labels, n_clusters
    X = X.to(t.float64)
    if not bool(t.isfinite(X).all()):
        if bool(t.isnan(X).any()):
            raise ValueError("Input contains NaN.")
        raise ValueError("Input contains infinity or a value too large for "
                         "dtype('float64').")
    so = _lib.lib()
    perm = _cell_order(X, eps, dims)
    if perm is None:
        orig = t.arange(n, dtype=t.int32, device=dev)
        Xs = X.contiguous()
    else:
        orig = perm.to(t.int32)
        Xs = X.index_select(0, perm)
    del X, perm
    wsb = int(so.dkm_dbscan_workspace_bytes(n, d))
    if wsb == 0:
        raise ValueError("DBSCAN takes fewer than 2**31 - 64 samples, got %d"
                         % n)
    ws = t.empty(wsb, dtype=t.uint8, device=dev)
    core = t.empty(n, dtype=t.int32, device=dev)
    parent = t.empty(n, dtype=t.int32, device=dev)
    attach = t.empty(n, dtype=t.int32, device=dev)
    wp = ctypes.c_void_p(ws.data_ptr())
    _lib.check(so.dkm_dbscan_core_f64(
        ptr(Xs), n, d, Xs.stride(0), eps, min_samples, flags, wp, wsb,
        ptr(core), stream_ptr()), "dkm_dbscan_core")
    _lib.check(so.dkm_dbscan_link_f64(
        ptr(Xs), n, d, Xs.stride(0), eps, flags, wp, wsb, ptr(core),
        ptr(orig), ptr(parent), ptr(attach), stream_ptr()),
        "dkm_dbscan_link")
    _lib.check(so.dkm_dbscan_finalize(
        n, min_samples, wp, wsb, ptr(core), ptr(orig), ptr(parent),
        ptr(attach), ptr(labels), ptr(n_clusters), stream_ptr()),
        "dkm_dbscan_finalize")
    return labels, n_clusters


def compute_neighbours(epsilon, min_samples, sparse, begin_idx, end_idx,
                       *subsets, device=None):
    """Same arguments and results as the reference task: a list of int64
    index arrays (one per query sample) and a list of core-point flags."""
    if sparse:
        return _compute_neighbours_csr(epsilon, min_samples, begin_idx,
                                       end_idx, subsets, device)
    t = torch()
    dev = resolve(device)
    with on(dev):
        X = _concat(subsets, dev)
        n, d = X.shape
        b, e = _slice_bounds(begin_idx, end_idx, n)
        Q = X[b:e]
        nq = e - b
        if nq == 0:
            return [], []
        so = _lib.lib()
        counts = t.empty(nq, dtype=t.int64, device=dev)
        _lib.check(so.dkm_radius_count_f64(
            ptr(Q), nq, X.stride(0), ptr(X), n, X.stride(0), d,
            float(epsilon), ptr(counts), stream_ptr()), "dkm_radius_count")
        c = counts.cpu().numpy()
        offsets = np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
        total = int(offsets[-1])
        off_d = t.from_numpy(offsets).to(dev)
        out_i = t.empty(max(total, 1), dtype=t.int64, device=dev)
        out_d = t.empty(max(total, 1), dtype=t.float64, device=dev)
        wsb = int(so.dkm_radius_workspace_bytes(nq, total))
        ws = t.empty(wsb, dtype=t.uint8, device=dev)
        _lib.check(so.dkm_radius_fill_f64(
            ptr(Q), nq, X.stride(0), ptr(X), n, X.stride(0), d,
            float(epsilon), ptr(off_d), ctypes.c_void_p(ws.data_ptr()), wsb,
            ptr(out_i), ptr(out_d), stream_ptr()), "dkm_radius_fill")
        idx = out_i[:total].cpu().numpy()
    neigh = [idx[offsets[i]:offsets[i + 1]] for i in range(nq)]
    core = [bool(c[i] >= min_samples) for i in range(nq)]
    return neigh, core


def _compute_neighbours_csr(epsilon, min_samples, begin_idx, end_idx,
                            subsets, device):
    m = _concat_csr(subsets)
    t = torch()
    dev = resolve(device)
    n, d = m.shape
    b, e = _slice_bounds(begin_idx, end_idx, n)
    nq = e - b
    if nq == 0:
        return [], []
    so = _lib.lib()
    with on(dev):
        indptr = t.from_numpy(m.indptr.astype(np.int64)).to(dev)
        indices = t.from_numpy(
            np.ascontiguousarray(m.indices, dtype=np.int32)).to(dev)
        data = t.from_numpy(
            np.ascontiguousarray(m.data, dtype=np.float64)).to(dev)
        if data.numel() == 0:  # keep valid device pointers
            indices = t.zeros(1, dtype=t.int32, device=dev)
            data = t.zeros(1, dtype=t.float64, device=dev)
        counts = t.empty(nq, dtype=t.int64, device=dev)
        f32 = 1 if getattr(m, "dkm_f32", False) else 0
        _lib.check(so.dkm_radius_count_csr_f64(
            ptr(indptr), ptr(indices), ptr(data), n, d, b, nq,
            float(epsilon), f32, ptr(counts), stream_ptr()),
            "dkm_radius_count_csr")
        c = counts.cpu().numpy()
        offsets = np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
        total = int(offsets[-1])
        off_d = t.from_numpy(offsets).to(dev)
        out_i = t.empty(max(total, 1), dtype=t.int64, device=dev)
        out_d = t.empty(max(total, 1), dtype=t.float64, device=dev)
        wsb = int(so.dkm_radius_workspace_bytes(nq, total))
        ws = t.empty(wsb, dtype=t.uint8, device=dev)
        _lib.check(so.dkm_radius_fill_csr_f64(
            ptr(indptr), ptr(indices), ptr(data), n, d, b, nq,
            float(epsilon), f32, ptr(off_d), ctypes.c_void_p(ws.data_ptr()),
            wsb, ptr(out_i), ptr(out_d), stream_ptr()),
            "dkm_radius_fill_csr")
        idx = out_i[:total].cpu().numpy()
    neigh = [idx[offsets[i]:offsets[i + 1]] for i in range(nq)]
    core = [bool(c[i] >= min_samples) for i in range(nq)]
    return neigh, core


def _concat_csr(subsets, who="compute_neighbours"):
    """The concatenated sparse samples as one CSR matrix with sorted column
    indices (``_concatenate_subsets`` -> ``vstack``, classes.py:144-150).
    Also the fit / query matrix of the sparse kNN (``who`` names the caller
    in the errors)."""
    import scipy.sparse as sp
    if not subsets:
        raise ValueError("%s: no Subsets" % who)
    parts = []
    for s in subsets:
        x = s.samples
        if not sp.issparse(x):
            raise ValueError("%s: sparse=True needs sparse Subsets" % who)
        parts.append(x)
    m = sp.csr_matrix(parts[0] if len(parts) == 1 else
                      sp.vstack(parts, format="csr"))
    f32 = m.dtype == np.float32   # sklearn's float32 (upcast) path
    m = sp.csr_matrix(m, dtype=np.float64)
    if not m.has_sorted_indices:
        m = m.sorted_indices()
    if m.shape[1] > np.iinfo(np.int32).max:
        raise ValueError("%s: too many features" % who)
    # duplicate column entries in a row (legal while a scipy matrix is not
    # in canonical format): scipy's csr_matmat multiplies every stored pair
    # in stored order, which the kernel's merge of two sorted rows does not
    # reproduce -- refuse them loudly instead of returning other distances
    ind = m.indices
    if ind.size > 1:
        same = ind[1:] == ind[:-1]
        if same.any():
            row_start = np.zeros(ind.size, bool)
            row_start[m.indptr[:-1][np.diff(m.indptr) > 0]] = True
            if (same & ~row_start[1:]).any():
                raise ValueError(
                    "%s: sparse samples hold duplicate column entries; call "
                    "sum_duplicates() on them first" % who)
    _device_assert_finite(m.data)
    m.dkm_f32 = bool(f32)
    return m


def _concat(subsets, dev):
    """The concatenated samples as one fp64 (n, d) device matrix
    (``_concatenate_subsets``, classes.py:144-150)."""
    t = torch()
    if not subsets:
        raise ValueError("compute_neighbours: no Subsets")
    parts = []
    for s in subsets:
        x = s.samples
        if _is_torch(x):
            parts.append(x.to(dev, dtype=t.float64))
        else:
            if hasattr(x, "toarray"):
                raise ValueError("compute_neighbours: sparse Subsets are not"
                                 " supported by the GPU path")
            parts.append(t.from_numpy(np.ascontiguousarray(
                np.asarray(x, dtype=np.float64))).to(dev))
    X = parts[0] if len(parts) == 1 else t.cat(parts, 0)
    return X.contiguous()


def _slice_bounds(begin, end, n):
    """``samples[begin:end]`` bounds with Python slice semantics."""
    b, e, _ = slice(begin, end).indices(n)
    return b, max(b, e)
