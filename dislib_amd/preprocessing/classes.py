"""``StandardScaler`` -- drop-in for ``dislib.preprocessing.StandardScaler``
(dislib v0.2.0, ``dislib/preprocessing/classes.py:7-147``) on a Dataset that
is resident in HBM.

Same constructor, attributes and arithmetic as the reference:

* ``StandardScaler(arity=50)`` stores ``_arity``; ``mean_`` and ``var_`` are
  None until fitted, then host ndarrays of shape ``(n_features,)``;
* ``fit``: per-Subset column sums (``_partial_sum``, :114-116), the ``arity``
  tree over ``(sum, n)`` (``_merge_sums``, :97-103, :119-123), ``mean = sum /
  n``, per-Subset column sums of ``(x - mean) ** 2`` (``_partial_var``,
  :126-129), the tree again (``_merge_vars``, :105-111, :132-134) and
  ``var_ = var / n`` (the population variance, :137-141);
* ``transform``: ``(x - mean) / sqrt(var)`` element by element (:144-147),
  assigned to the Subsets as NEW arrays; before a fit it raises
  ``Exception("Model has not been initialized.")`` (:91-92);
* a zero-variance column or a one-row Dataset gives numpy's NaN / inf;
* dtypes are numpy's: fp64 samples -> fp64 statistics and output; fp32
  samples -> fp32 statistics and output; integer samples -> fp64 (they are
  uploaded as fp64: exact while every \\|sum\\| < 2**53); fp32 samples scaled
  with fp64 statistics -> fp64 output.

``sums`` (keyword-only) selects the order of the sums, as in ``KMeans``:

``"fast"`` (the default): the two passes accumulate in fp64 (also for fp32
samples, whose mean stays fp64 for the second pass; ``mean_`` / ``var_`` are
rounded to fp32 once at the end) in block partials added in a fixed order
(dkm_col_stats_*): no floating-point atomic, the same bits from run to run
on one rank, within rounding of the reference, and ``arity`` has no effect.

``"reference"``: the reference's own order -- one sequential chain per
(Subset, column) in row order in the samples' dtype (dkm_col_chain_*),
merged by the ``arity`` tree as left folds (dkm_merge_tree; fp32 sums fold
in fp32).  ``mean_``, ``var_`` and the scaled samples are then bit-identical
to dislib's, from run to run and for any number of ranks.  Its parallelism
is Subsets x n_features chains, so a Dataset of few Subsets is slow in this
mode by definition of the order.  ``arity < 2`` with more than one Subset
(the reference never terminates) is a ValueError; ``n_features == 1`` is a
NotImplementedError (numpy sums a single column pairwise, not as a chain).

Sparse Datasets are refused (NotImplementedError): the reference's CSR path
goes through ``np.matrix`` and densifies.

Residency: ``transform`` writes ONE new (n, d) device matrix.  Subsets whose
samples were device tensors get row views of it; Subsets whose samples were
host ndarrays get row views of one host copy of it (a Dataset that mixes the
two gets host views everywhere).  Either way the Dataset's HBM image is
re-pointed at the scaled matrix, so the ``KMeans.fit`` / ``predict`` that
follows uploads nothing.  The caller's arrays are never written, cached
sample images are dropped and existing labels are untouched.

Under ``torch.distributed`` with more than one rank every rank passes its
own shard Dataset (:func:`dislib_amd.shard_dataset`); the statistics are
those of the whole Dataset on every rank.
"""
import numpy as np

from .. import _lib, _shard

_SUMS = ("fast", "reference")


class StandardScaler(object):
    """Standardize features by removing the mean and scaling to unit
    variance, on MI355X.  ``arity`` as in ``dislib.preprocessing
    .StandardScaler``; ``sums`` and ``device`` are keyword-only extensions
    (see the module docstring).

    Attributes
    ----------
    mean_ : ndarray, shape (n_features,)
    var_ : ndarray, shape (n_features,)
    """

    def __init__(self, arity=50, *, sums="fast", device=None):
        self._mean = None
        self._var = None
        self._arity = arity
        if sums not in _SUMS:
            raise ValueError("sums must be one of %s" % sorted(_SUMS))
        self._sums = sums
        self._device = device

    @property
    def mean_(self):
        return self._mean

    @property
    def var_(self):
        return self._var

    # -- public API (classes.py:50-95) ---------------------------------------
    def fit(self, dataset):
        """Compute the mean and variance used for later scaling."""
        dd = self._resident(dataset)
        from .._device import on
        with on(dd.device), np.errstate(all="ignore"):
            if self._sums == "reference":
                self._mean, self._var = _fit_reference(dd, self._arity)
            else:
                self._mean, self._var = _fit_fast(dd)

    def fit_transform(self, dataset):
        """Fit to data, then transform it."""
        self.fit(dataset)
        self.transform(dataset)

    def transform(self, dataset):
        """Standardize the samples of ``dataset``'s Subsets."""
        if self._mean is None or self._var is None:
            raise Exception("Model has not been initialized.")
        dd = self._resident(dataset)
        if dd.d != self._mean.shape[0]:
            raise ValueError("the scaler was fitted on %d features, the "
                             "Dataset has %d" % (self._mean.shape[0], dd.d))
        from .._device import DeviceData, on, scale_transform, torch
        t = torch()
        subsets = list(dataset)
        on_device = bool(subsets) and all(
            isinstance(s.samples, t.Tensor) for s in subsets)
        out = np.result_type(dd.dtype, self._mean.dtype)
        with on(dd.device):
            mean = t.from_numpy(np.ascontiguousarray(self._mean)).to(dd.device)
            var = t.from_numpy(np.ascontiguousarray(self._var)).to(dd.device)
            Y = t.empty((dd.n, dd.d), device=dd.device,
                        dtype=t.float32 if out == np.float32 else t.float64)
            scale_transform(dd, mean, var, Y)
            rows = Y if on_device else Y.cpu().numpy()
        for s, (a, b) in zip(subsets, dd.subset_slices()):
            s.samples = rows[a:b]           # new arrays, as classes.py:147
        dd.drop_images()
        dataset._adopt_device_data(DeviceData.from_matrix(Y, dd.sizes))

    # -- helpers ---------------------------------------------------------------
    def _resident(self, dataset):
        if dataset.sparse:
            raise NotImplementedError(
                "StandardScaler takes dense samples: the reference's CSR path "
                "goes through np.matrix and densifies")
        _lib.lib()                          # no GPU / no libdkm: raise here
        return dataset._device_data(self._device)


def _stat_dtype(dd):
    return np.float32 if dd.dtype == np.float32 else np.float64


def _fit_fast(dd):
    """Two dkm_col_stats_* passes in fp64; all-reduce of [sum | n], then of
    the squared deviations."""
    from .._device import col_stats, scale_workspace, torch
    t = torch()
    d = dd.d
    ws = scale_workspace(dd)
    head = np.zeros(d + 1)
    head[d] = dd.n
    buf = t.from_numpy(head).to(dd.device)
    col_stats(dd, None, ws, buf[:d])
    _shard.allreduce_sum_(buf)
    host = buf.cpu().numpy()
    n = int(host[d])
    mean = host[:d] / n
    dmean = t.from_numpy(mean).to(dd.device)
    var = t.empty(d, dtype=t.float64, device=dd.device)
    col_stats(dd, dmean, ws, var)
    _shard.allreduce_sum_(var)
    var = var.cpu().numpy() / n
    dt = _stat_dtype(dd)
    return mean.astype(dt), var.astype(dt)


def _fit_reference(dd, arity):
    """Per-Subset chains (dkm_col_chain_*), the slots of all ranks' Subsets
    all-reduced (adding +0.0 is exact and no chain ends in -0.0), the arity
    tree (dkm_merge_tree), the divisions in numpy on the host."""
    from .._device import ScaleSums, col_chain, merge_tree, torch
    t = torch()
    d = dd.d
    if d == 1:
        raise NotImplementedError(
            "sums='reference' takes n_features >= 2: numpy sums a single "
            "column pairwise, not as one chain in row order")
    first, total = _shard.subset_slots(len(dd.sizes), dd.device)
    sched, n_ops, n_slots = _shard.merge_schedule(total, arity)
    dt = _stat_dtype(dd)
    f32 = dt == np.float32
    ssum = ScaleSums(dd, first, total, sched, n_ops, n_slots)

    def tree(mean):
        ssum.reset(dd.sizes)
        col_chain(dd, mean, ssum)
        _shard.allreduce_sum_(ssum.partials)
        merge_tree(ssum, ssum.acc, f32)
        host = ssum.acc.cpu().numpy()
        # fp32 sums were widened exactly: back to the reference's dtype
        return host[:d].astype(dt), int(host[d])

    total_sum, n = tree(None)
    mean = total_sum / n                    # classes.py:128, :139
    total_var, _ = tree(t.from_numpy(np.ascontiguousarray(mean)).to(
        dd.device))
    return mean, total_var / n              # classes.py:140
