"""``PCA`` -- principal component analysis of a Dataset that is resident in
HBM, the estimator later dislib releases ship as ``dislib.decomposition.PCA``
(covariance, then ``eigh``).  dislib v0.2.0, the tree this package follows,
has none; constructor and attributes are those of the later releases.

``PCA(n_components=None, arity=50, *, device=None)``: ``n_components=None``
keeps all ``n_features`` components; ``arity`` is stored as ``_arity`` and has
no effect, as in ``GaussianMixture``.

``fit`` reads the samples ONCE: ``dkm_pca_gram_*`` accumulates, in fp64 on the
f64 MFMA, the Gram matrix G of the augmented rows ``[x - p | 1]``, which holds
the scatter about the pivot p, the column sums ``s = sum(x - p)`` and the row
count together.  p is the mean of the first 1024 rows: with it the update
``G[:d,:d] - s s^T / n`` does not cancel when the mean is large against the
spread.  The ``(d + 1)^2`` matrix comes to the host, where numpy forms
``mean_ = p + s / n`` and ``cov = (G[:d,:d] - s s^T / n) / (n - 1)`` and runs
``np.linalg.eigh``.  The eigenpairs are put in descending order and every
component is flipped so that its entry of largest magnitude (the first on a
tie) is positive.

``transform`` returns a NEW Dataset of ``n_components`` features holding
``(x - mean_) components_^T`` in fp64 (``dkm_pca_project_*``: the mean is
subtracted element by element before the product), with the input's Subset
sizes and label objects; the input Dataset is not changed.  Residency follows
``StandardScaler``: the result is one device matrix; its Subsets are row views
of it when every input Subset held a device tensor, else row views of one host
copy.  Either way the new Dataset's HBM image is that matrix, so the
``KMeans.fit`` that follows uploads nothing.

Results are a function of the input only: the same bits from run to run.

Refusals: a sparse Dataset and a ``torch.distributed`` world larger than 1
raise ``NotImplementedError``; fewer than 2 samples, more than
``_lib.PCA_MAX_D`` features (the host ``eigh`` and the read-back bound it),
``n_components`` outside ``[1, n_features]``, a non-finite Gram matrix, a
Dataset of another feature count in ``transform`` and buffers that would leave
less than 4 GiB of HBM free raise ``ValueError``; ``transform`` before ``fit``
raises sklearn's ``NotFittedError``.
"""
import numpy as np

from .. import _lib, _shard
from ..data import Dataset, Subset


class PCA(object):
    """Principal component analysis on MI355X (see the module docstring).

    Attributes
    ----------
    components_ : ndarray, shape (n_components, n_features)
        The principal axes, by decreasing explained variance.
    explained_variance_ : ndarray, shape (n_components,)
    explained_variance_ratio_ : ndarray, shape (n_components,)
        ``explained_variance_`` over the trace of the covariance.
    mean_ : ndarray, shape (n_features,)
    """

    def __init__(self, n_components=None, arity=50, *, device=None):
        self._n_components = n_components
        self._arity = arity
        self._device = device
        self.components_ = None
        self.explained_variance_ = None
        self.explained_variance_ratio_ = None
        self.mean_ = None

    def fit(self, dataset):
        """Compute the mean and the principal axes of ``dataset``."""
        n, d = self._checked(dataset)
        nc = d if self._n_components is None else self._n_components
        if n < 2:
            raise ValueError("PCA takes at least 2 samples, got %d" % n)
        if d > _lib.PCA_MAX_D:
            raise ValueError("PCA takes at most %d features, got %d"
                             % (_lib.PCA_MAX_D, d))
        if not (isinstance(nc, (int, np.integer)) and 1 <= nc <= d):
            raise ValueError("n_components must be an integer in [1, %d], got "
                             "%r" % (d, nc))
        _lib.lib()                          # no GPU / no libdkm: raise here
        from .._device import on, pca_gram, pca_pivot, preload
        dd = dataset._device_data(self._device)
        with on(dd.device):
            preload(dd.device)
            pivot = pca_pivot(dd)
            G = pca_gram(dd, pivot).cpu().numpy()
            p = pivot.cpu().numpy()
        if not np.isfinite(G).all():
            raise ValueError("PCA: the samples' sums are not finite (NaN or "
                             "infinity in the input, or an overflow)")
        s = G[:d, d]
        self.mean_ = p + s / n
        cov = (G[:d, :d] - np.outer(s, s) / n) / (n - 1)
        lam, vec = np.linalg.eigh(cov)
        lam, vec = lam[::-1], vec[:, ::-1].T
        big = np.argmax(np.abs(vec), axis=1)            # the first on a tie
        vec = vec * np.where(vec[np.arange(d), big] < 0, -1.0, 1.0)[:, None]
        self.components_ = np.ascontiguousarray(vec[:nc])
        self.explained_variance_ = np.ascontiguousarray(lam[:nc])
        self.explained_variance_ratio_ = lam[:nc] / np.trace(cov)

    def fit_transform(self, dataset):
        """Fit to ``dataset``, then project it."""
        self.fit(dataset)
        return self.transform(dataset)

    def transform(self, dataset):
        """A new Dataset: the samples of ``dataset`` projected onto the
        principal axes."""
        if self.components_ is None:
            from sklearn.exceptions import NotFittedError
            raise NotFittedError(
                "This PCA instance is not fitted yet. Call 'fit' with "
                "appropriate arguments before using this estimator.")
        _, d = self._checked(dataset)
        if d != self.mean_.shape[0]:
            raise ValueError("PCA was fitted on %d features, the Dataset has "
                             "%d" % (self.mean_.shape[0], d))
        _lib.lib()
        from .._device import (DeviceData, _is_torch, on, pca_project, preload,
                               torch)
        t = torch()
        dd = dataset._device_data(self._device)
        subsets = list(dataset)
        on_device = bool(subsets) and all(_is_torch(s.samples)
                                          for s in subsets)
        nc = self.components_.shape[0]
        with on(dd.device):
            preload(dd.device)
            if dd.n:
                Y = pca_project(dd, t.from_numpy(self.mean_).to(dd.device),
                                t.from_numpy(self.components_).to(dd.device))
            else:
                Y = t.empty((0, nc), dtype=t.float64, device=dd.device)
            rows = Y if on_device else Y.cpu().numpy()
        out = Dataset(n_features=nc)
        for s, (a, b) in zip(subsets, dd.subset_slices()):
            sub = Subset.__new__(Subset)        # views: no copy of either
            sub.samples = rows[a:b]
            sub._labels, sub._pending = s.labels, None
            out.append(sub)
        out._adopt_device_data(DeviceData.from_matrix(Y, dd.sizes))
        return out

    # -- helpers ---------------------------------------------------------------
    def _checked(self, dataset):
        """(n, d) of a Dataset this estimator takes; touches no library."""
        if dataset.sparse:
            raise NotImplementedError(
                "PCA takes dense samples: centring a CSR matrix densifies it")
        if _shard.active():
            raise NotImplementedError(
                "PCA runs on one rank: a torch.distributed world larger than "
                "1 is not supported")
        n = sum(int(s.samples.shape[0]) for s in dataset)
        return n, int(dataset.n_features)
