"""``LinearRegression`` -- ordinary least squares on a Dataset that is resident
in HBM, the estimator later dislib releases ship as
``dislib.regression.LinearRegression``.  dislib v0.2.0, the tree this package
follows, has none; in its data model the targets are the Subsets' ``labels``,
one number per sample, and ``predict`` writes its values into the labels.

``LinearRegression(fit_intercept=True, arity=50, *, device=None)``: ``arity``
is stored as ``_arity`` and has no effect, as in ``PCA``.

``fit`` reads the samples ONCE and never forms the normal equations, which
would square the condition number: ``dkm_tsqr_*`` reduces the
implicit matrix ``[1 | X | y]`` (``[X | y]`` without intercept) to its
``w x w`` upper-triangular Householder factor R in fp64, ``w = d + 1 +
fit_intercept``.  The ones column comes first, so the first reflector centres
every other column: ``R[0] = sqrt(n) [1, mean(X), mean(y)]`` and
``R[1:d+1, 1:d+1]``, ``R[1:d+1, -1]`` are the factor and the right-hand side
of the centred problem.  The ``w^2`` doubles come to the host, where
``scipy.linalg.lstsq`` (an SVD: the minimum-norm solution of a rank-deficient
or underdetermined system, as sklearn returns) gives ``coef_``, and
``intercept_ = (R[0,-1] - R[0,1:d+1] . coef_) / R[0,0]``.  Singular values
below ``eps w sqrt(n)`` times the largest are taken as zero: that is the size
of the rounding error R itself carries from its n rows (errors adding as a
random walk), so nothing below it is information about the samples.
``residual_norm_ = |R[-1,-1]|`` is the 2-norm of the residual.

``predict`` computes ``(x - mean_) . coef_ + mean(y)`` with the PCA projection
kernel (one component) and one addition, and stores it as fp64 labels: views
of one device vector when every Subset holds a device tensor, else slices of
one host copy.

Results are a function of the input only: the same bits from run to run.

Refusals, before the GPU library is touched: a sparse Dataset and a
``torch.distributed`` world larger than 1 raise ``NotImplementedError``; a
Subset without labels, labels that are not one finite number per sample, no
samples, and more than ``_lib.TSQR_MAX_W`` columns raise ``ValueError``;
``predict`` before ``fit`` raises sklearn's ``NotFittedError`` and a Dataset of
another feature count ``ValueError``.  After the kernel, a non-finite R (NaN
or infinity in the input, or squares beyond the fp64 range) and a workspace
that would leave less than 4 GiB of HBM free raise ``ValueError``.
"""
import numpy as np

from .. import _lib, _shard


class LinearRegression(object):
    """Ordinary least squares on MI355X (see the module docstring).

    Attributes
    ----------
    coef_ : ndarray, shape (n_features,)
    intercept_ : float
        ``0.0`` without ``fit_intercept``.
    residual_norm_ : float
    """

    def __init__(self, fit_intercept=True, arity=50, *, device=None):
        self._fit_intercept = bool(fit_intercept)
        self._arity = arity
        self._device = device
        self.coef_ = None
        self.intercept_ = None
        self.residual_norm_ = None
        self._mean = None
        self._ybar = 0.0

    def fit(self, dataset):
        """Least squares of the Subsets' labels on their samples."""
        n, d = self._checked(dataset)
        y = self._targets(dataset)
        fi = int(self._fit_intercept)
        w = d + 1 + fi
        if n < 1 or d < 1:
            raise ValueError("LinearRegression takes at least 1 sample and 1 "
                             "feature, got %d x %d" % (n, d))
        if w > _lib.TSQR_MAX_W:
            raise ValueError(
                "LinearRegression takes at most %d columns (features, target "
                "and intercept), got %d" % (_lib.TSQR_MAX_W, w))
        _lib.lib()                          # no GPU / no libdkm: raise here
        from scipy.linalg import lstsq
        from .._device import on, preload, torch, tsqr
        t = torch()
        dd = dataset._device_data(self._device)
        with on(dd.device):
            preload(dd.device)
            R = tsqr(dd, t.from_numpy(y).to(dd.device), fi).cpu().numpy()
        if not np.isfinite(R).all():
            raise ValueError("LinearRegression: the factor R is not finite "
                             "(NaN or infinity in the input, or an overflow)")
        A, b = R[fi:d + fi, fi:d + fi], R[fi:d + fi, -1]
        cond = np.finfo(np.float64).eps * w * np.sqrt(n)
        self.coef_ = np.ascontiguousarray(lstsq(A, b, cond=cond)[0])
        if fi:
            self.intercept_ = float((R[0, -1] - R[0, 1:d + 1] @ self.coef_) /
                                    R[0, 0])
            self._mean = R[0, 1:d + 1] / np.sqrt(n)
            self._ybar = float(R[0, -1] / np.sqrt(n))
        else:
            self.intercept_ = 0.0
            self._mean, self._ybar = np.zeros(d), 0.0
        self.residual_norm_ = float(abs(R[-1, -1]))

    def predict(self, dataset):
        """Write the predicted values into the labels of ``dataset``."""
        if self.coef_ is None:
            from sklearn.exceptions import NotFittedError
            raise NotFittedError(
                "This LinearRegression instance is not fitted yet. Call 'fit' "
                "with appropriate arguments before using this estimator.")
        _, d = self._checked(dataset)
        if d != self.coef_.shape[0]:
            raise ValueError("LinearRegression was fitted on %d features, the "
                             "Dataset has %d" % (self.coef_.shape[0], d))
        _lib.lib()
        from .._device import _is_torch, on, pca_project, preload, torch
        t = torch()
        dd = dataset._device_data(self._device)
        subsets = list(dataset)
        on_device = bool(subsets) and all(_is_torch(s.samples)
                                          for s in subsets)
        with on(dd.device):
            preload(dd.device)
            if dd.n:
                Y = pca_project(dd, t.from_numpy(self._mean).to(dd.device),
                                t.from_numpy(self.coef_[None]).to(dd.device))
                Y = Y[:, 0]
                if self._fit_intercept:
                    Y = Y + self._ybar
            else:
                Y = t.empty(0, dtype=t.float64, device=dd.device)
            rows = Y if on_device else Y.cpu().numpy()
        for s, (a, b) in zip(subsets, dd.subset_slices()):
            s.labels = rows[a:b]
        dataset._labels = None

    # -- helpers ---------------------------------------------------------------
    def _checked(self, dataset):
        """(n, d) of a Dataset this estimator takes; touches no library."""
        if dataset.sparse:
            raise NotImplementedError(
                "LinearRegression takes dense samples: the QR of a CSR matrix "
                "is not built")
        if _shard.active():
            raise NotImplementedError(
                "LinearRegression runs on one rank: a torch.distributed world "
                "larger than 1 is not supported")
        n = sum(int(s.samples.shape[0]) for s in dataset)
        return n, int(dataset.n_features)

    @staticmethod
    def _targets(dataset):
        """The Subsets' labels as one fp64 host vector."""
        parts = []
        for i, s in enumerate(dataset):
            lab = s.labels
            if lab is None:
                raise ValueError("LinearRegression: Subset %d has no labels "
                                 "(the targets)" % i)
            if hasattr(lab, "cpu"):
                lab = lab.cpu().numpy()
            try:
                v = np.asarray(lab).astype(np.float64)
            except (TypeError, ValueError):
                v = None
            if v is None or v.shape != (int(s.samples.shape[0]),) or \
                    not np.isfinite(v).all():
                raise ValueError("LinearRegression: the labels of Subset %d "
                                 "are not one finite number per sample" % i)
            parts.append(v)
        return np.ascontiguousarray(np.concatenate(parts)) if parts else \
            np.zeros(0)
