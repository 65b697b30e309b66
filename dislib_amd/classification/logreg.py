"""``LogisticRegression`` -- L2-penalised logistic (two classes) and softmax
(three or more) regression on a Dataset that is resident in HBM, shaped after
``sklearn.linear_model.LogisticRegression(solver="lbfgs")``.  dislib v0.2.0,
the tree this package follows, has no linear probabilistic classifier; in its
data model the targets are the Subsets' ``labels`` and ``predict`` writes the
class values into the labels.

``LogisticRegression(C=1.0, fit_intercept=True, tol=1e-4, max_iter=100, *,
device=None)`` minimises sklearn's objective

    (1 / n) sum_i loss_i + 1 / (2 C n) ||W||_F^2

(the intercept is not penalised): two classes use one logit column and the
binomial log-loss, K >= 3 classes K columns and the symmetric softmax.  The
optimiser is sklearn's: ``scipy.optimize.minimize(method="L-BFGS-B",
jac=True)`` on the host from zeros, ``gtol = tol``, ``ftol = 64 eps``,
``maxiter = max_iter``, ``maxls = 50``; so ``tol`` and ``n_iter_`` mean what
they mean there, and hitting ``max_iter`` emits sklearn's
``ConvergenceWarning``.

Every evaluation uploads the ``columns x (d + fit_intercept)`` weights,
launches ``dkm_logreg_lossgrad_*`` (logits, softmax and
gradient in ONE read of X, fp64 on the f64 MFMA) and brings ``[loss |
gradient]`` back in one small copy; the host adds the penalty and the
``1 / n``.  The encoded labels are uploaded once per fit.  Results are a
function of the input only: the same bits from run to run.

``predict`` stores the class values (not their indices): views of one device
vector when every Subset holds a device tensor and the classes are numbers,
else slices of one host array.  ``predict_proba`` and ``decision_function``
return host ndarrays, ``score`` the accuracy against the Subsets' labels.

Refusals, before the GPU library is touched: a sparse Dataset and a
``torch.distributed`` world larger than 1 raise ``NotImplementedError``;
``C <= 0``, ``tol < 0``, ``max_iter < 1``, a Subset without labels, labels
that are not one value per sample, no samples, fewer than 2 or more than
``_lib.LOGREG_MAX_CLASSES`` classes and more than ``_lib.LOGREG_MAX_D``
features raise ``ValueError``; ``predict*`` before ``fit`` raises sklearn's
``NotFittedError`` and a Dataset of another feature count ``ValueError``.
``fit`` raises ``ValueError`` on a non-finite loss or gradient (NaN or
infinity in the samples), and on a workspace that would leave less than 4 GiB
of HBM free.
"""
import warnings

import numpy as np

from .. import _lib, _shard


class LogisticRegression(object):
    """Logistic / softmax regression on MI355X (see the module docstring).

    Attributes
    ----------
    classes_ : ndarray, the sorted unique labels
    coef_ : ndarray, shape (1, n_features) for two classes, else
        (n_classes, n_features)
    intercept_ : ndarray, shape (1,) or (n_classes,); zeros without
        ``fit_intercept``
    n_iter_ : int
    """

    def __init__(self, C=1.0, fit_intercept=True, tol=1e-4, max_iter=100, *,
                 device=None):
        self.C = C
        self.fit_intercept = bool(fit_intercept)
        self.tol = tol
        self.max_iter = max_iter
        self._device = device
        self.classes_ = None
        self.coef_ = None
        self.intercept_ = None
        self.n_iter_ = None

    def fit(self, dataset):
        """Fit the Subsets' labels on their samples."""
        if not self.C > 0:
            raise ValueError("LogisticRegression: C must be positive, got %r"
                             % (self.C,))
        if not self.tol >= 0:
            raise ValueError("LogisticRegression: tol must be >= 0, got %r"
                             % (self.tol,))
        if not self.max_iter >= 1:
            raise ValueError("LogisticRegression: max_iter must be >= 1, got "
                             "%r" % (self.max_iter,))
        n, d = self._checked(dataset)
        labels = self._targets(dataset)
        if n < 1 or d < 1:
            raise ValueError("LogisticRegression takes at least 1 sample and "
                             "1 feature, got %d x %d" % (n, d))
        classes, codes = np.unique(labels, return_inverse=True)
        K = len(classes)
        if K < 2:
            raise ValueError("LogisticRegression needs samples of at least 2 "
                             "classes, got %d" % K)
        if K > _lib.LOGREG_MAX_CLASSES:
            raise ValueError("LogisticRegression takes at most %d classes, "
                             "got %d" % (_lib.LOGREG_MAX_CLASSES, K))
        if d > _lib.LOGREG_MAX_D:
            raise ValueError("LogisticRegression takes at most %d features, "
                             "got %d" % (_lib.LOGREG_MAX_D, d))
        _lib.lib()                          # no GPU / no libdkm: raise here
        from scipy.optimize import minimize
        from .._device import (logreg_lossgrad, logreg_workspace, on, preload,
                               torch)
        t = torch()
        fi = int(self.fit_intercept)
        cols = 1 if K == 2 else K
        l2 = 1.0 / (float(self.C) * n)
        dd = dataset._device_data(self._device)
        with on(dd.device):
            preload(dd.device)
            ws = logreg_workspace(dd, cols)
            y = t.from_numpy(np.ascontiguousarray(
                codes.reshape(-1).astype(np.int32))).to(dd.device)
            out = t.empty(1 + cols * (d + fi), dtype=t.float64,
                          device=dd.device)

            def func(theta):
                W = np.array(theta, dtype=np.float64).reshape(cols, d + fi)
                r = logreg_lossgrad(dd, y, t.from_numpy(W).to(dd.device), fi,
                                    ws, out).cpu().numpy()
                if not np.isfinite(r).all():
                    raise ValueError(
                        "LogisticRegression: the loss or its gradient is not "
                        "finite (NaN or infinity in the samples, or an "
                        "overflow)")
                G = r[1:].reshape(cols, d + fi) / n
                G[:, :d] += l2 * W[:, :d]
                f = r[0] / n + 0.5 * l2 * float(np.sum(W[:, :d] * W[:, :d]))
                return f, G.reshape(-1)

            res = minimize(
                func, np.zeros(cols * (d + fi)), method="L-BFGS-B", jac=True,
                options={"maxiter": int(self.max_iter), "maxls": 50,
                         "gtol": float(self.tol),
                         "ftol": 64 * np.finfo(np.float64).eps})
        if res.status == 1:
            from sklearn.exceptions import ConvergenceWarning
            warnings.warn(
                "lbfgs failed to converge after %d iteration(s) (status=1): "
                "increase the number of iterations (max_iter) or scale the "
                "data" % res.nit, ConvergenceWarning, stacklevel=2)
        W = np.asarray(res.x, dtype=np.float64).reshape(cols, d + fi)
        self.classes_ = classes
        self.coef_ = np.ascontiguousarray(W[:, :d])
        self.intercept_ = W[:, d].copy() if fi else np.zeros(cols)
        self.n_iter_ = int(min(res.nit, self.max_iter))
        return self

    def decision_function(self, dataset):
        """The logits as a host ndarray: (n,) for two classes, else (n, K)."""
        Z = self._run(dataset, logits=True)[0].cpu().numpy()
        return Z[:, 0] if Z.shape[1] == 1 else Z

    def predict_proba(self, dataset):
        """The class probabilities as a host (n, K) ndarray."""
        P = self._run(dataset, proba=True)[1].cpu().numpy()
        return np.hstack([1.0 - P, P]) if P.shape[1] == 1 else P

    def predict(self, dataset):
        """Write the predicted class values into the labels of ``dataset``."""
        from .._device import _is_torch, on, torch
        t = torch()
        L = self._run(dataset, labels=True)[2]
        dd = dataset._device_data(self._device)
        subsets = list(dataset)
        if subsets and all(_is_torch(s.samples) for s in subsets) and \
                self.classes_.dtype.kind in "biuf":
            with on(dd.device):
                rows = t.from_numpy(self.classes_).to(dd.device)[L.long()]
        else:
            rows = self.classes_[L.cpu().numpy()]
        for s, (a, b) in zip(subsets, dd.subset_slices()):
            s.labels = rows[a:b]
        dataset._labels = None

    def score(self, dataset):
        """The accuracy of the predictions against the Subsets' labels."""
        truth = self._targets(dataset)
        L = self._run(dataset, labels=True)[2].cpu().numpy()
        return float(np.mean(self.classes_[L] == truth))

    # -- helpers ---------------------------------------------------------------
    def _run(self, dataset, **what):
        """(logits, proba, labels) on the device, those asked for."""
        if self.coef_ is None:
            from sklearn.exceptions import NotFittedError
            raise NotFittedError(
                "This LogisticRegression instance is not fitted yet. Call "
                "'fit' with appropriate arguments before using this "
                "estimator.")
        n, d = self._checked(dataset)
        if d != self.coef_.shape[1]:
            raise ValueError("LogisticRegression was fitted on %d features, "
                             "the Dataset has %d" % (self.coef_.shape[1], d))
        _lib.lib()
        from .._device import logreg_predict, on, preload, torch
        t = torch()
        cols = self.coef_.shape[0]
        dd = dataset._device_data(self._device)
        with on(dd.device):
            preload(dd.device)
            if not dd.n:
                return (t.empty((0, cols), dtype=t.float64, device=dd.device),
                        t.empty((0, cols), dtype=t.float64, device=dd.device),
                        t.empty(0, dtype=t.int32, device=dd.device))
            W = self.coef_
            if self.fit_intercept:
                W = np.hstack([W, self.intercept_[:, None]])
            W = t.from_numpy(np.ascontiguousarray(W)).to(dd.device)
            return logreg_predict(dd, W, self.fit_intercept, **what)

    def _checked(self, dataset):
        """(n, d) of a Dataset this estimator takes; touches no library."""
        if dataset.sparse:
            raise NotImplementedError(
                "LogisticRegression takes dense samples: the CSR kernels are "
                "not built")
        if _shard.active():
            raise NotImplementedError(
                "LogisticRegression runs on one rank: a torch.distributed "
                "world larger than 1 is not supported")
        n = sum(int(s.samples.shape[0]) for s in dataset)
        return n, int(dataset.n_features)

    @staticmethod
    def _targets(dataset):
        """The Subsets' labels as one host vector."""
        parts = []
        for i, s in enumerate(dataset):
            lab = s.labels
            if lab is None:
                raise ValueError("LogisticRegression: Subset %d has no labels "
                                 "(the targets)" % i)
            if hasattr(lab, "cpu"):
                lab = lab.cpu().numpy()
            v = np.asarray(lab)
            if v.shape != (int(s.samples.shape[0]),) or v.dtype == object:
                raise ValueError("LogisticRegression: the labels of Subset %d "
                                 "are not one value per sample" % i)
            parts.append(v)
        return np.concatenate(parts) if parts else np.zeros(0)
