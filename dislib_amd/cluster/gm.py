"""``GaussianMixture`` -- drop-in for ``dislib.cluster.GaussianMixture``
(dislib v0.2.0, ``dislib/cluster/gm/base.py:360-785``) running EM with full
covariance matrices on a Dataset that is resident in HBM.

Same constructor, attributes and control flow as the reference:

* ``GaussianMixture(n_components=1, covariance_type='full', tol=1e-3,
  reg_covar=1e-6, max_iter=100, init_params='kmeans', weights_init=None,
  means_init=None, precisions_init=None, arity=50, verbose=False,
  random_state=None)`` stores the public attributes of the same names and
  ``_arity`` / ``_verbose``; ``_check_initial_parameters`` (:684-711) raises
  the reference's ValueErrors;
* ``fit`` runs ``_fit`` and one more E-step whose result is dropped;
  ``fit_predict`` and ``predict`` assign ``resp.argmax(axis=1)`` (numpy's
  first maximum) to every ``subset.labels`` as an int64 array; ``predict``
  before a fit raises sklearn's ``NotFittedError``;
* ``n_iter`` is assigned only on convergence: a run that hits ``max_iter``
  keeps ``n_iter == 0`` and ``converged_ == False`` and emits sklearn's
  ``ConvergenceWarning``; ``lower_bound_ = total / count`` of the last
  E-step of the loop;
* ``init_params='kmeans'`` draws ``random_state.randint(0, int(1e8))`` and
  runs this package's ``KMeans(n_components, random_state=seed,
  verbose=...).fit_predict`` (kept as ``self.kmeans``); the one-hot
  responsibilities are built from its labels on the device.
  ``init_params='random'`` draws one ``randint(np.iinfo(np.int32).max,
  size=n_subsets)`` over the Subsets of all ranks; every Subset's
  ``RandomState(seed).rand(n_s, K)`` is generated and normalised on the host
  as :780-784 and uploaded.  ``weights_init`` / ``means_init`` /
  ``precisions_init`` follow :748-767 (``covariances_`` is not set when
  ``precisions_init`` is given);
* ``weights_``, ``means_``, ``covariances_`` and ``precisions_cholesky_`` are
  host ndarrays of the reference's shapes.

Where the work runs.  What is n rows long runs in ``dkm_gm.hip``, in fp64 on
the f64 MFMA whatever the samples' dtype (numpy promotes fp32 and integer
samples in ``matmul(x, P)``, ``x - mean`` and ``resp.T @ x``; fp32 rows are
widened in the kernels' loads, integer samples are uploaded as fp64): the
E-step (``dkm_gm_estep_*``: responsibilities, labels and the sum of
``log_prob_norm``), ``[nk | resp^T X]`` (``dkm_gm_mstep_sums_*``) and, as a
second pass around the new means like the reference's, the weighted scatter
matrices (``dkm_gm_mstep_cov_*``).  What is K d or K d^2 in size stays on the
host in numpy / scipy exactly as :48-55 and :134-192: ``nk += 10 eps``, the
divisions, ``reg_covar`` on the diagonal, ``linalg.cholesky`` and
``solve_triangular``, and the reference's ValueError for an ill-defined
covariance.  That costs two small device-to-host copies per iteration.

Determinism.  There is no fast-math and no floating-point atomic: every sum
over rows is partials of fixed row ranges added in a fixed order, and the
launch grids depend on (n, d, K) only.  The same input on one rank gives the
same bits from run to run.  The order is not the reference's (per-Subset
BLAS calls merged by the ``arity`` tree), so parameters agree to rounding
(about 1e-12 relative on well-conditioned data), not bit for bit, and
``arity`` has no effect.

Refusals.  A sparse Dataset raises ``NotImplementedError``.  The valid but
unimplemented ``covariance_type`` values ``'tied'``, ``'diag'`` and
``'spherical'`` raise ``NotImplementedError`` at ``fit`` (the reference dies
there with ``KeyError``).  The responsibilities stay resident as one (n, K)
fp64 matrix; when allocating it would leave less than 4 GiB of HBM free,
``fit`` / ``predict`` raise ``ValueError`` (the rule of
``KMeans(sums="reference")``).

Under ``torch.distributed`` with more than one rank every rank passes its
own shard Dataset (:func:`dislib_amd.shard_dataset`); an iteration all-reduces
``[n | nk | resp^T X]``, the scatter matrices and ``[log_prob_sum | count]``,
and every rank ends with identical parameters.
"""
import warnings

import numpy as np
from numpy.random.mtrand import RandomState
from scipy import linalg

from .. import _lib, _shard
from .kmeans import KMeans

_ILL_DEFINED = (
    "Fitting the mixture model failed because some components have "
    "ill-defined empirical covariance (for instance caused by singleton "
    "or collapsed samples). Try to decrease the number of components, "
    "or increase reg_covar.")


def _compute_precision_cholesky(covariances):
    """gm/base.py:168-178 (covariance_type='full')."""
    n_components, n_features, _ = covariances.shape
    precisions_chol = np.empty((n_components, n_features, n_features))
    for k, covariance in enumerate(covariances):
        try:
            cov_chol = linalg.cholesky(covariance, lower=True)
        except linalg.LinAlgError:
            raise ValueError(_ILL_DEFINED)
        precisions_chol[k] = linalg.solve_triangular(cov_chol,
                                                     np.eye(n_features),
                                                     lower=True).T
    return precisions_chol


def _compute_log_det_cholesky(matrix_chol, n_features):
    """gm/base.py:332-336."""
    n_components, _, _ = matrix_chol.shape
    return np.sum(np.log(
        matrix_chol.reshape(n_components, -1)[:, ::n_features + 1]), 1)


class GaussianMixture:
    """Gaussian mixture model (full covariances) fitted by EM on MI355X.

    Parameters and attributes match ``dislib.cluster.GaussianMixture``;
    ``device`` is a keyword-only extension (see the module docstring).
    """

    def __init__(self, n_components=1, covariance_type='full', tol=1e-3,
                 reg_covar=1e-6, max_iter=100, init_params='kmeans',
                 weights_init=None, means_init=None, precisions_init=None,
                 arity=50, verbose=False, random_state=None, *, device=None):
        self.n_components = n_components
        self.tol = tol
        self.reg_covar = reg_covar
        self.max_iter = max_iter
        self.init_params = init_params
        self._arity = arity
        self._verbose = verbose
        self.random_state = random_state
        self.covariance_type = covariance_type
        self.weights_init = weights_init
        self.means_init = means_init
        self.precisions_init = precisions_init
        self._device = device

    # -- public API (gm/base.py:488-543) --------------------------------------
    def fit(self, dataset):
        """Estimate model parameters with the EM algorithm."""
        em = self._fit(dataset)
        # the reference's final E-step; its result is dropped
        em.e_step(self, None)

    def fit_predict(self, dataset):
        """Estimate the parameters and set the Subsets' labels."""
        em = self._fit(dataset)
        em.assign_predictions(self, dataset)

    def predict(self, dataset):
        """Set every sample's label to its most probable component."""
        from sklearn.exceptions import NotFittedError
        if not all(hasattr(self, a) for a in ('weights_', 'means_',
                                              'precisions_cholesky_')):
            raise NotFittedError(
                "This GaussianMixture instance is not fitted yet. Call 'fit' "
                "with appropriate arguments before using this estimator.")
        em = _EM(self._resident(dataset), self.n_components)
        em.assign_predictions(self, dataset)

    # -- EM loop (gm/base.py:545-580) -------------------------------------------
    def _fit(self, dataset):
        self._check_initial_parameters()
        if self.covariance_type != 'full':
            raise NotImplementedError(
                "covariance_type=%r is not implemented (only 'full' is, as "
                "in the reference)" % self.covariance_type)
        dd = self._resident(dataset)

        self.converged_ = False
        self.n_iter = 0

        from sklearn.utils import validation
        random_state = validation.check_random_state(self.random_state)

        em = self._initialize_parameters(dataset, dd, random_state)
        self.lower_bound_ = -np.inf
        if self._verbose:
            print("GaussianMixture EM algorithm start")
        for n_iter in range(1, self.max_iter + 1):
            prev_lower_bound = self.lower_bound_

            log_prob_total, log_prob_count = em.e_step(self, None)
            em.m_step(self)
            self.lower_bound_ = log_prob_total / log_prob_count

            diff = abs(self.lower_bound_ - prev_lower_bound)

            if self._verbose:
                print("Iteration %s - Convergence crit. = %s" % (n_iter, diff))

            if diff < self.tol:
                self.converged_ = True
                self.n_iter = n_iter
                break

        if not self.converged_:
            from sklearn.exceptions import ConvergenceWarning
            warnings.warn('The algorithm did not converge. '
                          'Try different init parameters, '
                          'or increase max_iter, tol '
                          'or check for degenerate data.',
                          ConvergenceWarning)
        return em

    def _resident(self, dataset):
        if dataset.sparse:
            raise NotImplementedError(
                "GaussianMixture takes dense samples: the reference's CSR "
                "path forms the scatter matrices row by row in Python")
        _lib.lib()                          # no GPU / no libdkm: raise here
        return dataset._device_data(self._device)

    def _check_initial_parameters(self):
        """Check values of the basic parameters (gm/base.py:684-711)."""
        if self.n_components < 1:
            raise ValueError("Invalid value for 'n_components': %d "
                             "Estimation requires at least one component"
                             % self.n_components)

        if self.tol < 0.:
            raise ValueError("Invalid value for 'tol': %.5f "
                             "Tolerance used by the EM must be non-negative"
                             % self.tol)

        if self.max_iter < 1:
            raise ValueError("Invalid value for 'max_iter': %d "
                             "Estimation requires at least one iteration"
                             % self.max_iter)

        if self.reg_covar < 0.:
            raise ValueError("Invalid value for 'reg_covar': %.5f "
                             "regularization on covariance must be "
                             "non-negative"
                             % self.reg_covar)

        if self.covariance_type not in ['spherical', 'tied', 'diag', 'full']:
            raise ValueError("Invalid value for 'covariance_type': %s "
                             "'covariance_type' should be in "
                             "['spherical', 'tied', 'diag', 'full']"
                             % self.covariance_type)

    def _initialize_parameters(self, dataset, dd, random_state):
        """gm/base.py:713-767; returns the fit's device state."""
        from .._device import gm_onehot, on, torch
        t = torch()
        n_components = self.n_components
        if self.init_params == 'kmeans':
            if self._verbose:
                print("KMeans initialization start")
            seed = random_state.randint(0, int(1e8))
            kmeans = KMeans(n_clusters=n_components, random_state=seed,
                            verbose=self._verbose, device=self._device)
            kmeans.fit_predict(dataset)
            self.kmeans = kmeans
            em = _EM(dd, n_components)
            with on(dd.device):
                labels = dataset._device_labels()
                if labels is None and dd.n:
                    host = np.concatenate([np.asarray(s.labels).astype(int)
                                           for s in dataset])
                    labels = t.from_numpy(host.astype(np.int32)).to(dd.device)
                if dd.n:
                    gm_onehot(labels, em.resp)
        elif self.init_params == 'random':
            first, total = _shard.subset_slots(len(dd.sizes), dd.device)
            seeds = random_state.randint(np.iinfo(np.int32).max, size=total)
            em = _EM(dd, n_components)
            chunks = []
            for i, n_samples in enumerate(dd.sizes):
                # _random_resp_subset (:779-784)
                resp_chunk = RandomState(seeds[first + i]).rand(n_samples,
                                                                n_components)
                resp_chunk /= resp_chunk.sum(axis=1)[:, np.newaxis]
                chunks.append(resp_chunk)
            if dd.n:
                em.resp.copy_(t.from_numpy(np.concatenate(chunks)))
        else:
            raise ValueError("Unimplemented initialization method '%s'"
                             % self.init_params)

        weights, nk, means = em.estimate_parameters()

        self.weights_ = (weights if self.weights_init is None else
                         self.weights_init)
        self.means_ = means if self.means_init is None else self.means_init

        if self.precisions_init is None:
            cov, p_c = em.estimate_covariances(nk, means, self.reg_covar)
            self.covariances_ = cov
            self.precisions_cholesky_ = p_c
        else:
            self.precisions_cholesky_ = np.array(
                [linalg.cholesky(prec_init, lower=True)
                 for prec_init in self.precisions_init])
        return em


class _EM:
    """Device state of one fit or predict: the resident samples, the (n, K)
    responsibilities, the kernels' workspace and the small all-reduce
    buffers."""

    def __init__(self, dd, n_components):
        from .._device import alloc_resp, gm_workspace, on, preload, torch
        t = torch()
        self.dd = dd
        self.k, self.d = int(n_components), dd.d
        k, d = self.k, self.d
        with on(dd.device):
            preload(dd.device)
            self.resp = alloc_resp(dd, k)
            self.ws = gm_workspace(dd, k)
            self.labels = None
            # [n | nk | resp^T X], the scatter matrices, [log_prob_sum | n]
            self.head = t.zeros(1 + k + k * d, dtype=t.float64,
                                device=dd.device)
            self.cov = t.empty((k, d, d), dtype=t.float64, device=dd.device)
            self.lpn = t.zeros(2, dtype=t.float64, device=dd.device)

    def _dev(self, a):
        t = self._t()
        return t.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(
            self.dd.device)

    @staticmethod
    def _t():
        from .._device import torch
        return torch()

    # -- E-step (gm/base.py:201-307, :582-635) ----------------------------------
    def e_step(self, gm, labels):
        """(log_prob_total, count) over all ranks; fills ``self.resp`` and
        ``labels`` (a device int64 vector, or None)."""
        from .._device import gm_estep, on
        means = np.asarray(gm.means_, dtype=np.float64)
        pc = np.asarray(gm.precisions_cholesky_, dtype=np.float64)
        k, d = self.k, self.d
        if means.shape != (k, d) or pc.shape != (k, d, d):
            raise ValueError(
                "the model has parameters of shapes %s / %s, the Dataset "
                "takes (%d, %d) / (%d, %d, %d)"
                % (means.shape, pc.shape, k, d, k, d, d))
        with np.errstate(all="ignore"):
            ldw = _compute_log_det_cholesky(pc, d) + np.log(
                np.asarray(gm.weights_, dtype=np.float64))
        upper = not np.tril(pc, -1).any()
        with on(self.dd.device):
            self.lpn[1] = float(self.dd.n)
            gm_estep(self.dd, self._dev(means), self._dev(pc),
                     self._dev(ldw), upper, self.ws, self.resp, labels,
                     self.lpn[:1])
            _shard.allreduce_sum_(self.lpn)
            total, count = self.lpn.tolist()
        return total, int(count)

    def assign_predictions(self, gm, dataset):
        """An E-step whose argmax goes to the Subsets' labels (:350-357)."""
        from .._device import on
        t = self._t()
        with on(self.dd.device):
            labels = t.empty(max(self.dd.n, 1), dtype=t.int64,
                             device=self.dd.device)
            self.e_step(gm, labels)
            host = labels[:self.dd.n].cpu().numpy()
        for s, (a, b) in zip(dataset, self.dd.subset_slices()):
            s.labels = host[a:b]
        dataset._labels = None

    # -- M-step (gm/base.py:19-55, :103-141, :637-657) --------------------------
    def m_step(self, gm):
        weights, nk, means = self.estimate_parameters()
        gm.weights_ = weights
        gm.means_ = means
        cov, p_c = self.estimate_covariances(nk, means, gm.reg_covar)
        gm.covariances_ = cov
        gm.precisions_cholesky_ = p_c

    def estimate_parameters(self):
        from .._device import gm_mstep_sums, on
        k, d = self.k, self.d
        with on(self.dd.device):
            self.head[0] = float(self.dd.n)
            gm_mstep_sums(self.dd, self.resp, self.ws, self.head[1:])
            _shard.allreduce_sum_(self.head)
            host = self.head.cpu().numpy()
        n_samples = int(host[0])
        # aggregate_parameters (:48-55)
        nk = host[1:1 + k].copy()
        nk += 10 * np.finfo(nk.dtype).eps
        means = host[1 + k:].reshape(k, d) / nk[:, np.newaxis]
        weights = nk / n_samples
        return weights, nk, means

    def estimate_covariances(self, nk, means, reg_covar):
        from .._device import gm_mstep_cov, on
        with on(self.dd.device):
            gm_mstep_cov(self.dd, self.resp, self._dev(means), self.ws,
                         self.cov)
            _shard.allreduce_sum_(self.cov)
            covariances = self.cov.cpu().numpy()
        # _aggregate_covariances_full (:134-141)
        n_components, n_features, _ = covariances.shape
        for k in range(n_components):
            covariances[k] /= nk[k]
            covariances[k].flat[::n_features + 1] += reg_covar
        precisions_chol = _compute_precision_cholesky(covariances)
        return covariances, precisions_chol
