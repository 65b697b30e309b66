"""``CascadeSVM`` -- drop-in for ``dislib.classification.CascadeSVM`` (dislib
v0.2.0, ``dislib/classification/csvm/base.py``) on a dense Dataset that is
resident in HBM.

Same constructor, asserts, private attributes, ``fit`` / ``predict`` /
``decision_function`` / ``score``, ``iterations`` and ``converged`` as the
reference, plus the keyword-only ``device``.

What is kept of the reference, line by line:

* The cascade (``base.py:217-257``): one first-level node per Subset, joined
  with the feedback (the last layer's support vectors) when there is one;
  the queue is reduced by popping its first ``arity`` entries until at most
  ``arity`` are left; the last layer trains on what is left; ``iterations +=
  1``.  ``_merge`` (``:381-398``) concatenates and keeps the first occurrence
  of every id in order.  The id of a sample is its global row number (the
  reference draws a ``uuid4`` per row), so a row can never enter a node twice.
* The classifier is collected after the last layer when ``check_convergence``
  or in the last iteration (``:247``); ``_clf`` is ``None`` otherwise.
* The convergence quantity ``W`` (``_lagrangian_fast``, ``:259-274``) as the
  reference computes it: the signed ``dual_coef_``, the raw labels with only
  ``0`` mapped to ``-1``, and the reference's own ``_rbf_kernel``
  (``:305-318``), which evaluates to ``exp(+gamma |x_i - x_j|^2)`` -- so ``W``
  overflows easily, and a non-finite ``W`` never converges.  ``if
  self._last_w:`` stays a truthiness test (``:284``).

What differs: a node is an index list into the resident samples and is
solved on the GPU by a working-set decomposition (``dkm_svm.hip``: up to
``dislib_amd._lib.SVM_QMAX`` rows per working set, libsvm's second-order
SMO inside it) to libsvm's stopping rule ``m(alpha) - M(alpha) < 1e-3`` (SVC's
default ``tol``; the reference passes none).  libsvm's solution is itself
only defined up to that tolerance, so support vectors, coefficients and
decision values agree with the reference within it, not bit for bit.  The
outer loop is capped: exceeding the cap raises ``RuntimeError`` with the gap
reached.

``_clf`` carries ``support_`` (global row numbers), ``support_vectors_``,
``dual_coef_`` (1 x n_SV), ``intercept_``, ``classes_`` and ``n_support_``
with sklearn's binary conventions: ``classes_`` sorted, support vectors
grouped by class, ``decision > 0`` means ``classes_[1]``, ``dual_coef_``
positive for ``classes_[1]``.  The intercept follows libsvm's
``calculate_rho``: the mean of ``y grad`` over the free vectors, else the
midpoint of the bounds.

Limits, each a loud error: binary problems only (a node that sees one class
raises ``ValueError`` as libsvm does, more than two classes raise
``ValueError``); dense Datasets only (CSR raises ``NotImplementedError``;
fp32 samples are widened in the kernels' loads); one rank only
(``NotImplementedError`` in a ``torch.distributed`` world larger than 1).
``random_state`` is stored and otherwise unused: libsvm uses it only for
probability estimates.
"""
import numpy as np

from .. import _lib
from .._device import on, preload, ptr, stream_ptr, torch

# libsvm's stopping tolerance (SVC's default ``tol``) and the tolerance of
# the solver inside a working set
EPS = 1e-3
INNER_EPS = 1e-4
# SMO steps inside one working set, at the most
MAX_INNER = 100000


def max_outer(m, q):
    """Working sets a node of ``m`` rows may take before the fit gives up."""
    return 1000 + 100 * ((m + q - 1) // q)


def working_set_size(m):
    """Rows of a working set for a node of ``m`` rows: the whole node (made
    even) up to ``SVM_QMAX``."""
    return min(_lib.SVM_QMAX, m + (m & 1))


def _merge(id_lists):
    """The ids of ``_merge`` / ``_merge_pair`` (``base.py:381-398``): pair by
    pair, concatenate and keep the first occurrence of every id in order."""
    ids = np.asarray(id_lists[0])
    for other in id_lists[1:]:
        ids = np.concatenate((ids, np.asarray(other)))
        ids, uniques = np.unique(ids, return_index=True)
        ids = ids[np.argsort(uniques)]
    return ids


def intercept(alpha, f, y, c):
    """libsvm's ``calculate_rho``, negated: ``f = y * gradient``."""
    ub, lb, nr_free, sum_free = np.inf, -np.inf, 0, 0.0
    for a, yg, yi in zip(alpha, f, y):
        if a >= c:
            if yi < 0:
                ub = min(ub, yg)
            else:
                lb = max(lb, yg)
        elif a <= 0:
            if yi > 0:
                ub = min(ub, yg)
            else:
                lb = max(lb, yg)
        else:
            nr_free += 1
            sum_free += yg
    rho = sum_free / nr_free if nr_free > 0 else (ub + lb) / 2
    return -rho


class _Model(object):
    """What a fitted node leaves, with sklearn's attribute names."""

    def __init__(self, support, dual_coef, b, classes, n_support, fit):
        self.support_ = support
        self.dual_coef_ = dual_coef
        self.intercept_ = np.array([b])
        self.classes_ = classes
        self.n_support_ = n_support
        self._fit = fit
        self._sv = None

    @property
    def support_vectors_(self):
        if self._sv is None:
            t = torch()
            idx = t.from_numpy(self.support_.astype(np.int64)).to(
                self._fit.X.device)
            self._sv = self._fit.X[idx].to(t.float64).cpu().numpy()
        return self._sv


class _Fit(object):
    """The device side of one fit: the resident samples, the +1 / -1 labels,
    the squared norms (rbf) and the kernel."""

    def __init__(self, so, dd, raw, classes, kernel, gamma, c):
        t = torch()
        self.so, self.X, self.n, self.d = so, dd.X, dd.n, dd.d
        self.device = dd.device
        self.f32 = dd.dtype == np.float32
        self.ldx = dd.X.stride(0)
        self.kernel = _lib.SVM_RBF if kernel == "rbf" else _lib.SVM_LINEAR
        self.gamma = float(gamma) if kernel == "rbf" else 0.0
        self.c = float(c)
        self.raw, self.classes = raw, classes
        self.ysign = np.where(raw == classes[-1], 1.0, -1.0)
        self.y = t.from_numpy(self.ysign).to(self.device)
        self.norms = norms(so, dd.X, self.f32) if self.kernel else None

    def solve(self, ids):
        """(alpha, f, y) of the node ``ids`` as host arrays."""
        t = torch()
        rows = t.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(
            self.device)
        y = self.y[rows.long()].contiguous()
        alpha, f = solve_node(self.so, self.X, self.f32, rows, y, self.norms,
                              self.kernel, self.gamma, self.c)
        return alpha.cpu().numpy(), f.cpu().numpy(), y.cpu().numpy()


def norms(so, X, f32):
    """fp64 device vector of every row's squared norm."""
    t = torch()
    out = t.empty(X.shape[0], dtype=t.float64, device=X.device)
    fn = so.dkm_svm_norms_f32 if f32 else so.dkm_svm_norms_f64
    _lib.check(fn(ptr(X), X.shape[0], X.shape[1], X.stride(0), ptr(out),
                  stream_ptr()), "dkm_svm_norms")
    return out


def solve_node(so, X, f32, rows, y, xnorm, kernel, gamma, c, q=None,
               eps=EPS, stats=None):
    """The dual solution of the node ``rows`` (device int32) with labels
    ``y`` (device fp64, +1 / -1): device ``(alpha, f)``.  The host drives the
    outer loop -- select, one scalar read back, rows, local solve, update --
    and raises ``RuntimeError`` past ``max_outer`` working sets."""
    t = torch()
    dev = X.device
    m = int(rows.shape[0])
    q = working_set_size(m) if q is None else int(q)
    alpha = t.zeros(m, dtype=t.float64, device=dev)
    f = -y.clone()
    ws = t.empty(q, dtype=t.int32, device=dev)
    mark = t.empty(m, dtype=t.int32, device=dev)
    gap = t.empty(3, dtype=t.float64, device=dev)
    K = t.empty((q, m), dtype=t.float64, device=dev)
    dy = t.empty(q, dtype=t.float64, device=dev)
    info = t.empty(2, dtype=t.int32, device=dev)
    rows_fn = so.dkm_svm_rows_f32 if f32 else so.dkm_svm_rows_f64
    s = stream_ptr()
    cap = max_outer(m, q)
    g = np.inf
    for it in range(cap + 1):
        _lib.check(so.dkm_svm_select(ptr(f), ptr(alpha), ptr(y), m, c, q,
                                     ptr(ws), ptr(gap), ptr(mark), s),
                   "dkm_svm_select")
        g = float(gap[0].item())
        if g < eps:
            if stats is not None:
                stats["outer"] = it
                stats["gap"] = g
            return alpha, f
        if it == cap:
            break
        _lib.check(rows_fn(ptr(X), X.shape[0], X.shape[1], X.stride(0),
                           ptr(rows), m, ptr(ws), q, ptr(xnorm), kernel,
                           gamma, ptr(K), m, s), "dkm_svm_rows")
        _lib.check(so.dkm_svm_local(ptr(K), m, ptr(ws), q, ptr(y), ptr(alpha),
                                    ptr(f), m, c, min(INNER_EPS, 0.1 * eps),
                                    MAX_INNER, ptr(dy), ptr(info), s),
                   "dkm_svm_local")
        _lib.check(so.dkm_svm_update(ptr(K), m, q, ptr(dy), ptr(f), m, s),
                   "dkm_svm_update")
    raise RuntimeError(
        "CascadeSVM: a node of %d rows did not reach m(alpha) - M(alpha) < "
        "%g within %d working sets of %d rows; the gap reached is %g"
        % (m, eps, cap, q, g))


def decision_values(so, Q, q32, X, x32, sv, coef, b, xnorm, kernel, gamma):
    """Device fp64 decision values of the rows of ``Q`` against the support
    rows ``sv`` (device int32) of ``X``."""
    t = torch()
    nq = int(Q.shape[0])
    out = t.empty(nq, dtype=t.float64, device=Q.device)
    if nq == 0:
        return out
    qnorm = norms(so, Q, q32) if kernel else None
    fn = so.dkm_svm_decision_f32 if q32 else so.dkm_svm_decision_f64
    _lib.check(fn(ptr(Q), nq, Q.shape[1], Q.stride(0), ptr(X),
                  1 if x32 else 0, X.shape[0], X.stride(0), ptr(sv),
                  int(sv.shape[0]), ptr(coef), float(b), ptr(qnorm),
                  ptr(xnorm), kernel, gamma, ptr(out), stream_ptr()),
               "dkm_svm_decision")
    return out


def lagrangian(so, X, x32, sv, coef, lab, xnorm, kernel, gamma):
    """The reference's ``W`` of the support rows ``sv`` as a device fp64
    scalar (``dkm_svm_w``)."""
    t = torch()
    ns = int(sv.shape[0])
    tmp = t.empty(ns, dtype=t.float64, device=X.device)
    out = t.empty(1, dtype=t.float64, device=X.device)
    _lib.check(so.dkm_svm_w(ptr(X), 1 if x32 else 0, X.shape[0], X.shape[1],
                            X.stride(0), ptr(sv), ns, ptr(coef), ptr(lab),
                            ptr(xnorm), kernel, gamma, ptr(tmp), ptr(out),
                            stream_ptr()), "dkm_svm_w")
    return out


class CascadeSVM(object):
    """Cascade support vector classification on MI355X (see the module
    docstring).

    Parameters match ``dislib.classification.CascadeSVM``; ``device`` is a
    keyword-only extension.
    """
    _name_to_kernel = {"linear": "_linear_kernel", "rbf": "_rbf_kernel"}

    def __init__(self, cascade_arity=2, max_iter=5, tol=1e-3,
                 kernel="rbf", c=1, gamma='auto', check_convergence=True,
                 random_state=None, verbose=False, *, device=None):
        assert (gamma == "auto" or type(gamma) == float
                or type(float(gamma)) == float), "Invalid gamma"
        assert (kernel is None or kernel in self._name_to_kernel.keys()), \
            "Incorrect kernel value [%s], available kernels are %s" % (
                kernel, self._name_to_kernel.keys())
        assert (c is None or type(c) == float or type(float(c)) == float), \
            "Incorrect C type [%s], type : %s" % (c, type(c))
        assert (type(tol) == float or type(float(tol)) == float), \
            "Incorrect tol type [%s], type : %s" % (tol, type(tol))
        assert cascade_arity > 1, "Cascade arity must be greater than 1"
        assert max_iter > 0, "Max iterations must be greater than 0"
        assert type(check_convergence) == bool, "Invalid value in " \
                                                "check_convergence"

        self._reset_model()

        self._arity = cascade_arity
        self._max_iter = max_iter
        self._tol = tol
        self._check_convergence = check_convergence
        self._random_state = random_state
        self._verbose = verbose
        self._gamma = gamma
        self._device = device
        self._kernel = "rbf" if kernel is None else kernel

        if kernel == "rbf":
            self._clf_params = {"kernel": kernel, "C": c, "gamma": gamma}
        else:
            self._clf_params = {"kernel": kernel, "C": c}

    def fit(self, dataset):
        """Fits a model using the labelled training ``dataset``."""
        from .. import _shard
        self._reset_model()
        if dataset.sparse:
            raise NotImplementedError(
                "CascadeSVM takes a dense Dataset: CSR samples are not "
                "supported")
        if _shard.active():
            raise NotImplementedError(
                "CascadeSVM runs on one rank: a torch.distributed world "
                "larger than 1 is not supported")
        self._set_gamma(dataset.n_features)
        raw, classes = _raw_labels(dataset)
        if len(classes) > 2:
            raise ValueError(
                "CascadeSVM is a binary classifier: the labels hold %d "
                "classes" % len(classes))
        if self._clf_params["C"] is None or not float(
                self._clf_params["C"]) > 0:
            raise ValueError("C must be positive, got %r"
                             % (self._clf_params["C"],))

        so = _lib.lib()                     # no GPU / no libdkm: raise here
        dd = dataset._device_data(self._device)
        with on(dd.device):
            preload(dd.device)
            self._fit_state = _Fit(so, dd, raw, classes, self._kernel,
                                   self._clf_params.get("gamma", 0.0),
                                   self._clf_params["C"])
            dataset_ids = [np.arange(a, b) for a, b in dd.subset_slices()]
            while not self._check_finished():
                self._do_iteration(dataset_ids)
                if self._check_convergence:
                    self._check_convergence_and_update_w()
                    self._print_iteration()

    def predict(self, dataset):
        """Writes the predicted class of every sample into the Subsets'
        labels."""
        dec = self._decide(dataset)
        cls = self._clf.classes_
        labels = cls[(dec > 0).astype(np.int64)] if len(cls) > 1 else \
            np.full(dec.shape, cls[0])
        _write_labels(dataset, labels)

    def decision_function(self, dataset):
        """Writes the fp64 decision value of every sample into the Subsets'
        labels."""
        _write_labels(dataset, self._decide(dataset))

    def score(self, dataset):
        """The mean accuracy of ``predict`` against the labels the Subsets
        hold (which stay as they are)."""
        true = [np.asarray(s.labels) for s in dataset]
        dec = self._decide(dataset)
        cls = self._clf.classes_
        labels = cls[(dec > 0).astype(np.int64)]
        total_correct, total_size, off = 0., 0., 0
        for tl in true:
            n = len(tl)
            total_correct += np.sum(np.equal(labels[off:off + n], tl))
            total_size += n
            off += n
        return total_correct / total_size

    # -- the reference's private members -----------------------------------
    def _reset_model(self):
        self.iterations = 0
        self.converged = False
        self._last_w = None
        self._clf = None
        self._feedback = None
        self._feedback_ids = None
        self._fit_state = None
        self.w_ = []             # W after every iteration that took it

    def _set_gamma(self, n_features):
        if self._gamma == "auto":
            self._gamma = 1. / n_features
            self._clf_params["gamma"] = self._gamma

    def _collect_clf(self):
        """No-op: there are no futures (kept for API compatibility)."""
        return None

    def _print_iteration(self):
        if self._verbose:
            print("Iteration %s of %s." % (self.iterations, self._max_iter))

    def _train(self, return_classifier, id_lists):
        st = self._fit_state
        ids = _merge(id_lists)
        labels = st.raw[ids]
        if len(np.unique(labels)) < 2:
            raise ValueError(
                "The number of classes has to be greater than one; got 1 "
                "class")
        alpha, f, y = st.solve(ids)
        # sklearn's order: the support vectors of classes_[0], then of [1]
        sv0 = np.flatnonzero((alpha > 0) & (y < 0))
        sv1 = np.flatnonzero((alpha > 0) & (y > 0))
        sup = np.concatenate((sv0, sv1))
        if not return_classifier:
            return ids[sup], None
        clf = _Model(ids[sup], (y * alpha)[sup][None, :],
                     intercept(alpha, f, y, st.c), st.classes,
                     np.array([len(sv0), len(sv1)], dtype=np.int32), st)
        return ids[sup], clf

    def _do_iteration(self, dataset_ids):
        q = []
        arity = self._arity

        # first level
        for subset_ids in dataset_ids:
            data = [subset_ids]
            if self._feedback is not None:
                data.append(self._feedback_ids)
            q.append(self._train(False, data)[0])

        # reduction
        while len(q) > arity:
            data = q[:arity]
            del q[:arity]
            q.append(self._train(False, data)[0])

        # last layer
        get_clf = (self._check_convergence or self._is_last_iteration())
        self._feedback_ids, self._clf = self._train(get_clf, q)
        self._feedback = self._feedback_ids
        self.iterations += 1

    def _is_last_iteration(self):
        return self.iterations == self._max_iter - 1

    def _check_finished(self):
        return self.iterations >= self._max_iter or self.converged

    def _lagrangian_fast(self, ids, labels, coef):
        st = self._fit_state
        t = torch()
        set_sl = set(labels)
        assert len(set_sl) == 2, "Only binary problem can be handled"
        new_sl = np.array(labels, dtype=np.float64)
        new_sl[labels == 0] = -1
        dev = st.device
        sv = t.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(dev)
        c = t.from_numpy(np.ascontiguousarray(coef, dtype=np.float64)
                         .ravel()).to(dev)
        lab = t.from_numpy(new_sl).to(dev)
        w = lagrangian(st.so, st.X, st.f32, sv, c, lab, st.norms, st.kernel,
                       st.gamma)
        return float(w.item())

    def _check_convergence_and_update_w(self):
        self._collect_clf()
        st = self._fit_state
        labels = st.raw[self._feedback_ids]
        w = self._lagrangian_fast(self._feedback_ids, labels,
                                  self._clf.dual_coef_)
        self.w_.append(w)
        delta = 0

        if self._last_w:
            delta = np.abs((w - self._last_w) / self._last_w)

            if delta < self._tol:
                self.converged = True

        if self._verbose:
            self._print_convergence(delta, w)

        self._last_w = w

    def _print_convergence(self, delta, w):
        print("Computed W %s" % w)
        if self._last_w:
            print("Checking convergence...")

            if self.converged:
                print("     Converged with delta: %s " % delta)
            else:
                print("     No convergence with delta: %s " % delta)

    # -- decision values ---------------------------------------------------
    def _decide(self, dataset):
        """Host fp64 decision values of every sample of ``dataset``."""
        assert (self._clf is not None or self._feedback is not None), \
            "Model has not been initialized. Call fit() first."
        assert self._clf is not None, \
            "The classifier was not collected: fit() ended before its " \
            "last iteration"
        if dataset.sparse:
            raise NotImplementedError(
                "CascadeSVM takes a dense Dataset: CSR samples are not "
                "supported")
        st, clf = self._fit_state, self._clf
        if int(dataset.n_features) != st.d:
            raise ValueError("the model was fitted on %d features, the "
                             "Dataset has %d" % (st.d, dataset.n_features))
        t = torch()
        dd = dataset._device_data(st.device)
        with on(st.device):
            sv = t.from_numpy(np.ascontiguousarray(
                clf.support_, dtype=np.int32)).to(st.device)
            coef = t.from_numpy(np.ascontiguousarray(
                clf.dual_coef_, dtype=np.float64).ravel()).to(st.device)
            out = decision_values(st.so, dd.X, dd.dtype == np.float32, st.X,
                                  st.f32, sv, coef, clf.intercept_[0],
                                  st.norms, st.kernel, st.gamma)
            return out.cpu().numpy()


def _raw_labels(dataset):
    """The Subsets' labels as one fp64 host vector, and their sorted distinct
    values in the labels' own dtype."""
    parts = []
    for s in dataset:
        if s.labels is None:
            raise ValueError("CascadeSVM.fit takes a labelled Dataset: a "
                             "Subset has no labels")
        parts.append(np.asarray(s.labels))
    if not parts:
        raise ValueError("CascadeSVM.fit takes a Dataset with samples")
    labels = np.concatenate(parts)
    return labels.astype(np.float64), np.unique(labels)


def _write_labels(dataset, values):
    off = 0
    for s in dataset:
        n = int(s.samples.shape[0])
        s.labels = values[off:off + n]
        off += n
    dataset._labels = None
