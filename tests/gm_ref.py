"""Sequential numpy / scipy restatement of the reference's GaussianMixture
tasks (dislib/cluster/gm/base.py), with the per-Subset partials and the
``arity`` tree, in two arithmetics.  Not a test module.

``float64``: ``np.matmul`` / ``np.dot`` / ``scipy.linalg`` as the reference.
``np.longdouble``: einsum and plain loops (its own Cholesky and triangular
solve) -- the "truth" the GPU tests bound the kernels against.

tests/test_gm_host.py pins both to the goldens (the reference's own output)
on the CPU.  ``estep`` / ``mstep`` are the single steps on one block;
``inputs(name)`` builds the inputs that tests/golden/gen_golden_gm.py and
the tests share.
"""
import numpy as np
from numpy.random.mtrand import RandomState
from scipy import linalg
from scipy.special import logsumexp

LD = np.longdouble


def split(x, sizes):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [x[a:b] for a, b in zip(off[:-1], off[1:])]


def uneven(n, pattern=(97, 250, 33)):
    """Subset sizes repeating ``pattern`` until n rows are covered."""
    sizes, i = [], 0
    while sum(sizes) < n:
        sizes.append(min(pattern[i % len(pattern)], n - sum(sizes)))
        i += 1
    return sizes


def tree(partials, arity, fold):
    partials = list(partials)
    while len(partials) > 1:
        group, partials = partials[:arity], partials[arity:]
        partials.append(fold(group))
    return partials[0]


def _sum(items):
    items = list(items)
    s = items[0]            # python's sum: 0 + first is exact
    for p in items[1:]:
        s = s + p
    return s


# ---------------------------------------------------------------------------
# longdouble linear algebra (plain loops)
# ---------------------------------------------------------------------------
def _cholesky_ld(a):
    n = a.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        s = a[j, j] - np.dot(L[j, :j], L[j, :j])
        if not s > 0:
            raise linalg.LinAlgError("not positive definite")
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, n):
            L[i, j] = (a[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def _inv_lower_ld(L):
    """solve_triangular(L, I, lower=True)."""
    n = L.shape[0]
    out = np.zeros((n, n), dtype=LD)
    for c in range(n):
        for i in range(c, n):
            s = (LD(1) if i == c else LD(0)) - np.dot(L[i, c:i], out[c:i, c])
            out[i, c] = s / L[i, i]
    return out


ILL_DEFINED = (
    "Fitting the mixture model failed because some components have "
    "ill-defined empirical covariance (for instance caused by singleton "
    "or collapsed samples). Try to decrease the number of components, "
    "or increase reg_covar.")


def precision_cholesky(covariances, dt):
    K, d, _ = covariances.shape
    out = np.empty((K, d, d), dtype=dt)
    for k, cov in enumerate(covariances):
        try:
            if dt == LD:
                out[k] = _inv_lower_ld(_cholesky_ld(cov)).T
            else:
                chol = linalg.cholesky(cov, lower=True)
                out[k] = linalg.solve_triangular(chol, np.eye(d),
                                                 lower=True).T
        except linalg.LinAlgError:
            raise ValueError(ILL_DEFINED)
    return out


# ---------------------------------------------------------------------------
# single steps on one block
# ---------------------------------------------------------------------------
def weighted_log_prob(x, w, mu, pc, dt=np.float64, ldw=None):
    """(wlp, y) of gm/base.py:240-307; y only in longdouble (K, n, d).
    ``ldw``: log det + log weights as given to a kernel, instead of their
    evaluation here.  d log(2 pi) is the reference's fp64 value in both."""
    n, d = x.shape
    K = mu.shape[0]
    log_det = np.sum(np.log(pc.reshape(K, -1)[:, ::d + 1]), 1)
    log_prob = np.empty((n, K), dtype=dt)
    ys = None
    if dt == LD:
        xl, ys = x.astype(LD), np.empty((K, n, d), dtype=LD)
        for k in range(K):
            ys[k] = np.einsum("ni,ij->nj", xl - mu[k].astype(LD),
                              pc[k].astype(LD))
            log_prob[:, k] = np.sum(np.square(ys[k]), axis=1)
    else:
        for k in range(K):
            y = np.matmul(x, pc[k]) - np.dot(mu[k], pc[k])
            log_prob[:, k] = np.sum(np.square(y), axis=1)
    cst = dt(d * np.log(2 * np.pi))
    if ldw is not None:
        return -.5 * (cst + log_prob) + np.asarray(ldw, dtype=dt), ys
    return -.5 * (cst + log_prob) + log_det + np.log(w), ys


def estep(x, w, mu, pc, dt=np.float64, ldw=None):
    """One block's E-step: dict(resp, lse, wlp, y, total)."""
    w, mu, pc = (np.asarray(a, dtype=dt) for a in (w, mu, pc))
    wlp, ys = weighted_log_prob(np.asarray(x), w, mu, pc, dt, ldw)
    if dt == LD:
        mx = wlp.max(axis=1)
        lse = np.log(np.sum(np.exp(wlp - mx[:, None]), axis=1)) + mx
    else:
        lse = logsumexp(wlp, axis=1)
    with np.errstate(under="ignore"):
        resp = np.exp(wlp - lse[:, np.newaxis])
    return dict(resp=resp, lse=lse, wlp=wlp, y=ys, total=np.sum(lse))


def mstep_sums(x, resp, dt=np.float64):
    if dt == LD:
        r = resp.astype(LD)
        return r.sum(axis=0), np.einsum("nk,nd->kd", r, x.astype(LD))
    return resp.sum(axis=0), np.matmul(resp.T, x)


def mstep_cov(x, resp, means, dt=np.float64):
    K, d = means.shape
    cov = np.empty((K, d, d), dtype=dt)
    for k in range(K):
        if dt == LD:
            diff = x.astype(LD) - means[k].astype(LD)
            cov[k] = np.einsum("n,na,nb->ab", resp[:, k].astype(LD), diff,
                               diff)
        else:
            diff = x - means[k]
            cov[k] = np.dot(resp[:, k] * diff.T, diff)
    return cov


def mstep(x, resp, reg_covar=1e-6, dt=np.float64):
    """One block's whole M-step: (weights, means, covariances, chol)."""
    return _mstep_blocks([x], [resp], reg_covar, 50, dt)[:4]


def _mstep_blocks(blocks, resps, reg_covar, arity, dt, with_cov=True):
    parts = [(b.shape[0],) + mstep_sums(b, r, dt)
             for b, r in zip(blocks, resps)]
    n, nk, s = tree(parts, arity, lambda g: tuple(
        _sum(p[i] for p in g) for i in range(3)))
    nk = nk + 10 * np.finfo(np.float64).eps
    means = s / nk[:, np.newaxis]
    weights = nk / n
    if not with_cov:
        return weights, means, None, None, nk
    cov = tree([mstep_cov(b, r, means, dt) for b, r in zip(blocks, resps)],
               arity, _sum).copy()
    d = means.shape[1]
    for k in range(len(nk)):
        cov[k] /= nk[k]
        cov[k].flat[::d + 1] += reg_covar
    return weights, means, cov, precision_cholesky(cov, dt), nk


# ---------------------------------------------------------------------------
# the whole class
# ---------------------------------------------------------------------------
class RefGM:
    """``GaussianMixture`` (gm/base.py:360-785) over a list of sample
    blocks, in arithmetic ``dt``; ``trace`` records every iteration's diff."""

    def __init__(self, n_components=1, tol=1e-3, reg_covar=1e-6,
                 max_iter=100, init_params='kmeans', weights_init=None,
                 means_init=None, precisions_init=None, arity=50,
                 random_state=None, dt=np.float64):
        self.n_components, self.tol, self.reg_covar = n_components, tol, \
            reg_covar
        self.max_iter, self.init_params = max_iter, init_params
        self.weights_init, self.means_init = weights_init, means_init
        self.precisions_init, self.arity = precisions_init, arity
        self.random_state, self.dt = random_state, dt

    def _e_step(self, blocks):
        es = [estep(b, self.weights_, self.means_, self.precisions_cholesky_,
                    self.dt) for b in blocks]
        total, count = tree([(e["total"], len(e["lse"])) for e in es],
                            self.arity, lambda g: tuple(map(_sum, zip(*g))))
        return (total, count), [e["resp"] for e in es]

    def _init(self, blocks, rs):
        K = self.n_components
        if self.init_params == 'kmeans':
            from oracle import kmeans_oracle as orc
            seed = rs.randint(0, int(1e8))
            km = orc.OracleKMeans(n_clusters=K, random_state=seed)
            lab = km.fit([np.asarray(b) for b in blocks], set_labels=True)
            self.kmeans_centers = km.centers
            resps = []
            for lb in split(lab, [len(b) for b in blocks]):
                r = np.zeros((len(lb), K))
                r[np.arange(len(lb)), lb.astype(int)] = 1
                resps.append(r)
        else:
            seeds = rs.randint(np.iinfo(np.int32).max, size=len(blocks))
            resps = []
            for b, seed in zip(blocks, seeds):
                r = RandomState(seed).rand(b.shape[0], K)
                r /= r.sum(axis=1)[:, np.newaxis]
                resps.append(r)
        with_cov = self.precisions_init is None
        w, mu, cov, pc, _ = _mstep_blocks(blocks, resps, self.reg_covar,
                                          self.arity, self.dt, with_cov)
        self.weights_ = w if self.weights_init is None else \
            np.asarray(self.weights_init)
        self.means_ = mu if self.means_init is None else \
            np.asarray(self.means_init)
        if with_cov:
            self.covariances_, self.precisions_cholesky_ = cov, pc
        else:
            self.precisions_cholesky_ = np.array(
                [linalg.cholesky(p, lower=True)
                 for p in self.precisions_init])

    def fit(self, blocks):
        from sklearn.utils import check_random_state
        self.converged_, self.n_iter, self.trace = False, 0, []
        self._init(blocks, check_random_state(self.random_state))
        self.lower_bound_ = -np.inf
        for n_iter in range(1, self.max_iter + 1):
            prev = self.lower_bound_
            (total, count), resps = self._e_step(blocks)
            (self.weights_, self.means_, self.covariances_,
             self.precisions_cholesky_, _) = _mstep_blocks(
                blocks, resps, self.reg_covar, self.arity, self.dt)
            self.lower_bound_ = total / count
            diff = abs(self.lower_bound_ - prev)
            self.trace.append(float(diff))
            if diff < self.tol:
                self.converged_, self.n_iter = True, n_iter
                break
        return self

    def resp(self, blocks):
        return np.concatenate(self._e_step(blocks)[1])

    def predict(self, blocks):
        return self.resp(blocks).argmax(axis=1)


def top_two_gap(resp):
    """Per row: largest minus second-largest responsibility (1 for K = 1)."""
    if resp.shape[1] == 1:
        return np.ones(resp.shape[0])
    s = np.sort(np.asarray(resp, dtype=np.float64), axis=1)
    return s[:, -1] - s[:, -2]


def max_cond(covariances):
    return float(max(np.linalg.cond(np.asarray(c, dtype=np.float64))
                     for c in covariances))


# ---------------------------------------------------------------------------
# The inputs of the goldens gm_a .. gm_g (tests/golden/gen_golden_gm.py runs
# the reference on them).  name -> dict(x, sizes, kw, x_test, test_sizes)
# ---------------------------------------------------------------------------
GAP = 1e-6          # rows with a smaller top-two gap may be left out
CASES = ("gm_a", "gm_b", "gm_c", "gm_d", "gm_e", "gm_f1", "gm_f2", "gm_f3",
         "gm_g")
TOY = ("gm_f1", "gm_f2", "gm_f3")
# precisions_cholesky_ is compared where the largest covariance condition
# number is <= 1e3: not on the toys, and not on test_init_random's 50 rows
# in 4 components (8.6e3), an input the reference's test fixes
NO_CHOL = TOY + ("gm_g",)


def _blobs(n, d, K, std, seed=7):
    from sklearn.datasets import make_blobs
    x, _ = make_blobs(n_samples=n + 257, n_features=d, centers=K,
                      cluster_std=std, center_box=(-6, 6), random_state=seed)
    return x[:n], x[n:]


def inputs(name):
    if name in ("gm_a", "gm_d", "gm_e"):
        x, xt = _blobs(1500, 4, 3, 2.5)
        kw = dict(n_components=3, random_state=3)
        if name == "gm_e":
            kw["max_iter"] = 3
        if name == "gm_d":
            rs = np.random.RandomState(11)
            a = rs.standard_normal((3, 4, 4)) * 0.1
            kw.update(weights_init=np.array([0.2, 0.3, 0.5]),
                      means_init=x[[5, 700, 1400]].copy(),
                      precisions_init=np.array(
                          [np.eye(4) * 0.2 + m @ m.T for m in a]))
        return dict(x=x, sizes=uneven(1500), kw=kw, x_test=xt,
                    test_sizes=uneven(257))
    if name == "gm_b":
        x, xt = _blobs(1201, 17, 5, 3.0)
        return dict(x=x, sizes=uneven(1201), x_test=xt,
                    test_sizes=uneven(257),
                    kw=dict(n_components=5, random_state=3, arity=2,
                            init_params='random'))
    if name == "gm_c":
        x, xt = _blobs(2400, 33, 4, 5.0)
        return dict(x=x.astype(np.float32), sizes=uneven(2400),
                    x_test=xt.astype(np.float32), test_sizes=uneven(257),
                    kw=dict(n_components=4, random_state=3))
    if name == "gm_f1":         # test_gm.py:46-77
        x = np.array([[1, 2], [2, 1], [-3, -3], [-1, -2], [-2, -1], [3, 3]])
        return dict(x=x, sizes=[3, 3], x_test=x, test_sizes=[3, 3],
                    kw=dict(n_components=2, random_state=666))
    if name == "gm_f2":         # test_gm.py:79-97
        x = np.array([[1, 2], [-1, -2], [2, 1], [-2, -1]])
        xt = np.concatenate([x, [[2, 2], [-1, -3]]])
        return dict(x=x, sizes=[2, 2], x_test=xt, test_sizes=[2, 2, 2],
                    kw=dict(n_components=2, random_state=666))
    if name == "gm_f3":         # test_gm.py:99-114
        from sklearn.datasets import make_blobs
        x, y = make_blobs(n_samples=1500, random_state=170)
        xf = np.vstack((x[y == 0][:500], x[y == 1][:100], x[y == 2][:10]))
        return dict(x=xf, sizes=[300, 300, 10], x_test=xf[::7].copy(),
                    test_sizes=uneven(len(xf[::7])),
                    kw=dict(n_components=3, random_state=170))
    if name == "gm_g":          # test_gm.py:169-177
        rs = np.random.RandomState(0)
        x = rs.rand(50, 3)
        return dict(x=x, sizes=[10] * 5, x_test=rs.rand(23, 3),
                    test_sizes=[10, 13],
                    kw=dict(init_params='random', n_components=4,
                            random_state=170))
    raise KeyError(name)
