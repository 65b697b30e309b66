"""GPU tests of GaussianMixture (dkm_gm.hip): the three kernels through the
C ABI against the longdouble restatement within running error bounds, the
whole class against the reference's goldens, determinism, residency, the
refusals, and the dense tests of the reference's tests/test_gm.py."""
import ctypes
import warnings

import numpy as np
import pytest

from dislib_amd import _device, _lib
from dislib_amd.cluster import GaussianMixture
from dislib_amd.data import Dataset, Subset, load_data
from dislib_amd.preprocessing import StandardScaler
from oracle import kmeans_oracle as orc
from tests import gm_ref as gr
from tests.conftest import load_golden
from tests.test_gm_host import ATTRS, PARAMS, close, keep

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    assert _lib.lib().dkm_build_flags() == 0


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _padded(x, ld, offset=0):
    """x in a device buffer with leading dimension ld (NaN in the padding:
    a kernel that reads it shows), starting ``offset`` elements into its
    allocation."""
    rows = max(1, x.shape[0])
    flat = torch.full((offset + rows * ld,), float("nan"),
                      dtype=torch.from_numpy(x[:0]).dtype, device="cuda")
    buf = flat[offset:].view(rows, ld)
    buf[:x.shape[0], :x.shape[1]] = torch.from_numpy(x).cuda()
    return buf


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _model(rs, d, K, lower=False):
    """Means, Cholesky factors of the precisions and log det + log weights
    of K random well-conditioned components."""
    mu = rs.uniform(-3, 3, (K, d))
    a = rs.standard_normal((K, d, d))
    cov = np.einsum("kij,klj->kil", a, a) / d + 0.5 * np.eye(d)
    pc = gr.precision_cholesky(cov, np.float64)
    if lower:
        pc = np.ascontiguousarray(pc.transpose(0, 2, 1))
    w = rs.uniform(0.5, 1.5, K)
    w /= w.sum()
    ldw = np.sum(np.log(pc.reshape(K, -1)[:, ::d + 1]), 1) + np.log(w)
    return mu, pc, w, ldw


GUARD_BYTE = 0xA5


class Kernels:
    """The C ABI on one padded device matrix, which starts ``offset``
    elements into its allocation.  ``guard``: bytes behind a workspace of
    exactly dkm_gm_workspace_bytes that every call must leave as they are."""

    def __init__(self, x, pad, K, offset=0, guard=0):
        self.so = _lib.lib()
        self.f32 = x.dtype == np.float32
        self.d, self.ld, self.K = x.shape[1], x.shape[1] + pad, K
        self.X = _padded(x, self.ld, offset)
        self.guard = guard

    def _ws(self, n):
        nb = self.so.dkm_gm_workspace_bytes(n, self.d, self.K)
        assert nb > 0
        ws = torch.empty(nb + self.guard, dtype=torch.uint8, device="cuda")
        ws[nb:] = GUARD_BYTE
        return ws, nb

    def _guard_kept(self, ws, nb):
        assert bool((ws[nb:] == GUARD_BYTE).all())

    def estep(self, n, mu, pc, ldw, flags, labels=True):
        """(resp, labels, total); ``labels`` False passes labels = NULL."""
        fn = self.so.dkm_gm_estep_f32 if self.f32 else self.so.dkm_gm_estep_f64
        ws, nb = self._ws(n)
        resp = torch.full((max(n, 1), self.K), -7.0, dtype=torch.float64,
                          device="cuda")
        lab = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
        tot = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
        par = [_dev(a) for a in (mu, pc, ldw)]     # alive through the call
        _lib.check(fn(_p(self.X) if n else None, n, self.d, self.ld,
                      _p(par[0]), _p(par[1]), _p(par[2]), self.K,
                      flags, _p(ws), nb, _p(resp),
                      _p(lab) if labels else None, _p(tot), _st()),
                   "estep")
        self._guard_kept(ws, nb)
        if not labels:
            assert bool((lab == -7).all())
        return (resp[:n].cpu().numpy(), lab[:n].cpu().numpy(),
                float(tot.item()))

    def sums(self, n, resp):
        fn = self.so.dkm_gm_mstep_sums_f32 if self.f32 else \
            self.so.dkm_gm_mstep_sums_f64
        ws, nb = self._ws(n)
        out = torch.full((self.K * (self.d + 1) + 1,), -7.0,
                         dtype=torch.float64, device="cuda")
        r = _dev(resp[:n]) if n else None
        _lib.check(fn(_p(self.X) if n else None, n, self.d, self.ld, _p(r),
                      self.K, _p(ws), nb, _p(out), _st()), "sums")
        got = out.cpu().numpy()
        self._guard_kept(ws, nb)
        assert got[-1] == -7.0
        return got[:self.K], got[self.K:-1].reshape(self.K, self.d)

    def cov(self, n, resp, means):
        fn = self.so.dkm_gm_mstep_cov_f32 if self.f32 else \
            self.so.dkm_gm_mstep_cov_f64
        ws, nb = self._ws(n)
        out = torch.full((self.K, self.d, self.d), -7.0, dtype=torch.float64,
                         device="cuda")
        r = _dev(resp[:n]) if n else None
        mu = _dev(means)
        _lib.check(fn(_p(self.X) if n else None, n, self.d, self.ld, _p(r),
                      _p(mu), self.K, _p(ws), nb, _p(out), _st()), "cov")
        got = out.cpu().numpy()
        self._guard_kept(ws, nb)
        return got


def check_estep(x, n, mu, pc, ldw, got, truth):
    """The E-step's running error bounds (u = 2^-53): |y - y^| <= (d + 8) u
    sum_i (|x_i| + |mu_i|) |P_ij|; B = (sum_j 2 |y_j| err_j + (d + 8) u sum
    y^2) / 2 + 4 u |wlp|; lse within B_max + 4 u |lse|; resp within resp
    (expm1(2 B_max) + 8 u) + 1e-300."""
    resp, lab, tot = got
    d, K = x.shape[1], mu.shape[0]
    ax = np.abs(x[:n].astype(np.float64))
    B = np.empty((n, K))
    for k in range(K):
        err = (d + 8) * U * (ax + np.abs(mu[k])) @ np.abs(pc[k])
        y = np.abs(truth["y"][k][:n].astype(np.float64))
        B[:, k] = ((2 * y * err).sum(axis=1) +
                   (d + 8) * U * (y * y).sum(axis=1)) / 2
    wlp = truth["wlp"][:n].astype(np.float64)
    B += 4 * U * np.abs(wlp)
    bmax = B.max(axis=1) if n else np.zeros(0)
    tr = truth["resp"][:n]
    bound = tr.astype(np.float64) * (np.expm1(2 * bmax) + 8 * U)[:, None] \
        + 1e-300
    assert resp.shape == (n, K)
    assert (np.abs((resp.astype(LD) - tr).astype(np.float64)) <= bound).all()
    lse = truth["lse"][:n]
    alse = np.abs(lse.astype(np.float64))
    assert abs(float(LD(tot) - lse.sum())) <= \
        (bmax + 4 * U * alse).sum() + (n + 8) * U * alse.sum()
    # numpy's first-maximum argmax of the device's own resp, bit for bit
    assert lab.dtype == np.int64
    assert np.array_equal(lab, resp.argmax(axis=1) if n else lab)


def check_mstep(kern, x, n, resp, means, truth=None):
    """``truth``: (nk, sums, cov) of the longdouble restatement on these
    inputs, where the caller has them already."""
    x64 = x[:n].astype(np.float64)
    r = resp[:n]
    nk, s = kern.sums(n, resp)
    tnk, ts = truth[:2] if truth else gr.mstep_sums(x[:n], r, LD)
    assert (np.abs((nk.astype(LD) - tnk).astype(np.float64)) <=
            (n + 8) * U * np.abs(r).sum(axis=0)).all()
    assert (np.abs((s.astype(LD) - ts).astype(np.float64)) <=
            (n + 8) * U * (np.abs(r).T @ np.abs(x64))).all()
    cov = kern.cov(n, resp, means)
    tcov = truth[2] if truth else gr.mstep_cov(x[:n], r, means, LD)
    for k in range(means.shape[0]):
        ad = np.abs(x64 - means[k])
        bound = (n + 8) * U * ((np.abs(r[:, k]) * ad.T) @ ad)
        assert (np.abs((cov[k].astype(LD) - tcov[k]).astype(np.float64))
                <= bound).all(), k
        assert np.array_equal(cov[k], cov[k].T)
    return nk, s, cov


# d in {1, 2, 3, 4, 5, 15, 16, 17, 33, 64} and K in {1, 2, 3, 16, 17}: every d
# with two K's, every K with four d's; 65 and 129 are the first sizes of the
# E-step's two other register layouts (d <= 128 in registers, beyond streamed)
SHAPES = [(1, 1), (1, 17), (2, 2), (2, 16), (3, 3), (3, 1), (4, 17), (4, 2),
          (5, 16), (5, 3), (15, 1), (15, 17), (16, 2), (16, 16), (17, 3),
          (17, 17), (33, 16), (33, 2), (64, 17), (64, 3), (65, 2), (129, 2)]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("d,K", SHAPES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_kernels_against_the_longdouble_restatement(dtype, d, K, pad):
    rs = np.random.RandomState(100 * d + K)
    blk = _device.gm_estep_block(d)
    # more than one E-step block; 513 rows are two M-step chunks
    nmax = 517 if d <= 64 else 2 * blk + 5
    x = (rs.standard_normal((nmax, d)) * 2.0).astype(dtype)
    mu, pc, w, ldw = _model(rs, d, K)
    truth = gr.estep(x, w, mu, pc, LD, ldw=ldw)
    kern = Kernels(x, pad, K)
    t, m = _device.GM_TILE, _device.GM_MSTEP_ROWS
    for n in (t - 1, t, t + 1, 2 * t + 1, 0, blk - 1, blk + 1, nmax):
        got = kern.estep(n, mu, pc, ldw, _lib.GM_UPPER)
        check_estep(x, n, mu, pc, ldw, got, truth)
        if K == 1:
            assert (got[0] == 1.0).all()
        # the panel skip changes no bit, and a rerun gives the same bytes
        for flags in (0, _lib.GM_UPPER):
            again = kern.estep(n, mu, pc, ldw, flags)
            assert again[0].tobytes() == got[0].tobytes()
            assert again[1].tobytes() == got[1].tobytes()
            assert again[2] == got[2]
    resp = truth["resp"].astype(np.float64)
    means = mu + 0.1
    for n in (m - 1, m, m + 1, 2 * m + 1, 0, 512, 513, nmax):
        if n > nmax:
            continue
        a = check_mstep(kern, x, n, resp, means)
        b = (kern.sums(n, resp), kern.cov(n, resp, means))
        assert a[0].tobytes() == b[0][0].tobytes()
        assert a[1].tobytes() == b[0][1].tobytes()
        assert a[2].tobytes() == b[1].tobytes()


def test_estep_takes_lower_triangular_factors():
    """``precisions_init`` gives LOWER Cholesky factors (gm/base.py:759-762)."""
    rs = np.random.RandomState(5)
    d, K, n = 17, 3, 150
    x = rs.standard_normal((n, d)) * 2.0
    mu, pc, w, ldw = _model(rs, d, K, lower=True)
    assert np.tril(pc, -1).any()
    truth = gr.estep(x, w, mu, pc, LD, ldw=ldw)
    got = Kernels(x, 0, K).estep(n, mu, pc, ldw, 0)
    check_estep(x, n, mu, pc, ldw, got, truth)


def test_estep_far_row_and_exact_tie():
    rs = np.random.RandomState(6)
    d, K, n = 5, 4, 40
    x = rs.standard_normal((n, d))
    mu, pc, w, ldw = _model(rs, d, K)
    # components 1 and 3 identical: an exact tie goes to the first
    mu[3], pc[3], ldw[3] = mu[1], pc[1], ldw[1]
    x[7] = mu[1]
    # 40 standard deviations from every mean: exp underflows
    x[0] = 40.0 * 3.0 * np.ones(d) + 10.0
    truth = gr.estep(x, w, mu, pc, LD, ldw=ldw)
    resp, lab, tot = got = Kernels(x, 3, K).estep(n, mu, pc, ldw,
                                                  _lib.GM_UPPER)
    check_estep(x, n, mu, pc, ldw, got, truth)
    assert truth["wlp"][0].max() < -700
    assert np.isfinite(resp).all()
    assert (np.abs(resp.sum(axis=1) - 1.0) <= 4 * U * K).all()
    assert (resp[:, 1] == resp[:, 3]).all()
    assert lab[7] == 1 and (lab != 3).all()


def test_mstep_exact_zeros_and_a_tiny_component():
    rs = np.random.RandomState(7)
    d, K, n = 17, 3, 700
    x = rs.standard_normal((n, d)) * 2.0 + 1.0
    resp = rs.rand(n, K)
    resp[rs.rand(n, K) < 0.3] = 0.0                 # exact zeros
    resp[:, 2] = 0.0
    resp[5, 2] = 1e-280                             # nk tiny but positive
    kern = Kernels(x, 3, K)
    nk, s, cov = check_mstep(kern, x, n, resp, rs.standard_normal((K, d)))
    assert nk[2] == 1e-280 and (s[2] == 1e-280 * x[5]).all()
    assert np.isfinite(cov).all()


def test_workspace_is_checked():
    so = _lib.lib()
    assert so.dkm_gm_workspace_bytes(10, 0, 2) == 0
    assert so.dkm_gm_workspace_bytes(10, 2, 0) == 0
    x = torch.zeros((10, 2), dtype=torch.float64, device="cuda")
    out = torch.zeros(8, dtype=torch.float64, device="cuda")
    rc = so.dkm_gm_mstep_sums_f64(_p(x), 10, 2, 2, _p(x), 2, _p(out), 8,
                                  _p(out), _st())
    assert rc == 10002


# ---------------------------------------------------------------------------
# the whole class against the goldens
# ---------------------------------------------------------------------------
def dataset(x, sizes):
    ds = Dataset(n_features=x.shape[1])
    for block in gr.split(x, sizes):
        ds.append(Subset(block))
    return ds


def run(name, predict=True):
    inp = gr.inputs(name)
    ds = dataset(inp["x"], inp["sizes"])
    gm = GaussianMixture(**inp["kw"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert gm.fit_predict(ds) is None
    test = dataset(inp["x_test"], inp["test_sizes"])
    gm.predict(test)
    return gm, ds, test


def check_against_golden(name, gm, labels, predict_labels):
    g = load_golden(name)
    assert gm.n_iter == g["n_iter"] and gm.converged_ == g["converged"]
    assert labels.dtype == np.int64
    assert np.array_equal(labels[keep(g)], g["labels"][keep(g)])
    if predict_labels is not None:
        kt = keep(g, "gap_test")
        assert np.array_equal(predict_labels[kt], g["predict_labels"][kt])
    for p, a in zip(PARAMS, ATTRS):
        got = getattr(gm, a)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64
        if p == "precisions_cholesky":
            if name not in gr.NO_CHOL:
                assert close(got, g[p], 1e-9 * float(g["cond"]))
        else:
            assert close(got, g[p], 1e-9), p
    assert abs(gm.lower_bound_ - g["lower_bound"]) <= \
        1e-9 * abs(g["lower_bound"])


@pytest.mark.parametrize("name", gr.CASES)
def test_class_equals_the_golden(name):
    gm, ds, test = run(name)
    for s in ds:
        assert isinstance(s.labels, np.ndarray) and s.labels.dtype == np.int64
    check_against_golden(name, gm, ds.labels, test.labels)
    g = load_golden(name)
    if "kmeans_centers" in g:
        # the k-means initialisation is the oracle's: KMeans' default order
        # of the sums gives its centres to the project's tolerances (1e-9
        # for fp64 samples, 1e-4 for fp32 ones, whose reference sums are
        # fp32: tests/test_gpu_parity.py), not bit for bit
        inp = gr.inputs(name)
        seed = np.random.RandomState(inp["kw"]["random_state"]).randint(
            0, int(1e8))
        ref = orc.OracleKMeans(n_clusters=gm.n_components, random_state=seed)
        ref.fit([np.asarray(b) for b in gr.split(inp["x"], inp["sizes"])])
        assert np.array_equal(ref.centers, g["kmeans_centers"])
        assert gm.kmeans.n_iter == ref.n_iter
        err = np.abs(gm.kmeans.centers - ref.centers) / \
            np.maximum(np.abs(ref.centers), 1.0)
        assert err.max() <= (1e-4 if inp["x"].dtype == np.float32 else 1e-9)
    if name in gr.TOY:                  # test_gm.py's own allclose
        for p, a in zip(PARAMS, ATTRS):
            assert np.allclose(getattr(gm, a), g[p])
    again, ds2, test2 = run(name)
    for a in ATTRS:
        assert getattr(gm, a).tobytes() == getattr(again, a).tobytes()
    assert gm.lower_bound_ == again.lower_bound_
    assert ds.labels.tobytes() == ds2.labels.tobytes()
    assert test.labels.tobytes() == test2.labels.tobytes()


def test_fit_then_predict_equals_fit_predict():
    inp = gr.inputs("gm_a")
    ds = dataset(inp["x"], inp["sizes"])
    gm = GaussianMixture(**inp["kw"])
    assert gm.fit(ds) is None
    gm.predict(ds)
    check_against_golden("gm_a", gm, ds.labels, None)


def test_convergence_warning_and_n_iter():
    from sklearn.exceptions import ConvergenceWarning
    inp = gr.inputs("gm_e")
    gm = GaussianMixture(**inp["kw"])
    with pytest.warns(ConvergenceWarning, match="did not converge"):
        gm.fit(dataset(inp["x"], inp["sizes"]))
    assert gm.n_iter == 0 and gm.converged_ is False


# ---------------------------------------------------------------------------
# residency
# ---------------------------------------------------------------------------
def _standardised(device):
    x = gr.inputs("gm_a")["x"]
    src = torch.from_numpy(x).cuda() if device else x
    ds = load_data(src, subset_size=250)
    StandardScaler().fit_transform(ds)
    return ds


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_fit_after_the_scaler_uploads_nothing(device):
    ds = _standardised(device)
    dd = ds._device
    assert dd is not None and dd.signature == ds._signature()
    Y, p = dd.X, dd.X.data_ptr()
    z = Y.cpu().numpy()
    gm = GaussianMixture(n_components=3, random_state=3)
    gm.fit_predict(ds)
    assert ds._device_data() is dd and dd.X is Y and Y.data_ptr() == p
    assert np.array_equal(Y.cpu().numpy(), z)
    gm.predict(ds)
    assert ds._device_data() is dd
    for s in ds:
        assert isinstance(s.samples, torch.Tensor if device else np.ndarray)
    # the same model as the restatement fits on the scaled rows
    ref = gr.RefGM(n_components=3, random_state=3).fit(
        gr.split(z, [250] * 6))
    assert gm.n_iter == ref.n_iter
    for a in ATTRS[:3]:
        assert close(getattr(gm, a), getattr(ref, a), 1e-9)
    lab = ref.predict([z])
    gap = gr.top_two_gap(ref.resp([z]))
    assert np.array_equal(ds.labels[gap >= gr.GAP], lab[gap >= gr.GAP])


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_collapsed_component_is_a_value_error():
    ds = load_data(np.array([[1.0, 2.0], [1.0, 2.0]]), subset_size=2)
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            GaussianMixture(n_components=2, reg_covar=0,
                            random_state=0).fit(ds)


def test_responsibilities_must_leave_headroom(monkeypatch):
    ds = load_data(gr.inputs("gm_a")["x"], subset_size=500)
    monkeypatch.setattr(_device, "_IMAGE_HEADROOM", 1 << 60)
    with pytest.raises(ValueError, match="responsibilities resident"):
        GaussianMixture(n_components=3, init_params='random',
                        random_state=0).fit(ds)


# ---------------------------------------------------------------------------
# the dense tests of the reference's tests/test_gm.py through the alias
# ---------------------------------------------------------------------------
def test_reference_suite_through_install_as_dislib():
    import dislib_amd
    dislib_amd.install_as_dislib()
    from dislib.cluster import GaussianMixture as GM
    from dislib.data import Dataset as D, Subset as S, load_data as load
    from sklearn.datasets import make_blobs

    # test_fit
    ds = D(n_features=2)
    ds.append(S(np.array([[1, 2], [2, 1], [-3, -3]])))
    ds.append(S(np.array([[-1, -2], [-2, -1], [3, 3]])))
    gm = GM(n_components=2, random_state=666)
    gm.fit(ds)
    cov = np.array([[0.66671688, 0.33338255], [0.33338255, 0.66671688]])
    pc = np.array([[1.22469875, -0.70714834], [0., 1.4141944]])
    assert np.allclose(gm.weights_, np.array([0.5, 0.5]))
    assert np.allclose(gm.means_, np.array([[-2, -2], [2, 2]]))
    assert np.allclose(gm.covariances_, np.array([cov, cov]))
    assert np.allclose(gm.precisions_cholesky_, np.array([pc, pc]))

    # test_predict
    ds = D(n_features=2)
    ds.append(S(np.array([[1, 2], [-1, -2]])))
    ds.append(S(np.array([[2, 1], [-2, -1]])))
    gm = GM(n_components=2, random_state=666)
    gm.fit(ds)
    ds.append(S(np.array([[2, 2], [-1, -3]])))
    gm.predict(ds)
    pr = ds.labels
    assert pr[0] != pr[1]
    assert pr[0] == pr[2] == pr[4] and pr[1] == pr[3] == pr[5]

    # test_fit_predict
    x, y = make_blobs(n_samples=1500, random_state=170)
    xf = np.vstack((x[y == 0][:500], x[y == 1][:100], x[y == 2][:10]))
    y_real = np.concatenate((np.zeros(500), np.ones(100), 2 * np.ones(10)))
    ds = load(xf, subset_size=300)
    GM(n_components=3, random_state=170).fit_predict(ds)
    assert len(ds.labels) == 610
    assert np.count_nonzero(ds.labels == y_real) / 610 > 0.99

    # test_init_random
    np.random.seed(0)
    ds = load(np.random.rand(50, 3), subset_size=10)
    gm = GM(init_params='random', n_components=4, random_state=170)
    gm.fit(ds)
    assert gm.n_iter > 5

    # the five validation errors
    ds = load(np.array([[0, 0], [0, 1], [1, 0]]), subset_size=10)
    for kw in (dict(n_components=0), dict(tol=-0.1), dict(max_iter=0),
               dict(reg_covar=-0.1), dict(covariance_type='')):
        with pytest.raises(ValueError):
            GM(**kw).fit(ds)
