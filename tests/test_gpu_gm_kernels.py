"""GPU tests of the kernels of dkm_gm.hip through the C ABI at the edges
tests/test_gpu_gm.py leaves out, entry by entry against the longdouble
restatement (tests/gm_ref.py) within the running error bounds of
``check_estep`` and ``check_mstep``:

the M-step's fold of 16 to 34 row chunks and of the 2048 chunks of the cap,
the covariances' own chunking under their workspace cap (with a guard behind
a workspace of exactly the promised size), more than 256 E-step blocks, the
full ends of the E-step's register layouts and streamed sizes beyond 129
with up to four trips of a lane over the components, lower-triangular
factors in every layout, labels = NULL, a misaligned base, rows that must
not depend on their neighbours in the MFMA tile (permuted, cut short,
replaced, non-finite), and dkm_gm_onehot.

The shapes are those of tests/kernel_edge_shapes.py;
tests/test_kernel_plans_host.py shows that each reaches its branch."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

from dislib_amd import _device, _lib
from tests import gm_ref as gr
from tests import kernel_edge_shapes as es
from tests.test_gpu_gm import LD, U, Kernels, _model, check_estep, check_mstep

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
PADS = [0, 3]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    assert _lib.lib().dkm_build_flags() == 0


def _name(v):
    return v.__name__ if isinstance(v, type) else None


def same_estep(a, b):
    assert a[0].tobytes() == b[0].tobytes()
    assert a[1].tobytes() == b[1].tobytes()
    assert np.array(a[2]).tobytes() == np.array(b[2]).tobytes()


def same_mstep(a, b):
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def mstep_truth(x, resp, means):
    return gr.mstep_sums(x, resp, LD) + (gr.mstep_cov(x, resp, means, LD),)


def mstep_twice(kern, x, n, resp, means, truth=None):
    """check_mstep, and a rerun that gives the same bytes."""
    a = check_mstep(kern, x, n, resp, means, truth)
    nk, s = kern.sums(n, resp)
    same_mstep(a, (nk, s, kern.cov(n, resp, means)))
    return a


def random_resp(rs, n, K):
    """Responsibilities with exact zeros, not normalised (the M-step is
    linear in them)."""
    resp = rs.rand(n, K)
    resp[rs.rand(n, K) < 0.3] = 0.0
    return resp


# ---------------------------------------------------------------------------
# 1. the fold of the M-step's row chunks; many E-step blocks
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fold_data(d, K, dtype):
    rs = np.random.RandomState(1000 * d + K)
    nmax = max(es.FOLD_N)
    x = (rs.standard_normal((nmax, d)) * 2.0 + 1.0).astype(dtype)
    return x, random_resp(rs, nmax, K), rs.standard_normal((K, d))


@functools.lru_cache(maxsize=None)
def _fold_truth(d, K, dtype, n):
    x, resp, means = _fold_data(d, K, dtype)
    return mstep_truth(x[:n], resp[:n], means)


@pytest.mark.parametrize(
    "dtype,dk,n,pad", itertools.product(DTYPES, es.FOLD_DK, es.FOLD_N, PADS),
    ids=_name)
def test_mstep_folds_16_to_34_chunks(dtype, dk, n, pad):
    d, K = dk
    x, resp, means = _fold_data(d, K, dtype)
    kern = Kernels(x[:n], pad, K)
    mstep_twice(kern, x, n, resp, means, _fold_truth(d, K, dtype, n))


@pytest.mark.parametrize("dtype,n,pad",
                         itertools.product(DTYPES, es.ESTEP_N, PADS),
                         ids=_name)
def test_estep_133_and_257_blocks(dtype, n, pad):
    d, K = es.ESTEP_DK
    rs = np.random.RandomState(n)
    x = (rs.standard_normal((n, d)) * 2.0).astype(dtype)
    mu, pc, w, ldw = _model(rs, d, K)
    truth = gr.estep(x, w, mu, pc, LD, ldw=ldw)
    kern = Kernels(x, pad, K)
    got = kern.estep(n, mu, pc, ldw, _lib.GM_UPPER)
    check_estep(x, n, mu, pc, ldw, got, truth)
    same_estep(got, kern.estep(n, mu, pc, ldw, 0))


# ---------------------------------------------------------------------------
# 2. the chunk cap
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _cap_data(d, K, dtype):
    rs = np.random.RandomState(10 * d + K)
    nmax = max(es.CAP_N)
    x = (rs.standard_normal((nmax, d)) * 2.0 + 0.5).astype(dtype)
    return (x, random_resp(rs, nmax, K), rs.standard_normal((K, d)),
            _model(rs, d, K))


@functools.lru_cache(maxsize=2)
def _cap_truth(d, K, dtype, n):
    x, resp, means, (mu, pc, w, ldw) = _cap_data(d, K, dtype)
    return (mstep_truth(x[:n], resp[:n], means),
            gr.estep(x[:n], w, mu, pc, LD, ldw=ldw))


CAP_CASES = [(np.float64, dk, n, pad) for dk in es.CAP_DK for n in es.CAP_N
             for pad in PADS] + [(np.float32, es.CAP_DK[1], es.CAP_N[2], 3)]


@pytest.mark.parametrize("dtype,dk,n,pad", CAP_CASES, ids=_name)
def test_mstep_and_estep_at_the_chunk_cap(dtype, dk, n, pad):
    d, K = dk
    x, resp, means, (mu, pc, w, ldw) = _cap_data(d, K, dtype)
    mtruth, etruth = _cap_truth(d, K, dtype, n)
    kern = Kernels(x[:n], pad, K)
    mstep_twice(kern, x, n, resp, means, mtruth)
    got = kern.estep(n, mu, pc, ldw, _lib.GM_UPPER)
    check_estep(x, n, mu, pc, ldw, got, etruth)
    if K == 1:
        assert (got[0] == 1.0).all()


# ---------------------------------------------------------------------------
# 3. the covariances' chunks capped below the sums'
# ---------------------------------------------------------------------------
# bytes behind the workspace: more than one chunk's covariance partials
# (K T 2048 B, about 8 MiB at both shapes), so that a ninth chunk -- the
# sums' chunking taken for the covariances' -- lands in the guard
GUARD = 16 << 20


def _cov_cap_data(d, K, n, dtype):
    rs = np.random.RandomState(d + K)
    x = (rs.standard_normal((n, d)) * 2.0 + 1.0).astype(dtype)
    return x, random_resp(rs, n, K), rs.standard_normal((K, d))


@pytest.mark.parametrize("dtype,pad", [(np.float64, 0), (np.float32, 3)],
                         ids=_name)
def test_cov_cap_fills_the_workspace_d1_k4096(dtype, pad):
    d, K, n = es.COV_CAP[0]
    x, resp, means = _cov_cap_data(d, K, n, dtype)
    kern = Kernels(x, pad, K, guard=GUARD)
    # the covariance partials are the whole workspace: the guard behind it
    # is checked after every call
    assert kern.so.dkm_gm_workspace_bytes(n, d, K) == \
        _device.gm_cov_chunks(n, d, K) * K * 2048 == _device.GM_COV_WORKSPACE
    mstep_twice(kern, x, n, resp, means)


def check_mstep_fp64(kern, x, n, resp, means, ks):
    """check_mstep against fp64 numpy (BLAS), whose own summation error has
    the bound's form: twice the bound; the components ``ks`` against the
    longdouble restatement with the bound itself."""
    K = means.shape[0]
    x64, r = x[:n].astype(np.float64), resp[:n]
    nk, s = kern.sums(n, resp)
    bnk = (n + 8) * U * np.abs(r).sum(axis=0)
    bs = (n + 8) * U * (np.abs(r).T @ np.abs(x64))
    rnk, rsum = gr.mstep_sums(x64, r)
    assert (np.abs(nk - rnk) <= 2 * bnk).all()
    assert (np.abs(s - rsum) <= 2 * bs).all()
    cov = kern.cov(n, resp, means)
    bounds = {}
    for k in range(K):
        diff = x64 - means[k]
        ad = np.abs(diff)
        bound = (n + 8) * U * ((np.abs(r[:, k]) * ad.T) @ ad)
        ref = np.dot(r[:, k] * diff.T, diff)
        assert (np.abs(cov[k] - ref) <= 2 * bound).all(), k
        assert np.array_equal(cov[k], cov[k].T), k
        if k in ks:
            bounds[k] = bound
    for k in ks:
        tnk, ts = gr.mstep_sums(x[:n], r[:, k:k + 1], LD)
        assert abs(float(LD(nk[k]) - tnk[0])) <= bnk[k]
        assert (np.abs((s[k].astype(LD) - ts[0]).astype(np.float64))
                <= bs[k]).all()
        tcov = gr.mstep_cov(x[:n], r[:, k:k + 1], means[k:k + 1], LD)[0]
        assert (np.abs((cov[k].astype(LD) - tcov).astype(np.float64))
                <= bounds[k]).all(), k
    return nk, s, cov


@pytest.mark.parametrize("dtype,pad", [(np.float64, 0), (np.float32, 3)],
                         ids=_name)
def test_cov_cap_three_tiles_d17_k1366(dtype, pad):
    d, K, n = es.COV_CAP[1]
    x, resp, means = _cov_cap_data(d, K, n, dtype)
    kern = Kernels(x, pad, K, guard=GUARD)
    assert kern.so.dkm_gm_workspace_bytes(n, d, K) == \
        _device.gm_cov_chunks(n, d, K) * K * 3 * 2048
    a = check_mstep_fp64(kern, x, n, resp, means, (0, K // 2, K - 1))
    nk, s = kern.sums(n, resp)
    same_mstep(a, (nk, s, kern.cov(n, resp, means)))


# ---------------------------------------------------------------------------
# 4. the E-step's register layouts
# ---------------------------------------------------------------------------
def _nmax(d):
    return 517 if d <= 64 else 2 * _device.gm_estep_block(d) + 5


def _mstep_rows(d):
    m = _device.GM_MSTEP_ROWS
    return (m - 1, m, m + 1, _nmax(d))


@functools.lru_cache(maxsize=2)
def _layout_data(d, K, dtype):
    rs = np.random.RandomState(100 * d + K)
    x = (rs.standard_normal((_nmax(d), d)) * 2.0).astype(dtype)
    mu, pc, w, ldw = _model(rs, d, K)
    truth = gr.estep(x, w, mu, pc, LD, ldw=ldw)
    resp, means = truth["resp"].astype(np.float64), mu + 0.1
    mtruth = {n: mstep_truth(x[:n], resp[:n], means) for n in _mstep_rows(d)}
    return x, (mu, pc, w, ldw), truth, resp, means, mtruth


@pytest.mark.parametrize("dtype,dk,pad",
                         itertools.product(DTYPES, es.LAYOUT_DK, PADS),
                         ids=_name)
def test_layout_ends_and_streamed_sizes(dtype, dk, pad):
    d, K = dk
    x, (mu, pc, w, ldw), truth, resp, means, mtruth = \
        _layout_data(d, K, dtype)
    kern = Kernels(x, pad, K)
    t, blk = _device.GM_TILE, _device.gm_estep_block(d)
    for n in (t - 1, t, t + 1, 2 * t + 1, 0, blk - 1, blk + 1, _nmax(d)):
        got = kern.estep(n, mu, pc, ldw, _lib.GM_UPPER)
        check_estep(x, n, mu, pc, ldw, got, truth)
        # the panel skip changes no bit, and a rerun gives the same bytes
        for flags in (0, _lib.GM_UPPER):
            same_estep(got, kern.estep(n, mu, pc, ldw, flags))
    for n in _mstep_rows(d):
        mstep_twice(kern, x, n, resp, means, mtruth[n])


# ---------------------------------------------------------------------------
# 5. lower-triangular factors in the other layouts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", itertools.product(DTYPES, es.LOWER_D),
                         ids=_name)
def test_lower_triangular_factors_in_every_layout(dtype, d):
    rs = np.random.RandomState(50 + d)
    K, n = 3, 2 * _device.gm_estep_block(d) + 5
    x = (rs.standard_normal((n, d)) * 2.0).astype(dtype)
    mu, pc, w, ldw = _model(rs, d, K, lower=True)
    assert np.tril(pc, -1).any() and not np.triu(pc, 1).any()
    truth = gr.estep(x, w, mu, pc, LD, ldw=ldw)
    got = Kernels(x, 3, K).estep(n, mu, pc, ldw, 0)
    check_estep(x, n, mu, pc, ldw, got, truth)


# ---------------------------------------------------------------------------
# 6. labels = NULL;  7. rows independent of their neighbours
# ---------------------------------------------------------------------------
def _rows(d, K, dtype, seed=0):
    rs = np.random.RandomState(7 * d + K + seed)
    n = 2 * _device.gm_estep_block(d) + 5
    x = (rs.standard_normal((n, d)) * 2.0).astype(dtype)
    return rs, n, x, _model(rs, d, K)


@pytest.mark.parametrize("dtype,dk",
                         itertools.product(DTYPES, es.PER_LAYOUT_DK),
                         ids=_name)
def test_labels_null_changes_no_byte(dtype, dk):
    d, K = dk
    rs, n, x, (mu, pc, w, ldw) = _rows(d, K, dtype)
    kern = Kernels(x, 3, K)
    got = kern.estep(n, mu, pc, ldw, _lib.GM_UPPER)
    check_estep(x, n, mu, pc, ldw, got, gr.estep(x, w, mu, pc, LD, ldw=ldw))
    bare = kern.estep(n, mu, pc, ldw, _lib.GM_UPPER, labels=False)
    assert bare[0].tobytes() == got[0].tobytes()
    assert np.array(bare[2]).tobytes() == np.array(got[2]).tobytes()


@pytest.mark.parametrize("dtype,dk",
                         itertools.product(DTYPES, es.PER_LAYOUT_DK),
                         ids=_name)
def test_rows_are_independent_of_their_neighbours(dtype, dk):
    d, K = dk
    rs, n, x, (mu, pc, w, ldw) = _rows(d, K, dtype, seed=1)

    def run(rows):
        return Kernels(rows, 3, K).estep(len(rows), mu, pc, ldw,
                                         _lib.GM_UPPER)

    resp, lab, tot = run(x)
    assert np.isfinite(resp).all() and np.isfinite(tot)
    # permuted rows give permuted bits
    perm = rs.permutation(n)
    assert not np.array_equal(perm // 16, np.arange(n) // 16)
    presp, plab, _ = run(np.ascontiguousarray(x[perm]))
    assert presp.tobytes() == resp[perm].tobytes()
    assert plab.tobytes() == lab[perm].tobytes()
    # a prefix alone gives the bits it has in the full run
    for m in (7, _device.gm_estep_block(d) + 3):
        fresp, flab, _ = run(np.ascontiguousarray(x[:m]))
        assert fresp.tobytes() == resp[:m].tobytes()
        assert flab.tobytes() == lab[:m].tobytes()
    # another row in one place changes that row alone
    i = 21
    y = x.copy()
    y[i] = (rs.standard_normal(d) * 2.0).astype(dtype)
    cresp, clab, _ = run(y)
    others = np.arange(n) != i
    assert cresp[others].tobytes() == resp[others].tobytes()
    assert clab[others].tobytes() == lab[others].tobytes()
    assert not np.array_equal(cresp[i], resp[i]) or K == 1


# ---------------------------------------------------------------------------
# 8. non-finite samples
# ---------------------------------------------------------------------------
def _nonfinite(x):
    """x with a NaN, a +inf, a -inf and (fp64: squares overflow) a 1e200
    row, in different tiles, blocks and lane groups: the rows changed."""
    d = x.shape[1]
    bad = x.copy()
    bad[3, 0] = np.nan
    bad[22, d - 1] = np.inf
    bad[41, d // 2] = -np.inf
    rows = [3, 22, 41]
    if x.dtype == np.float64:
        bad[140] = 1e200
        rows.append(140)
    return bad, np.array(rows)


@pytest.mark.parametrize("dtype,dk",
                         itertools.product(DTYPES, es.NONFINITE_DK),
                         ids=_name)
def test_nonfinite_rows_stay_in_their_rows(dtype, dk):
    d, K = dk
    rs = np.random.RandomState(3 * d + K)
    n = 2 * _device.gm_estep_block(d)
    x = (rs.standard_normal((n, d)) * 2.0).astype(dtype)
    mu, pc, w, ldw = _model(rs, d, K)
    bad, rows = _nonfinite(x)
    others = np.ones(n, dtype=bool)
    others[rows] = False
    # the fp64 restatement (numpy, scipy's logsumexp): those rows are NaN
    # throughout and their argmax is 0
    with np.errstate(all="ignore"):
        ref = gr.estep(bad, w, mu, pc, np.float64, ldw=ldw)
    assert np.isnan(ref["resp"][rows]).all()
    assert (ref["resp"][rows].argmax(axis=1) == 0).all()
    assert not np.isfinite(ref["total"])
    clean = Kernels(x, 3, K).estep(n, mu, pc, ldw, _lib.GM_UPPER)
    for flags in (_lib.GM_UPPER, 0):
        resp, lab, tot = Kernels(bad, 3, K).estep(n, mu, pc, ldw, flags)
        assert resp[others].tobytes() == clean[0][others].tobytes()
        assert lab[others].tobytes() == clean[1][others].tobytes()
        assert np.isnan(resp[rows]).all()
        assert (lab[rows] == 0).all()
        assert not np.isfinite(tot)


@pytest.mark.parametrize("dtype,dk",
                         itertools.product(DTYPES, es.NONFINITE_DK),
                         ids=_name)
def test_mstep_nan_sample_reaches_what_numpy_makes_nan(dtype, dk):
    d, K = dk
    rs = np.random.RandomState(5 * d + K)
    n, i, j = 600, 37, d // 2
    x = (rs.standard_normal((n, d)) * 2.0).astype(dtype)
    mu, pc, w, ldw = _model(rs, d, K)
    resp = gr.estep(x, w, mu, pc, np.float64, ldw=ldw)["resp"]
    assert np.isfinite(resp).all()
    means = mu + 0.1
    bad = x.copy()
    bad[i, j] = np.nan
    kern = Kernels(bad, 3, K)
    nk, s = kern.sums(n, resp)
    cov = kern.cov(n, resp, means)
    with np.errstate(all="ignore"):
        rnk, rsum = gr.mstep_sums(bad.astype(np.float64), resp)
        rcov = gr.mstep_cov(bad.astype(np.float64), resp, means)
    assert np.isfinite(nk).all() and np.isfinite(rnk).all()
    assert np.array_equal(np.isnan(s), np.isnan(rsum))
    assert np.array_equal(np.isnan(cov), np.isnan(rcov))
    # column j of the sums, row and column j of every covariance
    want = np.zeros((d, d), dtype=bool)
    want[j, :] = want[:, j] = True
    assert np.isnan(s[:, j]).all() and np.isnan(s).sum() == K
    assert all(np.array_equal(np.isnan(c), want) for c in cov)
    # every other entry has the bits of the run on the finite sample: an
    # entry of the MFMA's result depends on its own row and column alone
    good = Kernels(x, 3, K)
    gnk, gs = good.sums(n, resp)
    gcov = good.cov(n, resp, means)
    keep = np.arange(d) != j
    assert nk.tobytes() == gnk.tobytes()
    assert s[:, keep].tobytes() == gs[:, keep].tobytes()
    assert cov[:, ~want].tobytes() == gcov[:, ~want].tobytes()


# ---------------------------------------------------------------------------
# 9. dkm_gm_onehot
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,K", es.ONEHOT_NK + [es.ONEHOT_BIG])
def test_onehot_against_numpy(n, K):
    so = _lib.lib()
    rs = np.random.RandomState(n + K)
    lab = rs.randint(-1, K + 1, n).astype(np.int32)
    if n >= 2:
        lab[0], lab[-1] = -1, K             # outside [0, K): all-zero rows
    if n >= 100:
        lab[n // 2] = np.iinfo(np.int32).min
    want = (lab[:, None] == np.arange(K)).astype(np.float64)
    if n >= 2:
        assert not want[0].any() and not want[-1].any()
    buf = torch.full((n + 1, K), -7.0, dtype=torch.float64, device="cuda")
    ld = torch.from_numpy(lab).cuda() if n else None
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(so.dkm_gm_onehot(
        ctypes.c_void_p(ld.data_ptr()) if n else None, n, K,
        ctypes.c_void_p(buf.data_ptr()), st), "onehot")
    got = buf.cpu().numpy()
    assert (got[n] == -7.0).all()           # the guard row
    assert np.array_equal(got[:n], want)


# ---------------------------------------------------------------------------
# 10. a matrix that starts one element into its buffer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,pad", itertools.product(DTYPES, PADS),
                         ids=_name)
def test_misaligned_base(dtype, pad):
    rs = np.random.RandomState(17 + pad)
    d, K, n = 17, 3, 150
    x = (rs.standard_normal((n, d)) * 2.0).astype(dtype)
    mu, pc, w, ldw = _model(rs, d, K)
    truth = gr.estep(x, w, mu, pc, LD, ldw=ldw)
    kern = Kernels(x, pad, K, offset=1)
    assert kern.X.data_ptr() % 16 == x.itemsize
    got = kern.estep(n, mu, pc, ldw, _lib.GM_UPPER)
    check_estep(x, n, mu, pc, ldw, got, truth)
    same_estep(got, Kernels(x, pad, K).estep(n, mu, pc, ldw, _lib.GM_UPPER))
    resp = truth["resp"].astype(np.float64)
    a = check_mstep(kern, x, n, resp, mu + 0.1)
    aligned = Kernels(x, pad, K)
    nk, s = aligned.sums(n, resp)
    same_mstep(a, (nk, s, aligned.cov(n, resp, mu + 0.1)))
