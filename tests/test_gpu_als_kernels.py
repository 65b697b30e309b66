"""GPU tests of the ALS entries of the C ABI (dkm_als.hip) called one by one,
and of the device CSR transpose: every n_f tile count, every gather-chunk
edge, empty rows and rows of stored zeros, against fp64 numpy."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from dislib_amd import _lib

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CH = _lib.ALS_CHUNK
LAMBDA = 0.065
# lengths of the rows of a test matrix, in order (cycled over the rows)
ROW_LENGTHS = [0, 1, 3, 4, 5, CH - 1, CH, CH + 1, 3 * CH + 1]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ratings(n_rows, m, seed, zero_row=None):
    """CSR (n_rows x m) whose row i stores ROW_LENGTHS[i % 9] ratings 1-5 at
    sorted random columns (rows share columns: m is small); ``zero_row``
    stores zeros only."""
    rng = np.random.default_rng(seed)
    indptr, indices, data = [0], [], []
    for i in range(n_rows):
        ln = min(ROW_LENGTHS[i % len(ROW_LENGTHS)], m)
        cols = np.sort(rng.choice(m, ln, replace=False))
        vals = rng.integers(1, 6, ln).astype(np.float64)
        if zero_row is not None and i == zero_row:
            vals[:] = 0.0
        elif ln >= 4:
            vals[1] = 0.0              # a stored zero inside a row
        indices.extend(cols)
        data.extend(vals)
        indptr.append(len(indices))
    return sp.csr_matrix((np.array(data, dtype=np.float64),
                          np.array(indices, dtype=np.int32),
                          np.array(indptr, dtype=np.int64)),
                         shape=(n_rows, m))


def _update(so, r, x, lambda_=LAMBDA):
    xd = _dev(x)
    y = torch.full((r.shape[0], x.shape[1]), 7.0, dtype=torch.float32,
                   device="cuda")
    ind = _dev(r.indices.astype(np.int32) if r.nnz else
               np.zeros(1, np.int32))
    dat = _dev(r.data if r.nnz else np.zeros(1))
    ptr = _dev(r.indptr.astype(np.int64))   # held until the kernel has run
    fn = so.dkm_als_update_f32 if x.dtype == np.float32 else \
        so.dkm_als_update_f64
    _lib.check(fn(_p(ptr), _p(ind), _p(dat),
                  r.shape[0], _p(xd), x.shape[0], x.shape[1], x.shape[1],
                  lambda_, _p(y), _stream()), "dkm_als_update")
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _check_update(y, r, x, lambda_=LAMBDA):
    """Every row against np.linalg.solve of the same fp64 normal equations:
    |y - y64| <= 2^-24 |y64| + 8 n_f cond(A) 2^-53 max|y64| (the fp32 store;
    the forward bound of the Cholesky solve)."""
    n_f = x.shape[1]
    x64 = x.astype(np.float64)
    worst = 0.0
    for i in range(r.shape[0]):
        sl = slice(r.indptr[i], r.indptr[i + 1])
        idx, val = r.indices[sl], r.data[sl]
        idx, val = idx[val != 0], val[val != 0]
        if len(idx) == 0:
            assert np.array_equal(y[i], np.zeros(n_f, np.float32)), i
            continue
        xs = x64[idx]
        a = xs.T.dot(xs) + lambda_ * len(idx) * np.eye(n_f)
        y64 = np.linalg.solve(a, xs.T.dot(val))
        bound = 2.0 ** -24 * np.abs(y64) + \
            8 * n_f * np.linalg.cond(a) * 2.0 ** -53 * np.abs(y64).max()
        err = np.abs(y[i].astype(np.float64) - y64)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (i, len(idx), float((err / bound).max()))
    return worst


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n_f", [1, 3, 15, 16, 17, 33, 100, 128])
def test_update_every_tile_count_and_chunk_edge(n_f, dtype):
    so = _lib.lib()
    m = 3 * CH + 5
    x = np.random.default_rng(n_f).random((m, n_f)).astype(dtype)
    for n_rows in (1, 2, 257) if n_f in (3, 100) else (18,):
        # n_rows = 1: one row of 3 CH + 1 entries (ROW_LENGTHS rotated)
        r = _ratings(max(n_rows, 9), m, 100 + n_rows, zero_row=12)
        if n_rows < 9:
            r = sp.csr_matrix(r[9 - n_rows:9])
            r.sort_indices()
        y = _update(so, r, x)
        assert y.dtype == np.float32 and y.shape == (n_rows, n_f)
        worst = _check_update(y, r, x)
        print("n_f %d %s n_rows %d: worst err / bound %.3g" % (
            n_f, np.dtype(dtype).name, n_rows, worst))
        assert np.array_equal(y, _update(so, r, x))     # byte-identical


def test_update_rows_of_stored_zeros_and_empty_rows_are_zero():
    so = _lib.lib()
    r = sp.csr_matrix((np.zeros(5), np.array([0, 2, 3, 1, 2], np.int32),
                       np.array([0, 3, 3, 5], np.int64)), shape=(3, 4))
    x = np.random.default_rng(0).random((4, 5))
    assert np.array_equal(_update(so, r, x), np.zeros((3, 5), np.float32))


def test_update_bad_arguments_are_refused():
    so = _lib.lib()
    z = torch.zeros(4, dtype=torch.int64, device="cuda")
    rc = so.dkm_als_update_f64(_p(z), _p(z), _p(z), 1, _p(z), 1,
                               _lib.ALS_MAX_NF + 1, _lib.ALS_MAX_NF + 1,
                               LAMBDA, _p(z), _stream())
    assert rc == 10001
    assert so.dkm_als_workspace_bytes(10, _lib.ALS_MAX_NF + 1) == 0
    assert so.dkm_als_workspace_bytes(-1, 8) == 0
    assert so.dkm_als_workspace_bytes(10, 8) >= 160


def _sse(so, r, users, items, a, b, off):
    n_f = users.shape[1]
    wsb = int(so.dkm_als_workspace_bytes(b - a, n_f))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    out = torch.empty(2, dtype=torch.float64, device="cuda")
    # every operand is held until the kernel has run: a temporary's buffer
    # goes back to the allocator, and the next upload may land in it
    ptr, ind, dat = _dev(r.indptr.astype(np.int64)), \
        _dev(r.indices.astype(np.int32)), _dev(r.data)
    ud, idv = _dev(users), _dev(items)
    _lib.check(so.dkm_als_sse(
        _p(ptr), _p(ind), _p(dat), a, b, off, _p(ud), users.shape[0],
        _p(idv), items.shape[0], n_f, _p(ws), wsb, _p(out), _stream()),
        "dkm_als_sse")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("n_f", [1, 33, 100])
def test_sse_ranges_offsets_and_stored_zeros(n_f):
    from tests import als_ref as ref
    so = _lib.lib()
    rng = np.random.default_rng(n_f)
    n_u, n_i = 300, 70
    r = _ratings(n_u, n_i, 5)
    assert (r.data == 0).any()
    users = rng.random((n_u, n_f)).astype(np.float32)
    items = rng.random((n_i, n_f)).astype(np.float32)
    for a, b, off in [(0, n_u, 0), (0, 131, 0), (131, 258, 0),
                      (131, 258, 131), (7, 8, 292), (40, 40, 0)]:
        got = _sse(so, r, users, items, a, b, off)
        s, c = ref.sse(r, users, items, a, b, off)
        assert got[1] == c
        assert abs(got[0] - s) <= 1e-12 * abs(s), (a, b, off, got[0], s)
        assert np.array_equal(got, _sse(so, r, users, items, a, b, off))
    # users past the matrix: refused before any launch
    wsb = int(so.dkm_als_workspace_bytes(10, n_f))
    z = torch.zeros(max(wsb, 64), dtype=torch.uint8, device="cuda")
    rc = so.dkm_als_sse(_p(z), _p(z), _p(z), 0, 10, n_u - 9, _p(z), n_u,
                        _p(z), n_i, n_f, _p(z), wsb, _p(z), _stream())
    assert rc == 10001


def _random_csr(n, d, seed, density):
    rng = np.random.default_rng(seed)
    dense = rng.integers(1, 6, (n, d)) * (rng.random((n, d)) < density)
    dense[n // 2] = 0
    dense[:, d // 3] = 0
    dense[0] = 0
    dense[:, d - 1] = 0
    m = sp.csr_matrix(dense.astype(np.float64))
    m.data[::7] = 0.0                   # stored zeros travel with the rest
    return m


@pytest.mark.parametrize("shape", [(7, 5), (300, 41)])
def test_transpose_equals_scipy(shape):
    from dislib_amd.recommendation import als
    m = _random_csr(shape[0], shape[1], 1, 0.4)
    dm = als._Csr(_dev(m.indptr.astype(np.int64)),
                  _dev(m.indices.astype(np.int32)), _dev(m.data), *shape)
    got = als.csr_transpose(dm)
    want = m.T.tocsr()
    want.sort_indices()
    assert (got.n_rows, got.n_cols) == want.shape and got.nnz == want.nnz
    assert got.indptr.dtype == torch.int64
    assert got.indices.dtype == torch.int32
    assert np.array_equal(got.indptr.cpu().numpy(), want.indptr)
    assert np.array_equal(got.indices.cpu().numpy()[:want.nnz], want.indices)
    assert np.array_equal(got.data.cpu().numpy()[:want.nnz], want.data)


def test_row_means_within_4_ulp():
    from dislib_amd.recommendation import als
    so = _lib.lib()
    rng = np.random.default_rng(2)
    m = _random_csr(300, 200, 3, 0.6)
    m.data[:] = np.where(m.data == 0, 0.0, rng.random(m.nnz) * 5)
    dm = als._Csr(_dev(m.indptr.astype(np.int64)),
                  _dev(m.indices.astype(np.int32)), _dev(m.data), 300, 200)
    got = als.row_means(so, dm).cpu().numpy()
    for i in range(300):
        row = m.data[m.indptr[i]:m.indptr[i + 1]]
        if len(row) == 0:
            assert np.isnan(got[i])
        else:
            want = np.mean(row)
            assert abs(got[i] - want) <= 4 * np.spacing(want), i
