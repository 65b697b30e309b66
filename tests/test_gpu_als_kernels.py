"""GPU tests of the ALS entries of the C ABI (dkm_als.hip) called one by one,
and of the device CSR transpose.

``dkm_als_update_*``: each of the 8 tile counts NT = ceil(n_f / 16) at its
first and last n_f (1, 16 | 17 | 33, 48 | 49, 64 | 65, 80 | 81, 96 | 97, 100,
112 | 113, 128), every gather-chunk edge, grids of 1, 2 and 257 rows, a
strided X with NaN padding, rows of X that must stay unread (un-gathered,
gathered through stored zeros only, at or past the bound ``m``), column
indices outside [0, m), mixed-sign factors and ratings, a duplicated and a
descending column, and the small-lambda family where the Cholesky's accuracy
is what the bound measures.  ``dkm_als_sse``: two lane trips, every fold
edge of the final sum, ranges and offsets, columns past ``n_items``, an
exactly sized workspace.  ``dkm_als_row_means``: partly filled last blocks.

The yardstick is ``tests/als_ref.py`` in longdouble (the older tests keep
fp64 numpy); Y, the workspace and ``out`` carry guard elements, the CSR
arrays a poisoned entry past ``indptr[-1]``."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from dislib_amd import _lib
from tests import als_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CH = _lib.ALS_CHUNK
LAMBDA = 0.065
LD = np.longdouble
# lengths of the rows of a test matrix, in order (cycled over the rows)
ROW_LENGTHS = [0, 1, 3, 4, 5, CH - 1, CH, CH + 1, 3 * CH + 1]
GUARD = 7.0          # what Y's body and every guard element hold beforehand
# negative, fractional and large ratings
VALUES = np.array([-4.0, -0.5, 0.25, 1e6, -1e6, 3.75, 1.0, -2.5e-3, 1e-3])


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


def _x_buffer(x, pad, lead):
    """x in a device buffer with row stride n_f + pad and ``lead`` more rows
    in front of row 0, NaN in the padding columns and in those rows (a
    kernel that reads either shows; a column index of -1 .. -lead stays
    inside the allocation).  Returns the buffer and the pointer to row 0."""
    ld = x.shape[1] + pad
    buf = torch.full((lead + max(1, x.shape[0]), ld), float("nan"),
                     dtype=torch.from_numpy(x[:0]).dtype, device="cuda")
    buf[lead:lead + x.shape[0], :x.shape[1]] = torch.from_numpy(x).cuda()
    return buf, ctypes.c_void_p(buf.data_ptr() +
                                lead * ld * buf.element_size())


def _update(so, r, x, lambda_=LAMBDA, pad=0, m=None, lead=0):
    """Y of one half-step.  X has row stride n_f + pad; ``m`` is the bound
    on the columns handed to the kernel (``x.shape[0]`` by default: rows of
    x from m on are in the buffer, and must stay unread).  Y has 2 guard
    rows behind it, the CSR arrays one poisoned entry (a valid column with
    a NaN rating) past ``indptr[-1]``."""
    n_rows, n_f = r.shape[0], x.shape[1]
    xb, xp = _x_buffer(x, pad, lead)
    y = torch.full((n_rows + 2, n_f), GUARD, dtype=torch.float32,
                   device="cuda")
    ind = _dev(np.append(np.asarray(r.indices, dtype=np.int32), np.int32(0)))
    dat = _dev(np.append(np.asarray(r.data, dtype=np.float64), np.nan))
    ptr = _dev(r.indptr.astype(np.int64))   # held until the kernel has run
    fn = so.dkm_als_update_f32 if x.dtype == np.float32 else \
        so.dkm_als_update_f64
    _lib.check(fn(_p(ptr), _p(ind), _p(dat), n_rows, xp,
                  x.shape[0] if m is None else m, n_f, n_f + pad,
                  lambda_, _p(y), _stream()), "dkm_als_update")
    torch.cuda.synchronize()
    out = y.cpu().numpy()
    assert np.array_equal(out[n_rows:], np.full((2, n_f), GUARD, np.float32))
    del xb
    return out[:n_rows]


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


def _check_rows(y, r, x, lambda_=LAMBDA, m=None):
    """Every row of y against ``als_ref.update_rows`` in longdouble (entries
    with a zero rating or a column outside [0, m) dropped, duplicates kept
    apart), under the same bound with cond from the fp64 matrix; exact zeros
    for a row that uses no entry.  Returns the worst err / bound."""
    n_f = x.shape[1]
    assert y.dtype == np.float32 and y.shape == (r.shape[0], n_f)
    rows = ref.update_rows(r, x, lambda_, m, LD)
    worst = 0.0
    for i, (want, cond) in enumerate(rows):
        if cond == 0.0:
            assert np.array_equal(y[i], np.zeros(n_f, np.float32)), i
            continue
        err = np.abs((y[i].astype(LD) - want).astype(np.float64))
        bound = ref.update_bound(want, cond, n_f)
        ratio = float((err / bound).max())
        assert (err <= bound).all(), (i, ratio)      # a NaN fails here too
        worst = max(worst, ratio)
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


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n_f", [48, 49, 64, 65, 80, 81, 96, 97, 112, 113])
def test_update_first_and_last_n_f_of_every_tile_count(n_f, dtype):
    """NT = 3 .. 8 at their edges; NT = 4, 5, 6 (10, 15 and 21 Gram tiles on
    4 waves: some waves hold a surplus slot) run nowhere else.  Mixed-sign
    factors, so that a tile that lands in the wrong place does not look like
    its neighbour.  n_f = 65 also walks the grid of 1, 2 and 257 rows."""
    so = _lib.lib()
    m = 3 * CH + 5
    x = np.random.default_rng(n_f).uniform(-1, 1, (m, n_f)).astype(dtype)
    for n_rows in (1, 2, 257) if n_f == 65 else (18,):
        r = _ratings(max(n_rows, 9), m, 200 + n_rows, zero_row=12)
        if n_rows < 9:
            r = sp.csr_matrix(r[9 - n_rows:9])
            r.sort_indices()
        y = _update(so, r, x)
        worst = _check_rows(y, r, x)
        print("n_f %d %s n_rows %d: worst err / bound %.3g" % (
            n_f, np.dtype(dtype).name, n_rows, worst))
        assert np.array_equal(y, _update(so, r, x))     # byte-identical


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n_f", [1, 17, 49, 81, 128])
def test_update_strided_x_equals_contiguous(n_f, dtype):
    """ldx = n_f + 3 with NaN in the padding: the same bytes as ldx = n_f."""
    so = _lib.lib()
    m = 3 * CH + 5
    x = np.random.default_rng(n_f).uniform(-1, 1, (m, n_f)).astype(dtype)
    r = _ratings(18, m, 300, zero_row=12)
    y = _update(so, r, x, pad=0)
    worst = _check_rows(y, r, x)
    print("n_f %d %s: worst err / bound %.3g" % (n_f, np.dtype(dtype).name,
                                                  worst))
    ys = _update(so, r, x, pad=3)
    assert np.array_equal(ys, y)
    assert np.array_equal(ys, _update(so, r, x, pad=3))


def _unread_case(seed):
    """18 rows cycling ROW_LENGTHS over 60 factor rows with the bound m = 50:
    columns 0 .. 39 are rated, 40 .. 44 hold stored zeros only, 45 .. 49
    nothing, 50 .. 59 lie at or past m.  Returns the matrix and the mask of
    the factor rows that no used entry gathers."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(18):
        ln = min(ROW_LENGTHS[i % len(ROW_LENGTHS)], 40)
        cols = list(rng.choice(40, ln, replace=False))
        vals = list(rng.integers(1, 6, ln).astype(np.float64))
        if ln >= 4:
            vals[1] = 0.0
        if i:                                # row 0 stays empty
            cols += [40 + i % 5, 50 + i % 10]
            vals += [0.0, 3.0]
        rows.append((cols, vals))
    r = ref.Csr.from_rows(rows, 60)
    unread = np.ones(60, dtype=bool)
    for i in range(18):
        unread[ref.used_entries(r, i, 50)[0]] = False
    assert unread[40:].all() and not unread[:40].all()
    return r, unread


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_update_never_reads_rows_it_does_not_gather(dtype):
    """NaN in every factor row that no entry gathers, that only stored zeros
    reference, or that lies at or past m: finite, and the bytes of the run
    with finite garbage there.  Then the estimator's own shape: NaN in
    column 0 of the un-gathered rows only (an item without ratings has a NaN
    mean in the initial items)."""
    so = _lib.lib()
    n_f = 17
    r, unread = _unread_case(4)
    x = np.random.default_rng(5).uniform(-1, 1, (60, n_f)).astype(dtype)
    x_nan, x_fin, x_col0 = x.copy(), x.copy(), x.copy()
    x_nan[unread] = np.nan
    x_fin[unread] = 1e30
    x_col0[unread, 0] = np.nan
    y = _update(so, r, x_nan, pad=3, m=50)
    assert np.isfinite(y).all()
    worst = _check_rows(y, r, x_fin, m=50)
    print("%s: worst err / bound %.3g" % (np.dtype(dtype).name, worst))
    assert np.array_equal(y[0], np.zeros(n_f, np.float32))
    assert np.array_equal(y[9], np.zeros(n_f, np.float32))   # 0 and >= m only
    assert np.array_equal(y, _update(so, r, x_fin, pad=3, m=50))
    assert np.array_equal(y, _update(so, r, x_col0, pad=3, m=50))
    assert np.array_equal(y, _update(so, r, x_nan, pad=3, m=50))


def _index_bound_case(m, seed):
    """Rows whose columns leave [0, m) by at most 8 on either side (the
    caller's buffer holds NaN rows there, so that a kernel without the
    guard returns NaN and touches nothing outside the allocation)."""
    rng = np.random.default_rng(seed)

    def row(ln, out):
        cols = rng.choice(m, ln, replace=False)
        for pos, col in out.items():
            cols[pos] = col
        return cols, rng.integers(1, 6, ln).astype(np.float64)

    return ref.Csr.from_rows([
        row(4, {0: m, 1: m + 7, 2: -1, 3: m + 5}),            # none in range
        row(4, {0: m + 1, 2: -2, 3: m + 6}),                  # n_c = 1
        # the last entry of a full chunk and the first of the next
        row(CH + 3, {CH - 1: m + 4, CH: m + 2}),
        row(3 * CH + 1, {0: m, 2 * CH - 1: -1, 2 * CH: m + 3, 3 * CH: m + 7}),
        row(CH, {}),                                          # all in range
        row(1, {0: -8}),
        row(2 * CH, {CH - 1: -3, CH: -4}),
    ], m)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n_f", [17, 49])
def test_update_skips_columns_outside_the_factor_matrix(n_f, dtype):
    """Entries with a column < 0 or >= m are dropped from the Gram sum, from
    v and from n_c; a row of such entries only gives zeros."""
    so = _lib.lib()
    m = 3 * CH + 5
    r = _index_bound_case(m, 6)
    assert [len(ref.used_entries(r, i, m)[0]) for i in range(r.shape[0])] == \
        [0, 1, CH + 1, 3 * CH - 3, CH, 0, 2 * CH - 2]
    x = np.full((m + 8, n_f), np.nan, dtype=dtype)
    x[:m] = np.random.default_rng(n_f).uniform(-1, 1, (m, n_f))
    y = _update(so, r, x, pad=3, m=m, lead=8)
    assert np.isfinite(y).all()
    worst = _check_rows(y, r, x, m=m)
    print("n_f %d %s: worst err / bound %.3g" % (n_f, np.dtype(dtype).name,
                                                  worst))
    for i in (0, 5):
        assert np.array_equal(y[i], np.zeros(n_f, np.float32))
    # n_c = 1: y = x r / (|x|^2 + lambda), so n_c = 4 would show
    c = r.indices[r.indptr[1] + 1]
    x1 = x[c].astype(np.float64)
    want = x1 * r.data[r.indptr[1] + 1] / (x1.dot(x1) + LAMBDA)
    assert np.allclose(y[1], want, rtol=1e-6, atol=0)
    assert np.array_equal(y, _update(so, r, x, pad=3, m=m, lead=8))


def _merge_duplicates(cols, vals):
    """The row as ``sparse.find`` would hand it over: duplicates summed."""
    u = np.unique(cols)
    return u, np.array([np.sum(np.asarray(vals)[np.asarray(cols) == c])
                        for c in u])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n_f", [17, 65])
def test_update_signs_fractions_duplicates_and_column_order(n_f, dtype):
    """Factors uniform in [-1, 1); ratings negative, fractional and 1e6;
    a column stored twice stays two entries (not summed); a row with
    descending columns."""
    so = _lib.lib()
    m = 3 * CH + 5
    rng = np.random.default_rng(n_f + 1)
    x = rng.uniform(-1, 1, (m, n_f)).astype(dtype)
    rows = []
    for i in range(18):
        ln = ROW_LENGTHS[i % len(ROW_LENGTHS)]
        cols = rng.permutation(m)[:ln]                   # unsorted
        vals = rng.choice(VALUES, ln) * rng.choice([1.0, 0.5, 1.25], ln)
        if ln >= 4:
            vals[2] = 0.0
        rows.append((cols, vals))
    dup = ([3, 9, 3, 20, 9, 9], [2.0, -1.5, 0.75, 4.0, 2.5, -0.25])
    rows.append(dup)
    desc = np.sort(rng.choice(m, 3 * CH + 1, replace=False))[::-1]
    rows.append((desc, rng.choice(VALUES, len(desc))))
    rows.append((desc[::-1], rows[-1][1][::-1]))         # the same, ascending
    r = ref.Csr.from_rows(rows, m)
    y = _update(so, r, x)
    worst = _check_rows(y, r, x)
    print("n_f %d %s: worst err / bound %.3g" % (n_f, np.dtype(dtype).name,
                                                  worst))
    # summed duplicates are another system: beyond the bound somewhere
    merged = ref.Csr.from_rows([_merge_duplicates(*dup)], m)
    (ym, cond), = ref.update_rows(merged, x, LAMBDA)
    assert (np.abs((y[18].astype(LD) - ym).astype(np.float64)) >
            ref.update_bound(ym, cond, n_f)).any()
    assert np.array_equal(y, _update(so, r, x))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n_f", ref.COND_NF)
def test_update_small_lambda_and_fewer_entries_than_factors(n_f, dtype):
    """lambda = 1e-6, n_c = 1, 2, n_f - 1, n_f, n_f + 1: cond(A) up to 1e8,
    where an fp64 reference's own error would sit inside the bound; the
    longdouble one's does not.  ``tests/test_als_host.py`` shows that the
    bound's conditioning term stays below 2^-12 on these inputs."""
    so = _lib.lib()
    r, x = ref.conditioning_case(n_f, dtype)
    y = _update(so, r, x, ref.COND_LAMBDA)
    worst = _check_rows(y, r, x, ref.COND_LAMBDA)
    print("n_f %d %s: worst err / bound %.3g" % (n_f, np.dtype(dtype).name,
                                                  worst))
    assert np.array_equal(y, _update(so, r, x, ref.COND_LAMBDA))


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


def _sse(so, r, users, items, a, b, off, n_items=None):
    """(sum, count) of rows [a, b).  The workspace is as large as the ABI
    asks for b - a rows and no larger; 64 bytes behind it, 2 doubles behind
    ``out`` and a poisoned CSR entry past ``indptr[-1]`` must survive."""
    n_f = users.shape[1]
    wsb = int(so.dkm_als_workspace_bytes(b - a, n_f))
    assert wsb == 16 * max(b - a, 1)
    ws = torch.full((wsb + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((4,), GUARD, dtype=torch.float64, device="cuda")
    # every operand is held until the kernel has run: a temporary's buffer
    # goes back to the allocator, and the next upload may land in it
    ptr, ind, dat = _dev(r.indptr.astype(np.int64)), \
        _dev(np.append(np.asarray(r.indices, dtype=np.int32), np.int32(0))), \
        _dev(np.append(np.asarray(r.data, dtype=np.float64), np.nan))
    ud, idv = _dev(users), _dev(items)
    _lib.check(so.dkm_als_sse(
        _p(ptr), _p(ind), _p(dat), a, b, off, _p(ud), users.shape[0],
        _p(idv), items.shape[0] if n_items is None else n_items, n_f, _p(ws),
        wsb, _p(out), _stream()),
        "dkm_als_sse")
    torch.cuda.synchronize()
    assert (ws[wsb:] == 0xA5).all().item()
    got = out.cpu().numpy()
    assert np.array_equal(got[2:], [GUARD, GUARD])
    return got[:2]


@pytest.mark.parametrize("n_f", [1, 33, 100])
def test_sse_ranges_offsets_and_stored_zeros(n_f):
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
        sl, cl, bound = ref.sse_ld(r, users, items, a, b, off)
        assert cl == c and abs(float(LD(got[0]) - sl)) <= bound
        assert np.array_equal(got, _sse(so, r, users, items, a, b, off))
    # users past the matrix: refused before any launch
    wsb = int(so.dkm_als_workspace_bytes(10, n_f))
    z = torch.zeros(max(wsb, 64), dtype=torch.uint8, device="cuda")
    rc = so.dkm_als_sse(_p(z), _p(z), _p(z), 0, 10, n_u - 9, _p(z), n_u,
                        _p(z), n_i, n_f, _p(z), wsb, _p(z), _stream())
    assert rc == 10001


SSE_LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 200]
# (row_begin, row_end, user_offset): 0, 1, 3, 4, 5, 255, 256, 257, 300 rows
SSE_RANGES = [(40, 40, 3), (7, 8, 292), (5, 8, 1), (3, 7, 2), (11, 16, 9),
              (17, 272, 5), (44, 300, 2), (43, 300, 1), (0, 300, 7)]


def _sse_case():
    """300 x 200, row i storing SSE_LENGTHS[i % 9] mixed-sign ratings at
    sorted random columns: stored zeros inside the longer rows, row 12 (64
    entries) zeros only.  Columns from 180 on are past the n_items = 180
    that the kernel is given."""
    rng = np.random.default_rng(8)
    rows = []
    for i in range(300):
        ln = SSE_LENGTHS[i % len(SSE_LENGTHS)]
        cols = np.sort(rng.choice(200, ln, replace=False))
        vals = rng.choice(VALUES[[0, 1, 2, 5, 6]], ln) + rng.random(ln)
        vals[3::5] = 0.0
        if i == 12:
            vals[:] = 0.0
        rows.append((cols, vals))
    r = ref.Csr.from_rows(rows, 200)
    assert (r.indices >= 180).any() and (r.data == 0).any()
    return r


@pytest.mark.parametrize("n_f", [1, 16, 17, 128])
def test_sse_lane_trips_fold_edges_and_item_bound(n_f):
    """Rows of up to 200 entries (4 lane trips), 0 .. 300 rows in the final
    fold, non-zero row_begin and user_offset, items past n_items poisoned:
    the count exactly, the sum within ``als_ref.sse_ld``'s derived bound,
    the same bytes again, and the same bytes with NaN in every rating and
    user row outside the range."""
    so = _lib.lib()
    rng = np.random.default_rng(n_f)
    r = _sse_case()
    users = rng.uniform(-1, 1, (307, n_f)).astype(np.float32)
    items = rng.uniform(-1, 1, (200, n_f)).astype(np.float32)
    items[180:] = np.nan
    worst = 0.0
    for a, b, off in SSE_RANGES:
        nr = b - a
        got = _sse(so, r, users, items, a, b, off, n_items=180)
        s, c, bound = ref.sse_ld(r, users, items, a, b, off, n_items=180)
        assert got[1] == c, (a, b, off)
        err = abs(float(LD(got[0]) - s))
        if nr:
            worst = max(worst, err / bound)
        assert err <= bound, (a, b, off, got[0], float(s), err / bound)
        assert np.array_equal(got, _sse(so, r, users, items, a, b, off,
                                        n_items=180))
        data, u2 = r.data.copy(), users.copy()
        data[:r.indptr[a]] = np.nan
        data[r.indptr[b]:] = np.nan
        u2[:off] = np.nan
        u2[off + nr:] = np.nan
        r2 = ref.Csr(r.indptr, r.indices, data, r.shape)
        assert np.array_equal(got, _sse(so, r2, u2, items, a, b, off,
                                        n_items=180)), (a, b, off)
    assert np.array_equal(_sse(so, r, users, items, 40, 40, 3, n_items=180),
                          [0.0, 0.0])
    print("n_f %d: worst err / bound %.3g" % (n_f, worst))


def test_sse_refusals_before_any_launch():
    so = _lib.lib()
    n_f = 8
    wsb = int(so.dkm_als_workspace_bytes(10, n_f))
    z = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.full((2,), GUARD, dtype=torch.float64, device="cuda")

    def call(a=0, b=10, off=0, nf=n_f, ws_bytes=wsb):
        return so.dkm_als_sse(_p(z), _p(z), _p(z), a, b, off, _p(z), 20,
                              _p(z), 20, nf, _p(z), ws_bytes, _p(out),
                              _stream())

    assert call(ws_bytes=wsb - 1) == 10002            # DKM_E_WORKSPACE
    assert call(a=5, b=4) == 10001
    assert call(off=-1) == 10001
    assert call(nf=0) == 10001
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), [GUARD, GUARD])


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


def _check_transpose(m):
    from dislib_amd.recommendation import als
    shape = m.shape
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
    return got


@pytest.mark.parametrize("shape", [(7, 5), (300, 41)])
def test_transpose_equals_scipy(shape):
    _check_transpose(_random_csr(shape[0], shape[1], 1, 0.4))


@pytest.mark.parametrize("shape", [(0, 5), (5, 0), (1, 7), (7, 1)])
def test_transpose_of_degenerate_shapes(shape):
    rng = np.random.default_rng(9)
    dense = rng.integers(1, 6, shape) * (rng.random(shape) < 0.6)
    m = sp.csr_matrix(dense.astype(np.float64))
    if m.nnz:
        m.data[0] = 0.0                              # a stored zero travels
    assert m.nnz > 1 or 0 in shape
    got = _check_transpose(m)
    # what ALS.fit hands the kernels: valid pointers even without an entry
    assert got.indices.numel() >= 1 and got.data.numel() >= 1
    assert got.data.dtype == torch.float64


def test_transpose_without_entries_and_with_empty_last_columns():
    got = _check_transpose(sp.csr_matrix((4, 6), dtype=np.float64))
    assert got.nnz == 0 and got.indices.numel() == 1 == got.data.numel()
    dense = np.zeros((6, 9))
    dense[:, :6] = np.random.default_rng(10).integers(0, 6, (6, 6))
    dense[5] = 0                                     # ... and an empty row
    got = _check_transpose(sp.csr_matrix(dense))
    assert np.array_equal(got.indptr.cpu().numpy()[-4:], [got.nnz] * 4)


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


MEAN_LENGTHS = [0, 1, 63, 64, 65, 128, 129]


def _row_means(so, m):
    """out[0 .. n_rows) through the C ABI, with one guard element behind it
    that must survive and a NaN past the last stored entry."""
    n = m.shape[0]
    out = torch.full((n + 1,), GUARD, dtype=torch.float64, device="cuda")
    ptr = _dev(m.indptr.astype(np.int64))
    dat = _dev(np.append(m.data, np.nan))
    rc = so.dkm_als_row_means(_p(ptr), _p(dat), n, _p(out), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = out.cpu().numpy()
    assert got[n] == GUARD                  # the row >= n_rows return
    return got[:n]


@pytest.mark.parametrize("n_rows", [1, 2, 3, 4, 5, 257])
def test_row_means_partly_filled_last_block(n_rows):
    """4 rows per block: n_rows = 1, 2, 3, 5, 257 leave waves of the last
    block without a row, which must return before they store.  Mixed-sign
    entries cancel, so 4 ulp of the mean cannot be derived; the bound is
    ``als_ref.row_means_bound``: (len / 64 + 8) u sum |data| / len.  Stored
    zeros count; a row of stored zeros only is 0.0, an empty row NaN."""
    so = _lib.lib()
    rng = np.random.default_rng(n_rows)
    worst = 0.0
    for shift in range(len(MEAN_LENGTHS) if n_rows <= 5 else 1):
        rows = []
        for i in range(n_rows):
            ln = MEAN_LENGTHS[(i + shift) % len(MEAN_LENGTHS)]
            vals = rng.uniform(-5, 5, ln)
            vals[2::3] = 0.0
            if i == n_rows - 1 and shift % 2:
                vals[:] = 0.0
            rows.append((np.arange(ln), vals))
        m = ref.Csr.from_rows(rows, 129)
        got = _row_means(so, m)
        want, bound = ref.row_means_ld(m), ref.row_means_bound(m)
        empty = np.diff(m.indptr) == 0
        assert np.array_equal(np.isnan(got), empty)
        err = np.abs((got[~empty].astype(LD) - want[~empty])
                     .astype(np.float64))
        assert (err <= bound[~empty]).all(), (shift, err / bound[~empty])
        zero = ~empty & np.array([not np.any(v) for _, v in rows])
        assert np.array_equal(got[zero], np.zeros(zero.sum()))
        pos = bound[~empty] > 0
        if pos.any():
            worst = max(worst, float((err[pos] / bound[~empty][pos]).max()))
        assert np.array_equal(got, _row_means(so, m), equal_nan=True)
    print("n_rows %d: worst err / bound %.3g" % (n_rows, worst))


def test_row_means_of_no_rows_launches_nothing():
    so = _lib.lib()
    out = torch.full((2,), GUARD, dtype=torch.float64, device="cuda")
    ptr = _dev(np.zeros(1, np.int64))
    dat = _dev(np.full(1, np.nan))
    assert so.dkm_als_row_means(_p(ptr), _p(dat), 0, _p(out), _stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), [GUARD, GUARD])
