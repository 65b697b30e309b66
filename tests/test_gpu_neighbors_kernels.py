"""GPU tests of the seven kNN / epsilon-query entries of the C ABI
(dkm_neighbors.hip) called directly on raw device arrays, at every dispatch
edge: the register templates of d, the top-K templates, the passes with a
floor, the two-scan path with and without overflow and its second query
chunk, row strides, the segmented sort's runs, the 2^-48 band of the epsilon
decision, and the refusals.

Outputs start as a sentinel (-7).  Dense rows sit ``d + 3`` (queries) and
``d + 5`` (fit rows) doubles apart with NaN between them, and every such case
runs again with tight rows.  Everything is compared bit for bit with
tests/neighbors_ref.py (the oracle's arithmetic).  Every kNN case asserts
its path and partitions through ``dkm_knn_plan``, every two-scan case whether
a candidate list overflowed through ``two_scan_candidates``.
"""
import ctypes

import numpy as np
import pytest

from tests import neighbors_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E_ARG, E_WS = 10001, 10002
NAN = float("nan")


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _so():
    from dislib_amd import _lib
    return _lib.lib()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    from dislib_amd._device import stream_ptr
    return stream_ptr()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _padded(A, ld):
    """A's rows ``ld`` doubles apart, NaN between them."""
    n, d = A.shape
    out = torch.full((max(n, 1), ld), NAN, dtype=torch.float64, device="cuda")
    if n:
        out[:n, :d] = _dev(A)
    return out


def _full(shape, fill, dtype):
    return torch.full(shape, fill, dtype=dtype, device="cuda")


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")


def plan(nq, nx, kn):
    pl, P = ctypes.c_int64(-7), ctypes.c_int32(-7)
    path = _so().dkm_knn_plan(nq, nx, kn, ctypes.byref(pl), ctypes.byref(P))
    return path, pl.value, P.value


# --------------------------------------------------------------------------
# kNN, dense
# --------------------------------------------------------------------------
def run_knn(Q, X, kn, pad):
    """dkm_knn_f64; one guard row after the outputs must keep the
    sentinel."""
    so = _so()
    (nq, d), nx = Q.shape, X.shape[0]
    ldq, ldx = (d + 3, d + 5) if pad else (d, d)
    Qd, Xd = _padded(Q, ldq), _padded(X, ldx)
    wsb = int(so.dkm_knn_workspace_bytes(nq, nx, kn))
    assert wsb > 0
    ws = _ws(wsb)
    od = _full((nq + 1, kn), -7.0, torch.float64)
    oi = _full((nq + 1, kn), -7, torch.int64)
    rc = so.dkm_knn_f64(_ptr(Qd), nq, ldq, _ptr(Xd), nx, ldx, d, kn, _ptr(ws),
                        wsb, _ptr(od), _ptr(oi), _stream())
    assert rc == 0, so.dkm_last_error()
    torch.cuda.synchronize()
    od, oi = od.cpu().numpy(), oi.cpu().numpy()
    assert (od[nq] == -7).all() and (oi[nq] == -7).all()
    return od[:nq], oi[:nq]


def check_plan(Q, X, kn, path, P=None, overflow=None):
    """The path and partitions of the call, and for the two-scan path
    whether its candidate lists outgrow their cap."""
    nq, nx = len(Q), len(X)
    got, pl, parts = plan(nq, nx, kn)
    assert got == path
    assert (parts - 1) * pl < nx <= parts * pl
    if P is not None:
        assert parts == P
    if path == 2:
        cand = ref.two_scan_candidates(ref.seq_sq_distances(Q, X), pl, parts,
                                       kn)
        assert (cand >= kn).all()
        assert bool(cand.max() > ref.KB_CAP) == overflow
        return cand
    assert overflow is None
    return None


def check_knn(Q, X, kn, path, P=None, overflow=None):
    check_plan(Q, X, kn, path, P, overflow)
    rd, ri = ref.knn_exact(Q, X, kn)
    for pad in (True, False):
        gd, gi = run_knn(Q, X, kn, pad)
        assert np.array_equal(gi, ri), pad
        assert np.array_equal(gd, rd), pad
    return rd, ri


TPL_D = [1, 7, 8, 9, 16, 17, 32, 33, 64, 65]
TPL_KN = [1, 2, 3, 5, 9, 17, 32]
TPL_NQ = [1, 63, 64, 65, 257]
TPL_NX = [None, 255, 256, 257, 513, 1030]     # None: nx = kn
# partitions of the passes for nq <= 257: 256 rows or more each
TPL_P = {None: 1, 255: 1, 256: 1, 257: 1, 513: 2, 1030: 4}


def _template_cases():
    out = []
    for i, d in enumerate(TPL_D):
        for s in (0, 2, 4):
            c = len(out)
            out.append((d, TPL_KN[(i + s) % 7], TPL_NQ[c % 5],
                        TPL_NX[c % 6]))
    return out


TPL_CASES = _template_cases()


def test_template_cases_cover_the_edges():
    """Every d meets three kn, every kn four d or more, every K template
    (1, 2, 4, 8, 16, 32) a kn strictly inside it where there is one, every
    nq and nx edge is used, with one, two and four partitions."""
    for d in TPL_D:
        assert len({c[1] for c in TPL_CASES if c[0] == d}) == 3
    for kn in TPL_KN:
        assert len({c[0] for c in TPL_CASES if c[1] == kn}) >= 4
    assert {3, 5, 9, 17} <= set(TPL_KN)      # inside K = 4, 8, 16, 32
    assert {c[2] for c in TPL_CASES} == set(TPL_NQ)
    assert {c[3] for c in TPL_CASES} == set(TPL_NX)
    for nx in TPL_NX:      # each nx under a small and a large K template
        kns = {c[1] for c in TPL_CASES if c[3] == nx}
        assert min(kns) <= 3 and max(kns) >= 17


@pytest.mark.parametrize("d,kn,nq,nx", TPL_CASES)
def test_knn_template_edges(d, kn, nq, nx):
    P = TPL_P[nx]
    nx = kn if nx is None else nx
    Q, X = ref.normal(1000 + d, nq, d), ref.normal(2000 + d + kn, nx, d)
    check_knn(Q, X, kn, 1, P)


@pytest.mark.parametrize("kn,extra,nq,d", [
    (2049, 0, 3, 2), (2049, 7, 65, 20),      # a last pass of K = 1
    (2050, 0, 65, 20), (2050, 7, 3, 2),      # K = 2
    (2080, 0, 3, 20), (2080, 7, 65, 2),      # K = 32: 65 full passes
    (2081, 0, 65, 2), (2081, 7, 3, 20),      # 66 passes, K = 1
    (2081, 7, 3, 70),                        # the query read from memory
])
def test_knn_passes_with_a_floor(kn, extra, nq, d):
    """kn > 2048: passes of 32, each starting strictly after the (r, index)
    where the one before ended; the last pass's lists are narrower than the
    first's in the same workspace."""
    nx = kn + extra
    Q, X = ref.normal(kn + d, nq, d), ref.normal(kn + d + 1, nx, d)
    check_knn(Q, X, kn, 1, 8)
    assert (kn - 1) % 32 + 1 == {2049: 1, 2050: 2, 2080: 32, 2081: 1}[kn]


def test_knn_floor_inside_a_tie_group():
    """16 distinct points among 2088 rows: every distance is shared by about
    130 rows, so each pass ends inside a tie group and the next starts at
    the floor's own r with the larger indices."""
    kn, nx = 2081, 2088
    Q, X = ref.grid(5, 65, 2), ref.grid(6, nx, 2)
    rd, ri = check_knn(Q, X, kn, 1, 8)
    at_floor = rd[:, 31::32] == rd[:, 32::32][:, :rd[:, 31::32].shape[1]]
    assert at_floor.mean() > 0.8


@pytest.mark.parametrize("kn", [2048, 2000])
@pytest.mark.parametrize("d", [2, 20])
def test_knn_two_scan_overflow_falls_back(d, kn):
    """nx = 8500 rows in distance order for queries 0 and 2 (tests/
    neighbors_ref.sorted_line): with kn = 2048 the 65 partitions of 131
    rows give a threshold near row 63 * 131 + 31 and 8285 candidates, over
    the cap of 4096; query 1 stays below it.  The call reruns in passes of
    32 over the passes' 33 partitions."""
    nx = 8500
    Q, X = ref.sorted_line(nx, d)
    assert plan(3, nx, kn) == {2048: (2, 131, 65), 2000: (2, 135, 63)}[kn]
    assert plan(3, nx, 1) == (1, 258, 33)
    cand = check_plan(Q, X, kn, 2, overflow=True)
    assert cand[0] > ref.KB_CAP and cand[2] > ref.KB_CAP
    assert cand[1] <= ref.KB_CAP
    if kn == 2048:
        assert cand[0] == 63 * 131 + 32
    rd, ri = ref.knn_exact(Q, X, kn)
    assert np.array_equal(ri[0], np.arange(kn))
    assert np.array_equal(ri[2], nx - 1 - np.arange(kn))
    for pad in (True, False):
        gd, gi = run_knn(Q, X, kn, pad)
        assert np.array_equal(gi, ri) and np.array_equal(gd, rd)


TWO_SCAN = [(kn, nx, [3, 20, 70][c % 3]) for c, (kn, nx) in enumerate(
    (kn, nx) for kn in (33, 64, 100, 1000)
    for nx in (kn, kn + 1, 4 * kn))] + [(2047, 2047, 3), (2048, 2048, 20)]


@pytest.mark.parametrize("kn,nx,d", TWO_SCAN)
def test_knn_two_scan(kn, nx, d):
    """32 < kn <= 2048 without overflow; kn = nx = 2047 and 2048 cut the
    fit rows into 64 partitions of exactly 32 rows."""
    Q, X = ref.normal(kn + nx, 65, d), ref.normal(kn + nx + 1, nx, d)
    check_knn(Q, X, kn, 2, overflow=False)
    if kn >= 2047:
        assert plan(65, nx, kn) == (2, 32, 64)


def test_knn_two_scan_ties():
    """Duplicate rows on the two-scan path: the threshold pair falls inside
    a tie group and only the indices up to its own may be collected."""
    Q, X = ref.grid(11, 65, 2), ref.grid(12, 700, 2)
    check_knn(Q, X, 100, 2, overflow=False)


@pytest.mark.parametrize("nq", [8193, 8257])
def test_knn_two_scan_second_chunk(nq):
    """Queries beyond the 8192 of one chunk reuse its workspace: Q, and both
    outputs, advance by the chunk."""
    kn, nx, d = 33, 70, 9
    Q, X = ref.normal(nq, nq, d), ref.normal(nq + 1, nx, d)
    assert plan(nq, nx, kn) == (2, 35, 2)
    rd, ri = check_knn(Q, X, kn, 2, overflow=False)
    for pad in (True, False):
        gd, gi = run_knn(Q, X, kn, pad)
        td, ti = run_knn(Q[8192:], X, kn, pad)
        assert np.array_equal(gi[8192:], ri[8192:])
        assert gd[8192:].tobytes() == td.tobytes() == rd[8192:].tobytes()
        assert gi[8192:].tobytes() == ti.tobytes()


@pytest.mark.parametrize("kn", [1, 32, 33])
def test_knn_all_rows_equal(kn):
    """Every distance of a query equal: the first kn fit rows, in order."""
    Q = ref.normal(3, 65, 5)
    X = np.tile(ref.normal(4, 1, 5), (100, 1))
    rd, ri = check_knn(Q, X, kn, 1 if kn <= 32 else 2,
                       overflow=None if kn <= 32 else False)
    assert np.array_equal(ri, np.tile(np.arange(kn), (65, 1)))


@pytest.mark.parametrize("kn", [8, 32, 40])
def test_knn_rows_at_1e200(kn):
    """Squares that overflow to +inf: those rows fill the lists as real
    indices in index order, never a sentinel."""
    rng = np.random.default_rng(11)
    X = rng.standard_normal((40, 3))
    X[3:] = 1e200 * (1.0 + rng.random((37, 3)))
    Q = rng.standard_normal((5, 3))
    rd, ri = check_knn(Q, X, kn, 1 if kn <= 32 else 2,
                       overflow=None if kn <= 32 else False)
    assert np.isinf(rd[:, 3:]).all() and np.isfinite(rd[:, :3]).all()
    assert np.array_equal(ri[:, 3:], np.tile(np.arange(3, kn), (5, 1)))


# --------------------------------------------------------------------------
# kNN, CSR
# --------------------------------------------------------------------------
def _as_f32(csr):
    return csr[0], csr[1], csr[2].astype(np.float32).astype(np.float64)


def run_knn_csr(q, f, d, kn, f32):
    so = _so()
    nq, nx = len(q[0]) - 1, len(f[0]) - 1
    dq = [_dev(q[0]), _dev(np.append(q[1], 0).astype(np.int32)),
          _dev(np.append(q[2], NAN))]
    df = [_dev(f[0]), _dev(np.append(f[1], 0).astype(np.int32)),
          _dev(np.append(f[2], NAN))]
    wsb = int(so.dkm_knn_workspace_bytes(nq, nx, kn))
    assert wsb > 0
    ws = _ws(wsb)
    od = _full((nq + 1, kn), -7.0, torch.float64)
    oi = _full((nq + 1, kn), -7, torch.int64)
    rc = so.dkm_knn_csr_f64(_ptr(dq[0]), _ptr(dq[1]), _ptr(dq[2]), nq,
                            _ptr(df[0]), _ptr(df[1]), _ptr(df[2]), nx, d, kn,
                            int(f32), _ptr(ws), wsb, _ptr(od), _ptr(oi),
                            _stream())
    assert rc == 0, so.dkm_last_error()
    torch.cuda.synchronize()
    od, oi = od.cpu().numpy(), oi.cpu().numpy()
    assert (od[nq] == -7).all() and (oi[nq] == -7).all()
    return od[:nq], oi[:nq]


def csr_keys(q, f, f32):
    """The squared CSR distances of every pair, by the oracle."""
    from oracle import neighbors_oracle as orc
    out = np.empty((len(q[0]) - 1, len(f[0]) - 1))
    with np.errstate(all="ignore"):
        for i in range(len(out)):
            a, b = q[0][i], q[0][i + 1]
            out[i] = orc.csr_sq_distances_to(q[1][a:b], q[2][a:b], *f)
    return out.astype(np.float32).astype(np.float64) if f32 else out


def check_knn_csr(q, f, d, kn, path, overflow=None, both=(False, True)):
    nq, nx = len(q[0]) - 1, len(f[0]) - 1
    got, pl, P = plan(nq, nx, kn)
    assert got == path
    out = {}
    for f32 in both:
        qq, ff = (_as_f32(q), _as_f32(f)) if f32 else (q, f)
        if path == 2:
            cand = ref.two_scan_candidates(csr_keys(qq, ff, f32), pl, P, kn)
            assert bool(cand.max() > ref.KB_CAP) == overflow
        rd, ri = ref.knn_csr_exact(qq, ff, kn, f32)
        gd, gi = run_knn_csr(qq, ff, d, kn, f32)
        assert np.array_equal(gi, ri), f32
        assert np.array_equal(gd, rd, equal_nan=True), f32
        out[f32] = rd, ri
    return out


@pytest.mark.parametrize("kn", TPL_KN)
@pytest.mark.parametrize("kind", ["uniform", "grid"])
def test_knn_csr_k_templates(kn, kind):
    """Every top-K template at (65, 300): empty query rows and empty fit
    rows (a fifth of each), ties on integer values."""
    d = 30
    f = ref.random_csr(kn, 300, d, 6, kind, empty=0.2)
    q = ref.random_csr(kn + 50, 65, d, 6, kind, empty=0.2)
    assert (np.diff(f[0]) == 0).sum() > 30 and (np.diff(q[0]) == 0).sum() > 5
    check_knn_csr(q, f, d, kn, 1)


@pytest.mark.parametrize("kn,kind", [(2049, "uniform"), (2081, "grid")])
def test_knn_csr_passes_with_a_floor(kn, kind):
    d = 12
    f = ref.random_csr(kn, kn + 7, d, 4, kind, empty=0.1)
    q = ref.random_csr(kn + 1, 65, d, 4, kind, empty=0.1)
    out = check_knn_csr(q, f, d, kn, 1)
    if kind == "grid":       # the floors fall inside tie groups
        rd = out[False][0]
        assert (rd[:, 31:-1:32] == rd[:, 32::32]).mean() > 0.5


@pytest.mark.parametrize("kn,nx,kind", [(100, 400, "uniform"),
                                        (33, 33, "grid"), (64, 65, "grid")])
def test_knn_csr_two_scan(kn, nx, kind):
    d = 12
    f = ref.random_csr(kn, nx, d, 4, kind, empty=0.1)
    q = ref.random_csr(kn + 1, 65, d, 4, kind, empty=0.1)
    check_knn_csr(q, f, d, kn, 2, overflow=False)


@pytest.mark.parametrize("nq", [8193, 8257])
def test_knn_csr_two_scan_second_chunk(nq):
    """Queries beyond the 8192 of one chunk: the query row pointers advance
    by the chunk in both scans.  The later rows are 8 times as large, so
    their nearest fit row is farther than query 0's 33rd: a first scan that
    read the first chunk's rows again would leave them without candidates."""
    d, kn, nx = 9, 33, 70
    f = ref.random_csr(1, nx, d, 3)
    q = ref.random_csr(2, nq, d, 3, empty=0.05)
    q[2][q[0][8192]:] *= 8.0
    assert q[0][8193] > q[0][8192]
    head = np.sort(csr_keys((q[0][:2], q[1], q[2]), f, False)[0])
    tail = csr_keys((q[0][8192:8194], q[1], q[2]), f, False)[0]
    assert tail.min() > head[kn - 1]
    assert plan(nq, nx, kn) == (2, 35, 2)
    rd, ri = check_knn_csr(q, f, d, kn, 2, overflow=False,
                           both=(False,))[False]
    gd, gi = run_knn_csr(q, f, d, kn, False)
    td, ti = run_knn_csr((q[0][8192:], q[1], q[2]), f, d, kn, False)
    assert gd[8192:].tobytes() == td.tobytes() == rd[8192:].tobytes()
    assert gi[8192:].tobytes() == ti.tobytes() == ri[8192:].tobytes()


def test_knn_csr_query_equal_to_a_fit_row():
    """The fit matrix queried with itself: q.q and |q|^2 are the same sum,
    so each row finds itself (or an identical row before it) at exactly 0."""
    d = 30
    f = ref.random_csr(9, 200, d, 6, "uniform", empty=0.1)
    out = check_knn_csr(f, f, d, 5, 1)
    for f32 in (False, True):
        rd, ri = out[f32]
        assert (rd[:, 0] == 0.0).all()
        full = np.diff(f[0]) > 0
        assert np.array_equal(ri[full, 0], np.flatnonzero(full))


# --------------------------------------------------------------------------
# epsilon query, dense
# --------------------------------------------------------------------------
def run_radius(Q, X, eps, pad, ws_bytes=None):
    """count, exclusive scan, fill (with exactly the workspace asked for);
    returns counts, indices, distances."""
    so = _so()
    (nq, d), nx = Q.shape, X.shape[0]
    ldq, ldx = (d + 3, d + 5) if pad else (d, d)
    Qd, Xd = _padded(Q, ldq), _padded(X, ldx)
    cnt = _full((nq + 1,), -7, torch.int64)
    rc = so.dkm_radius_count_f64(_ptr(Qd), nq, ldq, _ptr(Xd), nx, ldx, d,
                                 float(eps), _ptr(cnt), _stream())
    assert rc == 0, so.dkm_last_error()
    torch.cuda.synchronize()
    assert int(cnt[nq]) == -7
    counts = cnt[:nq].cpu().numpy()
    assert (counts >= 0).all() and (counts <= nx).all()
    off = np.zeros(nq + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    total = int(off[nq])
    wsb = int(so.dkm_radius_workspace_bytes(nq, total))
    assert wsb == nq * 8 + total * 16 + 256
    ws = _ws(wsb)
    oi = _full((total + 1,), -7, torch.int64)
    od = _full((total + 1,), -7.0, torch.float64)
    offd = _dev(off)
    rc = so.dkm_radius_fill_f64(_ptr(Qd), nq, ldq, _ptr(Xd), nx, ldx, d,
                                float(eps), _ptr(offd), _ptr(ws), wsb,
                                _ptr(oi), _ptr(od), _stream())
    assert rc == 0, so.dkm_last_error()
    torch.cuda.synchronize()
    oi, od = oi.cpu().numpy(), od.cpu().numpy()
    assert oi[total] == -7 and od[total] == -7
    return counts, oi[:total], od[:total]


def check_radius(Q, X, eps):
    lists = ref.radius_exact(Q, X, eps)
    rc = np.array([len(i) for i, _ in lists], np.int64)
    ri = np.concatenate([i for i, _ in lists] + [np.zeros(0, np.int64)])
    rd = np.concatenate([v for _, v in lists] + [np.zeros(0)])
    for pad in (True, False):
        counts, gi, gd = run_radius(Q, X, eps, pad)
        assert np.array_equal(counts, rc), pad       # before the lists
        assert np.array_equal(gi, ri), pad
        assert np.array_equal(gd, rd), pad
    return lists


@pytest.mark.parametrize("d,nq,nx", ref.EPS_CASES)
def test_radius_template_edges(d, nq, nx):
    """Every register template of d and both sides of each change in
    numpy's pairwise order (8, every multiple of 8, 128), on data whose
    sums show the order (tests/test_neighbors_ref_host.py)."""
    Q, X, eps = ref.eps_case(d, nq, nx)
    lists = check_radius(Q, X, eps)
    if nx >= 255:
        assert 0.2 * nq * nx < sum(len(i) for i, _ in lists) < 0.5 * nq * nx


@pytest.mark.parametrize("d", [1, 20])
def test_radius_band(d):
    """eps at a fit row's distance D and at the doubles next to it: r is
    within 2^-48 of eps^2 each time, where the kernel takes sqrt(r) < eps
    like the reference.  At eps = D the d = 20 row has r < fl(D^2)."""
    b = ref.band_case(d)
    for eps, inside in zip(b.eps, b.inside):
        lists = check_radius(b.Q, b.X, eps)
        assert (b.at in lists[0][0].tolist()) == inside


@pytest.mark.parametrize("eps,size", [(0.0, 0), (-1.0, 0), (np.inf, 300),
                                      (1e-300, None)])
def test_radius_eps_edges(eps, size):
    """eps = 0 and eps < 0 take nothing, eps = inf every row; 1e-300 (its
    square underflows to 0) only the rows at distance 0."""
    X = ref.grid(3, 300, 3)
    Q = np.vstack([X[:40], ref.normal(4, 25, 3)])
    lists = check_radius(Q, X, eps)
    sizes = [len(i) for i, _ in lists]
    if size is not None:
        assert sizes == [size] * 65
    else:
        assert min(sizes[:40]) >= 1 and sizes[40:] == [0] * 25
        assert all((v == 0).all() for _, v in lists)


@pytest.mark.parametrize("m", [0, 1, 2, 3, 4095, 4096, 4097, 8192, 8193,
                               12289, 20481])
def test_radius_seg_sort_runs(m):
    """A list of m entries, mostly ties, next to a list of 5: nothing to
    sort, the LDS sort up to 4096, then 2, 3 (a run without a partner) and
    5 runs (6 with a last run of one entry), merged through a workspace of
    exactly dkm_radius_workspace_bytes."""
    Q, X, eps = ref.seg_sort_case(m)
    lists = check_radius(Q, X, eps)
    assert [len(i) for i, _ in lists] == [m, 5]


# --------------------------------------------------------------------------
# epsilon query, CSR
# --------------------------------------------------------------------------
def run_radius_csr(csr, d, q0, nq, eps, f32):
    so = _so()
    n = len(csr[0]) - 1
    ip, ix, dv = (_dev(csr[0]), _dev(np.append(csr[1], 0).astype(np.int32)),
                  _dev(np.append(csr[2], NAN)))
    cnt = _full((nq + 1,), -7, torch.int64)
    rc = so.dkm_radius_count_csr_f64(_ptr(ip), _ptr(ix), _ptr(dv), n, d, q0,
                                     nq, float(eps), int(f32), _ptr(cnt),
                                     _stream())
    assert rc == 0, so.dkm_last_error()
    torch.cuda.synchronize()
    assert int(cnt[nq]) == -7
    counts = cnt[:nq].cpu().numpy()
    assert (counts >= 0).all() and (counts <= n).all()
    off = np.zeros(nq + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    total = int(off[nq])
    wsb = int(so.dkm_radius_workspace_bytes(nq, total))
    ws = _ws(wsb)
    oi = _full((total + 1,), -7, torch.int64)
    od = _full((total + 1,), -7.0, torch.float64)
    offd = _dev(off)
    rc = so.dkm_radius_fill_csr_f64(_ptr(ip), _ptr(ix), _ptr(dv), n, d, q0,
                                    nq, float(eps), int(f32), _ptr(offd),
                                    _ptr(ws), wsb, _ptr(oi), _ptr(od),
                                    _stream())
    assert rc == 0, so.dkm_last_error()
    torch.cuda.synchronize()
    oi, od = oi.cpu().numpy(), od.cpu().numpy()
    assert oi[total] == -7 and od[total] == -7
    return counts, oi[:total], od[:total]


def check_radius_csr(csr, d, q0, nq, eps):
    out = {}
    for f32 in (False, True):
        c = _as_f32(csr) if f32 else csr
        lists = ref.radius_csr_exact(c, q0, nq, eps, f32)
        counts, gi, gd = run_radius_csr(c, d, q0, nq, eps, f32)
        assert np.array_equal(counts, [len(i) for i, _ in lists]), f32
        assert np.array_equal(gi, np.concatenate(
            [i for i, _ in lists] + [np.zeros(0, np.int64)])), f32
        assert np.array_equal(gd, np.concatenate(
            [v for _, v in lists] + [np.zeros(0)])), f32
        out[f32] = lists
    return out


@pytest.mark.parametrize("nq", [1, 64, 65])
@pytest.mark.parametrize("q0", [0, 1, 63, None])        # None: n - nq
@pytest.mark.parametrize("kind", ["uniform", "grid"])
def test_radius_csr_query_ranges(kind, q0, nq):
    """Query rows q0 .. q0 + nq of 130, a fifth of the rows empty."""
    n, d = 130, 30
    csr = ref.random_csr(7, n, d, 6, kind, empty=0.2)
    q0 = n - nq if q0 is None else q0
    out = check_radius_csr(csr, d, q0, nq, 1.1 if kind == "uniform" else 2.5)
    total = sum(len(i) for i, _ in out[False])
    assert nq <= total < nq * n          # itself at least, never every row


def test_radius_csr_list_of_4097():
    """4097 rows within eps of each other (integer values: ties) and three
    rows 1e6 away: two lists of 4097 (two sorted runs, the second of one
    entry), then the three short ones."""
    d = 8
    ip, ix, dv = ref.random_csr(3, 4097, d, 4, "grid", empty=0.1)
    ip = np.concatenate([ip, ip[-1] + np.arange(1, 4)])
    ix = np.concatenate([ix, np.zeros(3, np.int32)]).astype(np.int32)
    dv = np.concatenate([dv, [1e6, 1e6, 1e6]])
    out = check_radius_csr((ip, ix, dv), d, 0, 2, 100.0)
    assert [len(i) for i, _ in out[False]] == [4097, 4097]
    out = check_radius_csr((ip, ix, dv), d, 4097, 3, 100.0)
    assert [len(i) for i, _ in out[True]] == [3, 3, 3]


# --------------------------------------------------------------------------
# refusals and early returns: the exact code, the sentinels untouched
# --------------------------------------------------------------------------
class _Knn:
    """A valid dkm_knn_f64 call (nq = 5, nx = 40, d = 3, kn = 4) to spoil
    one argument at a time."""

    def __init__(self):
        self.Q, self.X = _dev(ref.normal(1, 5, 3)), _dev(ref.normal(2, 40, 3))
        self.wsb = int(_so().dkm_knn_workspace_bytes(5, 40, 4))
        self.ws = _ws(self.wsb)
        self.od = _full((5, 4), -7.0, torch.float64)
        self.oi = _full((5, 4), -7, torch.int64)

    def call(self, **kw):
        a = dict(Q=_ptr(self.Q), nq=5, ldq=3, X=_ptr(self.X), nx=40, ldx=3,
                 d=3, kn=4, ws=_ptr(self.ws), wsb=self.wsb, od=_ptr(self.od),
                 oi=_ptr(self.oi))
        a.update(kw)
        rc = _so().dkm_knn_f64(a["Q"], a["nq"], a["ldq"], a["X"], a["nx"],
                               a["ldx"], a["d"], a["kn"], a["ws"], a["wsb"],
                               a["od"], a["oi"], _stream())
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return bool((self.od == -7).all()) and bool((self.oi == -7).all())


def test_knn_refusals():
    k = _Knn()
    big = 2 ** 31
    for kw in (dict(nq=-1), dict(nx=0), dict(d=0), dict(ldq=2), dict(ldx=2),
               dict(kn=0), dict(kn=41), dict(nx=big), dict(d=big, ldq=big,
                                                           ldx=big),
               dict(Q=None), dict(X=None), dict(od=None), dict(oi=None)):
        assert k.call(**kw) == E_ARG, kw
        assert k.untouched(), kw
    assert k.call(wsb=k.wsb - 1) == E_WS and k.untouched()
    assert k.call(ws=None) == E_WS and k.untouched()
    assert b"workspace" in _so().dkm_last_error()
    # no queries: nothing is read, not even NULL pointers
    assert k.call(nq=0, Q=None, X=None, ws=None, wsb=0, od=None,
                  oi=None) == 0
    assert k.untouched()
    assert k.call() == 0 and not k.untouched()
    so = _so()
    for nq, nx, kn in [(-1, 40, 4), (5, 0, 1), (5, 40, 0), (5, 40, 41)]:
        assert so.dkm_knn_workspace_bytes(nq, nx, kn) == 0
    assert so.dkm_knn_workspace_bytes(0, 40, 4) > 0


def test_knn_csr_refusals():
    so = _so()
    f = ref.random_csr(1, 40, 6, 3)
    q = ref.random_csr(2, 5, 6, 3)
    dev = [_dev(q[0]), _dev(q[1]), _dev(q[2]), _dev(f[0]), _dev(f[1]),
           _dev(f[2])]
    wsb = int(so.dkm_knn_workspace_bytes(5, 40, 4))
    ws = _ws(wsb)
    od = _full((5, 4), -7.0, torch.float64)
    oi = _full((5, 4), -7, torch.int64)

    def call(null=(), **kw):
        a = dict(nq=5, nx=40, d=6, kn=4, ws=_ptr(ws), wsb=wsb, od=_ptr(od),
                 oi=_ptr(oi))
        a.update(kw)
        p = [None if i in null else _ptr(t) for i, t in enumerate(dev)]
        rc = so.dkm_knn_csr_f64(p[0], p[1], p[2], a["nq"], p[3], p[4], p[5],
                                a["nx"], a["d"], a["kn"], 0, a["ws"],
                                a["wsb"], a["od"], a["oi"], _stream())
        torch.cuda.synchronize()
        return rc

    def untouched():
        return bool((od == -7).all()) and bool((oi == -7).all())

    for kw in (dict(nq=-1), dict(nx=0), dict(d=0), dict(d=2 ** 31),
               dict(nx=2 ** 31), dict(kn=0), dict(kn=41), dict(od=None),
               dict(oi=None)):
        assert call(**kw) == E_ARG and untouched(), kw
    for i in range(6):
        assert call(null=(i,)) == E_ARG and untouched(), i
    assert call(wsb=wsb - 1) == E_WS and untouched()
    assert call(ws=None) == E_WS and untouched()
    assert call(null=range(6), nq=0, ws=None, wsb=0, od=None, oi=None) == 0
    assert untouched()
    assert call() == 0 and not untouched()


def test_radius_refusals_and_early_returns():
    so = _so()
    Q, X = _dev(ref.normal(1, 5, 3)), _dev(ref.normal(2, 40, 3))
    cnt = _full((5,), -7, torch.int64)
    off = _dev(np.arange(6, dtype=np.int64))        # five lists of one
    wsb = int(so.dkm_radius_workspace_bytes(5, 5))
    ws = _ws(wsb)
    oi = _full((5,), -7, torch.int64)
    od = _full((5,), -7.0, torch.float64)

    def count(**kw):
        a = dict(Q=_ptr(Q), nq=5, ldq=3, X=_ptr(X), nx=40, ldx=3, d=3,
                 eps=1.0, cnt=_ptr(cnt))
        a.update(kw)
        rc = so.dkm_radius_count_f64(a["Q"], a["nq"], a["ldq"], a["X"],
                                     a["nx"], a["ldx"], a["d"], a["eps"],
                                     a["cnt"], _stream())
        torch.cuda.synchronize()
        return rc

    def fill(**kw):
        a = dict(Q=_ptr(Q), nq=5, ldq=3, X=_ptr(X), nx=40, ldx=3, d=3,
                 eps=1.0, off=_ptr(off), ws=_ptr(ws), wsb=wsb, oi=_ptr(oi),
                 od=_ptr(od))
        a.update(kw)
        rc = so.dkm_radius_fill_f64(a["Q"], a["nq"], a["ldq"], a["X"],
                                    a["nx"], a["ldx"], a["d"], a["eps"],
                                    a["off"], a["ws"], a["wsb"], a["oi"],
                                    a["od"], _stream())
        torch.cuda.synchronize()
        return rc

    def untouched():
        return bool((cnt == -7).all()) and bool((oi == -7).all()) and \
            bool((od == -7).all())

    big = 2 ** 31
    for kw in (dict(nq=-1), dict(nx=-1), dict(d=0), dict(ldq=2), dict(ldx=2),
               dict(d=big, ldq=big, ldx=big), dict(eps=NAN), dict(Q=None),
               dict(X=None)):
        assert count(**kw) == E_ARG and fill(**kw) == E_ARG, kw
        assert untouched(), kw
    assert count(cnt=None) == E_ARG
    for kw in (dict(off=None), dict(oi=None), dict(od=None)):
        assert fill(**kw) == E_ARG and untouched(), kw
    assert fill(wsb=wsb - 1) == E_WS and fill(ws=None) == E_WS
    neg = _dev(np.array([0, 0, 0, 0, 0, -1], np.int64))
    assert fill(off=_ptr(neg)) == E_ARG and untouched()
    assert so.dkm_radius_workspace_bytes(-1, 0) == 0
    assert so.dkm_radius_workspace_bytes(0, -1) == 0
    # no queries: nothing is read
    assert count(nq=0, Q=None, X=None, cnt=None) == 0
    assert fill(nq=0, Q=None, X=None, off=None, ws=None, wsb=0, oi=None,
                od=None) == 0
    assert untouched()
    # no fit rows: zero counts, and a fill that touches nothing
    assert fill(nx=0, X=None, off=None, ws=None, wsb=0, oi=None,
                od=None) == 0 and untouched()
    assert count(nx=0, X=None) == 0 and bool((cnt == 0).all())
    # total == 0: the fill runs (nothing is within eps) and writes nothing
    zero = _dev(np.zeros(6, np.int64))
    w0 = int(so.dkm_radius_workspace_bytes(5, 0))
    assert fill(eps=0.0, off=_ptr(zero), wsb=w0) == 0
    assert fill(eps=0.0, off=_ptr(zero), wsb=w0 - 1) == E_WS
    assert bool((oi == -7).all()) and bool((od == -7).all())


def test_radius_csr_refusals_and_early_returns():
    so = _so()
    csr = ref.random_csr(1, 40, 6, 3)
    dev = [_dev(csr[0]), _dev(csr[1]), _dev(csr[2])]
    cnt = _full((5,), -7, torch.int64)
    off = _dev(np.arange(6, dtype=np.int64))
    wsb = int(so.dkm_radius_workspace_bytes(5, 5))
    ws = _ws(wsb)
    oi = _full((5,), -7, torch.int64)
    od = _full((5,), -7.0, torch.float64)

    def both(null=(), only=None, **kw):
        a = dict(n=40, d=6, q0=2, nq=5, eps=1.0, cnt=_ptr(cnt),
                 off=_ptr(off), ws=_ptr(ws), wsb=wsb, oi=_ptr(oi),
                 od=_ptr(od))
        a.update(kw)
        p = [None if i in null else _ptr(t) for i, t in enumerate(dev)]
        out = []
        if only in (None, "count"):
            out.append(so.dkm_radius_count_csr_f64(
                p[0], p[1], p[2], a["n"], a["d"], a["q0"], a["nq"], a["eps"],
                0, a["cnt"], _stream()))
        if only in (None, "fill"):
            out.append(so.dkm_radius_fill_csr_f64(
                p[0], p[1], p[2], a["n"], a["d"], a["q0"], a["nq"], a["eps"],
                0, a["off"], a["ws"], a["wsb"], a["oi"], a["od"], _stream()))
        torch.cuda.synchronize()
        return out

    def untouched():
        return bool((cnt == -7).all()) and bool((oi == -7).all()) and \
            bool((od == -7).all())

    for kw in (dict(n=-1), dict(d=0), dict(d=2 ** 31), dict(nq=-1),
               dict(q0=-1), dict(q0=36), dict(nq=41, q0=0), dict(eps=NAN),
               dict(null=(0,)), dict(null=(1,)), dict(null=(2,))):
        assert both(**kw) == [E_ARG, E_ARG] and untouched(), kw
    assert both(only="count", cnt=None) == [E_ARG]
    for kw in (dict(off=None), dict(oi=None), dict(od=None)):
        assert both(only="fill", **kw) == [E_ARG] and untouched(), kw
    assert both(only="fill", wsb=wsb - 1) == [E_WS]
    assert both(only="fill", ws=None) == [E_WS] and untouched()
    # no queries: indices and data may be NULL
    assert both(null=(1, 2), nq=0, cnt=None, off=None, ws=None, wsb=0,
                oi=None, od=None) == [0, 0]
    assert both(null=(0, 1, 2), n=0, q0=0, nq=0) == [0, 0] and untouched()
    # total == 0: nothing to fill, no workspace needed
    zero = _dev(np.zeros(6, np.int64))
    assert both(only="fill", eps=0.0, off=_ptr(zero), ws=None,
                wsb=0) == [0] and untouched()
    assert both(only="count", eps=0.0) == [0] and bool((cnt == 0).all())
