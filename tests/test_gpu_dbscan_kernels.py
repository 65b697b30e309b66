"""GPU tests of the three DBSCAN entries of the C ABI (dkm_dbscan.hip) called
directly: any row order and ``orig_index`` permutation, padded rows, the tie
rule, the intermediate ``core`` / ``parent`` / ``attach`` arrays, and the
argument checks.  Everything is integer equality against
tests/dbscan_ref.py.
"""
import ctypes
import types

import numpy as np
import pytest

from tests import dbscan_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _i32(n, fill=None):
    if fill is None:
        return torch.empty(n, dtype=torch.int32, device="cuda")
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


def run_entries(rows, orig, eps, ms, flags=0, ldx=None):
    """core / link / finalize on the host rows ``rows`` in this order, row i
    being Dataset row ``orig[i]``; rows are ``ldx`` doubles apart, the pad
    NaN.  Returns core, parent, attach, labels (numpy) and n_clusters."""
    from dislib_amd import _lib
    from dislib_amd._device import ptr, stream_ptr
    so = _lib.lib()
    n, d = rows.shape
    ldx = d if ldx is None else ldx
    X = torch.full((n, ldx), float("nan"), dtype=torch.float64, device="cuda")
    X[:, :d] = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    og = torch.from_numpy(np.asarray(orig).astype(np.int32)).cuda()
    wsb = int(so.dkm_dbscan_workspace_bytes(n, d))
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    wp = ctypes.c_void_p(ws.data_ptr())
    core, parent, attach, labels = _i32(n), _i32(n), _i32(n), _i32(n, -7)
    ncl = _i32(1, -7)
    _lib.check(so.dkm_dbscan_core_f64(
        ptr(X), n, d, ldx, eps, ms, flags, wp, wsb, ptr(core), stream_ptr()),
        "dkm_dbscan_core")
    _lib.check(so.dkm_dbscan_link_f64(
        ptr(X), n, d, ldx, eps, flags, wp, wsb, ptr(core), ptr(og),
        ptr(parent), ptr(attach), stream_ptr()), "dkm_dbscan_link")
    _lib.check(so.dkm_dbscan_finalize(
        n, ms, wp, wsb, ptr(core), ptr(og), ptr(parent), ptr(attach),
        ptr(labels), ptr(ncl), stream_ptr()), "dkm_dbscan_finalize")
    torch.cuda.synchronize()
    return types.SimpleNamespace(
        core=core.cpu().numpy(), parent=parent.cpu().numpy().astype(np.int64),
        attach=attach.cpu().numpy().astype(np.int64),
        labels=labels.cpu().numpy().astype(np.int64), n_clusters=int(ncl))


def check_against(out, p, orig):
    """Every array of ``run_entries`` against ``dbscan_parts`` of the
    Dataset-order samples."""
    orig = np.asarray(orig)
    n = len(orig)
    assert np.array_equal(out.labels, p.labels)
    assert out.n_clusters == p.n_clusters
    assert set(np.unique(out.core)) <= {0, 1}
    core = out.core.astype(bool)
    assert np.array_equal(core, p.core[orig])
    has = out.attach >= 0
    assert np.array_equal(has, p.attach[orig] >= 0)
    assert (out.attach < n).all() and (out.attach >= -1).all()
    assert np.array_equal(orig[out.attach[has]], p.attach[orig][has])
    idx = np.arange(n)
    assert (out.parent <= idx).all() and (out.parent >= 0).all()
    assert np.array_equal(out.parent[~core], idx[~core])
    root = out.parent.copy()
    for _ in range(n):                # parent[i] <= i: ends at the roots
        nxt = root[root]
        if np.array_equal(nxt, root):
            break
        root = nxt
    assert core[root[core]].all()
    # components of the core rows, named by their smallest Dataset row
    smallest = np.full(n, n)
    np.minimum.at(smallest, root[core], orig[core])
    assert np.array_equal(smallest[root[core]], p.comp[orig[core]])


def cell_order(x, eps):
    from dislib_amd.cluster import dbscan as mod
    perm = mod._cell_order(torch.from_numpy(x).cuda(), eps,
                           list(range(x.shape[1])))
    assert perm is not None
    return perm.cpu().numpy()


def _high_d():
    """600 x 24 that differs in features 16..23 only."""
    rng = np.random.default_rng(24)
    which = rng.integers(0, 3, 600)
    x = 0.25 * rng.standard_normal((600, 24))
    x[:, 16:] += rng.uniform(-4, 4, (3, 8))[which]
    x[540:, 16:] = rng.uniform(-5, 5, (60, 8))
    return np.ascontiguousarray(x[rng.permutation(600)])


DATA = {3: (lambda: ref.blobs_noise(21, n_blob=540, n_noise=60, d=3), 0.45),
        24: (_high_d, 1.4)}
_CACHE = {}


def _data(d):
    if d not in _CACHE:
        make, eps = DATA[d]
        x = make()
        _CACHE[d] = x, eps, ref.dbscan_parts(x, eps, 5)
    return _CACHE[d]


def _not_degenerate(p):
    assert p.n_clusters >= 2
    assert np.count_nonzero(p.labels == -1) >= 1
    assert np.count_nonzero(~p.core & (p.labels >= 0)) >= 1


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("order", ["cell", "identity", "random",
                                   "cell_reversed"])
@pytest.mark.parametrize("d", sorted(DATA))
def test_any_row_order(d, order, flags):
    from dislib_amd import _lib
    assert _lib.DBSCAN_NOPRUNE == 1
    x, eps, p = _data(d)
    assert x.shape == (600, d)
    _not_degenerate(p)
    if order == "identity":
        orig = np.arange(600)
    elif order == "random":
        orig = np.random.default_rng(5).permutation(600)
    else:
        orig = cell_order(x, eps)
        if order == "cell_reversed":
            orig = orig[::-1].copy()
    check_against(run_entries(x[orig], orig, eps, 5, flags), p, orig)


# c of eps = c * sqrt(d) for three blobs of std 0.25 and uniform noise
STRIDE_C = {3: 0.26, 9: 0.27, 24: 0.3, 70: 0.32, 130: 0.33}
_STRIDE = {}


def _stride_data(d):
    if d not in _STRIDE:
        x = ref.blobs_noise(100 + d, n_blob=260, n_noise=40, d=d, centers=3)
        eps = STRIDE_C[d] * np.sqrt(d)
        _STRIDE[d] = x, eps, ref.dbscan_parts(x, eps, 5)
    return _STRIDE[d]


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("d", sorted(STRIDE_C))
def test_row_stride(d, flags):
    """Rows d + 5 doubles apart with NaN between them, in the class's cell
    order: the padded run, the contiguous run and the reference agree."""
    x, eps, p = _stride_data(d)
    assert x.shape == (300, d)
    _not_degenerate(p)
    orig = cell_order(x, eps)
    wide = run_entries(x[orig], orig, eps, 5, flags, ldx=d + 5)
    check_against(wide, p, orig)
    tight = run_entries(x[orig], orig, eps, 5, flags)
    for name in ("core", "attach", "labels"):
        assert np.array_equal(getattr(wide, name), getattr(tight, name)), name
    assert wide.n_clusters == tight.n_clusters


@pytest.mark.parametrize("d", sorted(STRIDE_C))
def test_row_stride_of_the_boxes(d):
    """Three tight blobs on the diagonal (features within 0.05 of 0, 10 and
    20), the blob changing every 24 rows, so every tile holds all three and
    no tile pair may be pruned.  Every blob is a clique at this eps and
    min_samples is the size of the smallest, so a box taken with any other
    row stride (blocks of other rows: other blobs) costs a row neighbours
    and makes it noise."""
    n, ldx = 300, d + 5
    rng = np.random.default_rng(d)
    blob = (np.arange(n) // 24) % 3
    x = 10.0 * blob[:, None] + rng.uniform(-0.05, 0.05, (n, d))
    eps = 0.11 * np.sqrt(d)           # a blob's diameter is below 0.1 sqrt(d)
    ms = int(np.bincount(blob).min())
    assert ms == 96
    orig = np.arange(n)
    for flags in (0, 1):
        out = run_entries(x, orig, eps, ms, flags, ldx=ldx)
        assert np.array_equal(out.labels, blob) and out.n_clusters == 3
        assert out.core.all() and (out.attach == -1).all()


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("variant", ref.TIE_VARIANTS)
def test_tie_goes_to_the_smallest_dataset_row(variant, flags):
    t = ref.tie_case(variant)
    n = len(t.x)
    orig = t.order
    rows = t.x[orig]
    pos = {c: int(np.flatnonzero(orig == c)[0]) for c in t.cores}
    out = run_entries(rows, orig, t.eps, t.min_samples, flags)
    check_against(out, ref.dbscan_parts(t.x, t.eps, t.min_samples), orig)
    assert np.array_equal(out.labels, t.labels)
    bpos = int(np.flatnonzero(orig == t.b)[0])
    assert out.attach[bpos] == pos[t.cores[0]]
    assert out.labels[t.b] == out.labels[t.cores[0]]
    # The same rows in the same order; the two smallest tied cores exchange
    # their Dataset rows: b follows the row number, not the position.
    c0, c1 = t.cores[:2]
    swapped = orig.copy()
    swapped[pos[c0]], swapped[pos[c1]] = c1, c0
    x2 = np.empty_like(t.x)
    x2[swapped] = rows
    p2 = ref.dbscan_parts(x2, t.eps, t.min_samples)
    out2 = run_entries(rows, swapped, t.eps, t.min_samples, flags)
    check_against(out2, p2, swapped)
    assert out2.attach[bpos] == pos[c1]       # the row that now is c0
    assert np.array_equal(out2.core, out.core)
    # b's cluster: the one of the other arm now
    arm0, arm1 = out.labels[c0], out.labels[c1]
    assert arm0 != arm1
    assert out.labels[t.b] == arm0
    assert out2.labels[t.b] == out2.labels[c0]
    assert np.array_equal(rows[pos[c1]], x2[c0])
    others = np.setdiff1d(np.arange(n), [t.b, c0, c1])
    same_arm = out.labels[others] == arm1
    assert same_arm.sum() == 4
    assert (out2.labels[others][same_arm] == out2.labels[t.b]).all()


# ---------------------------------------------------------------------------
# Arguments: refused before anything is launched.

class _Args:
    """Good arguments of the three entries on n = 70 rows of 2 features."""

    def __init__(self):
        from dislib_amd import _lib
        self.so = _lib.lib()
        self.n, self.d = 70, 2
        x = ref.blobs_noise(4, n_blob=60, n_noise=10)
        self.X = torch.from_numpy(x).cuda()
        self.wsb = int(self.so.dkm_dbscan_workspace_bytes(self.n, self.d))
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")
        self.orig = torch.arange(self.n, dtype=torch.int32, device="cuda")
        self.core = _i32(self.n, -7)
        self.parent = _i32(self.n, -7)
        self.attach = _i32(self.n, -7)
        self.labels = _i32(self.n, -7)
        self.ncl = _i32(1, -7)

    def call(self, entry, **kw):
        from dislib_amd._device import ptr, stream_ptr
        a = dict(X=ptr(self.X), n=self.n, d=self.d, ldx=self.d, eps=0.3,
                 ms=5, ws=ctypes.c_void_p(self.ws.data_ptr()), wsb=self.wsb,
                 core=ptr(self.core), orig=ptr(self.orig),
                 parent=ptr(self.parent), attach=ptr(self.attach),
                 labels=ptr(self.labels), ncl=ptr(self.ncl))
        a.update(kw)
        if entry == "core":
            return self.so.dkm_dbscan_core_f64(
                a["X"], a["n"], a["d"], a["ldx"], a["eps"], a["ms"], 0,
                a["ws"], a["wsb"], a["core"], stream_ptr())
        if entry == "link":
            return self.so.dkm_dbscan_link_f64(
                a["X"], a["n"], a["d"], a["ldx"], a["eps"], 0, a["ws"],
                a["wsb"], a["core"], a["orig"], a["parent"], a["attach"],
                stream_ptr())
        return self.so.dkm_dbscan_finalize(
            a["n"], a["ms"], a["ws"], a["wsb"], a["core"], a["orig"],
            a["parent"], a["attach"], a["labels"], a["ncl"], stream_ptr())

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == -7).all()) for t in (
            self.core, self.parent, self.attach, self.labels, self.ncl))


BAD = [("core", dict(n=-1)), ("core", dict(d=0)), ("core", dict(ldx=1)),
       ("core", dict(eps=float("nan"))), ("core", dict(ms=-1)),
       ("core", dict(wsb=-1)), ("core", dict(X=None)),
       ("core", dict(ws=None)), ("core", dict(core=None)),
       ("link", dict(n=-1)), ("link", dict(d=0)), ("link", dict(ldx=1)),
       ("link", dict(eps=float("nan"))), ("link", dict(wsb=-1)),
       ("link", dict(X=None)), ("link", dict(ws=None)),
       ("link", dict(core=None)), ("link", dict(orig=None)),
       ("link", dict(parent=None)), ("link", dict(attach=None)),
       ("finalize", dict(n=-1)), ("finalize", dict(ms=-1)),
       ("finalize", dict(wsb=-1)), ("finalize", dict(ws=None)),
       ("finalize", dict(core=None)), ("finalize", dict(orig=None)),
       ("finalize", dict(parent=None)), ("finalize", dict(attach=None)),
       ("finalize", dict(labels=None)), ("finalize", dict(ncl=None))]


@pytest.fixture(scope="module")
def args():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _Args()


@pytest.mark.parametrize("entry,bad", BAD,
                         ids=["%s-%s" % (e, next(iter(b))) for e, b in BAD])
def test_bad_argument_is_refused(args, entry, bad):
    if "wsb" in bad:
        bad = dict(wsb=args.wsb - 1)          # one byte short
    rc = args.call(entry, **bad)
    assert rc != 0
    assert ("dbscan " + entry) in args.so.dkm_last_error().decode()
    assert args.untouched()


def test_good_arguments_are_accepted(args):
    """The arguments that every refusal above changes one of."""
    for entry in ("core", "link", "finalize"):
        assert args.call(entry) == 0, args.so.dkm_last_error()
    torch.cuda.synchronize()
    x = args.X.cpu().numpy()
    want, ncl = ref.dbscan_ref(x, 0.3, 5)
    assert np.array_equal(args.labels.cpu().numpy(), want)
    assert int(args.ncl) == ncl
    for t in (args.core, args.parent, args.attach, args.labels, args.ncl):
        t.fill_(-7)


def test_no_rows(args):
    from dislib_amd._device import ptr, stream_ptr
    so = args.so
    assert so.dkm_dbscan_core_f64(None, 0, 2, 2, 0.3, 5, 0, None, 0, None,
                                  stream_ptr()) == 0
    assert so.dkm_dbscan_link_f64(None, 0, 2, 2, 0.3, 0, None, 0, None, None,
                                  None, None, stream_ptr()) == 0
    ncl = _i32(1, -7)
    assert so.dkm_dbscan_finalize(0, 5, None, 0, None, None, None, None, None,
                                  ptr(ncl), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert int(ncl) == 0
    assert args.untouched()


def test_workspace_bytes():
    from dislib_amd import _lib
    so = _lib.load()
    assert so.dkm_dbscan_workspace_bytes(2 ** 31 - 64, 2) == 0
    assert so.dkm_dbscan_workspace_bytes(2 ** 31 - 65, 2) > 0
    for n in (1, 64, 65, 16384, 16385, 32769, 10 ** 6):
        assert 0 < so.dkm_dbscan_workspace_bytes(n, 2) <= 64 * n + 2 ** 20, n
