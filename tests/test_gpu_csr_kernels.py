"""GPU tests of the CSR k-means entries of the C ABI (dkm_sparse.hip and the
CSR part of k_prepare) called one by one on raw device arrays: sliced centre
tables (S = 2, 4, 8, empty slices), every k / pass-count edge, every row
length of the staging scheme, signs, stored zeros, stored order, fp32
overflow and underflow, the delta hand-off, small workspaces, the segmented
and the atomic sums -- labels bit-exact against the oracle's sklearn-order
arithmetic, and the number of rows the exact arithmetic took against the
host restatement of the screen's bound (tests/csr_ref.py)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from dislib_amd import _device, _lib
from tests import csr_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROW_LENGTHS = list(range(27)) + [32, 33, 40, 64, 65]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _slices(k, d):
    w = ctypes.c_int64(-1)
    s = _lib.lib().dkm_csr_slices(k, d, ctypes.byref(w))
    return int(s), int(w.value)


def _close(a, b, rtol):
    err = np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)) if a.size else 0
    assert err <= rtol, "max rel err %g > %g" % (err, rtol)


class Case:
    """The operands of one case on the device (all held until the case is
    over) and a fresh workspace; the three entries through the C ABI."""

    def __init__(self, ptr, ind, dat, d, C, nq=0):
        self.so = _lib.lib()
        self.n, self.d, self.k = len(ptr) - 1, int(d), C.shape[0]
        self.ptr = _dev(ptr.astype(np.int64))
        self.ind = _dev(ind.astype(np.int32) if len(ind) else
                        np.zeros(1, np.int32))
        self.dat = _dev(dat.astype(np.float64) if len(dat) else np.zeros(1))
        self.C = _dev(np.asarray(sp.csr_matrix(C).toarray(), np.float64))
        self.ws = _device.Workspace(self.k, self.d, nq or max(self.n, 1),
                                    torch.device("cuda"))
        self.acc = torch.empty(self.k * (self.d + 1), dtype=torch.float64,
                               device="cuda")

    def _run(self, name, lab, acc):
        """(labels, acc as (sums, counts), rows the exact arithmetic took)"""
        _device.prepare(self.C, self.ws, acc, csr=True)
        r0 = _device.rechecked(self.ws)
        args = [_p(self.ptr), _p(self.ind), _p(self.dat), self.n, self.d,
                _p(self.C), self.k, self.ws.p, self.ws.nbytes, _p(lab)]
        if name != "dkm_predict_csr_f64":
            args.append(_p(acc))
        _lib.check(getattr(self.so, name)(*args, _device.stream_ptr()), name)
        torch.cuda.synchronize()
        grown = _device.rechecked(self.ws) - r0
        out = None
        if acc is not None:
            a = acc.cpu().numpy()
            out = (a[:self.k * self.d].reshape(self.k, self.d),
                   a[self.k * self.d:])
        return (lab.cpu().numpy() if lab is not None else None), out, grown

    def predict(self):
        lab = torch.full((self.n,), -7, dtype=torch.int32, device="cuda")
        return self._run("dkm_predict_csr_f64", lab, None)

    def partial_sum(self, labels=True):
        lab = torch.full((self.n,), -7, dtype=torch.int32, device="cuda") \
            if labels else None
        return self._run("dkm_partial_sum_csr_f64", lab, self.acc)

    def delta(self, prev):
        lab = _dev(np.asarray(prev, np.int32))
        return self._run("dkm_assign_delta_csr_f64", lab, self.acc)


def _prev_kinds(labels, k):
    """Previous labels cycling through: correct, wrong but in range, -1 and
    k + 5 (out of range: nothing is subtracted)."""
    prev = labels.copy()
    prev[1::4] = (prev[1::4] + 1) % k
    prev[2::4] = -1
    prev[3::4] = k + 5
    return prev


def _check(ptr, ind, dat, d, C, exact=True, nq=0, grow=None, tag=""):
    """The three entries on one input: labels, counts, sums and the delta
    against csr_ref.expected, the growth of the resolve count within
    [surely undecided, n - surely decided] (or ``grow`` = (lo, hi)), a
    second predict identical.  Returns the oracle's labels."""
    k, n = C.shape[0], len(ptr) - 1
    labels, sums, counts = ref.expected(ptr, ind, dat, d, C)
    if grow is None:
        decided, undecided = ref.classify(ptr, ind, dat, d, C)
        grow = (int(undecided.sum()), n - int(decided.sum()))
    case = Case(ptr, ind, dat, d, C, nq)
    want = sums.toarray()

    def same_sums(got, w):
        if exact:
            assert np.array_equal(got, w)
        else:
            _close(got, w, 1e-12)

    lab, _, g = case.predict()
    print("%s n %d k %d d %d: resolved %d of [%d, %d]" % (
        tag, n, k, d, g, grow[0], grow[1]))
    assert np.array_equal(lab, labels)
    assert grow[0] <= g <= grow[1], (g, grow)
    lab2, _, g2 = case.predict()
    assert np.array_equal(lab2, lab) and g2 == g

    lab, (s, c), g = case.partial_sum()
    assert np.array_equal(lab, labels)
    assert np.array_equal(c, counts.astype(np.float64))
    same_sums(s, want)
    assert grow[0] <= g <= grow[1], (g, grow)

    prev = _prev_kinds(labels, k)
    lab, (s, c), g = case.delta(prev)
    assert np.array_equal(lab, labels)
    ds, dc = ref.expected_delta(ptr, ind, dat, d, k, labels, prev)
    assert np.array_equal(c, dc)
    same_sums(s, ds.toarray())
    assert grow[0] <= g <= grow[1], (g, grow)
    return labels, grow


# ---------------------------------------------------------------------------
# sliced centre tables
# ---------------------------------------------------------------------------
# (k, d) -> (S, width): 16 MiB of bf16 per slice (CSR_SLICE_BYTES).  At
# (65, 65537) the second slice holds one centre; at (129, 65537) slice 2
# holds one and slice 3 none; at (257, 65537) slice 4 holds one and slices
# 5-7 none (the merge's empty-slice sentinel); (1024, 16385) is one column
# past two 512-wide slices of exactly 16 MiB, so it takes four 256-wide
# ones (four passes per walk), (1024, 16384) the two 512-wide ones (two
# walks of four passes)
SLICED = {(65, 65537): (2, 64), (129, 65537): (4, 64), (257, 65537): (8, 64),
          (1024, 16385): (4, 256), (1024, 16384): (2, 512)}


def _sliced(k, d):
    S, w = _slices(k, d)
    assert (S, w) == SLICED[(k, d)] and S > 1
    return S, w


@pytest.mark.parametrize("k,d", sorted(SLICED))
def test_sliced_own_rows_every_centre_of_every_slice_wins(k, d):
    _sliced(k, d)
    n = max(300, k + 3)
    ptr, ind, dat, C = ref.own_rows(k, d, n, k)
    labels, grow = _check(ptr, ind, dat, d, C, tag="own")
    assert grow == (0, 0)
    assert np.array_equal(np.unique(labels), np.arange(k))


@pytest.mark.parametrize("k,d", sorted(SLICED))
def test_sliced_twin_rows_tie_across_slices_first_index(k, d):
    S, w = _sliced(k, d)
    n = 300
    ptr, ind, dat, C = ref.twin_rows(k, d, n, k)
    labels, grow = _check(ptr, ind, dat, d, C, tag="twin")
    assert grow == (n, n)
    h = (k + 1) // 2
    assert (labels // w != (labels + h) // w).any()   # twins in two slices


@pytest.mark.parametrize("k,d", sorted(SLICED))
def test_sliced_near_twin_rows_pairs_in_two_slices(k, d):
    S, w = _sliced(k, d)
    n = 300
    ptr, ind, dat, C = ref.near_twin_rows(k, d, n, 0, w)
    labels, grow = _check(ptr, ind, dat, d, C, exact=False, tag="near")
    pairs = ref.near_twin_pairs(k, w)
    lo = np.array([pairs[i % len(pairs)][0] for i in range(n)])
    assert (lo // w != (lo + w) // w).all()
    high = labels == lo + w
    assert ((labels == lo) | high).all() and high.sum() >= n // 4


# ---------------------------------------------------------------------------
# k edges: one slice; 1, 2 and 4 passes per walk, a dead pass block, a
# second walk
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 192,
                               193, 256, 257])
def test_k_edges(k):
    d = 40
    assert _slices(k, d) == (1, (k + 63) // 64 * 64)
    n = 2 * k + 3
    ptr, ind, dat, C = ref.own_rows(k, d, n, k)
    labels, grow = _check(ptr, ind, dat, d, C, tag="own")
    assert grow == (0, 0)
    assert np.array_equal(np.unique(labels), np.arange(k))
    if k >= 2:
        ptr, ind, dat, C = ref.twin_rows(k, d, n, k)
        labels, grow = _check(ptr, ind, dat, d, C, tag="twin")
        assert grow == (n, n) and (labels < (k + 1) // 2).all()


# ---------------------------------------------------------------------------
# row lengths: two pipelined 8-entry chunks, then direct loads; the 2-entry
# tail chunk voted by the wave
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 130, 257])     # 1, 2 and 4 passes per walk
@pytest.mark.parametrize("shuffled", [False, True])
def test_row_lengths(k, shuffled):
    d = 70
    C = ref.dense_int_centres(k, d, k)
    rng = np.random.default_rng(k)
    for n in (1, 7, 8, 9, 63, 65, 257):
        lengths = [ROW_LENGTHS[i % len(ROW_LENGTHS)] for i in range(n)]
        if shuffled:                # one wave holds mixed lengths
            lengths = list(rng.choice(ROW_LENGTHS, n))
            lengths[n // 2] = 0
        ptr, ind, dat = ref.length_rows(lengths, d, n, zeros=(n % 2 == 1))
        labels, grow = _check(ptr, ind, dat, d, C,
                              tag="lengths%s" % ("*" if shuffled else ""))
        empty = np.diff(ptr) == 0
        assert (labels[empty] == 0).all()   # first of the equal-norm centres
        assert grow[0] >= empty.sum()


# ---------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------
def test_descending_stored_order_is_the_arithmetic_order():
    k, d, n = 64, 2000, 300
    ptr, ind, dat, C = ref.near_twin_rows(k, d, n, 0, 32, descending=True)
    assert all((np.diff(ind[a:b]) < 0).all()
               for a, b in zip(ptr[:-1], ptr[1:]))
    labels, _ = _check(ptr, ind, dat, d, C, exact=False, tag="descending")
    assert (labels < 32).any() and (labels >= 32).any()


@pytest.mark.parametrize("xs,cs", [(1e25, 1.0), (1e25, 1e25), (1e-25, 1.0),
                                   (1e-25, 1e-25)])
def test_fp32_overflow_and_underflow_fall_through_to_fp64(xs, cs):
    """x 1e25: xx (and with the centres scaled too, every score) overflows
    fp32, so B is not finite and no row may be decided.  x 1e-25 with the
    centres scaled too: every fp32 norm and product lies below 2^-149 and
    rounds to 0, every score is 0: all tied, none decided.  x 1e-25 alone:
    centres of equal norm tie in fp32 (any count may be resolved)."""
    k, d, n = 9, 200, 67
    ptr, ind, dat, C = ref.own_rows(k, d, n, 5)
    C = sp.csr_matrix(C * cs)
    grow = (0, n) if (xs, cs) == (1e-25, 1.0) else (n, n)
    _check(ptr, ind, dat * xs, d, C, exact=False, grow=grow,
           tag="x%g c%g" % (xs, cs))


# ---------------------------------------------------------------------------
# small workspaces: several chunks, a ragged last one, every list slot used
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,d,S", [(65, 65537, 2), (60, 40, 1)])
def test_chunks_of_a_small_workspace(k, d, S):
    assert _slices(k, d)[0] == S
    n, nq = 150, 64
    ptr, ind, dat, C = ref.twin_rows(k, d, n, 1)
    # 64 slots of 12 bytes: 64 * 12 / (12 S + 12) rows per chunk
    assert n % (nq * 12 // (12 * S + 12)) != 0 and n > 2 * nq
    _, grow = _check(ptr, ind, dat, d, C, nq=nq, tag="chunks")
    assert grow == (n, n)
    ptr, ind, dat, C = ref.own_rows(k, d, n, 2)
    _, grow = _check(ptr, ind, dat, d, C, nq=nq, tag="chunks")
    assert grow == (0, 0)


# ---------------------------------------------------------------------------
# full sums over the label-sorted rows: blocks of 4096 positions, two column
# tiles
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[4096, 0, 100, 3996, 0, 809],
                                   [5000, 0, 3000, 0, 1000, 1]])
def test_segmented_sums_block_starts_and_column_tiles(sizes):
    """n = 9001 rows in interleaved order; block starts 4096 and 8192 fall
    on a cluster boundary followed by an empty cluster (first sizes) or
    inside a cluster (second); entries at columns 0, 16383, 16384 and d - 1
    straddle the 16384-column tile."""
    k, d = 6, 16390
    n = sum(sizes)
    assert n == 9001
    rng = np.random.default_rng(sizes[0])
    special = np.array([0, 16383, 16384, d - 1])
    rows = np.repeat(np.arange(k), 4)
    cols = np.concatenate([[10 + j, 5000 + j, 16300 + j, 16385 + (j % 4)]
                           for j in range(k)])
    C = sp.csr_matrix((8.0 * rng.choice([-1.0, 1.0], 4 * k), (rows, cols)),
                      shape=(k, d))
    owners = rng.permutation(np.repeat(np.arange(k), sizes))
    ptr, ind, dat = [0], [], []
    for j in owners:
        sl = slice(C.indptr[j], C.indptr[j + 1])
        extra = special[rng.random(4) < 0.5]
        c = np.concatenate([C.indices[sl], extra])
        v = np.concatenate([C.data[sl],
                            rng.integers(1, 3, len(extra)) *
                            rng.choice([-1.0, 1.0], len(extra))])
        o = rng.permutation(len(c))
        ind.extend(c[o])
        dat.extend(v[o])
        ptr.append(len(ind))
    ptr, ind, dat = (np.array(ptr, np.int64), np.array(ind, np.int32),
                     np.array(dat))
    labels, sums, counts = ref.expected(ptr, ind, dat, d, C)
    assert np.array_equal(labels, owners) and list(counts) == sizes
    decided, _ = ref.classify(ptr, ind, dat, d, C)
    assert decided.all()
    want = sums.toarray()
    assert all(want[:, t].any() for t in special)
    case = Case(ptr, ind, dat, d, C)
    lab, (s, c), g = case.partial_sum()
    assert g == 0
    assert np.array_equal(lab, labels)
    assert np.array_equal(c, np.array(sizes, np.float64))
    assert np.array_equal(s, want)
    # a small workspace: the label sort runs in spans of 4160 rows, whose
    # blocks start at other positions
    case = Case(ptr, ind, dat, d, C, nq=4160)
    lab, (s, c), g = case.partial_sum()
    assert g == 0 and np.array_equal(lab, labels)
    assert np.array_equal(c, np.array(sizes, np.float64))
    assert np.array_equal(s, want)


# ---------------------------------------------------------------------------
# atomic sums: no label array, or k beyond the label sort
# ---------------------------------------------------------------------------
def test_atomic_sums_without_labels():
    k, d, n = 9, 200, 203
    for gen, grow in ((ref.own_rows, 0), (ref.twin_rows, n)):
        ptr, ind, dat, C = gen(k, d, n, 7)
        labels, sums, counts = ref.expected(ptr, ind, dat, d, C)
        case = Case(ptr, ind, dat, d, C)
        lab, (s, c), g = case.partial_sum(labels=False)
        assert lab is None and g == grow
        assert np.array_equal(c, counts.astype(np.float64))
        assert np.array_equal(s, sums.toarray())


def test_atomic_sums_when_k_is_beyond_the_label_sort():
    k, d, n = 16385, 8, 300
    j = np.arange(k)
    C = sp.csr_matrix(np.stack([(j // 5 ** t) % 5 - 2.0 for t in range(d)],
                               axis=1))
    assert len(np.unique(C.toarray(), axis=0)) == k
    rng = np.random.default_rng(0)
    ptr, ind, dat = ref.length_rows(rng.integers(0, d + 1, n), d, 1)
    labels, grow = _check(ptr, ind, dat, d, C, tag="k > SORT_KMAX")
    assert labels.max() > 64
