"""The tile form of the list re-check's stage 1 ("The
re-check's stage 1 on fp32 MFMA tiles") against the lane form it replaces.

``k_recheck_tile`` scores a wave's 64 listed rows on the fp32 MFMA; with
``DKM_RECHECK_TILE=0`` the list re-check runs the lane-per-row
``k_recheck_list`` instead.  Every case runs the same Lloyd loop once in each
form, on rows ``ldx > d`` apart with NaN in the padding columns (a kernel that
reads a padding column, or addresses rows by d, gets a wrong label), in the
list form and the image form of the bounds call (``DKM_BOUNDS_LIST_FRAC`` = 1 /
0), and checks per iteration:

* labels identical in both forms and equal to ``orc.partial_sum``'s;
* ``rechecked()`` equal in both forms, and positive (the re-check ran);
* ``ub`` / ``lb`` pass ``bounds_ref.check_valid`` in both forms;
* at the end, centres within 1e-12 of each other.

* the run with the knob unset launched ``k_recheck_tile`` and the run with
  ``DKM_RECHECK_TILE=0`` did not (``dkm_list_stats``).

The data are ``tests/test_gpu_bounds_settle.py``'s split blobs (STD 0.5): a
large share of the rows is left to the re-check, in lists whose lengths are no
multiples of 64 (asserted).  At these sizes every screen wave sees at most one
32-row tile, so a segment holds one partial batch;
``test_segments_of_64_and_65`` runs 600k rows, where a screen wave walks
several tiles, and places tie rows so that segments of exactly 64 and exactly
65 entries, and longer ones, occur (read back through ``dkm_list_stats``).
"""
import numpy as np
import pytest

from oracle import kmeans_oracle as orc
from tests import bounds_ref as br
from tests import test_gpu_bounds_settle as ts

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ITERS = 5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def list_stats(ws):
    from dislib_amd._device import list_stats as f
    return f(ws)


def _widen(st, pad):
    """Rows ``d + pad`` apart, NaN in the padding columns."""
    X = st.dd.X
    n, d = X.shape
    wide = torch.full((max(n, 1), d + pad), float("nan"), dtype=X.dtype,
                      device=X.device)
    wide[:n, :d] = X
    st.dd.X = wide[:n, :d]
    assert st.dd.X.stride(0) == d + pad


def _fit(x, C0, frac, tile, monkeypatch, mode="auto", pin=None, iters=ITERS):
    monkeypatch.setenv("DKM_BOUNDS_LIST_FRAC", frac)
    monkeypatch.setenv("DKM_RECHECK_TILE", tile)
    n, d = x.shape
    st = ts._lloyd(x, C0, mode)
    assert st.bounding, "the shape keeps no bounds"
    # a multiple of 16 B keeps the 16-B row pieces for d % 8 == 0
    _widen(st, 8 if d % 8 == 0 else 3)
    st.prepare()
    xs = st.dd.X.cpu().numpy()
    rows = []
    for it in range(iters):
        if pin is not None:
            st.C.copy_(torch.from_numpy(pin(st.C.cpu().numpy())))
        C = st.C.cpu().numpy().copy()
        r0, s0 = st.rechecked(), st.bounds_settled()
        l0 = list_stats(st.ws)
        st.assign()
        l1 = list_stats(st.ws)
        rec = dict(C=C, lab=st.labels[:n].cpu().numpy().copy(),
                   rechecked=st.rechecked() - r0,
                   settled=st.bounds_settled() - s0,
                   tile=l1[0] - l0[0], lane=l1[1] - l0[1], seg=l1[2])
        if st.bounds_valid:
            b = st.bounds[:, :n].cpu().numpy()
            rec["ub"], rec["lb"] = b[0].copy(), b[1].copy()
        rows.append(rec)
        st.reduce_update()
        st.read_flags()
    return xs, rows, st.C.cpu().numpy().copy()


def _both(x, C0, frac, monkeypatch, name, bounds=True, **kw):
    xs, new, Cn = _fit(x, C0, frac, "1", monkeypatch, **kw)
    _, old, Co = _fit(x, C0, frac, "0", monkeypatch, **kw)
    for it, (a, b) in enumerate(zip(new, old)):
        what = "%s frac=%s iteration %d" % (name, frac, it)
        with np.errstate(invalid="ignore", over="ignore"):
            ref = orc.partial_sum(xs, a["C"])[0]
        print("%s: re-checked new/old %d/%d settled new/old %d/%d"
              % (what, a["rechecked"], b["rechecked"], a["settled"],
                 b["settled"]))
        assert np.array_equal(a["lab"], b["lab"]), what
        assert np.array_equal(a["lab"], ref), what
        assert a["rechecked"] == b["rechecked"], what
        # the forms are the ones asked for (short re-screen lists take the
        # lane form's wave-per-row path in either run)
        assert a["tile"] >= 1 and b["tile"] == 0 and b["lane"] >= 1, what
        assert ("ub" in a) == ("ub" in b), what
        for form, r in (("tile", a), ("lane", b)):
            if bounds and "ub" in r:
                D = br.exact_distances(xs, r["C"])
                br.check_valid(r["ub"], r["lb"], r["lab"], D,
                               what + " (" + form + ")")
    fin = np.isfinite(Co)
    assert np.array_equal(fin, np.isfinite(Cn)), name
    rel = np.max(np.abs(Cn[fin] - Co[fin]) / np.maximum(np.abs(Co[fin]), 1.0),
                 initial=0.0)
    assert rel <= 1e-12, (name, rel)
    return new, old


@pytest.mark.parametrize("frac", ["1", "0"])
@pytest.mark.parametrize("n,d,k,dtype,mode", [
    (4099, 32, 100, np.float64, "auto"),
    (1000, 17, 37, np.float64, "auto"),
    (3000, 8, 256, np.float64, "bf16x3"),
    (2051, 32, 100, np.float32, "auto"),
])
def test_tile_form_equals_lane_form(n, d, k, dtype, mode, frac, monkeypatch):
    x = np.ascontiguousarray(ts._blobs(n, d, k).astype(dtype))
    new, old = _both(x, ts._c0(d, k), frac, monkeypatch,
                     "tile %s" % ((n, d, k, np.dtype(dtype).name),),
                     mode=mode)
    # the re-check ran at every iteration, on lists that are no multiples of
    # 64, and its stage 1 wrote bounds in both forms
    assert all(r["rechecked"] > 0 for r in new)
    assert any(r["rechecked"] % 64 for r in new)
    assert sum(r["settled"] for r in new) > 0
    assert sum(r["settled"] for r in old) > 0


@pytest.mark.parametrize("frac", ["1", "0"])
def test_ties(frac, monkeypatch):
    """``test_ties_are_never_settled``'s construction: centres 2 = 5 bit for
    bit and rows exactly on the bisector of centres 7 and 9, put back before
    every call.  Equal fp32 scores are never 2B apart: stage 2 decides them,
    the lower index as the oracle has it."""
    n, d, k = 2048, 32, 16
    x = ts._blobs(n, d, k).copy()
    C0 = ts._c0_uniform(d, k) * 8.0 - 4.0
    A = np.full(d, 24.0)
    B = A.copy()
    B[0] += 2.0
    tie = np.arange(64)
    x[tie] = 0.5 * (A + B)
    x[tie, 1] += 0.25 * (1 + tie % 4)

    def pin(C):
        C = C.copy()
        C[5] = C[2]
        C[7], C[9] = A, B
        return C

    new, _ = _both(x, pin(C0), frac, monkeypatch, "tile ties", pin=pin)
    assert all(r["rechecked"] >= 64 for r in new)
    for r in new:
        assert np.all(r["lab"][tie] == 7) and not np.any(r["lab"] == 5)
        if "ub" in r:
            assert not np.any(r["ub"][tie] < r["lb"][tie])


@pytest.mark.parametrize("frac", ["1", "0"])
def test_nonfinite_rows(frac, monkeypatch):
    """NaN, +-Inf and overflowing rows: never sane in stage 1, decided by the
    reference arithmetic; the centres they are summed into turn non-finite
    and every row then meets non-finite centres.  Labels only: the bounds
    of such a fit are tests/test_gpu_nonfinite.py's subject."""
    n, d, k = 1027, 32, 100
    x = ts._blobs(n, d, k).copy()
    x[5, 3] = np.nan
    x[70, 0] = np.inf
    x[71, 31] = -np.inf
    x[200, 7] = 1e200
    x[1026, :] = np.nan
    new, _ = _both(x, ts._c0(d, k), frac, monkeypatch, "tile nonfinite",
                   bounds=False, iters=3)
    assert all(r["rechecked"] > 0 for r in new)


def test_segments_of_64_and_65(monkeypatch):
    """Segments longer than one batch: 600k rows, so that a screen wave walks
    several 32-row tiles, of which a share p are tie rows (on the bisector of
    centres 7 and 9: never decided by the screen or by stage 1) and the rest
    sit 0.05 from one of 14 distinct centres (always decided by the
    screen).  A first pass with every row a tie row reads the rows per
    segment m back, whatever grid the screen took; p = 64.5 / max(m) then
    puts the longest segments' lengths around 64 (binomial, standard
    deviation about 4.5: some 8 % of them at each of 64 and 65).  One full
    pass in each form: labels equal and the oracle's, ``rechecked()`` equal,
    and the segment lengths read back hold 64, 65 and more (batch index 1
    with 1 entry, with more, and batch index 0 exactly full)."""
    n, d, k = 600_000, 32, 16
    C0 = ts._c0_uniform(d, k) * 8.0 - 4.0
    A = np.full(d, 24.0)
    B = A.copy()
    B[0] += 2.0
    C0[5] = C0[2]
    C0[7], C0[9] = A, B
    rs = np.random.RandomState(7)

    def rows(tie):
        # (not the duplicate centres 2 = 5: their rows are ties as well)
        lab = np.array([0, 1, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14,
                        15])[rs.randint(0, 14, n)]
        x = C0[lab] + 0.05 * rs.standard_normal((n, d))
        i = np.flatnonzero(tie)
        x[i] = 0.5 * (A + B)
        x[i, 1] += 0.25 * (1 + i % 4)
        return x

    _, probe, _ = _fit(rows(np.ones(n, bool)), C0, "1", "1", monkeypatch,
                       iters=1)
    m = probe[0]["seg"]
    assert probe[0]["rechecked"] == n and m.sum() == n, (m.sum(), n)
    assert m.max() > 65, "no screen wave walks more than two tiles"
    tie = rs.random_sample(n) < 64.5 / m.max()
    new, old = _both(rows(tie), C0, "1", monkeypatch, "tile segments",
                     iters=1)
    seg = new[0]["seg"]
    print("segments %d, entries %d, of 64: %d, of 65: %d, longest %d"
          % (seg.size, seg.sum(), (seg == 64).sum(), (seg == 65).sum(),
             seg.max()))
    assert new[0]["rechecked"] == seg.sum() >= tie.sum()
    assert np.array_equal(seg, old[0]["seg"])
    assert np.all(new[0]["lab"][tie] == 7)
    assert (seg == 64).any() and (seg == 65).any() and seg.max() > 65
