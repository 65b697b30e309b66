"""The fused list form of the bounds call ("The fused list
form") against the three launches it replaces.

An update call whose previous bounds call left at most half the list form's
share of the rows active runs the bounds pass and the list form of the screen
as one kernel (``k_screen_w32`` with FUSE); ``DKM_BOUNDS_FUSED=0`` launches
``k_bounds_pass`` and the unfused forms only.  Every case steps a Lloyd loop
with ``DKM_BOUNDS_LIST_FRAC=1`` (both runs take the list form) and runs every
call twice from one snapshot of the device state (labels, bounds, centres,
the whole workspace: header and previous centres included), fused on and off:

* labels bit-identical, and ``orc.partial_sum``'s;
* ``ub`` and ``lb`` bit-identical on every row;
* equal ``bounds_counters``, ``bounds_settled`` and ``rechecked`` deltas;
* ``acc`` within 1e-12 of each other relative to max(|acc|, 1), element by
  element (the fp64 atomics come in another order);
* the host counter of fused launches advanced by one in the on run of an
  update call and not at all in the off run, and the device says the fused
  form took the call (``bounds_fused_stats``).

At 8192 rows of the split blobs most rows stay active, so the previous share
a call finds is usually above one half and the device would choose the unfused
form: before such a call the test writes a previous count of 0 into the
header (``bnd_last``, whose place is checked against ``bounds_fused_stats``
first).  The kernel then finishes as a list form whatever the count: that is
also the "every row active after a small share" contract.
"""
import numpy as np
import pytest

from oracle import kmeans_oracle as orc
from tests import bounds_ref as br
from tests import test_gpu_bounds_settle as ts
from tests import test_gpu_recheck_tile as tr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CALLS = 6            # iterations 0, 1 full; 2 init; 3-5 update calls
OFF_LAST = 180       # WsHeader::bnd_last (checked in _set_prev)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def fused_stats(ws):
    from dislib_amd._device import bounds_fused_stats as f
    return f(ws)


def _set_prev(st, nact):
    """The previous bounds call's active rows, as the next call reads it."""
    w = st.ws.buf[OFF_LAST:OFF_LAST + 4].view(torch.int32)
    assert int(w.item()) == fused_stats(st.ws)[2] + 1, "bnd_last moved"
    w.fill_(nact + 1)


def _run(st, n, fused, monkeypatch):
    monkeypatch.setenv("DKM_BOUNDS_FUSED", fused)
    s0, c0, r0 = st.bounds_settled(), st.bounds_counters(), st.rechecked()
    f0 = fused_stats(st.ws)
    st.assign()
    f1 = fused_stats(st.ws)
    out = dict(lab=st.labels[:n].cpu().numpy().copy(),
               acc=st.acc.cpu().numpy().copy(),
               settled=st.bounds_settled() - s0,
               cnt=tuple(a - b for a, b in zip(st.bounds_counters(), c0)),
               rechecked=st.rechecked() - r0,
               launched=f1[0] - f0[0], taken=f1[1] - f0[1], last=f1[2])
    if st.bounds_valid:
        b = st.bounds[:, :n].cpu().numpy()
        out["ub"], out["lb"] = b[0].copy(), b[1].copy()
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _compare(x, C0, monkeypatch, mode="auto", pin=None, pre=None, widen=0,
             calls=CALLS, oracle=True, valid=True, frac="1", name=""):
    """The Lloyd loop with every call run fused on and off from one state.
    ``pre(st, it)`` may edit the state before an update call and returns the
    active rows that call must count (or None).  Returns the on runs of the
    update calls."""
    monkeypatch.setenv("DKM_BOUNDS_LIST_FRAC", frac)
    n, d = x.shape
    st = ts._lloyd(x, C0, mode)
    assert st.bounding, "the shape keeps no bounds"
    if widen:
        tr._widen(st, widen)
    st.prepare()
    xs = st.dd.X.cpu().numpy()
    ups = []
    for it in range(calls):
        if pin is not None:
            st.C.copy_(torch.from_numpy(pin(st.C.cpu().numpy())))
        what = "%s call %d" % (name, it)
        upd = st.bounds_valid and not st._full()
        want = None
        if upd:
            if pre is not None:
                want = pre(st, it)
            if frac != "0" and not 0 <= fused_stats(st.ws)[2] <= int(n * 0.5):
                _set_prev(st, 0)      # (none after the init call, or large)
        C = st.C.cpu().numpy().copy()
        snap = ts._snapshot(st)
        on = _run(st, n, "1", monkeypatch)
        ts._restore(st, snap)
        off = _run(st, n, "0", monkeypatch)       # the fit goes on from here
        assert upd == (on["cnt"][0] == 1), what
        fuses = upd and frac != "0"
        assert on["launched"] == (1 if fuses else 0), what
        assert on["taken"] == (1 if fuses else 0), what
        assert off["launched"] == 0 and off["taken"] == 0, what
        assert on["last"] == off["last"], what
        assert np.array_equal(on["lab"], off["lab"]), what
        if oracle:
            with np.errstate(invalid="ignore", over="ignore"):
                ref = orc.partial_sum(xs, C)[0]
            assert np.array_equal(on["lab"], ref), what
        assert on["cnt"] == off["cnt"], what
        assert on["settled"] == off["settled"], what
        assert on["rechecked"] == off["rechecked"], what
        fin = np.isfinite(off["acc"])
        assert np.array_equal(fin, np.isfinite(on["acc"])), what
        rel = np.max(np.abs(on["acc"][fin] - off["acc"][fin]) /
                     np.maximum(np.abs(off["acc"][fin]), 1.0), initial=0.0)
        print("%s: update %s active %s re-checked %d settled %d acc rel %.2e"
              % (what, upd, on["cnt"][1], on["rechecked"], on["settled"],
                 rel))
        assert rel <= 1e-12, (what, rel)
        assert ("ub" in on) == ("ub" in off), what
        if "ub" in on:
            assert np.array_equal(_bits(on["ub"]), _bits(off["ub"])), what
            assert np.array_equal(_bits(on["lb"]), _bits(off["lb"])), what
            if valid:
                br.check_valid(on["ub"], on["lb"], on["lab"],
                               br.exact_distances(xs, C), what)
        if upd:
            assert on["last"] == on["cnt"][1], what
            if want is not None:
                assert on["cnt"][1] == want, (what, on["cnt"], want)
            ups.append(on)
        st.reduce_update()
        st.read_flags()
    return ups


@pytest.mark.parametrize("n,d,k,dtype,mode,widen", [
    (8192, 32, 100, np.float64, "auto", 0),
    (8192, 32, 100, np.float32, "auto", 0),
    (8192, 17, 37, np.float64, "auto", 0),       # rows element by element
    (8192, 8, 256, np.float64, "bf16x3", 0),
    (4099, 32, 100, np.float64, "auto", 8),      # strided rows, NaN padding
    (1000, 17, 37, np.float64, "auto", 3),       # strided and unaligned
])
def test_fused_equals_unfused(n, d, k, dtype, mode, widen, monkeypatch):
    x = np.ascontiguousarray(ts._blobs(n, d, k).astype(dtype))
    ups = _compare(x, ts._c0(d, k), monkeypatch, mode=mode, widen=widen,
                   name="fused %s" % ((n, d, k, np.dtype(dtype).name, widen),))
    assert len(ups) == CALLS - 3
    # the screen, the re-check and its bounds all ran behind the fused kernel
    assert all(0 < r["cnt"][1] for r in ups)
    assert sum(r["rechecked"] for r in ups) > 0
    assert sum(r["settled"] for r in ups) > 0


def _c16(d, k=16):
    return ts._c0_uniform(d, k) * 8.0 - 4.0


@pytest.mark.parametrize("n", [1, 3, 1023, 1025, 4 * 256 * 7 + 5])
def test_ragged_rows(n, monkeypatch):
    """The ragged 4-row lane tail and the ragged last block of the stream."""
    d, k = 32, 16
    x = np.ascontiguousarray(ts._blobs(8192, d, k)[:n])
    ups = _compare(x, _c16(d), monkeypatch, name="ragged n=%d" % n)
    assert len(ups) == CALLS - 3


@pytest.mark.parametrize("m", [0, 31, 32, 33, 65])
def test_active_counts(m, monkeypatch):
    """Exactly m active rows: ub = 0 and lb = 3e38 on every row but m, which
    get ub = +inf (spread over the stream, so that several waves drain a
    partial step).  The skipped rows keep their labels whatever the centres,
    so the oracle is not asked."""
    n, d, k = 4 * 256 * 7 + 5, 32, 16
    x = np.ascontiguousarray(ts._blobs(8192, d, k)[:n])
    rows = torch.from_numpy(
        np.random.RandomState(m).permutation(n)[:m].astype(np.int64))

    def pre(st, it):
        st.bounds[0, :n] = 0.0
        st.bounds[1, :n] = 3e38
        st.bounds[0, rows.to(st.bounds.device)] = float("inf")
        return m

    ups = _compare(x, _c16(d), monkeypatch, pre=pre, oracle=False,
                   valid=False, name="active m=%d" % m)
    assert len(ups) == CALLS - 3


def test_every_row_active_after_small_share(monkeypatch):
    """One centre jumps far away before each update call: its drift takes
    every lower bound to 0, so every row is active, after a previous share
    the header gives as 0.  The fused kernel finishes as a list form."""
    n, d, k = 8192, 32, 16
    x = ts._blobs(n, d, k)

    def pre(st, it):
        st.C[3] += 1000.0
        _set_prev(st, 0)
        return n

    ups = _compare(x, _c16(d), monkeypatch, pre=pre, name="all active")
    assert len(ups) == CALLS - 3 and all(r["cnt"][3] == 1 for r in ups)


def test_nonfinite_drift(monkeypatch):
    """A centre turns NaN before the last call: the drift is not finite,
    every row is active and enters the screen with ub = +inf."""
    n, d, k = 2048, 32, 16
    x = ts._blobs(n, d, k)

    def pre(st, it):
        if it < CALLS - 1:
            return None
        st.C[5] = float("nan")
        return n

    ups = _compare(x, _c16(d), monkeypatch, pre=pre, valid=False,
                   name="nan drift")
    assert ups[-1]["cnt"][1] == n


def test_ties(monkeypatch):
    """``test_ties_are_never_settled``'s construction: centres 2 = 5 bit for
    bit and rows exactly on the bisector of centres 7 and 9, put back before
    every call."""
    n, d, k = 8192, 32, 16
    x = ts._blobs(n, d, k).copy()
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

    ups = _compare(x, pin(_c16(d)), monkeypatch, pin=pin, name="fused ties")
    for r in ups:
        assert np.all(r["lab"][tie] == 7) and not np.any(r["lab"] == 5)
        assert not np.any(r["ub"][tie] < r["lb"][tie])
        assert r["rechecked"] >= 64


def test_list_frac_zero_never_fuses(monkeypatch):
    """``DKM_BOUNDS_LIST_FRAC=0``: the image form at every call, and no fused
    kernel is launched (``_compare`` asserts it call by call)."""
    n, d, k = 2048, 32, 16
    ups = _compare(ts._blobs(n, d, k), _c16(d), monkeypatch, frac="0",
                   name="frac 0")
    assert len(ups) == CALLS - 3
    assert all(r["launched"] == 0 and r["taken"] == 0 for r in ups)
