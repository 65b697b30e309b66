"""Bounds written by the exact re-check's fp32 stage (DESIGN.md 3.14,
"Bounds from the re-check").

A row the bf16x3 screen cannot decide used to keep (+inf, 0) and came back to
the screen and the re-check at every later iteration.  Stage 1 of the
re-check now gives such a row ``(ub, lb)`` from its two best fp32 scores when
those decide it.  Here every bounds call is run twice from the same device
state (labels, bounds, centres, workspace), with ``DKM_BOUNDS_SETTLE=0`` and
``=1``; the rows whose ``ub`` is +inf in the off run and finite in the on run
are the re-check-written set R.  Checked per call, in the list form and in
the image form of the screen (``DKM_BOUNDS_LIST_FRAC`` = 1 / 0):

* labels of both runs are bit-identical and the oracle's;
* ``bounds_ref.check_valid`` on every row of the on run (long double);
* R is tight within ``settle_slack`` of the truth, and every row left at
  (+inf, 0) by the off run whose true squared gap exceeds twice that slack is
  in R (a re-check that writes nothing fails here);
* |R| >= 100, and the host model predicted as much before the call;
* the ``dkm_bounds_settled`` counter gained exactly |R|;
* tied rows (duplicate centres, rows on a bisector) are never in R.

The data are k/2 blobs fitted with k centres: pairs of centres split blobs
and a large share of the rows lies inside the bf16x3 window of a bisector.
Every call continues from the off run's state, so each compared call meets
the whole population of near-tie rows; the bounds the re-check wrote are
followed through later bounds passes by the fit-level test, which runs
``check_valid`` at every iteration of a fit with the default switch.

Rows counted at iterations 2-5.  Predicted on the host before any GPU run
(oracle Lloyd loop: rows whose true squared gap lies between 2 settle_slack
and bound2 / 4, a quarter of the bf16x3 window); observed: |R| on an MI355X,
the same in the list form and the image form:

    shape                 predicted (it 2..5)      observed |R| (it 2..5)
    (8192, 32, 100) f64   713 / 583 / 523 / 492    4816 / 4482 / 4345 / 4264
    (8192, 32, 100) f32   713 / 583 / 523 / 492    4818 / 4483 / 4344 / 4264
    (8192,  8, 256)       301 / 236 / 204 / 204    1448 / 1266 / 1163 / 1101
    (8192, 17,  37)       678 / 612 / 546 / 549    3601 / 3393 / 3271 / 3196

(The screen's real window is the whole B2 and its scores err by far less
than B2 / 2, so R holds several times the predicted rows.)  The tie case
(8192, 32, 16) gave |R| = 34 / 100 / 164 / 216 and is not held to the 100.
Fit-level, list form: re-checked rows at iterations 4-11, off 4443 ... 4140,
on 4415, 4217, 3670, 3497, 3561, 2890, 3237, 3217.
"""
import functools

import numpy as np
import pytest

from oracle import kmeans_oracle as orc
from tests import bounds_ref as br

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CALLS = 6            # iterations 0, 1 full; 2 init; 3-5 after a bounds pass
MIN_R = 100
STD = 0.5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _blobs(n, d, k):
    """k / 2 blobs (std 0.5: the squared gap across a pair's bisector grows
    with std^2, the bf16x3 window with the norms) for k centres."""
    x, _ = orc.make_blobs_rows(0, n, d, max(1, k // 2), 3, std=STD)
    x = np.ascontiguousarray(x, dtype=np.float64)
    x.setflags(write=False)
    return x


def _c0(d, k):
    """Two centres per blob, a quarter of a unit either side of the
    blob's centre in a random direction (an odd k: one more at the first
    blob): each pair's bisector passes through its blob."""
    cen = orc.blob_centres(max(1, k // 2), d, 3, 10.0)
    z = np.random.RandomState(1).standard_normal(cen.shape)
    z *= 0.5 * STD / np.sqrt(np.einsum("ij,ij->i", z, z))[:, None]
    C = np.concatenate([cen + z, cen - z, cen[:k % 2] + 2.0 * z[:k % 2]])
    assert C.shape == (k, d)
    return np.ascontiguousarray(C, dtype=np.float64)


def _c0_uniform(d, k):
    from dislib_amd.cluster.kmeans import _init_centers
    return np.array(_init_centers(d, False, k, 0), dtype=np.float64)


def _lloyd(x, C0, mode="auto"):
    from dislib_amd.cluster import kmeans as km
    from dislib_amd.data import load_data
    old = km.BOUNDS
    km.BOUNDS = True
    try:
        ds = load_data(x, subset_size=max(1, x.shape[0]))
        return km._Lloyd(ds, np.array(C0, dtype=np.float64), 0.0, True,
                         mode=mode)
    finally:
        km.BOUNDS = old


def bound_f32(xn, cm, d):
    """``screen_bound<P_F32>(d, xn, cm, false)`` in fp64: the B of the
    re-check's stage 1."""
    rel = (d + 6.0) * 2.0 ** -24
    s = xn + cm
    mag = 2.0 * xn * cm + cm * cm
    b = 2.0 * rel * mag + 16.0 * 2.0 ** -52 * s * s + \
        (8.0 * d) * 2.0 ** -120 * (s + 1.0)
    return b * 1.0001


def settle_slack(x, C, d):
    """Per row, in fp64: what the square of a bound that stage 1 of the
    re-check has just written may differ from the true squared distance by,

        s32 = 2^-17 |x|^2 + 2.1 B(x),   B = bound_f32(|x|, cm, d),

    cm = ``bounds_ref.centre_norm_max``.  The kernel writes (settle_bounds in
    dkm_recheck.hip), in fp64 from fp32 inputs,

        u2 = xx (1 + 2^-18) + b1 + Bk,  ub = sqrt(u2) rounded up to fp32
        l2 = xx (1 - 2^-18) + b2 - Bk,  lb = sqrt(l2) rounded down to fp32

    with Bk its own fp32 ``screen_bound<P_F32>``, b1 the label's fp32 score
    and b2 the least score of the other centres.

    * A score's own error: |score - (|c|^2 - 2 x.c)| <= Bk / 2 (DESIGN.md
      3.14: fl32 of x and c, cn32, the d-term fma chain and the last fma
      make (d + 3) 2^-24 mag, and Bk >= 2 (d + 6) 2^-24 mag).  So b1 + Bk <=
      s_own + 1.5 Bk and b2 - Bk >= s_other - 1.5 Bk.
    * xx is the fp32 fma chain of d <= 32 squares of fl32(x): within 35 x
      2^-24 < 2^-18.8 of |x|^2.  With the kernel's 2^-18: at most (2^-18 +
      2^-18.8 + 2^-36) |x|^2 < 2^-17.3 |x|^2; the model grants 2^-17.
    * Bk against this fp64 B: the kernel's xn is sqrtf(xx) (1 + (d + 4)
      2^-24) <= |x| (1 + 2^-18), its cm the fp64 value rounded to fp32 times
      1.000001f, the polynomial a few fp32 ulp: Bk <= B (1 + 2^-16), so 1.5 Bk
      < 1.51 B.  The model grants 2.1, because the must-settle clause needs
      2 s32 > 4 Bk: stage 1 decides when b2 - b1 > 2 Bk, which a true gap
      above 3 Bk ensures (both scores within Bk / 2).
    * The fp64 evaluation (2^-53) is nothing here; the outward rounding of
      the roots to fp32 is one ulp, 2^-23 of the root and 2^-22 of its
      square: inside the 2^-19 of the check below.

    The checks are then ``bounds_ref.check_screen_tight``'s, with this slack:
    ub^2 <= (D_own^2 + s32)(1 + 2^-19), lb^2 >= (D_other^2 - s32)(1 - 2^-19),
    and a row with D_other^2 - D_own^2 > 2 s32 is settled."""
    xw = np.asarray(x).astype(np.float64)
    assert xw.shape[1] == d and d <= 32
    x2 = np.einsum("ij,ij->i", xw, xw)
    xn = np.sqrt(x2)
    return 2.0 ** -17 * x2 + 2.1 * bound_f32(xn, br.centre_norm_max(C), d)


def _snapshot(st):
    return dict(lab=st.labels.clone(), ws=st.ws.buf.clone(),
                bounds=None if st.bounds is None else st.bounds.clone(),
                valid=st.bounds_valid, C=st.C.clone())


def _restore(st, s):
    st.labels.copy_(s["lab"])
    st.ws.buf.copy_(s["ws"])
    st.C.copy_(s["C"])
    if s["bounds"] is not None:
        st.bounds.copy_(s["bounds"])
    elif st.bounds is not None:
        st.bounds.zero_()
    st.bounds_valid = s["valid"]


def _run(st, n, settle, monkeypatch):
    monkeypatch.setenv("DKM_BOUNDS_SETTLE", settle)
    s0, c0, r0 = st.bounds_settled(), st.bounds_counters(), st.rechecked()
    st.assign()
    out = dict(lab=st.labels[:n].cpu().numpy().copy(),
               settled=st.bounds_settled() - s0,
               cnt=tuple(a - b for a, b in zip(st.bounds_counters(), c0)),
               rechecked=st.rechecked() - r0)
    if st.bounds_valid:
        b = st.bounds[:, :n].cpu().numpy()
        out["ub"], out["lb"] = b[0].copy(), b[1].copy()
    return out


def _compare_calls(x, C0, frac, monkeypatch, mode="auto", pin=None,
                   tied=None, calls=CALLS, min_r=MIN_R, name=""):
    """The Lloyd loop with every bounds call run off and on from one state;
    returns the per-call |R|."""
    monkeypatch.setenv("DKM_BOUNDS_LIST_FRAC", frac)
    n, d = x.shape
    st = _lloyd(x, C0, mode)
    assert st.bounding, "the shape keeps no bounds"
    st.prepare()             # the workspace header: the counters read it
    xs = st.dd.X.cpu().numpy()
    sizes = []
    for it in range(calls):
        if pin is not None:
            st.C.copy_(torch.from_numpy(pin(st.C.cpu().numpy())))
        C = st.C.cpu().numpy().copy()
        what = "%s frac=%s call %d" % (name, frac, it)
        snap = _snapshot(st)
        on = _run(st, n, "1", monkeypatch)
        bounds_call = st.bounds_valid
        if not bounds_call:
            assert on["settled"] == 0, what
            st.reduce_update()
            st.read_flags()
            continue
        _restore(st, snap)
        off = _run(st, n, "0", monkeypatch)      # the fit goes on from here
        assert off["settled"] == 0, what
        assert off["cnt"] == on["cnt"], what
        with np.errstate(invalid="ignore"):
            ref = orc.partial_sum(xs, C)[0]
        assert np.array_equal(on["lab"], off["lab"]), what
        assert np.array_equal(on["lab"], ref), what
        lab = on["lab"]
        D = br.exact_distances(xs, C)
        br.check_valid(on["ub"], on["lb"], lab, D, what + " (on)")
        br.check_valid(off["ub"], off["lb"], lab, D, what + " (off)")
        undecided = np.isinf(off["ub"])
        assert np.all(off["lb"][undecided] == 0), what
        R = undecided & np.isfinite(on["ub"])
        # nothing else differs between the two runs
        same = ~R
        assert np.array_equal(on["ub"][same], off["ub"][same]), what
        assert np.array_equal(on["lb"][same], off["lb"][same]), what
        s32 = settle_slack(xs, C, d)
        own, other = br.own_other(D, lab)
        gap = (other * other - own * own).astype(np.float64)
        model = undecided & (gap > 2.0 * s32)
        print("%s: undecided %d model (gap > 2 s32) %d R %d settled counter "
              "%d re-checked on/off %d/%d"
              % (what, undecided.sum(), model.sum(), R.sum(), on["settled"],
                 on["rechecked"], off["rechecked"]))
        # tight on R, and every clearly separated undecided row is in R
        br.check_screen_tight(on["ub"], on["lb"], lab, D, s32, undecided,
                              what + " (re-check)")
        assert on["settled"] == int(R.sum()), what
        assert on["rechecked"] == off["rechecked"], what
        if tied is not None:
            t = tied(lab)
            assert t.sum() >= 64 and np.all(undecided[t]), what
            assert not np.any(R & t), what
            assert not np.any(on["ub"][t] < on["lb"][t]), what
        assert int(model.sum()) >= min_r, (what, int(model.sum()))
        assert int(R.sum()) >= min_r, (what, int(R.sum()))
        sizes.append(int(R.sum()))
        st.reduce_update()
        st.read_flags()
    assert len(sizes) == calls - 2, sizes
    return sizes


@pytest.mark.parametrize("frac", ["1", "0"])
@pytest.mark.parametrize("n,d,k,dtype,mode", [
    (8192, 32, 100, np.float64, "auto"),
    (8192, 32, 100, np.float32, "auto"),
    (8192, 8, 256, np.float64, "bf16x3"),
    (8192, 17, 37, np.float64, "auto"),
])
def test_recheck_writes_bounds(n, d, k, dtype, mode, frac, monkeypatch):
    """Both forms of the bounds call, fp64 and fp32 rows, rows in 16-B pieces
    (d = 32, 8) and element by element (d = 17).  k = 256 at d = 8 runs in
    mode "bf16x3" (in auto mode that shape takes the label-sorted image,
    which keeps no bounds)."""
    x = np.ascontiguousarray(_blobs(n, d, k).astype(dtype))
    _compare_calls(x, _c0(d, k), frac, monkeypatch, mode=mode,
                   name="settle %s" % ((n, d, k, np.dtype(dtype).name),))


@pytest.mark.parametrize("frac", ["1", "0"])
def test_ties_are_never_settled(frac, monkeypatch):
    """tests/test_gpu_bounds.py's ties: centres 2 = 5 bit for bit, and rows
    exactly on the bisector of centres 7 and 9, put back before every call.
    Stage 1 cannot separate them (equal fp32 scores), so they go to stage 2
    and keep (+inf, 0): never in R, never ``ub < lb``."""
    n, d, k = 8192, 32, 16
    x = _blobs(n, d, k).copy()
    C0 = _c0_uniform(d, k) * 8.0 - 4.0
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

    def tied(lab):
        t = np.zeros(n, bool)
        t[tie] = True
        return t | (lab == 2)

    _compare_calls(x, pin(C0), frac, monkeypatch, pin=pin, tied=tied,
                   min_r=1, name="ties")


def test_fit_rechecks_less(monkeypatch):
    """(8192, 32, 100), 12 iterations, the switch on against off: identical
    labels at every iteration, centres within 1e-12, and from iteration 4 on
    the on fit re-checks strictly fewer rows and keeps strictly fewer
    active.  The on fit's bounds are valid at every iteration (bounds the
    re-check wrote, moved by later bounds passes, included).  Both fits take
    the list form at every pass (``DKM_BOUNDS_LIST_FRAC=1``), as the steady
    iterations of a large fit do: with these split blobs most rows are still
    active at 8192 rows, and the image form, which the default 0.45 would
    pick, screens and re-checks every row whatever the bounds say."""
    import os
    monkeypatch.setenv("DKM_BOUNDS_LIST_FRAC", "1")
    n, d, k, iters = 8192, 32, 100, 12
    x = _blobs(n, d, k)
    res = {}
    old = os.environ.get("DKM_BOUNDS_SETTLE")
    try:
        for sw in ("0", "1"):
            os.environ["DKM_BOUNDS_SETTLE"] = sw
            st = _lloyd(x, _c0(d, k))
            assert st.bounding
            st.prepare()
            rows = []
            for it in range(iters):
                C = st.C.cpu().numpy().copy()
                r0, c0 = st.rechecked(), st.bounds_counters()
                st.assign()
                lab = st.labels[:n].cpu().numpy().copy()
                rows.append((lab, st.rechecked() - r0,
                             st.bounds_counters()[1] - c0[1]))
                if sw == "1" and st.bounds_valid:
                    b = st.bounds[:, :n].cpu().numpy()
                    br.check_valid(b[0], b[1], lab, br.exact_distances(x, C),
                                   "fit iteration %d" % it)
                st.reduce_update()
                st.read_flags()
            res[sw] = (rows, st.C.cpu().numpy().copy(), st.bounds_settled())
    finally:
        if old is None:
            os.environ.pop("DKM_BOUNDS_SETTLE", None)
        else:
            os.environ["DKM_BOUNDS_SETTLE"] = old
    off, on = res["0"], res["1"]
    for it in range(iters):
        assert np.array_equal(on[0][it][0], off[0][it][0]), it
    rel = np.max(np.abs(on[1] - off[1]) / np.maximum(np.abs(off[1]), 1.0))
    print("re-checked per iteration off", [r[1] for r in off[0]])
    print("re-checked per iteration on ", [r[1] for r in on[0]])
    print("active per iteration off", [r[2] for r in off[0]])
    print("active per iteration on ", [r[2] for r in on[0]])
    print("settled", on[2], "centres rel", rel)
    assert rel <= 1e-12
    assert off[2] == 0 and on[2] > 0
    assert sum(r[1] for r in on[0][4:]) < sum(r[1] for r in off[0][4:])
    assert sum(r[2] for r in on[0][4:]) < sum(r[2] for r in off[0][4:])
