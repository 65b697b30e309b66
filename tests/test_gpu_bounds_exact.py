"""The per-row bounds of the d <= 32 Lloyd loop against exact distances
("Checked by").

``tests/test_gpu_bounds.py`` compares labels with the bounds on and off; a
bound that is a few per cent too tight flips no label on separated blobs.
Here every ``ub`` / ``lb`` the device holds after every bounds call is held
against long-double distances under the centres of that call
(``tests/bounds_ref.py``):

* ``check_valid``: ub >= the distance to the own centre, lb <= the distance
  to every other centre, on every row;
* ``check_screen_tight``: a bound the screen has just written lies within the
  documented slack of the truth, and a clearly separated row was decided;
* ``check_pass_tight``: a bound the bounds pass moved, moved by the drift of
  the right centre and no more.

Which rows the pass settled and which it listed for the screen is recomputed
on the host (``pass_f32``: the pass in numpy fp32, bit for bit) and its count
of active rows must equal the device's.  Every case runs with
``DKM_BOUNDS_LIST_FRAC`` = 1 (the list form of the screen at every pass) and
= 0 (the image form), and the fourth counter proves which one ran.
"""
import functools

import numpy as np
import pytest

from oracle import kmeans_oracle as orc
from tests import bounds_ref as br

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ITERS = 8
DEFAULT_FRAC = 0.45            # BOUNDS_LIST_FRAC (dkm_internal.h)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _blobs(n, d, k, std=1.0):
    x, _ = orc.make_blobs_rows(0, n, d, k, 3, std=std)
    x = np.ascontiguousarray(x, dtype=np.float64)
    x.setflags(write=False)
    return x


def _c0(d, k):
    from dislib_amd.cluster.kmeans import _init_centers
    return np.array(_init_centers(d, False, k, 0), dtype=np.float64)


def _set_frac(monkeypatch, frac):
    if frac is None:
        monkeypatch.delenv("DKM_BOUNDS_LIST_FRAC", raising=False)
    else:
        monkeypatch.setenv("DKM_BOUNDS_LIST_FRAC", frac)


def _expect_list(frac, act, n):
    """Does a pass that left ``act`` of n rows active take the list form?
    (list form iff act <= floor(n frac): bounds_list_cap)"""
    f = DEFAULT_FRAC if frac is None else float(frac)
    return act <= int(n * f)


def _lloyd(x, C0, mode="auto"):
    """test_gpu_bounds._lloyd with the bounds on, and the screen's mode."""
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


class _Checker:
    """One `_Lloyd` fit with bounds on; ``assign()`` runs one assignment and
    checks everything the call left behind."""

    def __init__(self, x, C0, frac, tight=True, pass_tight=True, name="",
                 mode="auto"):
        self.st = _lloyd(x, C0, mode)
        assert self.st.bounding, "the shape keeps no bounds"
        self.n, self.d = x.shape
        self.k = C0.shape[0]
        self.frac = frac
        self.tight, self.pass_tight = tight, pass_tight
        self.name = name
        self.f32 = x.dtype == np.float32
        self.xs = self.st.dd.X.cpu().numpy()        # as stored
        assert self.xs.dtype == x.dtype
        self.C_prev = None      # the centres of the last bounds call
        self.cnt = (0, 0, 0, 0)
        self.kinds = []         # per assign: full / delta / init / list / image
        self.zero_active = 0
        self.moved = []
        self.last = None

    def reload_x(self):
        self.xs = self.st.dd.X.cpu().numpy()

    def _bounds(self):
        b = self.st.bounds[:, :self.n].cpu().numpy()
        return b[0].copy(), b[1].copy()

    def assign(self):
        st, n = self.st, self.n
        what = "%s frac=%s call %d" % (self.name, self.frac, len(self.kinds))
        C = st.C.cpu().numpy().copy()
        lab0 = st.labels[:n].cpu().numpy().copy()
        had = st.bounds is not None and st.bounds_valid
        ub0, lb0 = self._bounds() if had else (None, None)
        st.assign()
        lab = st.labels[:n].cpu().numpy().copy()
        self.moved.append(float(np.mean(lab != lab0)))
        with np.errstate(invalid="ignore"):
            ref = orc.partial_sum(self.xs, C)[0]
        assert np.array_equal(lab, ref), what
        cnt = st.bounds_counters()
        if not st.bounds_valid:                 # no bounds call
            assert cnt == self.cnt, what
            self.kinds.append("full" if st._full() else "delta")
            self.C_prev = None
            return None
        ub, lb = self._bounds()
        D = br.exact_distances(self.xs, C)
        if not had:
            # an init call: no bounds pass, every row screened from the image
            assert cnt == self.cnt, (what, cnt, self.cnt)
            kind = "init"
            screened = np.ones(n, bool)
            settled = np.zeros(n, bool)
        else:
            assert cnt[0] == self.cnt[0] + 1, (what, cnt, self.cnt)
            act = cnt[1] - self.cnt[1]
            assert cnt[2] - self.cnt[2] == n - act, (what, cnt, self.cnt)
            listed = cnt[3] - self.cnt[3]
            assert listed == int(_expect_list(self.frac, act, n)), \
                (what, act, cnt, self.cnt)
            self.zero_active += act == 0
            kind = "list" if listed else "image"
            # the pass on the host: the same rows active
            lo, hi = br.drift_f32(self.C_prev, C)
            _, _, a_lo = br.pass_f32(ub0, lb0, lab0, lo)
            _, _, a_hi = br.pass_f32(ub0, lb0, lab0, hi)
            assert min(a_lo.sum(), a_hi.sum()) <= act <= \
                max(a_lo.sum(), a_hi.sum()), (what, act, a_lo.sum(),
                                              a_hi.sum())
            if listed:
                screened = a_lo & a_hi
                settled = ~a_lo & ~a_hi
                assert np.array_equal(lab[settled], lab0[settled]), what
            else:
                screened = np.ones(n, bool)
                settled = np.zeros(n, bool)
        form = "%s (%s form)" % (what, kind)
        br.check_valid(ub, lb, lab, D, form)
        decided = -1
        if self.tight:
            slack = br.screen_slack(self.xs, C, self.d, self.f32)
            decided = br.check_screen_tight(ub, lb, lab, D, slack, screened,
                                            form)
        if self.pass_tight and settled.any():
            lim = br.pass_model(ub0, lb0, lab0, self.C_prev, C)
            br.check_pass_tight(ub, lb, lim, settled, lab0, form)
        print("%s: screened %d decided %d settled %d moved %.4f"
              % (form, screened.sum(), decided, settled.sum(),
                 self.moved[-1]))
        self.kinds.append(kind)
        self.cnt = cnt
        self.C_prev = C
        self.last = dict(ub0=ub0, lb0=lb0, ub=ub, lb=lb, lab0=lab0, lab=lab,
                         settled=settled, screened=screened, D=D, C=C)
        return self.last

    def finish(self):
        self.st.reduce_update()
        self.st.read_flags()

    def check_forms(self):
        """Both forms have provably run: with DKM_BOUNDS_LIST_FRAC = 1 every
        pass took the list form; with 0 none did (but a pass that left no
        row active, which the list form of 0 rows serves)."""
        passes = sum(k in ("list", "image") for k in self.kinds)
        assert self.cnt[0] == passes
        if self.frac == "1":
            assert self.cnt[3] == passes, (self.cnt, self.kinds)
        elif self.frac == "0":
            assert self.cnt[3] == self.zero_active, (self.cnt, self.kinds)


def _fit(x, k, frac, monkeypatch, iters=ITERS, C0=None, before=None,
         refresh=None, **kw):
    _set_frac(monkeypatch, frac)
    ck = _Checker(x, _c0(x.shape[1], k) if C0 is None else C0, frac, **kw)
    if refresh is not None:
        ck.st.refresh = refresh
    for it in range(iters):
        if before is not None:
            before(ck, it)
        ck.assign()
        ck.finish()
    ck.check_forms()
    print(ck.name, frac, ck.kinds, ck.cnt)
    return ck


def _assert_passes(ck, iters=ITERS):
    assert ck.kinds[:3] == ["full", "full", "init"], ck.kinds
    assert all(k in ("list", "image") for k in ck.kinds[3:]), ck.kinds
    assert ck.cnt[0] == iters - 3


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("frac", ["1", "0", None])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_blobs(dtype, frac, monkeypatch):
    """The headline arithmetic: (20000, 32, 100), std 1."""
    x = np.ascontiguousarray(_blobs(20000, 32, 100).astype(dtype))
    ck = _fit(x, 100, frac, monkeypatch, name="blobs")
    _assert_passes(ck)
    if frac is None:
        assert "list" in ck.kinds, ck.kinds


@pytest.mark.parametrize("frac", ["1", "0"])
@pytest.mark.parametrize("n,d,k,std", [(20000, 32, 100, 4.0),
                                       (9001, 17, 37, 3.0)])
def test_overlap(n, d, k, std, frac, monkeypatch):
    """Rows that move during bounds iterations (the ``so = r2`` branch), a
    ragged tail, element-wise list loads.  At each of iterations 2-5 at
    least 0.5 % of the rows change label (the CPU oracle gives 24 / 9.0 /
    4.9 / 1.0 % and 20 / 6.0 / 3.1 / 1.1 %), else the case does not exercise
    the branch."""
    ck = _fit(_blobs(n, d, k, std), k, frac, monkeypatch, name="overlap")
    _assert_passes(ck)
    for it in range(2, 6):
        assert ck.moved[it] >= 0.005, (it, ck.moved)


@pytest.mark.parametrize("frac", ["1", "0"])
@pytest.mark.parametrize("n,d,k,mode", [(2051, 1, 2, "auto"),
                                        (4099, 8, 10, "auto"),
                                        (8192, 32, 192, "auto"),
                                        (8192, 8, 256, "bf16x3")])
def test_small(n, d, k, mode, frac, monkeypatch):
    """The edges of dkm_bounds_ok (d = 1, k = 2; k = 192 at d = 32, the most
    whose sums fit LDS beside the centres; k = 256 at d = 8), and a last
    group of fewer than 4 rows in the bounds pass (n % 4 = 3).  With k = 256
    the auto mode takes the single-product screen with the label-sorted
    image, which keeps no bounds: that shape runs in mode "bf16x3"."""
    ck = _fit(_blobs(n, d, k), k, frac, monkeypatch, name="small", mode=mode)
    _assert_passes(ck)


def test_k256_d32_bf16x3_fits_without_bounds():
    """(8192, 32, 256) in mode "bf16x3": dkm_bounds_ok used to accept the
    shape and dkm_assign_delta_bounds_* to refuse it (its delta calls take
    their sums from the labels and list no moved rows), so the fit raised at
    iteration 2.  It now keeps no bounds and labels like the oracle."""
    n, d, k = 8192, 32, 256
    x = _blobs(n, d, k)
    st = _lloyd(x, _c0(d, k), "bf16x3")
    assert not st.bounding
    for _ in range(5):
        C = st.C.cpu().numpy().copy()
        st.step()
        lab = st.labels[:n].cpu().numpy()
        assert np.array_equal(lab, orc.partial_sum(x, C)[0])
    assert st.bounds is None and st.bounds_counters() == (0, 0, 0, 0)


@pytest.mark.parametrize("frac", ["1", "0"])
@pytest.mark.parametrize("case", ["plus1000", "times2^20", "times2^-20"])
def test_shifted(case, frac, monkeypatch):
    """Cancellation in ``xx + score``: the bounds may be loose but must be
    valid (check_valid, labels, and the pass model).  The shifted data meet
    the usual initial centres in [0, 1); the scaled data meet those centres
    scaled alike, so that the fit is the blobs fit at another exponent."""
    x = _blobs(20000, 32, 100)
    C0 = _c0(32, 100)
    if case == "plus1000":
        x = x + 1000.0
    else:
        s = 2.0 ** (20 if case == "times2^20" else -20)
        x, C0 = x * s, C0 * s
    ck = _fit(np.ascontiguousarray(x), 100, frac, monkeypatch, C0=C0,
              tight=False, name=case)
    _assert_passes(ck)


@pytest.mark.parametrize("frac", ["1", "0"])
def test_tiny(frac, monkeypatch):
    """blobs x 1e-30: the fp32 squares underflow.  Valid bounds and the
    oracle's labels only."""
    x = np.ascontiguousarray(_blobs(20000, 32, 100) * 1e-30)
    ck = _fit(x, 100, frac, monkeypatch, tight=False, pass_tight=False,
              name="tiny")
    _assert_passes(ck)


@pytest.mark.parametrize("frac", ["1", "0"])
def test_outliers(frac, monkeypatch):
    """|x| >> cm and distance 0: 16 rows of the blobs times 1e6, and 16 rows
    that are, at every assignment, bit for bit the current centres 0-15.

    The library treats the samples as immutable (the split image is built
    once), so the test that rewrites 16 rows before an assignment also
    rebuilds the image from X (dkm_x_image_f64) and declares the bounds of
    those rows unknown, (+inf, 0): they were bounds of other samples."""
    from dislib_amd import _lib
    from dislib_amd._device import ptr, stream_ptr
    x = _blobs(20000, 32, 100).copy()
    far = np.arange(100, 116)
    on = np.arange(200, 216)
    x[far] *= 1e6

    def before(ck, it):
        st = ck.st
        dd = st.dd
        with st._on():
            dd.X[torch.from_numpy(on).to(dd.X.device)] = st.C[:16]
            img = dd.images.get(_lib.IMAGE_SPLIT)
            if img is not None and _lib.IMAGE_SPLIT not in dd._unbuilt:
                _lib.check(_lib.lib().dkm_x_image_f64(
                    ptr(dd.X), dd.n, dd.d, dd.X.stride(0), _lib.IMAGE_SPLIT,
                    ptr(img), img.numel(), stream_ptr()), "dkm_x_image_f64")
            if st.bounds is not None:
                st.bounds[0, on[0]:on[-1] + 1] = float("inf")
                st.bounds[1, on[0]:on[-1] + 1] = 0.0
        ck.reload_x()
        assert np.array_equal(ck.xs[on], st.C[:16].cpu().numpy())

    ck = _fit(x, 100, frac, monkeypatch, before=before, name="outliers")
    _assert_passes(ck)
    r = ck.last
    assert np.all(r["D"][on, np.arange(16)] == 0)
    assert np.array_equal(r["lab"][on], np.arange(16))


# ---------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v)


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_drift_is_charged_to_the_right_rows(case, monkeypatch):
    """``k_drift`` and the d1 / d2 choice of ``k_bounds_pass``: five steps,
    then the centres are edited on the host before one assignment (the list
    form, so that the settled rows keep what the pass wrote).

    a: centre 3 jumps to 0.25 from centre 40.  Rows of 40 charged the second
       largest drift would keep an lb far above their distance to centre 3.
    b: centres 3 and 77 move by 5 and by 4: rows of 3 lose 4 of their lb,
       rows of 77 and all others 5; rows of 3 gain 5 on ub, rows of 77 gain 4.
    c: every centre moves by the same vector of length 2.
    Then a second assignment under the same centres: the drift is 0 and the
    settled rows' bounds change by the 2^-22 factors only."""
    n, d, k = 20000, 32, 100
    _set_frac(monkeypatch, "1")
    ck = _Checker(_blobs(n, d, k), _c0(d, k), "1", name="drift " + case)
    for _ in range(5):
        ck.assign()
        ck.finish()
    assert ck.kinds == ["full", "full", "init", "list", "list"]
    st = ck.st
    C = st.C.cpu().numpy().copy()
    lab = st.labels[:n].cpu().numpy()
    for c in (3, 40, 77):
        assert np.sum(lab == c) >= 50, (c, np.sum(lab == c))
    rng = np.random.RandomState(11)
    if case == "a":
        C[3] = C[40] + 0.25 * _unit(C[3] - C[40])
    elif case == "b":
        C[3] += 5.0 * _unit(rng.standard_normal(d))
        C[77] += 4.0 * _unit(rng.standard_normal(d))
    else:
        C += 2.0 * _unit(rng.standard_normal(d))
    st.C.copy_(torch.from_numpy(C))
    delta = br.drift_exact(ck.C_prev, C)    # since the last bounds call
    r = ck.assign()
    assert ck.kinds[-1] == "list"
    s, l0 = r["settled"], r["lab0"]
    du = r["ub"].astype(np.float64) - r["ub0"]
    dl = r["lb0"].astype(np.float64) - r["lb"]
    rest = np.delete(delta, [3, 77])
    if case == "a":
        # the rows of 40 cannot have stayed settled (their lb fell by the
        # jump of centre 3, about the distance 3-40): they were re-screened
        # and check_valid above held their new lb against the new centre 3
        assert delta[3] > 10 * rest.max()
        assert not np.any(s & (l0 == 40))
    elif case == "b":
        # (the centres also moved by the update of iteration 4: up to 0.5)
        assert delta[3] > delta[77] + 0.25 > rest.max() + 0.5, \
            (delta[3], delta[77], rest.max())
        m3, m77 = s & (l0 == 3), s & (l0 == 77)
        other = s & (l0 != 3) & (l0 != 77)
        for m in (m3, m77, other):
            assert m.sum() >= 25, m.sum()
        # (check_pass_tight held both sides; in plain figures:) rows of 3 pay
        # their own drift on ub and the SECOND largest on lb
        assert np.all(du[m3] >= delta[3])
        assert np.all(dl[m3] >= delta[77]) and np.all(dl[m3] < delta[3])
        assert np.all(du[m77] >= delta[77]) and np.all(du[m77] < delta[3])
        assert np.all(dl[m77] >= delta[3])
        assert np.all(dl[other] >= delta[3])
        assert np.all(du[other] < delta[77])
    else:
        assert np.all(delta > 1.4) and np.all(delta < 2.6), delta
        assert s.sum() >= 0.5 * n, s.sum()
        assert np.all(du[s] >= delta[l0[s]])
        assert np.all(dl[s] >= np.sort(delta)[-2])
    # a second assignment, centres untouched
    r2 = ck.assign()
    assert ck.kinds[-1] == "list"
    s2 = r2["settled"]
    assert s2.sum() > 0
    assert np.all(r2["ub"][s2] >= r2["ub0"][s2])
    assert np.all(r2["lb"][s2] <= r2["lb0"][s2])
    assert np.all(r2["ub"][s2] <= r2["ub0"][s2].astype(np.float64) *
                  (1 + 2.0 ** -21))
    assert np.all(r2["lb"][s2] >= r2["lb0"][s2].astype(np.float64) *
                  (1 - 2.0 ** -21))


@pytest.mark.parametrize("frac", ["1", "0"])
def test_full_pass_invalidates_the_bounds(frac, monkeypatch):
    """With refresh = 4 a full recomputation (iterations 4 and 8) falls
    between bounds iterations.  The call after it is an init call: no bounds
    pass is counted, every row is screened, and its bounds hold against the
    NEW centres (valid, and within the screen's slack: nothing stale
    survives).  The data overlap, so rows move at every iteration and the
    refresh is due."""
    n, d, k = 9001, 17, 37
    ck = _fit(_blobs(n, d, k, 3.0), k, frac, monkeypatch, iters=10,
              refresh=4, name="invalidate")
    assert ck.kinds[:3] == ["full", "full", "init"], ck.kinds
    assert ck.kinds[3] in ("list", "image") and ck.kinds[4] == "full", ck.kinds
    for i in range(3, len(ck.kinds) - 1):
        if ck.kinds[i] == "full":
            assert ck.kinds[i + 1] == "init", ck.kinds
    assert ck.kinds.count("init") >= 2 and ck.cnt[0] >= 2, ck.kinds
