"""Per-row distance bounds in the d <= 32 Lloyd loop.

A fit that keeps Hamerly's pair of bounds per row (``kmeans.BOUNDS``) must
label every row exactly like the fit without them: a row is skipped only
when its upper bound to its own centre is strictly below its lower bound to
every other centre, and every other row goes through the screen and the
exact re-check as before.  The tests run the same `_Lloyd` loop with the
bounds on and off, compare the labels of every iteration bit for bit with
each other and with the oracle's ``partial_sum`` under the device's centres
of that iteration, and read ``dkm_bounds_counters`` so that they cannot pass
with the path idle.

Data: ``oracle.kmeans_oracle.make_blobs_rows``; initial centres:
``_init_centers``.  The bounds pass first runs at iteration 3: iterations 0
and 1 recompute in full, iteration 2 is the first hinted image screen and
writes the first bounds.

(30001, 17, 37) has a ragged last tile and rows that are not 16-B pieces:
the image screen takes any d <= 32, and the list form then reads its rows
element by element.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from oracle import kmeans_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ITERS = 12
SHAPES = [(40000, 32, 100, np.float64), (30001, 17, 37, np.float64),
          (20000, 8, 10, np.float64), (40000, 32, 100, np.float32)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _data(n, d, k, dtype=np.float64, seed=3):
    x, _ = orc.make_blobs_rows(0, n, d, k, seed)
    return np.ascontiguousarray(x.astype(dtype))


def _lloyd(x, C0, bounds):
    from dislib_amd.cluster import kmeans as km
    from dislib_amd.data import load_data
    old = km.BOUNDS
    km.BOUNDS = bounds
    try:
        ds = load_data(x, subset_size=max(1, x.shape[0]))
        return km._Lloyd(ds, np.array(C0, dtype=np.float64), 0.0, True)
    finally:
        km.BOUNDS = old


def _run(x, k, iters, bounds, seed=0):
    """[(centres before, labels after, counters)] per iteration, final state
    and centres."""
    from dislib_amd.cluster.kmeans import _init_centers
    st = _lloyd(x, _init_centers(x.shape[1], False, k, seed), bounds)
    n = x.shape[0]
    trace = []
    for _ in range(iters):
        c = st.C.cpu().numpy().copy()
        st.assign()
        lab = st.labels[:n].cpu().numpy().copy()
        trace.append((c, lab, st.bounds_counters()))
        st.reduce_update()
        st.read_flags()
    return trace, st.state.cpu().numpy(), st.centers_host()


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))


@pytest.mark.parametrize("n,d,k,dtype", SHAPES)
def test_fit_parity_bounds_on_off(n, d, k, dtype):
    x = _data(n, d, k, dtype)
    on, s_on, c_on = _run(x, k, ITERS, True)
    off, s_off, c_off = _run(x, k, ITERS, False)
    for it in range(ITERS):
        assert np.array_equal(on[it][1], off[it][1]), it
        ref = orc.partial_sum(x, on[it][0])[0]
        assert np.array_equal(on[it][1], ref), it
    print("state rel", _rel(s_on, s_off), "centres rel", _rel(c_on, c_off))
    assert _rel(s_on, s_off) <= 1e-12
    assert _rel(c_on, c_off) <= 1e-12
    # an oracle Lloyd loop on the host.  fp64: 1e-9.  fp32 samples: the
    # reference adds each cluster's rows in fp32 in sample order while the
    # device adds them in fp64 and rounds once, so a centre coordinate may
    # differ by the error of a sequential fp32 sum of m terms, at most
    # m 2^-24 max|x| (m: the largest cluster), plus one rounding of the
    # quotient; labels are pinned per iteration above
    C = np.array(on[0][0])
    for _ in range(ITERS):
        labs, sums, counts = orc.partial_sum(x, C)
        C = orc.recompute_centers(C.copy(), (sums, counts))
    tol = 1e-9
    if dtype == np.float32:
        m = int(np.bincount(labs).max())
        tol = (m + 2) * 2.0 ** -24 * float(np.abs(x).max())
    print("oracle loop rel", _rel(c_on, C), "tol", tol)
    assert _rel(c_on, C) <= tol
    # the path ran: no bounds pass without bounds, one per iteration from
    # iteration 3 on, and at iterations 8-11 it skipped >= 80 % of the rows
    assert off[-1][2] == (0, 0, 0, 0)
    cnt = [t[2] for t in on]
    print("counters", cnt)
    for it in range(3, ITERS):
        assert cnt[it][0] == it - 2, (it, cnt[it])
    for it in range(8, ITERS):
        skipped = cnt[it][2] - cnt[it - 1][2]
        assert skipped >= 0.8 * n, (it, skipped)


def test_near_ties_and_duplicates():
    """Two bit-identical centres and a block of rows exactly on the bisector
    of two others, kept so at EVERY iteration: the centres 2 = 5, 7 = A and
    9 = B are put back before each assignment (the update would move them),
    so the bounds pass and the list screen of iterations 3-5 face the ties.
    Labels are the oracle's (first index on ties); the tied rows -- the
    bisector rows and every row of cluster 2, whose twin is exactly as near
    -- never satisfy ub < lb and are counted active."""
    n, d, k = 4096, 32, 16
    x = _data(n, d, k)
    from dislib_amd.cluster.kmeans import _init_centers
    C0 = _init_centers(d, False, k, 0) * 8.0 - 4.0
    # A, B: dyadic, away from the blobs' box, 2 apart in feature 0; the tie
    # rows: their midpoint plus dyadic steps in feature 1 (orthogonal)
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
    res = {}
    for b in (True, False):
        st = _lloyd(x, pin(C0), b)
        labs = []
        prev = (0, 0, 0, 0)
        for it in range(6):
            c = pin(st.C.cpu().numpy())
            st.C.copy_(torch.from_numpy(c))
            st.assign()
            lab = st.labels[:n].cpu().numpy().copy()
            ref = orc.partial_sum(x, c)[0]
            assert np.array_equal(lab, ref), (b, it)
            assert np.all(lab[tie] == 7) and not np.any(lab == 5)
            tied = np.zeros(n, bool)
            tied[tie] = True
            tied |= lab == 2
            if b and it >= 2:
                # the bounds after this call: no tied row is settled
                ub = st.bounds[0][:n].cpu().numpy()
                lb = st.bounds[1][:n].cpu().numpy()
                assert not np.any(ub[tied] < lb[tied]), it
            if b and it >= 3:
                cnt = st.bounds_counters()
                assert cnt[0] == it - 2
                # (tied under the previous call's labels too: cluster 2
                # keeps its rows while the centres are pinned)
                assert cnt[1] - prev[1] >= int(tied.sum()), (it, cnt, prev)
                prev = cnt
            labs.append(lab)
            st.reduce_update()
            st.read_flags()
        res[b] = labs
    for a, b in zip(res[True], res[False]):
        assert np.array_equal(a, b)


def _assign_once(st):
    st.assign()
    return st.labels[:st.dd.n].cpu().numpy().copy()


@pytest.mark.parametrize("case", ["far", "nan", "xinf"])
def test_drift_comes_from_the_library(case):
    n, d, k = 40000, 32, 100
    x = _data(n, d, k)
    if case == "xinf":
        x[123, 4] = np.inf
    out = {}
    for b in (True, False):
        from dislib_amd.cluster.kmeans import _init_centers
        st = _lloyd(x, _init_centers(d, False, k, 0), b)
        for _ in range(5):
            st.step()
        C = st.C.cpu().numpy().copy()
        if case == "far":
            C[[3, 40, 77]] += 50.0
        elif case == "nan":
            C[11, 2] = np.nan
        st.C.copy_(torch.from_numpy(C))
        lab = _assign_once(st)
        out[b] = (lab, C, st.bounds_counters())
    assert np.array_equal(out[True][0], out[False][0])
    assert out[True][2][0] == 3            # bounds passes at iterations 3-5
    with np.errstate(invalid="ignore"):
        ref = orc.partial_sum(x, out[True][1])[0]
    assert np.array_equal(out[True][0], ref)


@pytest.mark.parametrize("n", [0, 31])
def test_empty_and_tiny_shards(n):
    d, k = 32, 10
    x = _data(max(n, 1), d, k)[:n]
    tr_on, s_on, c_on = _run(x, k, 6, True)
    tr_off, s_off, c_off = _run(x, k, 6, False)
    for a, b in zip(tr_on, tr_off):
        assert np.array_equal(a[1], b[1])
        if n:
            assert np.array_equal(a[1], orc.partial_sum(x, a[0])[0])
    assert np.array_equal(c_on, c_off)
    if n:
        assert tr_on[-1][2][0] == 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("case", ["ragged", "empty"])
def test_world2_equals_single_rank(case, tmp_path):
    """Two ranks on cuda:0 (gloo), bounds on: the bounds are rank-local and
    the drift comes from the all-reduced centres every rank holds, so the
    labels (concatenated in rank order) equal the single-rank fit's bit for
    bit and the centres agree within the rounding of the split sums.  Every
    rank that owns rows ran its own bounds pass from iteration 3 on; in
    "empty" one rank owns none and still joins every all-reduce."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bounds_dist_worker as w
    out = str(tmp_path / case)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "bounds_dist_worker.py"), "--case",
           case, "--out", out]
    r = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rs = [dict(np.load("%s.%d.npz" % (out, i))) for i in range(2)]
    x = w.data(case)
    ds = w.dataset(case, x)
    cen, st = w.fit(case, ds)
    iters = w.CASES[case][2]
    assert st.bounding and st.bounds_counters()[0] == iters - 3
    assert sum(int(r_["nrows"]) for r_ in rs) == x.shape[0]
    assert np.array_equal(np.concatenate([r_["labels"] for r_ in rs]),
                          ds.labels_int32())
    assert np.array_equal(rs[0]["centers"], rs[1]["centers"])
    print("centres rel", _rel(rs[0]["centers"], cen))
    assert _rel(rs[0]["centers"], cen) <= 1e-12
    for r_ in rs:
        if int(r_["nrows"]):
            assert bool(r_["bounding"])
            c = tuple(int(v) for v in r_["counters"])
            assert c[0] == iters - 3, c
            assert c[1] + c[2] == c[0] * int(r_["nrows"]), c
    if case == "empty":
        assert sorted(int(r_["nrows"]) for r_ in rs) == [0, x.shape[0]]
