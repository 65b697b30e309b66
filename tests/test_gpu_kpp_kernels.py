"""GPU tests of the k-means++ entries of the C ABI (dkm_kpp.hip), one by one
against the longdouble restatement of tests/kpp_ref.py; X has ``ldx = d + 3``
with NaN in the padding and in two rows past n; u = 2^-53.  eval: every group
width, the 64-lane cap, one feature past an LDS chunk, two tiles per block,
each trial bucket and its edge; ``|dc - ref| <= (d + 4) u ref`` (one rounding
per difference and fma, a sum tree shallower than d, all terms >= 0)."""
import numpy as np
import pytest

from dislib_amd import _lib
from tests import kpp_ref
from tests.test_gpu_svm_kernels import _dev, _p, _stream

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
EVAL = sorted({(d, 65, 3) for d in (1, 2, 3, 5, 31, 32, 33, 64, 65, 513)} |
              {(33, n, 3) for n in (1, 2, 63, 64, 65, 1025)} |
              {(5, 65, L) for L in (1, 2, 3, 8, 9, 32)} | {(33, 8200, 17)})
DTYPES = [np.float64, np.float32]


def _xbuf(n, d, dtype, rng):
    buf = np.full((n + 2, d + 3), np.nan, dtype=dtype)
    buf[:n, :d] = rng.standard_normal((n, d)).astype(dtype)
    return _dev(buf), buf[:n, :d].astype(np.float64)


def _eval(X, n, d, dtype, trials, mind):
    so = _lib.lib()
    L = len(trials)
    nb = so.dkm_kpp_blocks(n, d, L)
    dc = torch.full((L, n + 2), 7.0, dtype=torch.float64, device="cuda")
    part = torch.full((nb, L), np.nan, dtype=torch.float64, device="cuda")
    tr, md = _dev(trials), None if mind is None else _dev(mind)
    fn = so.dkm_kpp_eval_f32 if dtype == np.float32 else so.dkm_kpp_eval_f64
    _lib.check(fn(_p(X), n, d, X.stride(0), _p(tr), L, _p(md), _p(dc), n + 2,
                  _p(part), _stream()), "eval")
    return dc.cpu().numpy(), part.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,n,L", EVAL)
def test_eval(d, n, L, dtype):
    rng = np.random.default_rng(1000 * d + n + L)
    X, xs = _xbuf(n, d, dtype, rng)
    trows = rng.integers(n, size=L)
    ref = np.stack([kpp_ref.sqdist(xs, xs[r]) for r in trows])
    mind = rng.random(n) * 2 * d
    for md in (mind, None):
        dc, part = _eval(X, n, d, dtype, xs[trows], md)
        again = _eval(X, n, d, dtype, xs[trows], md)
        assert dc.tobytes() == again[0].tobytes()
        assert part.tobytes() == again[1].tobytes()
        assert np.all(dc[:, n:] == 7.0)                  # ldc is honoured
        err = np.abs(dc[:, :n].astype(LD) - ref)
        assert np.all(err <= (d + 4) * U * ref), float((err / ref.max()).max())
        assert np.all(dc[np.arange(L), trows] == 0.0)
        pref = (ref if md is None else np.minimum(md, ref)).sum(axis=1)
        perr = np.abs(part.astype(LD).sum(axis=0) - pref)
        assert np.all(perr <= (n + d + 4) * U * pref)


def _commit(n, dc, part, rows, first, mind):
    so = _lib.lib()
    mind = mind.clone()
    bsum = torch.full(((n + 1023) // 1024,), np.nan, dtype=torch.float64,
                      device="cuda")
    pot = torch.zeros(1, dtype=torch.float64, device="cuda")
    best = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    index = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    _lib.check(so.dkm_kpp_commit(n, dc.shape[0], _p(dc), dc.stride(0),
                                 _p(part), part.shape[0], _p(rows), first,
                                 _p(mind), _p(bsum), _p(pot), _p(best),
                                 _p(index), _stream()), "commit")
    return (mind.cpu().numpy(), bsum.cpu().numpy(), pot.item(), best.item(),
            index.item())


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_commit(n):
    rng = np.random.default_rng(n)
    dc = rng.random((4, n + 2))
    part = rng.random((37, 4)) + 1.0
    part[:, 1] -= 0.5
    part[:, 2] = part[:, 1]                   # an exact tie: the first wins
    prev = rng.random(n)
    rows = np.array([n - 1, n // 2, 0, n // 3], dtype=np.int32)
    args = (n, _dev(dc), _dev(part), _dev(rows))
    for first in (0, 1):
        mind, bsum, pot, best, index = _commit(*args, first, _dev(prev))
        again = _commit(*args, first, _dev(prev))
        assert mind.tobytes() == again[0].tobytes()
        assert bsum.tobytes() == again[1].tobytes() and pot == again[2]
        assert best == 1 and index == rows[1]
        want = part[:, 1].astype(LD).sum()
        assert abs(pot - want) <= 37 * U * want
        new = dc[1, :n] if first else np.minimum(prev, dc[1, :n])
        assert mind.tobytes() == new.tobytes()
        for s in range(len(bsum)):
            seg = new[1024 * s:1024 * s + 1024].astype(LD).sum()
            assert abs(bsum[s] - seg) <= 1024 * U * seg


N_S = 5000
SAMPLE = {
    # leading zero rows, a whole zero segment, a zero last row
    "lead": (np.r_[0:7, 1024:2048, N_S - 1],
             [1e-4, 0.03, 0.21, 0.2605, 0.55, 0.97, 1 - 1e-7]),
    # a first row that is not zero: u = 0 lands on it
    "first": (np.r_[2048:3072, N_S - 1],
              [0.0, 0.11, 0.5, 0.8, 1 - 1e-7]),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(SAMPLE))
def test_sample(name, dtype):
    zeros, us = SAMPLE[name]
    rng = np.random.default_rng(11)
    n, d = N_S, 5
    mind = rng.random(n)
    mind[zeros] = 0.0
    mind[n - 2] = 0.9
    us = np.array(us)
    pot = float(mind.astype(LD).sum())
    want, cs = kpp_ref.sample(mind, us.astype(LD) * LD(pot))
    # a condition on the inputs: every target keeps the margin
    gap = np.abs(cs[:, None] - (us.astype(LD) * LD(pot))[None, :]).min()
    assert gap > 1e-9 * pot
    segs = set(want // 1024)              # first, a middle, the last segment
    assert {0, 4} <= segs and segs & {1, 2, 3} and (n - 2) in want
    X, xs = _xbuf(n, d, dtype, rng)
    nseg = (n + 1023) // 1024
    bsum = np.array([mind[1024 * s:1024 * s + 1024].sum()
                     for s in range(nseg)])
    so = _lib.lib()
    fn = so.dkm_kpp_sample_f32 if dtype == np.float32 else \
        so.dkm_kpp_sample_f64
    out = []
    for _ in range(2):
        L = len(us)
        rows = torch.full((L,), -1, dtype=torch.int32, device="cuda")
        tr = torch.full((L, d), np.nan, dtype=torch.float64, device="cuda")
        bscan = torch.empty(nseg, dtype=torch.float64, device="cuda")
        bufs = [_dev(mind), _dev(bsum), _dev(np.array([pot])), _dev(us)]
        _lib.check(fn(_p(X), n, d, X.stride(0), _p(bufs[0]), _p(bufs[1]),
                      _p(bscan), _p(bufs[2]), _p(bufs[3]), L, _p(rows),
                      _p(tr), _stream()), "sample")
        out.append((rows.cpu().numpy(), tr.cpu().numpy()))
    assert np.array_equal(out[0][0], want)
    assert out[0][1].tobytes() == xs[want].tobytes()
    assert out[0][0].tobytes() == out[1][0].tobytes()
    assert out[0][1].tobytes() == out[1][1].tobytes()
