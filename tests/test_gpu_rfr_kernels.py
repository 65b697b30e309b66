"""GPU tests of the ``dkm_rfr.hip`` kernels against ``tests/rfr_ref.py``: the
split search in every regime, the node statistics and the prediction."""
from types import SimpleNamespace

import numpy as np
import pytest

from dislib_amd import _lib
from dislib_amd.classification import rf
from dislib_amd.regression import forest
from tests import rfr_ref
from tests.test_gpu_rf_kernels import NODE, _state

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
L, U, LD = _lib.RFR_LDS_MAX, 2.0 ** -53, np.longdouble


def _term(x, err, length):
    """Error bound of fl(x^ * x^ / length) for |x^ - x| <= err."""
    return (2 * abs(x) * err + err * err) / length + 3 * U * x * x / length


def _check(v, y, w=None, inside=None):
    """Integer-valued ``y``: everything equals the restatement.  Otherwise the
    bounds of DESIGN.md 3.26 in longdouble, err(SL), err(S) <= size u A."""
    n = len(y)
    v = np.asarray(v, dtype=np.float64)
    w = np.ones(n, dtype=np.int64) if w is None else w
    inside = (np.ones(n, dtype=bool) if inside is None else inside) & (w > 0)
    prep, b, mem = _state(v[:, None], np.zeros(n, np.int64), w, inside)
    yt = torch.from_numpy(np.asarray(y, dtype=np.float64)).cuda()
    size = len(mem)
    score, pos, lo, hi = rfr_ref.split(v[mem], y[mem])
    ref, _ = rfr_ref.scores(v[mem], y[mem], LD)
    ys = y[mem][np.argsort(v[mem], kind="stable")].astype(LD)
    dist = np.unique(v)
    nodes = rf._i32([[0, 3, size, NODE]], "cuda")
    nsum = torch.tensor([y[mem].sum()], dtype=torch.float64, device="cuda")
    for mode in [_lib.RF_STREAM, _lib.RF_AUTO] + ([_lib.RF_LDS] if size <= L
                                                  else []):
        s, cut = forest.split_search(_lib.lib(), prep, yt, b, nodes, nsum,
                                     rf._i32([[0, 0]], "cuda"), size, mode)
        s, cut = s.cpu().numpy()[0], cut.cpu().numpy()[0]
        if np.array_equal(y, np.round(y)):
            assert s.tobytes() == np.float64(score).tobytes(), (mode, s, score)
            assert cut[0] == pos, (mode, cut, pos)
            if pos < size - 1:
                assert (dist[cut[1]], dist[cut[2]]) == (lo, hi), mode
            continue
        p = int(cut[0])
        assert 0 <= p < size and np.isfinite(ref[p]), (mode, cut)
        SL, SR = ys[:p + 1].sum(), ys.sum() - ys[:p + 1].sum()
        e = size * U * np.abs(ys).sum()
        bound = _term(SL, e, p + 1) + _term(SR, 2 * e + U * abs(SR),
                                            max(size - p - 1, 1))
        print("mode", mode, "size", size, "err", float(abs(LD(s) - ref[p])),
              "gap", float(ref[p] - ref.min()), "bound", float(bound))
        assert abs(LD(s) - ref[p]) <= bound, mode
        assert ref[p] - ref.min() <= 2 * bound, mode


@pytest.mark.parametrize("kind", ["int", "randn", "1e6+randn"])
@pytest.mark.parametrize("size", [1, 2, 3, 63, 64, 65, 257, L - 1, L, L + 1])
def test_split_sizes(size, kind):
    """Ties, multiplicities 0..3, a node scattered over a larger tree."""
    rng = np.random.RandomState(size)
    n = size + 700
    w = rng.randint(0, 4, n)
    pick = rng.rand(n) < 0.6
    inside = pick & (np.cumsum(np.where(pick, w, 0)) <= size)
    short = size - int(w[inside].sum())
    if short:                              # top the node up to `size` exactly
        j = np.flatnonzero(~inside)[0]
        w[j], inside[j] = short, True
    v = rng.randint(0, size // 2 + 2, n).astype(np.float64)
    y = {"int": rng.randint(-50, 50, n).astype(np.float64),
         "randn": rng.randn(n), "1e6+randn": 1e6 + rng.randn(n)}[kind]
    _check(v, y, w, inside)


@pytest.mark.parametrize("name", ["constant", "distinct", "long_runs",
                                  "two_minima", "signed_zero"])
def test_split_special(name):
    """Integer targets; at 4000 entries the streamed buffer flushes."""
    rng = np.random.RandomState(11)
    n = 4000
    y = rng.randint(-50, 50, n).astype(np.float64)
    v = np.repeat(np.arange(4.0), n // 4)  # long_runs
    if name == "constant":                 # no cut
        v = np.full(n, 2.5)
    elif name == "distinct":
        v = rng.permutation(n).astype(np.float64)
    elif name == "two_minima":             # after runs 0 and 2: the last wins
        y = np.isin(v, [0., 3.]).astype(np.float64)
    elif name == "signed_zero":
        v = np.where(rng.rand(n) < 0.3, 1.0,
                     np.where(rng.rand(n) < 0.5, -0.0, 0.0))
    _check(v, y)


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("size", [1, 255, 256, 257, 5000])
def test_node_stats(size, kind):
    rng = np.random.RandomState(size)
    n = 6000
    y = rng.randint(-50, 50, n).astype(np.float64) if kind == "int" else \
        1e3 + rng.randn(n)
    mem = rng.randint(0, n, size)          # repeats: the multiplicities
    prep = SimpleNamespace(n=n, device=torch.device("cuda"))
    batch = SimpleNamespace(members=rf._i32(
        np.concatenate(([0] * 3, mem, [0] * n)), "cuda"))
    st = forest.node_stats(
        _lib.lib(), prep, torch.from_numpy(y).cuda(), batch,
        rf._i32([[0, 3, size, 0], [0, 3, 0, 0]], "cuda")).cpu().numpy()
    assert (st[0, 1], st[0, 2]) == (y[mem].min(), y[mem].max())
    assert list(st[1]) == [0.0, np.inf, -np.inf]
    err = abs(LD(st[0, 0]) - y[mem].astype(LD).sum())
    assert err <= (0 if kind == "int" else size * U * np.abs(y[mem]).sum())


@pytest.mark.parametrize("dtype,stride", [(np.float64, 3), (np.float32, 3),
                                          (np.float64, 7), (np.float32, 7)])
def test_predict_hand_built(dtype, stride):
    """Three trees; rows on a threshold go left; strided fp32 / fp64 rows."""
    f = forest.Forest()
    g = f.add_nodes([0, 0, 0, 0, 0, 1, 1, 1, 2])
    f.roots = np.array([0, 5, 8], dtype=np.int32)
    f.feature[[0, 1, 5]] = [0, 2, 1]
    f.value[[0, 1, 5]] = [0.5, -1.0, 2.0]
    f.child[[0, 1, 5]] = [[1, 2], [3, 4], [6, 7]]
    f.close(g[[2, 3, 4, 6, 7, 8]], np.array([0.1, 1e16, -7.3, 1.0, 2.5, 1e-3]),
            np.array([3, 1, 7, 5, 2, 4]))
    rows = np.array([[0.5, 9, -1.0], [0.5, 2.0, -0.5], [0.75, 2.5, 0],
                     [0.25, 0, -2], [1, 2, 3]] * 70, dtype=dtype)[:333]
    X = torch.zeros((len(rows), stride), dtype=torch.from_numpy(rows).dtype,
                    device="cuda")
    X[:, :3] = torch.from_numpy(rows).cuda()
    out = forest.forest_predict(_lib.lib(), X[:, :3], dtype == np.float32, f)
    want = rfr_ref.predict([f.tree_arrays(i) for i in range(3)], rows)
    assert out.cpu().numpy().tobytes() == want.tobytes()
