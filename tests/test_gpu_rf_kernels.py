"""GPU tests of the ``dkm_rf.hip`` kernels against the numpy restatement
``tests/rf_ref.py``: the split search in both regimes (score bits, position
and ranks equal, no tolerance), best of a node, partition and predict."""
import numpy as np
import pytest

from dislib_amd import _lib
from dislib_amd.classification import rf
from tests import rf_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
B = _lib.RF_LDS_MAX
NODE = 5


def _state(cols, y, w, inside):
    """One tree over the samples of ``cols`` (n, d) drawn ``w`` times each;
    the node NODE holds the samples of ``inside``, the others sit in node 9."""
    dev = torch.device("cuda")
    n = len(y)
    prep = rf.Prepared(torch.from_numpy(np.ascontiguousarray(cols)).to(dev),
                       y)
    mem = np.repeat(np.flatnonzero(inside), w[inside])
    b = rf.Batch(prep, [np.repeat(np.arange(n), w)])
    b.node_of = rf._i32(np.where(w == 0, -1, np.where(inside, NODE, 9)), dev)
    # the node's segment starts at 3; what lies around it is never read
    b.members = rf._i32(np.concatenate(([0] * 3, mem, [0] * n)), dev)
    b.spare = torch.zeros_like(b.members)
    return prep, b, mem


def _check(v, y, C, w=None, inside=None):
    n = len(y)
    w = np.ones(n, dtype=np.int64) if w is None else w
    inside = np.ones(n, dtype=bool) if inside is None else inside
    inside = inside & (w > 0)
    prep, b, mem = _state(np.asarray(v, dtype=np.float64)[:, None], y, w,
                          inside)
    size = len(mem)
    score, pos, lo, hi = rf_ref.split(np.asarray(v)[mem], y[mem], C)
    dist = np.unique(np.asarray(v, dtype=np.float64))
    nodes = rf._i32([[0, 3, size, NODE]], "cuda")
    ncounts = rf._i32([np.bincount(y[mem], minlength=C)], "cuda")
    pairs = rf._i32([[0, 0]], "cuda")
    modes = [_lib.RF_STREAM, _lib.RF_AUTO] + ([_lib.RF_LDS] if size <= B
                                              else [])
    for mode in modes:
        s, cut = rf.split_search(_lib.lib(), prep, C, b, nodes, ncounts,
                                 pairs, size, mode)
        s, cut = s.cpu().numpy(), cut.cpu().numpy()[0]
        assert s[0].tobytes() == np.float64(score).tobytes(), (mode, s, score)
        assert cut[0] == pos, (mode, cut, pos)
        if pos < size - 1:
            assert (dist[cut[1]], dist[cut[2]]) == (lo, hi), mode


@pytest.mark.parametrize("C", [2, 3, 32])
@pytest.mark.parametrize("size", [1, 2, 3, 63, 64, 65, 257, B - 1, B, B + 1])
def test_split_sizes(size, C):
    """Random ties, bootstrap multiplicities up to 3 and a node scattered
    over a larger tree; the streamed walk has tile edges inside."""
    rng = np.random.RandomState(size + C)
    n = size + 700
    w = rng.randint(0, 4, n)
    pick = rng.rand(n) < 0.6
    cum = np.cumsum(np.where(pick, w, 0))
    inside = pick & (cum <= size)
    short = size - int(w[inside].sum())
    if short:                              # top the node up to `size` exactly
        j = np.flatnonzero(~inside)[0]
        w[j], inside[j] = short, True
    v = rng.randint(0, size // 2 + 2, n).astype(np.float64)
    _check(v, rng.randint(0, C, n), C, w, inside)


def _special(name):
    rng = np.random.RandomState(11)
    n = 4000                  # the streamed walk flushes its buffer at 1792
    y = rng.randint(0, 3, n)
    if name == "constant":
        return np.full(n, 2.5), y
    if name == "distinct":
        return rng.permutation(n).astype(np.float64), y
    if name == "long_runs":            # runs longer than a thread's and a tile
        return np.repeat(np.arange(4.0), n // 4), y
    if name == "pure":
        return rng.rand(n), np.full(n, 1)
    if name == "equal_proportions":
        return np.repeat(np.arange(n // 2), 2).astype(np.float64), \
            np.tile([0, 1], n // 2)
    if name == "two_minima":
        v = np.repeat([0., 1., 2., 3.], n // 4)
        return v, (np.isin(v, [1., 2.])).astype(np.int64)
    if name == "signed_zero":
        return np.where(rng.rand(n) < 0.5, -0.0, 0.0) + \
            (rng.rand(n) < 0.3), y


@pytest.mark.parametrize("name", ["constant", "distinct", "long_runs",
                                  "pure", "equal_proportions", "two_minima",
                                  "signed_zero"])
def test_split_special(name):
    v, y = _special(name)
    _check(v, y, 3)


def test_best_partition():
    """Two equal features: the first drawn wins; the partition keeps the
    member multiset, orders it, counts the left classes and names the
    children in node_of; a node without a cut is copied."""
    rng = np.random.RandomState(3)
    n, C = 2500, 3
    v = rng.randint(0, 50, n).astype(np.float64)
    y = ((v > 20) ^ (rng.rand(n) < 0.1)).astype(np.int64) + (v > 40)
    w = rng.randint(0, 3, n)
    inside = rng.rand(n) < 0.7
    cols = np.stack((v, v, np.full(n, 1.0)), axis=1)
    prep, b, mem = _state(cols, y, w, inside & (w > 0))
    so = _lib.lib()
    size = len(mem)
    nodes = rf._i32([[0, 3, size, NODE], [0, 3, size, NODE]], "cuda")
    cnt = np.bincount(y[mem], minlength=C)
    ncounts = rf._i32([cnt, cnt], "cuda")
    pairs = rf._i32([[0, 2], [0, 1], [0, 0], [1, 2]], "cuda")
    pspan = rf._i32([[0, 3], [3, 1]], "cuda")
    score, cut = rf.split_search(so, prep, C, b, nodes, ncounts, pairs, size)
    best = rf.best_of_node(so, nodes, pspan, pairs, score, cut)
    bh = best.cpu().numpy()
    _, pos, lo, hi = rf_ref.split(v[mem], y[mem], C)
    assert list(bh[0]) == [1, lo, hi, pos + 1] and bh[1][0] == -1
    kids = rf._i32([[0, 3, size, 20]], "cuda")
    lc = rf.partition(so, prep, C, b, kids, best[:1]).cpu().numpy()[0]
    after = b.members.cpu().numpy()[3:3 + size]
    left = v[mem] <= lo
    assert np.array_equal(after[:pos + 1], mem[left])
    assert np.array_equal(after[pos + 1:], mem[~left])
    assert np.array_equal(lc, np.bincount(y[mem[left]], minlength=C))
    nof = b.node_of.cpu().numpy()
    ins = inside & (w > 0)
    assert np.array_equal(nof[ins], np.where(v[ins] <= lo, 20, 21))
    assert set(nof[~ins]) <= {-1, 9}
    lc0 = rf.partition(so, prep, C, b, kids, best[1:]).cpu().numpy()[0]
    assert not lc0.any()
    assert np.array_equal(b.members.cpu().numpy()[3:3 + size], after)


@pytest.mark.parametrize("dtype,stride", [(np.float64, 3), (np.float32, 3),
                                          (np.float64, 7)])
@pytest.mark.parametrize("hard", [False, True])
def test_predict_hand_built(dtype, stride, hard):
    """Three trees; rows on a threshold go left; strided fp32 / fp64 rows;
    a hard-vote tie goes to the class voted first."""
    f = rf.Forest(3)
    g = f.add_nodes([0, 0, 0, 0, 0, 1, 1, 1, 2])
    f.roots = np.array([0, 5, 8], dtype=np.int32)
    f.feature[[0, 1, 5]] = [0, 2, 1]
    f.value[[0, 1, 5]] = [0.5, -1.0, 2.0]
    f.child[[0, 1, 5]] = [[1, 2], [3, 4], [6, 7]]
    f.close(g[[2, 3, 4, 6, 7, 8]], np.array(
        [[0, 3, 1], [2, 0, 0], [1, 1, 5], [4, 1, 0], [0, 0, 2], [1, 2, 1]]))
    rows = np.array([[0.5, 9, -1.0], [0.5, 2.0, -0.5], [0.75, 2.5, 0],
                     [0.25, 0, -2], [1, 2, 3]] * 70, dtype=dtype)[:333]
    X = torch.zeros((len(rows), stride), dtype=torch.from_numpy(rows).dtype,
                    device="cuda")
    X[:, :3] = torch.from_numpy(rows).cuda()
    proba, labels = rf.forest_predict(_lib.lib(), X[:, :3], dtype ==
                                      np.float32, f, hard)
    p, soft, hv = rf_ref.predict([f.tree_arrays(i) for i in range(3)], rows, 3)
    assert np.array_equal(proba.cpu().numpy(), p)
    assert np.array_equal(labels.cpu().numpy(), hv if hard else soft)
