"""Sequential numpy restatement of the reference's StandardScaler arithmetic
(dislib/preprocessing/classes.py:97-147), written out as the order the GPU
path reproduces: one chain per (Subset, column) in row order from +0.0, the
arity tree as left folds, numpy's dtype rules.  Not a test module.

tests/test_scaler_host.py pins it to the goldens (the reference's own
output) on the CPU; the GPU tests then use it as the oracle for shapes that
have no golden.  Needs n_features >= 2 (numpy sums one column pairwise).
"""
import numpy as np


def _work(samples):
    """The dtype the chains run in: the samples' for floats; integer sums
    are exact in int64 (and in the fp64 the GPU path holds them in)."""
    x = np.asarray(samples)
    if np.issubdtype(x.dtype, np.integer):
        return x.astype(np.int64)
    return x


def chain(rows):
    """Column sums of a 2-d array as sequential chains in row order, every
    add rounded in the array's dtype (np.sum(rows, axis=0) for d >= 2)."""
    rows = np.asarray(rows)
    acc = np.zeros(rows.shape[1], dtype=rows.dtype)
    for r in rows:
        acc = acc + r
    return acc


def tree(partials, arity, fold):
    """The reference's reduction loop (classes.py:97-111): pop the first
    ``arity`` partials, fold them left to right, append the result."""
    partials = list(partials)
    if len(partials) > 1 and arity < 2:
        raise ValueError("arity < 2 never terminates")
    while len(partials) > 1:
        group, partials = partials[:arity], partials[arity:]
        partials.append(fold(group))
    return partials[0]


def _fold_sums(group):
    s, n = group[0]
    for p, m in group[1:]:
        s, n = s + p, n + m
    return s, n


def _fold_vars(group):
    s = group[0]
    for p in group[1:]:
        s = s + p
    return s


def fit(subsets, arity=50):
    """(mean_, var_) of a list of 2-d sample arrays."""
    xs = [_work(s) for s in subsets]
    assert xs[0].shape[1] >= 2
    total, n = tree([(chain(x), x.shape[0]) for x in xs], arity, _fold_sums)
    with np.errstate(all="ignore"):
        mean = total / n
        var = tree([chain((x - mean) ** 2) for x in xs], arity, _fold_vars)
        return mean, var / n


def transform(subsets, mean, var):
    with np.errstate(all="ignore"):
        return [(np.asarray(s) - mean) / np.sqrt(var) for s in subsets]


def fit_fp64(x):
    """Plain fp64 numpy statistics of a matrix (the yardstick of the fast
    mode on fp32 samples)."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=0)
    return mean, ((x - mean) ** 2).mean(axis=0)


def split(x, sizes):
    """Row blocks of ``x`` of the given sizes."""
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [x[a:b] for a, b in zip(off[:-1], off[1:])]


def blocks(n, size):
    """Subset sizes of ``load_data(x, subset_size=size)`` for n rows."""
    return [min(size, n - a) for a in range(0, n, size)]


# ---------------------------------------------------------------------------
# The inputs of the goldens s01 .. s07 (tests/golden/gen_golden_scaler.py
# runs the reference on them; the tests rebuild them and check their sha256).
# name -> list of (key, x, Subset sizes, arities)
# ---------------------------------------------------------------------------
S01_SIZES = [700, 0, 1, 1300, 50, 2100, 849]
S01_OFFSET = np.array([0.0, 5.0, -10.0, 20.0, 1.0, -3.0, 8.0])


def golden_path(name):
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                        name + ".npz")


def _stored(name, key):
    with np.load(golden_path(name), allow_pickle=False) as z:
        return z[key]


def inputs(name):
    from sklearn.datasets import make_blobs
    if name in ("s01", "s07"):
        x, _ = make_blobs(n_samples=5000, n_features=7, centers=3,
                          random_state=21)
        return [("", x + S01_OFFSET, S01_SIZES, (50,))]
    if name == "s02":
        x = _stored("f13_arity", "x")
        return [("", x, blocks(len(x), 50), (50, 2))]
    if name == "s03":
        x = _stored("f10_fp32", "x")
        return [("", x, blocks(len(x), 500), (50,))]
    if name == "s04":
        x = np.random.RandomState(4).randint(-50, 50, (300, 5))
        return [("", x, blocks(300, 64), (50,))]
    if name == "s05":
        x = np.random.RandomState(5).standard_normal((40, 5))
        x[:, 2] = 3.5                                  # 0 / 0
        x[:, 3] = 1e-170 * (1 - 2 * (np.arange(40) % 2))   # x / 0
        return [("a_", x, blocks(40, 16), (50,)),
                ("b_", np.array([[1.0, 2.0, 3.0]]), [1], (50,))]
    if name == "s06":
        rs = np.random.RandomState(6)
        a = rs.standard_normal((3000, 130)) * 3.0 + 2.0
        b = rs.standard_normal((3000, 33)) * 0.5 - 1.0
        return [("a_", a, blocks(3000, 1000), (50,)),
                ("b_", b, blocks(3000, 1000), (50,))]
    raise KeyError(name)


def s07_input():
    """The fp32 Dataset that s07 transforms with s01's fp64 statistics."""
    x = np.random.RandomState(7).standard_normal((257, 7)) * 5.0
    return x.astype(np.float32), blocks(257, 100)
