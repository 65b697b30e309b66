"""GPU tests of ``RandomForestClassifier``: whole fits against the numpy
restatement node for node, the re-draw, impure leaves, repeatability,
prediction, the refusals and the accuracy against the yardstick of
``rf_ref.npz``."""
import numpy as np
import pytest

from dislib_amd.classification import RandomForestClassifier, rf
from dislib_amd.data import Dataset, Subset
from tests import rf_ref
from tests.conftest import load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _dataset(x, y, sizes):
    ds = Dataset(n_features=x.shape[1])
    off = 0
    for s in sizes:
        ds.append(Subset(x[off:off + s], None if y is None else
                         y[off:off + s]))
        off += s
    return ds


def _data(dtype=np.float64):
    rng = np.random.RandomState(5)
    x = np.round(rng.randn(300, 5), 1).astype(dtype)     # ties inside
    y = (x[:, 0] + x[:, 3] > 0).astype(np.int64) + (x[:, 1] > 0.5) + 3
    y[rng.rand(300) < 0.05] = 4
    return x, y


def _same_trees(est, x, y, tf, depth, seed):
    C = len(est.classes)
    ref = rf_ref.forest(x, np.searchsorted(est.classes, y), C,
                        est.n_estimators, tf, depth, seed)
    for t, r in zip(est.trees, ref):
        for k in r:
            assert np.array_equal(t[k], r[k]), k
    return ref


@pytest.mark.parametrize("depth", [1, 3, np.inf])
@pytest.mark.parametrize("tf", [1, 'sqrt', None])
def test_fit_equals_the_restatement(tf, depth):
    x, y = _data()
    est = RandomForestClassifier(n_estimators=3, try_features=tf,
                                 max_depth=depth, random_state=1)
    est.fit(_dataset(x, y, [110, 190]))
    assert list(est.classes) == [3, 4, 5]
    _same_trees(est, x, y, est.try_features, depth, 1)


def test_predict_score_and_repeatability():
    x, y = _data(np.float32)
    probe = x[:120] + np.float32(0.05)
    for hard in (False, True):
        est = RandomForestClassifier(n_estimators=4, hard_vote=hard,
                                     random_state=2)
        est.fit(_dataset(x, y, [300]))
        ref = _same_trees(est, x, y, 2, np.inf, 2)
        again = RandomForestClassifier(n_estimators=4, random_state=2)
        again.fit(_dataset(x, y, [100, 200]))
        for a, b in zip(est.trees, again.trees):
            assert all(np.array_equal(a[k], b[k]) for k in a)
        p, soft, hv = rf_ref.predict(ref, probe, 3)
        want = est.classes[hv if hard else soft]
        ds = _dataset(probe, y[:120], [50, 70])
        assert est.score(ds) == np.mean(want == y[:120])
        est.predict(ds)
        assert np.array_equal(ds.labels, want)
        est.predict_proba(ds)
        assert np.array_equal(np.vstack([s.labels for s in ds]), p)


def test_impure_leaf():
    """Duplicated rows of different classes end in an impure leaf once all
    features are tried."""
    rng = np.random.RandomState(0)
    x = np.repeat(rng.randint(0, 3, (20, 3)).astype(np.float64), 2, axis=0)
    y = np.tile([0, 1], 20)
    est = RandomForestClassifier(n_estimators=2, try_features=1,
                                 random_state=0)
    est.fit(_dataset(x, y, [40]))
    _same_trees(est, x, y, 1, np.inf, 0)
    assert all((t["frequencies"] > 0).sum(axis=1).max() > 1
               for t in est.trees)


def test_redraw_after_a_constant_slice():
    """The feature the root draws first is constant: it finds no cut, draws
    again and splits on the other one."""
    rs = np.random.RandomState(4)
    seed = [rs.randint(np.iinfo(np.int32).max) for _ in range(2)][1]
    const = int(rf.feature_order([seed], [0], 2)[0, 0])
    x = np.random.RandomState(1).rand(60, 2)
    y = (x[:, 1 - const] > 0.5).astype(np.int64)
    x[:, const] = -0.0
    est = RandomForestClassifier(n_estimators=1, try_features=1,
                                 random_state=4)
    est.fit(_dataset(x, y, [60]))
    assert est.trees[0]["feature"][0] == 1 - const
    _same_trees(est, x, y, 1, np.inf, 4)


def test_refusals():
    x, y = _data()
    bad = x.copy()
    bad[7, 2] = np.nan
    with pytest.raises(ValueError, match="finite"):
        RandomForestClassifier().fit(_dataset(bad, y, [300]))
    with pytest.raises(ValueError, match="try_features"):
        RandomForestClassifier(try_features=9).fit(_dataset(x, y, [300]))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.cuda, "mem_get_info",
                   lambda *a: (rf.hbm_bytes(300, 5) + (4 << 30) - 1, 1 << 40))
        with pytest.raises(ValueError, match="HBM"):
            RandomForestClassifier().fit(_dataset(x, y, [300]))
    est = RandomForestClassifier(n_estimators=2, random_state=0)
    est.fit(_dataset(x, y, [300]))
    with pytest.raises(ValueError, match="features"):
        est.predict(_dataset(x[:, :4], None, [300]))


@pytest.mark.parametrize("seed", range(5))
def test_accuracy_against_the_yardstick(seed):
    """Probe accuracy >= the yardstick's mean - 3 standard deviations over
    its ten seeds (both from rf_ref.npz)."""
    from sklearn.datasets import make_classification
    g = load_golden("rf_ref")
    x, y = make_classification(1200, 12, n_informative=6, n_classes=3,
                               random_state=0)
    est = RandomForestClassifier(n_estimators=10, random_state=seed)
    est.fit(_dataset(x[:900], y[:900], [300, 300, 300]))
    acc = est.score(_dataset(x[900:], y[900:], [300]))
    print("rf accuracy seed", seed, acc, "yardstick", g["acc"].mean(),
          g["acc"].std())
    assert acc >= g["acc"].mean() - 3 * g["acc"].std()
