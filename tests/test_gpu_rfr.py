"""GPU tests of ``RandomForestRegressor``: whole fits against the restatement
node for node, a constant target, refusals, R^2 against sklearn's forest."""
import numpy as np
import pytest

from dislib_amd import _lib
from dislib_amd.classification import rf
from dislib_amd.regression import RandomForestRegressor
from tests import rfr_ref
from tests.test_gpu_rf import _dataset

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _data(n, dtype=np.float64):
    rng = np.random.RandomState(5)
    x = np.round(rng.randn(n, 5), 1).astype(dtype)       # ties inside
    y = np.round(10 * (x[:, 0] + x[:, 3])) + 7 * (x[:, 1] > 0.5) + \
        rng.randint(-2, 3, n)
    return x, y.astype(np.int64)


@pytest.mark.parametrize("n,trees,tf,depth,dtype", [
    (600, 3, None, np.inf, np.float64), (600, 3, 2, np.inf, np.float64),
    (600, 3, 2, 3, np.float64), (600, 3, 2, np.inf, np.float32),
    (_lib.RFR_LDS_MAX + 300, 1, 2, 3, np.float64)])   # the root streams
def test_fit_and_predict_equal_the_restatement(n, trees, tf, depth, dtype):
    x, y = _data(n, dtype)
    fits = []
    for sizes in ([n], [n // 3, n - n // 3]):       # one seed, two fits
        est = RandomForestRegressor(n_estimators=trees, try_features=tf,
                                    max_depth=depth, random_state=1)
        est.fit(_dataset(x, y, sizes))
        fits.append(est.trees)
    ref = rfr_ref.forest(x.astype(np.float64), y, trees, est.try_features,
                         depth, 1)
    for t, again, r in zip(fits[0], fits[1], ref):
        assert sorted(t) == sorted(r)
        for k in r:
            assert np.array_equal(t[k], r[k]), k
            assert t[k].tobytes() == again[k].tobytes(), k
    probe, true = x[:200] + dtype(0.05), y[:200]
    ds = _dataset(probe, true, [80, 120])
    want = rfr_ref.predict(ref, probe)
    assert est.score(ds) == 1 - np.sum((true - want) ** 2) / np.sum(
        (true - true.mean()) ** 2)
    assert np.array_equal(ds.labels, true)
    est.predict(ds)
    assert ds.labels.dtype == np.float64
    assert ds.labels.tobytes() == want.tobytes()


def test_constant_target_is_one_leaf():
    x, _ = _data(600)
    ds = _dataset(x, np.full(600, 3.25), [600])
    est = RandomForestRegressor(n_estimators=3, random_state=0)
    est.fit_predict(ds)
    for t in est.trees:
        assert [list(t[k]) for k in ("feature", "leaf_value", "size")] == [
            [-1], [3.25], [600]]
    assert np.array_equal(ds.labels, np.full(600, 3.25))


def test_refusals_on_the_device(monkeypatch):
    x, y = _data(300)
    with pytest.raises(ValueError, match="finite samples"):
        RandomForestRegressor().fit(_dataset(np.where(x == x[7, 2], np.inf, x), y, [300]))
    need = rf.hbm_bytes(300, 5) + 8 * 300 + (4 << 30)
    monkeypatch.setattr(torch.cuda, "mem_get_info",
                        lambda *a: (need - 1, 1 << 40))
    with pytest.raises(ValueError, match="HBM"):
        RandomForestRegressor().fit(_dataset(x, y, [300]))


def test_accuracy_against_sklearn():
    """Friedman #1, 2000 rows to fit, 500 held out, five seeds each: our mean
    R^2 is no lower than sklearn's minus sklearn's own max - min spread (two
    correct forests with different draws differ by about that much)."""
    from sklearn.datasets import make_friedman1
    from sklearn.ensemble import RandomForestRegressor as Sk
    x, y = make_friedman1(2500, noise=1.0, random_state=0)
    train = _dataset(x[:2000], y[:2000], [1000, 1000])
    ours, theirs = [], []
    for seed in range(5):
        est = RandomForestRegressor(n_estimators=10, try_features=3,
                                    random_state=seed)
        est.fit(train)
        ours.append(est.score(_dataset(x[2000:], y[2000:], [500])))
        theirs.append(Sk(n_estimators=10, max_features=3, random_state=seed)
                      .fit(x[:2000], y[:2000]).score(x[2000:], y[2000:]))
    print("rfr R^2 ours", ours, "sklearn", theirs)
    assert np.mean(ours) >= np.mean(theirs) - (max(theirs) - min(theirs))
