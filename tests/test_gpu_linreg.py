"""GPU tests of the tall-skinny QR (dkm_qr.hip) and of LinearRegression
against numpy in ``np.longdouble`` built from the same inputs; u = 2^-53.

Kernel: with A = [1 | X | y] (or [X | y]) in longdouble, every entry of
``R^T R - A^T A`` is within ``4 n w u ||a_i|| ||a_j||``, Higham's column-wise
bound for Householder QR (loose on purpose: it catches a wrong reflector, not
rounding); R is upper triangular with a non-negative diagonal, and with the
ones column ``R[0, 0] == sqrt(n)`` to 2 ulp.

Estimator, ill-conditioned (columns a, a + e, b with a, b integers below 2^20
and e in {-1, 0, 1}: condition number 1.7e6, its square for the normal
equations, which reach 4.4e-5 on these arrays).  Measured on MI355X: relative
error 2.2e-12 against the integer truth, 4.5e-11 for fp64 ``np.linalg.lstsq``,
ratio 0.05; the bound is 16 times lstsq's error, the margin
for a different reflector order.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from dislib_amd import _device
from dislib_amd.data import Dataset, Subset
from dislib_amd.regression import LinearRegression

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
T, RANGE = _device.TSQR_TILE, _device.TSQR_RANGE_ROWS
# (n, d): one row; fewer rows than columns; w = 16 and 17 at the tile's edges;
# three panels; w = 128; two ranges and three (the merge stacks them)
SHAPES = [(1, 1), (3, 5), (T - 1, 14), (T, 14), (T + 1, 15), (1000, 31),
          (700, 126), (RANGE + 1, 5), (2 * RANGE + 1, 5)]


def _factor(x, y, pad, ones):
    """R of the device copy of x (rows of a wider matrix, NaN in the padding
    and past row n) and y."""
    n, d = x.shape
    buf = np.full((n + 2, d + pad), np.nan, dtype=x.dtype)
    buf[:n, :d] = x
    X = torch.from_numpy(buf).cuda()[:n, :d]
    dd = SimpleNamespace(X=X, n=n, d=d, dtype=x.dtype.type, device=X.device)
    return _device.tsqr(dd, torch.from_numpy(y).cuda(), ones)


def _check(R, x, y, ones):
    n, d = x.shape
    w = d + 1 + ones
    a = np.concatenate([np.ones((n, ones), LD), x.astype(LD),
                        y.astype(LD)[:, None]], axis=1)
    norm = np.sqrt((a * a).sum(0))
    err = np.abs(R.astype(LD).T @ R.astype(LD) - a.T @ a)
    bound = 4 * n * w * U * np.outer(norm, norm)
    assert R.shape == (w, w) and np.all(np.tril(R, -1) == 0)
    assert np.all(np.diag(R) >= 0)
    assert np.all(err <= bound), float((err / bound)[bound > 0].max())
    if ones:
        assert abs(R[0, 0] - np.sqrt(n)) <= 2 * np.spacing(np.sqrt(n))


@pytest.mark.parametrize("ones", [1, 0])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,d", SHAPES)
def test_r_factor(n, d, dtype, pad, ones):
    assert [_device.tsqr_ranges(m) for m in (RANGE, RANGE + 1, 2 * RANGE + 1)
            ] == [1, 2, 3]
    rng = np.random.default_rng(100 * n + d)
    x = (rng.standard_normal((n, d)) + 0.5).astype(dtype)
    y = rng.standard_normal(n)
    _check(_factor(x, y, pad, ones).cpu().numpy(), x, y, ones)


@pytest.mark.parametrize("ones", [1, 0])
@pytest.mark.parametrize("kind", ["zero column", "equal columns"])
def test_r_factor_degenerate(kind, ones):
    """The tau = 0 guard: a zero column, and a column that the reflectors of
    an equal one before it have already annihilated (up to rounding)."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((150, 20))
    x[:, 17] = 0.0 if kind == "zero column" else x[:, 2]
    y = rng.standard_normal(150)
    R = _factor(x, y, 0, ones).cpu().numpy()
    _check(R, x, y, ones)
    if kind == "zero column":
        assert np.all(R[:, 17 + ones] == 0)


def test_run_to_run_identity():
    rng = np.random.default_rng(9)
    x, y = rng.standard_normal((2 * RANGE + 1, 20)), rng.standard_normal(
        2 * RANGE + 1)
    assert torch.equal(_factor(x, y, 0, 1), _factor(x, y, 0, 1))


def _dataset(x, y, sizes, on_device=False):
    ds = Dataset(n_features=x.shape[1])
    xs = torch.from_numpy(x).cuda() if on_device else x
    for a, b in zip(np.cumsum((0,) + sizes[:-1]), np.cumsum(sizes)):
        ds.append(Subset(xs[a:b], labels=None if y is None else y[a:b]))
    return ds


@pytest.mark.parametrize("on_device", [False, True])
def test_estimator_well_conditioned(on_device):
    rng = np.random.default_rng(1)
    x = rng.standard_normal((500, 8)) * np.arange(1, 9) + 3.0
    y = x @ rng.standard_normal(8) + 2.0 + 0.1 * rng.standard_normal(500)
    lr = LinearRegression()
    lr.fit(_dataset(x, y, (200, 1, 299), on_device))
    mx, my = x.astype(LD).mean(0), y.astype(LD).mean()
    coef = np.linalg.lstsq((x - mx).astype(np.float64),
                           (y - my).astype(np.float64), rcond=None)[0]
    icpt = float(my - mx @ coef)
    assert lr.coef_.shape == (8,) and lr.coef_.dtype == np.float64
    assert np.linalg.norm(lr.coef_ - coef) <= 1e-12 * np.linalg.norm(coef)
    assert abs(lr.intercept_ - icpt) <= 1e-12 * abs(icpt)
    res = np.linalg.norm(y - x @ coef - icpt)
    assert abs(lr.residual_norm_ - res) <= 1e-12 * res
    x2 = rng.standard_normal((100, 8)) + 3.0
    ds2 = _dataset(x2, None, (30, 70), on_device)
    lr.predict(ds2)
    want = x2 @ coef + icpt
    for s, (a, b) in zip(ds2, ((0, 30), (30, 100))):
        assert isinstance(s.labels, torch.Tensor if on_device else np.ndarray)
        got = s.labels.cpu().numpy() if on_device else s.labels
        assert got.dtype == np.float64 and got.shape == (b - a,)
        assert np.all(np.abs(got - want[a:b]) <= 1e-12 * np.abs(want).max())
    lr0 = LinearRegression(fit_intercept=False)
    lr0.fit(_dataset(x, y, (500,), on_device))
    coef0 = np.linalg.lstsq(x, y, rcond=None)[0]
    assert lr0.intercept_ == 0.0
    assert np.linalg.norm(lr0.coef_ - coef0) <= 1e-12 * np.linalg.norm(coef0)


def test_estimator_ill_conditioned():
    """The test a normal-equations fit fails (its error is O(1))."""
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 2 ** 20, (2, 2000))
    x = np.stack([a, a + rng.integers(-1, 2, 2000), b], axis=1)
    beta = np.array([3, -2, 5])
    y = x @ beta                                     # int64: exact
    x, y = x.astype(np.float64), y.astype(np.float64)
    ref = np.linalg.norm(np.linalg.lstsq(x, y, rcond=None)[0] - beta) / \
        np.linalg.norm(beta)
    assert 0 < ref < 1e-3 / 16                       # a condition on the seed
    lr = LinearRegression(fit_intercept=False)
    lr.fit(_dataset(x, y, (1500, 500)))
    err = np.linalg.norm(lr.coef_ - beta) / np.linalg.norm(beta)
    print("ill-conditioned: error %.3e, lstsq %.3e, ratio %.2f"
          % (err, ref, err / ref))
    assert err <= 16 * ref and err < 1e-3


@pytest.mark.parametrize("kind", ["underdetermined", "equal columns"])
def test_estimator_minimum_norm(kind):
    from sklearn.linear_model import LinearRegression as Sk
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, 5) if kind == "underdetermined" else (200, 4))
    if kind == "equal columns":
        x[:, 3] = x[:, 1]
    y = rng.standard_normal(x.shape[0])
    lr = LinearRegression()
    lr.fit(_dataset(x, y, (x.shape[0],)))
    sk = Sk().fit(x, y)
    assert np.linalg.norm(lr.coef_ - sk.coef_) <= \
        1e-10 * np.linalg.norm(sk.coef_)
    assert abs(lr.intercept_ - sk.intercept_) <= 1e-10 * max(
        1.0, abs(sk.intercept_))
