"""GPU tests of ``dislib_amd.fft.fft`` (``dkm_fft.hip``) against plain numpy.

Tolerance (derived, not tuned).  Higham, *Accuracy and Stability of
Numerical Algorithms*, Theorem 24.2: a radix-2 FFT of n = 2^t points whose
twiddles satisfy |w^ - w| <= mu computes y^ with

    ||y^ - y||_2 / ||y||_2 <= t eta / (1 - t eta),
    eta = mu + gamma_4 (sqrt(2) + mu),   gamma_4 = 4u / (1 - 4u),

u = 2^-53 the unit roundoff.  The table is rounded once from long double, so
mu = u and eta = (1 + 4 sqrt(2)) u + O(u^2) = 6.66 u = 3.33 eps with eps =
2^-52.  A radix-16 butterfly is four radix-2 levels whose inner twiddles are
literals rounded once or exact (+-1, +-i), and the twiddles between passes
are applied once per pass instead of once per level, so the radix-2 bound
covers the kernels.  With c = 3.5 (3.33, and the second-order terms for t <=
28) and ||y||_2 = sqrt(n) ||x||_2:

    ||y^ - y||_2 <= c eps log2(n) sqrt(n) ||x||_2 ,

which also caps every single bin.  Against ``np.fft.fft`` the bound is
doubled, because numpy's own result gets the same allowance.  An indexing or
twiddle bug is wrong by about ||x||_2: ten orders of magnitude more.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1 << e for e in range(14)] + [1 << 20, 1 << 21]
C, EPS = 3.5, np.finfo(np.float64).eps


def bound(n, x):
    return C * EPS * np.log2(n) * np.sqrt(n) * np.linalg.norm(x)


@functools.lru_cache(maxsize=2)
def roots(n):
    """exp(-2 pi i k / n), k < n, in long double."""
    a = (8 * np.arctan(np.longdouble(1)) / n) * np.arange(n,
                                                          dtype=np.longdouble)
    return np.cos(a) - 1j * np.sin(a)


@functools.lru_cache(maxsize=2)
def random_case(n):
    from dislib_amd.fft import fft
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    x.setflags(write=False)
    return x, fft(x)


@pytest.mark.parametrize("n", SIZES)
def test_impulse_every_bin(n):
    from dislib_amd.fft import fft
    v, p = 0.75 - 0.5j, (n // 2 + 1 if n > 2 else 0)
    x = np.zeros(n, dtype=complex)
    x[p] = v
    y = fft(x)
    assert y.shape == (n,) and y.dtype == np.complex128
    want = v * roots(n)[(p * np.arange(n, dtype=np.int64)) % n]
    err = np.abs(y - want).max()
    print("impulse n=%d: max bin error %.3g, bound %.3g" % (n, err,
                                                            bound(n, x)))
    assert err <= bound(n, x)


@pytest.mark.parametrize("n", SIZES)
def test_random_sampled_bins_in_longdouble(n):
    x, y = random_case(n)
    rng = np.random.default_rng(n + 1)
    ks = np.unique(np.r_[rng.integers(0, n, 16), 0, n // 2, n - 1])
    j, xl, w = np.arange(n, dtype=np.int64), x.astype(np.clongdouble), roots(n)
    err = max(abs(y[k] - (xl * w[(j * k) % n]).sum()) for k in ks)
    print("random n=%d: max sampled bin error %.3g, bound %.3g"
          % (n, err, bound(n, x)))
    assert err <= bound(n, x)


@pytest.mark.parametrize("n", SIZES)
def test_random_all_bins_against_numpy(n):
    x, y = random_case(n)
    err = np.linalg.norm(y - np.fft.fft(x))
    print("random n=%d: ||y - np.fft.fft||_2 %.3g, bound %.3g"
          % (n, err, 2 * bound(n, x)))
    assert err <= 2 * bound(n, x)


@pytest.mark.parametrize("dtype", [np.float64, np.int32, np.complex64])
def test_host_input_is_flattened_as_the_reference_does(dtype):
    from dislib_amd.fft import fft
    a = (np.arange(32).reshape(4, 8) % 7 - 3).astype(dtype)
    if dtype == np.complex64:
        a = a + 1j * a[::-1]
    y = fft(a)
    x = a.flatten().astype(complex)
    assert y.shape == (32,) and y.dtype == np.complex128
    assert np.linalg.norm(y - np.fft.fft(x)) <= 2 * bound(32, x)


@pytest.mark.parametrize("b,n", [(3, 64), (5, 4096)])
def test_rows_equal_the_row_wise_results(b, n):
    from dislib_amd.fft import fft
    rng = np.random.default_rng(b)
    x = rng.standard_normal((b, n)) + 1j * rng.standard_normal((b, n))
    y = fft(x, rows=True)
    assert y.shape == (b, n)
    for i in range(b):
        assert np.array_equal(y[i], fft(x[i]))
        assert np.linalg.norm(y[i] - np.fft.fft(x[i])) <= 2 * bound(n, x[i])


def test_device_tensor_in_device_tensor_out_and_same_bits():
    import torch
    from dislib_amd.fft import fft
    x, y = random_case(1 << 13)
    xd = torch.from_numpy(x.copy()).cuda()
    yd = fft(xd)
    assert yd.is_cuda and yd.dtype == torch.complex128
    assert yd.data_ptr() != xd.data_ptr()
    assert np.array_equal(xd.cpu().numpy(), x)          # input unchanged
    assert yd.cpu().numpy().tobytes() == y.tobytes()     # run to run
    assert fft(xd).cpu().numpy().tobytes() == y.tobytes()
