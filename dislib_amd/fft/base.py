"""``dislib.fft.fft`` on the GPU: a one-dimensional complex FFT in fp64.

The reference (``dislib/fft/base.py:6-68``) is a radix-2 decimation in time
over a list of one-element arrays, one task per butterfly group, with an
n x n twiddle table.  Here the transform runs in the Stockham kernels of
``dkm_fft.hip``: radix-16 butterflies in registers, the
points of a block exchanged through LDS, one table of n twiddles.
"""
import numpy as np

from .. import _device as dev

__all__ = ["fft"]


def _check_n(n):
    if n == 0:
        raise ValueError("fft: the input is empty")
    if n & (n - 1):
        raise ValueError(
            "fft: the length %d is not a power of two (the reference "
            "returns fewer than n values, which are no transform, for such "
            "a length; this one refuses it)" % n)
    if n > dev.FFT_MAX_N:
        raise ValueError("fft: the length %d is above 2**28" % n)


def fft(a, *, rows=False, device=None):
    """Compute the one-dimensional discrete Fourier transform.

    Parameters
    ----------
    a : array-like or torch.Tensor
        Host input of any real, integer or complex dtype and any shape: it
        is flattened to ``n = a.size`` complex128 values, as the reference
        does (``a.flatten()``, ``dtype=complex``).  Or a complex128 tensor
        that is already on the GPU: it is transformed in HBM, nothing
        crosses PCIe, and the tensor itself is not written.
    rows : bool, keyword-only (not in the reference)
        ``a`` is two-dimensional ``(b, n)`` and every row is transformed on
        its own; the result has shape ``(b, n)``.
    device : keyword-only (not in the reference)
        The GPU for host input (default: the current one).

    Returns
    -------
    out : ndarray of complex128, shape ``(n,)`` (``(b, n)`` with ``rows``);
        a tensor on the input's device for device input.

    ``n`` must be a power of two, at most 2**28: anything else raises
    ``ValueError``.  This deviates from the reference, which is correct for
    powers of two only: at other lengths its ``int(ln / 2)`` drops a list at
    a merge level, and it returns fewer than ``n`` values that are no DFT.
    ``n == 1`` returns the value unchanged.  A transform whose buffers would
    leave less than 4 GiB of HBM free raises ``ValueError`` too.  There are
    no atomics: the same input gives the same bits on every run.

    Examples
    --------
    >>> from dislib.fft import fft
    >>> fft(np.exp(2j * np.pi * np.arange(8) / 8))
    """
    on_device = dev._is_torch(a) and a.is_cuda
    if not on_device:
        a = np.asarray(a.cpu() if dev._is_torch(a) else a)
    if rows:
        if a.ndim != 2:
            raise ValueError("fft: rows=True takes a two-dimensional input, "
                             "got %d dimensions" % a.ndim)
        batch, n = int(a.shape[0]), int(a.shape[1])
        if batch == 0:
            raise ValueError("fft: the input is empty")
    else:
        batch, n = 1, int(np.prod(a.shape, dtype=np.int64))
    _check_n(n)
    shape = (batch, n) if rows else (n,)
    if on_device:
        t = dev.torch()
        if a.dtype != t.complex128:
            raise TypeError("fft: a device tensor must be complex128, got %s"
                            % a.dtype)
        x = a.contiguous().reshape(shape)
        return x.clone() if n == 1 else dev.fft_z(x, n, batch)
    x = np.ascontiguousarray(a.reshape(shape), dtype=np.complex128)
    if n == 1:
        return x.copy() if x is a else x
    t = dev.torch()
    if not x.flags.writeable:          # torch takes writable arrays only
        x = x.copy()
    xd = t.from_numpy(x).to(dev.resolve(device))
    return dev.fft_z(xd, n, batch).cpu().numpy()
