from dislib_amd.fft.base import fft

__all__ = ["fft"]
