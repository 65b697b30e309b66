"""CPU tests of ``dislib_amd.fft``: the refusals come before the library is
loaded, ``install_as_dislib`` aliases ``dislib.fft``, and the plan."""
import numpy as np
import pytest


def _boom():
    raise AssertionError("the library was loaded")


@pytest.mark.parametrize("a", [np.zeros(0), np.zeros((4, 0)), np.zeros(12),
                               np.zeros((3, 5)),
                               np.broadcast_to(0.0, (1 << 28) + 1)])
def test_bad_lengths_are_refused_before_any_gpu_use(monkeypatch, a):
    from dislib_amd import _lib
    from dislib_amd.fft import fft
    monkeypatch.setattr(_lib, "lib", _boom)
    with pytest.raises(ValueError, match="empty|power of two"):
        fft(a)


def test_length_above_the_limit_is_refused(monkeypatch):
    from dislib_amd import _lib
    from dislib_amd.fft import fft
    monkeypatch.setattr(_lib, "lib", _boom)
    with pytest.raises(ValueError, match=r"above 2\*\*28"):
        fft(np.broadcast_to(0.0, 1 << 29))
    with pytest.raises(ValueError, match="two-dimensional"):
        fft(np.zeros(8), rows=True)


def test_install_as_dislib_aliases_fft():
    import dislib_amd
    dislib_amd.install_as_dislib()
    from dislib.fft import fft
    assert fft is dislib_amd.fft.fft


def test_plan_passes_and_radices():
    from dislib_amd._device import fft_plan
    assert [len(fft_plan(1 << e)) for e in (12, 13, 20, 21)] == [1, 2, 2, 3]
    for e in range(29):
        plan = fft_plan(1 << e)
        assert int(np.prod(plan, dtype=np.int64)) == 1 << e
        assert all(r <= 256 for r in plan[:-1]) and plan[-1] <= 4096
    with pytest.raises(ValueError):
        fft_plan(1 << 29)
