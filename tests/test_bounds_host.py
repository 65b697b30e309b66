"""Host side of the per-row bounds (no GPU): which shapes keep them
(``dkm_bounds_ok``)."""
import os

import pytest

from dislib_amd import _lib

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH),
                                reason="libdkm.so not built")


def test_bounds_ok_shapes():
    so = _lib.load()
    # (256, 32), (193, 32): the [sums | counts] do not fit LDS beside the
    # centres, the delta call takes its sums from the labels and lists no
    # moved rows, and dkm_assign_delta_bounds_* refuses the shape
    for k, d in [(100, 32), (37, 17), (10, 8), (2, 1), (192, 32), (256, 8)]:
        assert so.dkm_bounds_ok(k, d) == 1, (k, d)
    for k, d in [(1, 32), (257, 32), (100, 33), (1000, 64), (0, 8),
                 (256, 32), (193, 32)]:
        assert so.dkm_bounds_ok(k, d) == 0, (k, d)
