"""Helpers of tests/test_gpu_dense_f32.py: grid data on which every partial
sum is exact, its oracle reference (computed once per shape), the calls
through ``_device`` and the calls through the C ABI on a strided, padded
buffer.

Grid data.  Samples are multiples of 2^-10 in [-64, 64]: 17 significant
bits, exact in fp32.  A sum of m <= 2^13 of them is a multiple of 2^-10 of
magnitude <= 2^19, 29 bits, so every partial sum in every order is exact in
fp64 -- LDS atomics, global atomics, a delta's +x / -x and sorted-segment
sums all give the same bits, and the comparison needs no tolerance.
"""
import ctypes
import functools

import numpy as np

from oracle import kmeans_oracle as orc

GRID = 2.0 ** -10
MODE_NAMES = ["exact", "screen32", "bf16x3", "bf16", "auto"]


def mode_id(mode):
    from dislib_amd import _lib
    return {"exact": _lib.MODE_EXACT, "screen32": _lib.MODE_SCREEN32,
            "bf16x3": _lib.MODE_BF16X3, "bf16": _lib.MODE_BF16,
            "auto": _lib.MODE_AUTO}[mode]


class GridCase:
    """x (fp64 values on the grid), C (fp64, unquantised) and the oracle's
    labels / sums / counts; ``prev`` and ``delta`` are the previous labels of
    the delta calls and the exact [sums | counts] delta they must produce."""

    def __init__(self, n, d, k, seed):
        assert n <= 2 ** 13
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((n, d)) * rng.uniform(0.5, 20)
        x += rng.uniform(-5, 5, (1, d))
        x = np.clip(np.round(x / GRID) * GRID, -64.0, 64.0)
        C = x[rng.choice(n, k, replace=False)] + \
            rng.standard_normal((k, d)) * 0.1
        # preconditions (a shape that stops satisfying them fails here)
        x32 = x.astype(np.float32)
        assert np.array_equal(x32.astype(np.float64), x), "fp32 round trip"
        dist = orc.dense_distances(x, C)
        if k > 1:
            two = np.partition(dist, 1, axis=1)[:, :2]
            assert (two[:, 0] < two[:, 1]).all(), "exact tie in the oracle"
        # the reference: fp64-accumulated sums (the oracle's fp32-accumulated
        # form rounds; the kernels add the exactly upcast rows in fp64)
        rl, rs, rc = orc.partial_sum(x, C)
        assert np.array_equal(rl, np.argmin(dist, axis=1))
        assert rs.dtype == np.float64
        self.n, self.d, self.k = n, d, k
        self.x, self.x32, self.C = x, x32, C
        self.labels, self.sums = rl, rs
        self.counts = rc.astype(np.float64)
        prev = rl.copy()
        prev[::5] = (prev[::5] + 1) % k
        prev[3::11] = -1
        self.prev = prev
        want = np.zeros((k, d + 1))
        for i in np.nonzero(prev != rl)[0]:
            want[rl[i], :d] += x[i]
            want[rl[i], d] += 1
            if prev[i] >= 0:
                want[prev[i], :d] -= x[i]
                want[prev[i], d] -= 1
        self.delta = want

    def samples(self, dtype):
        return self.x32 if np.dtype(dtype) == np.float32 else self.x


@functools.lru_cache(maxsize=None)
def grid_case(n, d, k):
    return GridCase(n, d, k, seed=1000 * d + k)


class _Run:
    """One set of centres with its workspace.  ``call`` runs one assignment
    and returns (labels, sums, counts, rechecked): ``rechecked`` is the rows
    THIS call sent to the exact re-check (the workspace's counter runs over
    its whole life, so the value after ``prepare`` is subtracted)."""

    def _setup(self, n, C):
        import torch
        from dislib_amd import _device
        self.dev = torch.device("cuda")
        self.n = n
        self.k, self.d = C.shape
        self.Ct = torch.from_numpy(np.ascontiguousarray(C)).to(self.dev)
        self.ws = _device.Workspace(self.k, self.d, n, self.dev)

    def call(self, kind, mode, labels_in=None):
        import torch
        from dislib_amd import _device
        k, d = self.k, self.d
        acc = torch.zeros(k * (d + 1), dtype=torch.float64, device=self.dev)
        if labels_in is None:
            lab = torch.full((self.n,), -7, dtype=torch.int32,
                             device=self.dev)
        else:
            lab = torch.from_numpy(labels_in.astype(np.int32)).to(self.dev)
        _device.prepare(self.Ct, self.ws, acc)
        before = _device.rechecked(self.ws)
        self._launch(kind, mode_id(mode), lab, acc)
        a = acc.cpu().numpy()
        return (lab.cpu().numpy().astype(np.int64), a[:k * d].reshape(k, d),
                a[k * d:], _device.rechecked(self.ws) - before)


# ---------------------------------------------------------------------------
# through _device (DeviceData: contiguous rows; the *_img_* entry points)
# ---------------------------------------------------------------------------
class DeviceRun(_Run):
    """A resident dataset.  It keeps its sample image between calls, as a
    fit does: the first call that takes one builds it, the later ones stream
    it."""

    def __init__(self, x, C):
        from dislib_amd.data import load_data
        self.dd = load_data(x, subset_size=x.shape[0])._device_data()
        assert self.dd.dtype == x.dtype
        self._setup(self.dd.n, C)

    def _launch(self, kind, m, lab, acc):
        from dislib_amd import _device
        if kind == "partial":
            _device.partial_sum(self.dd, self.Ct, self.ws, lab, acc, m)
        elif kind == "delta":
            _device.assign_delta(self.dd, self.Ct, self.ws, lab, acc, m)
        else:
            _device.predict(self.dd, self.Ct, self.ws, lab, m)


# ---------------------------------------------------------------------------
# through the C ABI: strided rows, misaligned base
# ---------------------------------------------------------------------------
class StridedRun(_Run):
    """The logical (n, d) matrix ``x`` at element offset ``off`` of one
    device buffer of off + n * ldx + 64 elements filled with ``pad``, rows
    ``ldx`` apart: the gap before the first row, the padding columns and the
    elements after the last row keep ``pad``.  A kernel that adds one into a
    sum gives a NaN or a wrong sum; one read into a distance gives a wrong
    label, or (NaN in a screen's norm) a row sent to the exact re-check."""

    def __init__(self, x, ldx, off, C, pad=np.nan):
        import torch
        n, d = x.shape
        assert ldx >= d
        self.ldx, self.off = ldx, off
        host = np.full(off + n * ldx + 64, pad, dtype=x.dtype)
        host[off:off + n * ldx].reshape(n, ldx)[:, :d] = x
        self.host = host
        self._setup(n, C)
        self.buf = torch.from_numpy(host).to(self.dev)

    def _launch(self, kind, m, lab, acc):
        """dkm_partial_sum_* / dkm_assign_delta_* / dkm_predict_* with
        ``_device``'s argument order."""
        from dislib_amd import _device, _lib
        so = _lib.lib()
        sfx = "_f32" if self.host.dtype == np.float32 else "_f64"
        xp = ctypes.c_void_p(self.buf.data_ptr() +
                             self.off * self.host.dtype.itemsize)
        ptr = _device.ptr
        head = (xp, self.n, self.d, self.ldx, ptr(self.Ct), self.k, self.ws.p,
                self.ws.nbytes, ptr(lab))
        if kind == "predict":
            name = "dkm_predict" + sfx
            rc = getattr(so, name)(*head, m, _device.stream_ptr())
        else:
            name = ("dkm_partial_sum" if kind == "partial"
                    else "dkm_assign_delta") + sfx
            rc = getattr(so, name)(*head, ptr(acc), m, _device.stream_ptr())
        _lib.check(rc, name)

    def untouched(self):
        """Is the sample buffer byte-identical to what was uploaded?"""
        return self.buf.cpu().numpy().tobytes() == self.host.tobytes()


def sum_bound(x, labels, k):
    """Per (cluster j, feature t): cnt_j 2^-52 sum_{i in j} |x_it| -- the
    distance between two fp64 sums of the same cnt_j exactly upcast terms in
    different orders (each is within (cnt_j - 1) 2^-53 sum |x| of the true
    sum)."""
    ax = np.zeros((k, x.shape[1]))
    np.add.at(ax, labels, np.abs(x.astype(np.float64)))
    cnt = np.bincount(labels, minlength=k).astype(np.float64)
    return cnt[:, None] * 2.0 ** -52 * ax
