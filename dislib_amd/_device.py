"""Device residency and thin launch wrappers around ``libdkm.so``.

PyTorch is used only as the device allocator / stream provider: tensors are
HBM buffers whose ``data_ptr()`` goes through the C ABI.  All compute is in
the HIP kernels of ``dislib_amd/csrc``.

``DeviceData`` is the HBM image of a :class:`dislib_amd.data.Dataset`: every
Subset's rows concatenated into one row-major matrix (or one CSR matrix),
with the Subset boundaries kept as row offsets.  It replaces PyCOMPSs'
per-task pickling of Subsets (reference ``cluster/kmeans/base.py:113-115``,
``data/classes.py:298-304``): the data is uploaded once and stays resident
for every Lloyd iteration.
"""
import ctypes

import numpy as np

from . import _lib

# False: never build the sample image (the screen then converts X itself;
# identical labels -- the parity tests switch it through this attribute)
X_IMAGE = True
# HBM left free after an image is allocated
_IMAGE_HEADROOM = 4 << 30
# (what, bytes, host seconds) of every workspace / image allocation: lets a
# caller (bench.py) attribute host time inside a fit to its allocations
ALLOC_LOG = []


def _alloc(what, nbytes, fn):
    import time
    t0 = time.perf_counter()
    out = fn()
    ALLOC_LOG.append((what, int(nbytes), time.perf_counter() - t0))
    return out


def torch():
    import torch as _t
    return _t


def stream_ptr():
    t = torch()
    return ctypes.c_void_p(t.cuda.current_stream().cuda_stream)


def resolve(device=None):
    """A concrete ``torch.device('cuda', i)``: ``None`` / ``'cuda'`` mean the
    current device, so a fit keeps using the GPU it started on."""
    t = torch()
    dev = t.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise ValueError("dislib_amd runs on a ROCm GPU, got device %s" % dev)
    if dev.index is None:
        dev = t.device("cuda", t.cuda.current_device())
    return dev


def on(device):
    """Context in which launches go to ``device``: HIP launches and
    ``stream_ptr()`` use the current device, so every entry point that
    touches the data of a Dataset runs inside ``with on(dd.device):``."""
    return torch().cuda.device(device)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class DeviceData:
    """HBM image of a Dataset (dense or CSR)."""

    def __init__(self, dataset, device=None):
        self.device = resolve(device)
        self.images = {}            # sample images by kind (screen_image)
        self._unbuilt = set()       # kinds allocated, not yet built
        self._image_failed = set()
        subsets = list(dataset)
        self.sizes = [int(s.samples.shape[0]) for s in subsets]
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(
            np.int64)
        self.n = int(self.offsets[-1])
        self.d = int(dataset.n_features)
        self.sparse = bool(dataset.sparse)
        if self.sparse:
            self._upload_csr(subsets, getattr(dataset, "_host_image", None))
        else:
            self._upload_dense(subsets)

    # -- dense -------------------------------------------------------------
    def _upload_dense(self, subsets):
        t = torch()
        dev_parts = [s.samples for s in subsets
                     if _is_torch(s.samples)]
        if dev_parts and len(dev_parts) == len(subsets):
            # already device-resident (e.g. bench data): view/concat on device
            xs = [s.samples for s in subsets]
            dt = xs[0].dtype
            self.dtype = np.float32 if dt == t.float32 else np.float64
            X = _adjacent_view(xs)
            if X is None:
                X = xs[0] if len(xs) == 1 else t.cat(xs, 0)
            self.X = X.to(self.device, dtype=(t.float32 if self.dtype ==
                                             np.float32 else t.float64))
            self.X = self.X.contiguous()
            return
        arrs = [np.asarray(s.samples) for s in subsets]
        dts = {a.dtype for a in arrs}
        if dts == {np.dtype(np.float32)}:
            self.dtype = np.float32
        else:
            # fp64 samples; integer samples are exact in fp64 below 2**53
            self.dtype = np.float64
        host = np.concatenate([a.astype(self.dtype, copy=False)
                               for a in arrs]) if arrs else \
            np.zeros((0, self.d), self.dtype)
        host = np.ascontiguousarray(host.reshape(self.n, self.d))
        self.X = t.from_numpy(host).to(self.device)
        self.int_input = any(np.issubdtype(a.dtype, np.integer) for a in arrs)

    # -- CSR ---------------------------------------------------------------
    def _upload_csr(self, subsets, image=None):
        import scipy.sparse as sp
        t = torch()
        if image is not None and image.shape == (self.n, self.d):
            m = image      # file loaders: the parser's concatenated output
        else:
            mats = [sp.csr_matrix(s.samples) for s in subsets]
            m = sp.vstack(mats, format="csr") if mats else \
                sp.csr_matrix((0, self.d))
        # keep each row's stored order: it is the reference's dot order
        assert_all_finite(m.data)
        self.dtype = np.float64
        self.indptr = t.from_numpy(m.indptr.astype(np.int64)).to(self.device)
        self.indices = t.from_numpy(m.indices.astype(np.int32)).to(
            self.device)
        self.data = t.from_numpy(m.data.astype(np.float64)).to(self.device)

    # -- the sample image ---------------------------------------------------
    def screen_image(self, k, mode):
        """The resident bf16 operand image of X (dkm_x_image_*) when the
        screen that (k, d, mode) selects reads one, as (tensor, kind); kept
        with the data, which is immutable (one image per kind).  On first
        use it is only allocated and returned as kind | IMAGE_BUILD: the
        assignment call that receives it builds it (the d <= 32 screen's
        full-sums pass writes it while it converts X anyway) and
        :meth:`image_built` records that.  (None, 0) when not useful,
        disabled (DKM_X_IMAGE=0) or when it would leave less than 4 GiB of
        HBM free."""
        if self.sparse or not X_IMAGE or self.n == 0:
            return None, 0
        so = _lib.lib()
        kind = int(so.dkm_x_image_kind(int(k), self.d, int(mode)))
        if kind == 0:
            return None, 0
        if self.images.get(kind) is not None:
            return self.images[kind], kind | (
                _lib.IMAGE_BUILD if kind in self._unbuilt else 0)
        if kind in self._image_failed:
            return None, 0
        t = torch()
        nb = int(so.dkm_x_image_bytes(self.n, self.d, kind))
        free = t.cuda.mem_get_info(self.device)[0]
        if nb == 0 or nb + _IMAGE_HEADROOM > free:
            self._image_failed.add(kind)
            return None, 0
        img = _alloc("image%d" % kind, nb, lambda: t.empty(
            nb, dtype=t.uint8, device=self.device))
        self.images[kind] = img
        self._unbuilt.add(kind)
        return img, kind | _lib.IMAGE_BUILD

    def image_built(self, kind):
        """The call that received kind | IMAGE_BUILD returned: built."""
        self._unbuilt.discard(kind & ~_lib.IMAGE_BUILD)

    def drop_images(self):
        """Free the resident sample images (up to 16.5 GB at C3): later
        calls convert X in the screen, or build an image again."""
        self.images = {}
        self._unbuilt = set()
        self._image_failed = set()

    # -- a matrix that is already resident ----------------------------------
    @classmethod
    def from_matrix(cls, X, sizes):
        """The image of a dense Dataset whose rows already are the resident
        (n, d) fp32 / fp64 device matrix ``X`` (StandardScaler.transform's
        output), cut into Subsets of ``sizes`` rows: nothing is uploaded or
        copied."""
        t = torch()
        if X.dim() != 2 or X.dtype not in (t.float32, t.float64) or \
                not X.is_cuda or sum(int(s) for s in sizes) != X.shape[0]:
            raise ValueError("from_matrix: an (n, d) fp32 / fp64 device "
                             "matrix and Subset sizes that sum to n")
        dd = cls.__new__(cls)
        dd.device = X.device
        dd.images = {}
        dd._unbuilt = set()
        dd._image_failed = set()
        dd.sizes = [int(s) for s in sizes]
        dd.offsets = np.concatenate([[0], np.cumsum(dd.sizes)]).astype(
            np.int64)
        dd.n, dd.d = int(X.shape[0]), int(X.shape[1])
        dd.sparse = False
        dd.dtype = np.float32 if X.dtype == t.float32 else np.float64
        dd.X = X.contiguous()
        dd.int_input = False
        return dd

    # -- helpers -----------------------------------------------------------
    def subset_slices(self):
        return [(int(a), int(b)) for a, b in zip(self.offsets[:-1],
                                                 self.offsets[1:])]


def assert_all_finite(values):
    """The sparse path's input check: the reference computes its sparse
    distances with sklearn's ``pairwise_distances`` (kmeans/base.py:169,
    196; dbscan/classes.py:130), whose ``check_array`` raises ValueError on
    NaN or inf in either operand -- with these messages."""
    v = np.asarray(values)
    if v.size and not np.isfinite(v).all():
        if np.isnan(v).any():
            raise ValueError("Input contains NaN.")
        raise ValueError("Input contains infinity or a value too large for "
                         "dtype('float64').")


def _adjacent_view(xs):
    """One (n, d) view over row blocks that are consecutive slices of one
    device buffer (e.g. ``load_data`` of a device tensor): no copy."""
    t = torch()
    x0 = xs[0]
    if x0.dim() != 2 or x0.stride(1) != 1:
        return None
    ld, es = x0.stride(0), x0.element_size()
    nxt = x0.data_ptr()
    for x in xs:
        if (x.dim() != 2 or x.dtype != x0.dtype or x.stride(1) != 1 or
                x.shape[1] != x0.shape[1] or
                (x.shape[0] > 1 and x.stride(0) != ld) or
                x.data_ptr() != nxt or x.device != x0.device):
            return None
        nxt += x.shape[0] * ld * es
    n = sum(int(x.shape[0]) for x in xs)
    return t.as_strided(x0, (n, x0.shape[1]), (ld, 1))


def _is_torch(x):
    try:
        import torch as _t
        return isinstance(x, _t.Tensor)
    except ImportError:          # pragma: no cover
        return False


class Workspace:
    """Caller-owned scratch for the C ABI (``dkm_workspace_bytes``)."""

    def __init__(self, k, d, n_queue, device):
        t = torch()
        so = _lib.lib()
        self.k, self.d = int(k), int(d)
        self.nbytes = int(so.dkm_workspace_bytes(self.k, self.d,
                                                 int(n_queue)))
        if self.nbytes == 0:
            raise _lib.DkmError("dkm_workspace_bytes: bad k/d")
        self.buf = _alloc("workspace", self.nbytes, lambda: t.zeros(
            self.nbytes, dtype=t.uint8, device=device))
        preload(self.buf.device)

    @property
    def p(self):
        return ctypes.c_void_p(self.buf.data_ptr())


_PRELOADED = set()


def preload(device):
    """Load the library's kernels on ``device`` now (``dkm_preload``), once
    per process and device: the runtime loads each source file's kernels on
    first launch, several ms apiece, which otherwise lands inside the first
    Lloyd iterations."""
    t = torch()
    idx = t.device(device).index
    if idx in _PRELOADED:
        return
    with on(device):
        _lib.check(_lib.lib().dkm_preload(), "dkm_preload")
    _PRELOADED.add(idx)


# ---------------------------------------------------------------------------
# launch wrappers (all stream-ordered on torch's current stream)
# ---------------------------------------------------------------------------
def prepare(C, ws, acc, csr=False):
    so = _lib.lib()
    k, d = C.shape
    _lib.check(so.dkm_prepare_centers(ptr(C), k, d,
                                      _lib.PREP_CSR if csr else 0, ws.p,
                                      ws.nbytes, ptr(acc), stream_ptr()),
               "dkm_prepare_centers")


def _image_for(dd, k, mode, labels, image):
    """The image an assignment call streams: ``image`` = (tensor, kind) when
    the caller owns one (the fit's label-sorted image), else the dataset's
    cached image for the screen (k, mode) selects (labels needed: the
    image screens write labels only)."""
    if image is not None:
        return image
    if labels is None:
        return None, 0
    return dd.screen_image(k, mode)


def partial_sum(dd, C, ws, labels, acc, mode, image=None):
    so = _lib.lib()
    k = C.shape[0]
    if dd.sparse:
        _lib.check(so.dkm_partial_sum_csr_f64(
            ptr(dd.indptr), ptr(dd.indices), ptr(dd.data), dd.n, dd.d,
            ptr(C), k, ws.p, ws.nbytes, ptr(labels), ptr(acc), stream_ptr()),
            "dkm_partial_sum_csr_f64")
        return
    img, kind = _image_for(dd, k, mode, labels, image)
    if img is not None:
        fn = so.dkm_partial_sum_img_f32 if dd.dtype == np.float32 else \
            so.dkm_partial_sum_img_f64
        _lib.check(fn(ptr(dd.X), ptr(img), kind, img.numel(), dd.n, dd.d,
                      dd.X.stride(0), ptr(C), k, ws.p, ws.nbytes, ptr(labels),
                      ptr(acc), mode, stream_ptr()), "dkm_partial_sum_img")
        dd.image_built(kind)
        return
    fn = so.dkm_partial_sum_f32 if dd.dtype == np.float32 else \
        so.dkm_partial_sum_f64
    _lib.check(fn(ptr(dd.X), dd.n, dd.d, dd.X.stride(0), ptr(C), k, ws.p,
                  ws.nbytes, ptr(labels), ptr(acc), mode, stream_ptr()),
               "dkm_partial_sum")


def assign_delta(dd, C, ws, labels, delta, mode, image=None):
    """Incremental assignment: labels in/out, delta +=."""
    so = _lib.lib()
    k = C.shape[0]
    if dd.sparse:
        _lib.check(so.dkm_assign_delta_csr_f64(
            ptr(dd.indptr), ptr(dd.indices), ptr(dd.data), dd.n, dd.d,
            ptr(C), k, ws.p, ws.nbytes, ptr(labels), ptr(delta),
            stream_ptr()), "dkm_assign_delta_csr_f64")
        return
    img, kind = _image_for(dd, k, mode, labels, image)
    if img is not None:
        fn = so.dkm_assign_delta_img_f32 if dd.dtype == np.float32 else \
            so.dkm_assign_delta_img_f64
        _lib.check(fn(ptr(dd.X), ptr(img), kind, img.numel(), dd.n, dd.d,
                      dd.X.stride(0), ptr(C), k, ws.p, ws.nbytes, ptr(labels),
                      ptr(delta), mode, stream_ptr()), "dkm_assign_delta_img")
        dd.image_built(kind)
        return
    fn = so.dkm_assign_delta_f32 if dd.dtype == np.float32 else \
        so.dkm_assign_delta_f64
    _lib.check(fn(ptr(dd.X), dd.n, dd.d, dd.X.stride(0), ptr(C), k, ws.p,
                  ws.nbytes, ptr(labels), ptr(delta), mode, stream_ptr()),
               "dkm_assign_delta")


def bounds_ok(dd, k, mode, ws):
    """Can a fit of (k, d, mode) on ``dd`` keep per-row distance bounds
    (dkm_assign_delta_bounds_*)?  The shapes of the d <= 32 hinted screen in
    auto / bf16x3 mode, a workspace with n label slots and the sample image
    enabled."""
    if dd.sparse or dd.n == 0 or not X_IMAGE or dd.n >= 2 ** 31:
        return False
    if mode not in (_lib.MODE_AUTO, _lib.MODE_BF16X3):
        return False
    so = _lib.lib()
    if not so.dkm_bounds_ok(int(k), dd.d):
        return False
    if int(so.dkm_x_image_kind(int(k), dd.d, int(mode))) != _lib.IMAGE_SPLIT:
        return False
    return int(so.dkm_workspace_bytes(int(k), dd.d, dd.n)) <= ws.nbytes


def alloc_bounds(dd):
    """The fit's (ub, lb): two fp32 arrays of n entries, or None when they
    would leave less than 4 GiB of HBM free (the image's rule)."""
    t = torch()
    nb = 8 * dd.n
    free = t.cuda.mem_get_info(dd.device)[0]
    if nb + _IMAGE_HEADROOM > free:
        return None
    # (rows padded to 64 entries: both arrays start 16-B aligned)
    npad = (dd.n + 63) // 64 * 64
    return _alloc("bounds", 8 * npad, lambda: t.empty(
        (2, npad), dtype=t.float32, device=dd.device))


def assign_delta_bounds(dd, C, ws, labels, delta, mode, image, bounds, init):
    """assign_delta with per-row bounds: ``bounds`` = the (2, >= n) fp32 tensor
    of alloc_bounds, ``init`` = it holds nothing valid for ``labels``."""
    so = _lib.lib()
    img, kind = image
    fn = so.dkm_assign_delta_bounds_f32 if dd.dtype == np.float32 else \
        so.dkm_assign_delta_bounds_f64
    _lib.check(fn(ptr(dd.X), ptr(img), kind, img.numel(), dd.n, dd.d,
                  dd.X.stride(0), ptr(C), C.shape[0], ws.p, ws.nbytes,
                  ptr(labels), ptr(delta), mode, ptr(bounds[0]),
                  ptr(bounds[1]), _lib.BOUNDS_INIT if init else 0,
                  stream_ptr()), "dkm_assign_delta_bounds")


def bounds_counters(ws):
    """(calls that ran the bounds pass, rows it left active, rows it
    skipped, calls that screened the active rows as a list) over the
    workspace's life (dkm_bounds_counters)."""
    so = _lib.lib()
    out = (ctypes.c_int64 * 4)()
    _lib.check(so.dkm_bounds_counters(ws.p, out, stream_ptr()),
               "dkm_bounds_counters")
    return tuple(int(x) for x in out)


def bounds_settled(ws):
    """Rows the exact re-check's fp32 stage gave bounds to, over the
    workspace's life (dkm_bounds_settled)."""
    so = _lib.lib()
    out = ctypes.c_int64(0)
    _lib.check(so.dkm_bounds_settled(ws.p, ctypes.byref(out), stream_ptr()),
               "dkm_bounds_settled")
    return int(out.value)


def sorted_image_ok(dd, k):
    """Does the fit's auto mode on (k, d) run the single-product screen that
    takes a label-sorted image (dkm_x_image_sorted_ok)?"""
    if dd.sparse or dd.n == 0 or not X_IMAGE:
        return False
    # the screen that maintains the image reads 16-B pieces of X's rows
    # (dkm_dense.hip plan_screen `vec`): rows a multiple of 16 B apart,
    # X 16-B aligned (d % 8 == 0 is checked by dkm_x_image_sorted_ok)
    isz = dd.X.element_size()
    if (dd.X.stride(0) * isz) % 16 or dd.X.data_ptr() % 16:
        return False
    so = _lib.lib()
    return (int(so.dkm_x_image_kind(int(k), dd.d, _lib.MODE_AUTO)) ==
            _lib.IMAGE_SINGLE and bool(so.dkm_x_image_sorted_ok(int(k), dd.d)))


def sorted_image(dd, labels, k, ws, old=None, acc=None):
    """dkm_x_image_sorted_*: the sample image with its rows grouped by
    ``labels`` (a fit's current assignment), as (tensor, IMAGE_SORTED); the
    buffer of ``old`` is reused.  (None, 0) when it would leave less than
    4 GiB of HBM free or the workspace's label scratch is shorter than n
    (then ``acc`` is untouched).  With ``acc``: also acc += the [sums |
    counts] of X by ``labels`` (dkm_x_image_sorted_sums_*, one pass over X).
    The image carries a copy of the labels: pass it to every later call
    that updates them (partial_sum / assign_delta ``image=``)."""
    t = torch()
    so = _lib.lib()
    nb = int(so.dkm_x_image_bytes(dd.n, dd.d, _lib.IMAGE_SORTED))
    if old is not None and old[0] is not None and old[0].numel() >= nb:
        img = old[0]
    else:
        free = t.cuda.mem_get_info(dd.device)[0]
        if nb == 0 or nb + _IMAGE_HEADROOM > free:
            return None, 0
        img = _alloc("image_sorted", nb, lambda: t.empty(
            nb, dtype=t.uint8, device=dd.device))
    if int(so.dkm_workspace_bytes(int(k), dd.d, dd.n)) > ws.nbytes:
        return None, 0
    f32 = dd.dtype == np.float32
    if acc is not None:
        fn = so.dkm_x_image_sorted_sums_f32 if f32 else \
            so.dkm_x_image_sorted_sums_f64
        _lib.check(fn(ptr(dd.X), dd.n, dd.d, dd.X.stride(0), ptr(labels),
                      int(k), ws.p, ws.nbytes, ptr(img), nb, ptr(acc),
                      stream_ptr()), "dkm_x_image_sorted_sums")
        return img, _lib.IMAGE_SORTED
    fn = so.dkm_x_image_sorted_f32 if f32 else so.dkm_x_image_sorted_f64
    _lib.check(fn(ptr(dd.X), dd.n, dd.d, dd.X.stride(0), ptr(labels), int(k),
                  ws.p, ws.nbytes, ptr(img), nb, stream_ptr()),
               "dkm_x_image_sorted")
    return img, _lib.IMAGE_SORTED


def label_sums(dd, ws, labels, acc, k):
    """acc += [sums | counts] of X by labels (dkm_label_sums_*)."""
    so = _lib.lib()
    fn = so.dkm_label_sums_f32 if dd.dtype == np.float32 else \
        so.dkm_label_sums_f64
    _lib.check(fn(ptr(dd.X), dd.n, dd.d, dd.X.stride(0), ptr(labels), int(k),
                  ws.p, ws.nbytes, ptr(acc), stream_ptr()), "dkm_label_sums")


class OrderedSums:
    """Buffers of a sums="reference" fit (dkm_ordered_sums_* and
    dkm_merge_tree): the grouping workspace, the Subset offsets on the
    device, the partials of ALL ranks' Subsets (``n_total`` x k (d + 1) fp64;
    this rank fills the ``dd``'s Subsets from slot ``first``) and the merge
    schedule with its scratch.  Raises ValueError when the partials and the
    scratch would leave less than 4 GiB of HBM free."""

    def __init__(self, dd, k, first, n_total, schedule, n_ops, n_slots):
        t = torch()
        so = _lib.lib()
        self.k, self.len = int(k), int(k) * (dd.d + 1)
        self.n_local, self.first = len(dd.sizes), int(first)
        self.n_total, self.n_ops = int(n_total), int(n_ops)
        nb = (self.n_total + int(n_slots)) * self.len * 8
        free = t.cuda.mem_get_info(dd.device)[0]
        if nb + _IMAGE_HEADROOM > free:
            raise ValueError(
                "sums='reference' keeps one partial [sums | counts] per "
                "Subset: %d Subsets x k (d + 1) = %d values need %.2f GiB "
                "of HBM, and %.2f GiB are free (4 GiB stay free); use "
                "larger Subsets" % (self.n_total, self.len, nb / 2.0 ** 30,
                                    free / 2.0 ** 30))
        self.partials = _alloc("partials", self.n_total * self.len * 8,
                               lambda: t.zeros(self.n_total * self.len,
                                               dtype=t.float64,
                                               device=dd.device))
        self.scratch = t.empty(max(1, int(n_slots)) * self.len,
                               dtype=t.float64, device=dd.device)
        self.schedule = t.from_numpy(np.ascontiguousarray(
            schedule, dtype=np.int32)).to(dd.device) if n_ops else None
        self.offsets = t.from_numpy(np.ascontiguousarray(
            dd.offsets, dtype=np.int64)).to(dd.device)
        self.ws = None
        if self.n_local:
            nws = int(so.dkm_ordered_workspace_bytes(dd.n, self.n_local,
                                                     self.k, dd.d))
            if nws == 0:
                raise ValueError(
                    "sums='reference' takes n < 2**31 - 1 rows per rank and "
                    "k <= 8191, got n = %d, k = %d" % (dd.n, self.k))
            self.ws = _alloc("ordered", nws, lambda: t.empty(
                nws, dtype=t.uint8, device=dd.device))

    def group_order(self, n):
        """The row indices grouped stably by (Subset, label) that the last
        :func:`ordered_sums` left in the workspace (int32 view)."""
        return self.ws[:4 * n].view(torch().int32)


def ordered_sums(dd, labels, osum):
    """This rank's slots of ``osum.partials`` <- the per-Subset [sums |
    counts] of X by labels in the reference's order (dkm_ordered_sums_*)."""
    if osum.n_local == 0:
        return
    so = _lib.lib()
    fn = so.dkm_ordered_sums_f32 if dd.dtype == np.float32 else \
        so.dkm_ordered_sums_f64
    own = osum.partials[osum.first * osum.len:]
    _lib.check(fn(ptr(dd.X), dd.n, dd.d, dd.X.stride(0) if dd.n else dd.d,
                  ptr(labels), osum.k, ptr(osum.offsets), osum.n_local,
                  ptr(osum.ws), osum.ws.numel(), ptr(own), stream_ptr()),
               "dkm_ordered_sums")


def merge_tree(osum, acc, f32):
    """acc <- the arity tree's root over ``osum.partials``
    (dkm_merge_tree); fp32 samples' sums fold in fp32."""
    so = _lib.lib()
    _lib.check(so.dkm_merge_tree(
        ptr(osum.partials), osum.n_total, osum.len, ptr(osum.schedule),
        osum.n_ops, osum.k * (osum.len // osum.k - 1) if f32 else 0,
        ptr(osum.scratch), ptr(acc), stream_ptr()), "dkm_merge_tree")


# ---------------------------------------------------------------------------
# StandardScaler (dkm_scale.hip)
# ---------------------------------------------------------------------------
# rows whose loads a dkm_col_chain_* chain issues together (CH_U)
SCALE_CHAIN_TILE = 16
# the grid of dkm_col_stats_* / dkm_scale_transform_*: a block per 16384
# elements, 2048 blocks at the most (SC_GRID)
SCALE_GRID_UNIT = 16384
SCALE_GRID_CAP = 2048


def scale_grid(n, d):
    """Blocks of dkm_col_stats_* / dkm_scale_transform_* on (n, d): the
    plan of dkm_scale.hip restated, for the tests to name the branch a
    shape reaches."""
    if n <= 0:
        return 0
    work = (n * d + SCALE_GRID_UNIT - 1) // SCALE_GRID_UNIT
    return max(1, min(work, SCALE_GRID_CAP))


def scale_workspace_bytes(n, d):
    """dkm_scale_workspace_bytes restated: a partial per block and column."""
    return (max(1, scale_grid(n, d)) * d * 8 + 255) // 256 * 256


def scale_row_tile(d, dtype, vector=True):
    """Rows one block of dkm_col_stats_* / dkm_scale_transform_* takes per
    step on d columns (SC_B / pieces x SC_U of dkm_scale.hip): the sizes
    around which the tests cut their Subsets."""
    v = 16 // np.dtype(dtype).itemsize
    cv = d // v if vector and d % v == 0 else d
    return 256 // min(256, cv) * 4


class ScaleSums:
    """Buffers of a StandardScaler(sums="reference") fit: the Subset offsets
    on the device, the partials of ALL ranks' Subsets (``n_total`` x (d + 1)
    fp64, a row = [column sums | rows]; this rank fills its Subsets from slot
    ``first``) and the merge schedule with its scratch -- the slot scheme of
    :class:`OrderedSums` with one cluster, so :func:`merge_tree` takes it."""

    def __init__(self, dd, first, n_total, schedule, n_ops, n_slots):
        t = torch()
        self.k, self.len = 1, dd.d + 1
        self.n_local, self.first = len(dd.sizes), int(first)
        self.n_total, self.n_ops = int(n_total), int(n_ops)
        self.partials = _alloc("scale partials", self.n_total * self.len * 8,
                               lambda: t.zeros(self.n_total * self.len,
                                               dtype=t.float64,
                                               device=dd.device))
        self.scratch = t.empty(max(1, int(n_slots)) * self.len,
                               dtype=t.float64, device=dd.device)
        self.schedule = t.from_numpy(np.ascontiguousarray(
            schedule, dtype=np.int32)).to(dd.device) if n_ops else None
        self.offsets = t.from_numpy(np.ascontiguousarray(
            dd.offsets, dtype=np.int64)).to(dd.device)
        self.acc = t.empty(self.len, dtype=t.float64, device=dd.device)

    def reset(self, sizes):
        """Zero every slot (the other ranks' add +0.0) and write this rank's
        row counts."""
        t = torch()
        self.partials.zero_()
        if self.n_local:
            own = self.partials.view(self.n_total, self.len)[
                self.first:self.first + self.n_local]
            own[:, self.len - 1] = t.tensor(
                [float(s) for s in sizes], dtype=t.float64).to(own.device)


def col_chain(dd, mean, ssum):
    """This rank's slots of ``ssum.partials`` <- the per-Subset column sums
    of x (``mean`` None) or (x - mean)^2 in the reference's order
    (dkm_col_chain_*); ``mean``: a device vector of X's dtype."""
    if ssum.n_local == 0:
        return
    so = _lib.lib()
    fn = so.dkm_col_chain_f32 if dd.dtype == np.float32 else \
        so.dkm_col_chain_f64
    own = ssum.partials[ssum.first * ssum.len:]
    _lib.check(fn(ptr(dd.X), dd.n, dd.d, dd.X.stride(0) if dd.n else dd.d,
                  ptr(mean), ptr(ssum.offsets), ssum.n_local, ptr(own),
                  ssum.len, stream_ptr()), "dkm_col_chain")


def scale_workspace(dd):
    """The workspace of :func:`col_stats` for ``dd``."""
    t = torch()
    nb = int(_lib.lib().dkm_scale_workspace_bytes(dd.n, dd.d))
    if nb == 0:
        raise _lib.DkmError("dkm_scale_workspace_bytes: bad n/d")
    return _alloc("scale", nb, lambda: t.empty(nb, dtype=t.uint8,
                                               device=dd.device))


def col_stats(dd, mean, ws, out):
    """out[d] (fp64) <- the column sums of x (``mean`` None) or of
    (x - mean)^2 (``mean``: device fp64[d]), dkm_col_stats_*."""
    so = _lib.lib()
    fn = so.dkm_col_stats_f32 if dd.dtype == np.float32 else \
        so.dkm_col_stats_f64
    _lib.check(fn(ptr(dd.X), dd.n, dd.d, dd.X.stride(0) if dd.n else dd.d,
                  ptr(mean), ptr(ws), ws.numel(), ptr(out), stream_ptr()),
               "dkm_col_stats")


def scale_transform(dd, mean, var, Y):
    """Y <- (X - mean) / sqrt(var) (dkm_scale_transform_*): ``mean`` / ``var``
    device vectors of one dtype, Y of numpy's promotion of it and X's."""
    t = torch()
    so = _lib.lib()
    s64 = mean.dtype == t.float64
    if dd.dtype == np.float32:
        fn = so.dkm_scale_transform_f32_f64 if s64 else \
            so.dkm_scale_transform_f32
    else:
        fn = so.dkm_scale_transform_f64 if s64 else \
            so.dkm_scale_transform_f64_f32
    ld = dd.X.stride(0) if dd.n else dd.d
    _lib.check(fn(ptr(dd.X), dd.n, dd.d, ld, ptr(mean), ptr(var), ptr(Y),
                  Y.stride(0) if dd.n else dd.d, stream_ptr()),
               "dkm_scale_transform")


# ---------------------------------------------------------------------------
# GaussianMixture (dkm_gm.hip)
# ---------------------------------------------------------------------------
# rows of a dkm_gm_estep_* wave tile / block and of an M-step MFMA step: the
# sizes around which the tests cut their row counts
GM_TILE = 16
GM_MSTEP_ROWS = 4


def gm_estep_block(d):
    """Rows one block of dkm_gm_estep_* takes on d columns."""
    return 64 if 64 < d <= 128 else 128


# the plan of dkm_gm.hip restated, for the tests to name the branch a shape
# reaches: rows of an M-step chunk (at least), most chunks, the size the
# covariance partials are capped at (about), threads of a block (the E-step's
# final sum and the folds of the M-step take that many partials per trip)
GM_CHUNK_ROWS = 512
GM_MAX_CHUNKS = 2048
GM_COV_WORKSPACE = 64 << 20
GM_BLOCK = 256


def gm_estep_blocks(n, d):
    """Blocks of dkm_gm_estep_* on n rows of d columns."""
    b = gm_estep_block(d)
    return (n + b - 1) // b


def gm_sums_chunks(n):
    """Row chunks of dkm_gm_mstep_sums_*."""
    return max(1, min((n + GM_CHUNK_ROWS - 1) // GM_CHUNK_ROWS,
                      GM_MAX_CHUNKS))


def gm_cov_tiles(d):
    """16 x 16 tiles of a covariance on or above the diagonal."""
    p = (d + 15) // 16
    return p * (p + 1) // 2


def gm_cov_chunks(n, d, k):
    """Row chunks of dkm_gm_mstep_cov_*: the sums' chunks, capped so that
    the partials (2048 B per chunk, component and tile) stay within about
    GM_COV_WORKSPACE -- but never below 8."""
    cap = max(8, GM_COV_WORKSPACE // (k * gm_cov_tiles(d) * 2048))
    return max(1, min(gm_sums_chunks(n), cap))


def gm_chunk_rows(n, chunks):
    """Rows of an M-step chunk: a multiple of 4."""
    return ((n + chunks - 1) // chunks + 3) // 4 * 4


def gm_workspace_bytes(n, d, k):
    """dkm_gm_workspace_bytes restated: the largest of the E-step's block
    partials, the sums' partials and the covariances' partials."""
    b = max(1, gm_estep_blocks(n, d)) * 8
    b = max(b, gm_sums_chunks(n) * k * (d + 1) * 8)
    b = max(b, gm_cov_chunks(n, d, k) * k * gm_cov_tiles(d) * 2048)
    return (b + 255) // 256 * 256


def gm_workspace(dd, k):
    """The workspace of the three GaussianMixture passes on ``dd``."""
    t = torch()
    nb = int(_lib.lib().dkm_gm_workspace_bytes(dd.n, dd.d, int(k)))
    if nb == 0:
        raise _lib.DkmError("dkm_gm_workspace_bytes: bad n/d/k")
    return _alloc("gm", nb, lambda: t.empty(nb, dtype=t.uint8,
                                            device=dd.device))


def alloc_resp(dd, k):
    """The resident (n, k) fp64 responsibilities; ValueError when they would
    leave less than 4 GiB of HBM free (the rule of sums="reference")."""
    t = torch()
    nb = 8 * dd.n * int(k)
    free = t.cuda.mem_get_info(dd.device)[0]
    if nb + _IMAGE_HEADROOM > free:
        raise ValueError(
            "GaussianMixture keeps the responsibilities resident: %d x %d "
            "fp64 need %.2f GiB of HBM, and %.2f GiB are free (4 GiB stay "
            "free)" % (dd.n, k, nb / 2.0 ** 30, free / 2.0 ** 30))
    return _alloc("resp", nb, lambda: t.empty((dd.n, int(k)),
                                              dtype=t.float64,
                                              device=dd.device))


def gm_onehot(labels, resp):
    """resp[i, c] <- labels[i] == c (``labels``: device int32)."""
    n, k = resp.shape
    _lib.check(_lib.lib().dkm_gm_onehot(ptr(labels), n, k, ptr(resp),
                                        stream_ptr()), "dkm_gm_onehot")


def gm_estep(dd, means, pc, ldw, upper, ws, resp, labels, out):
    """resp, labels (device int64 or None) and out[0] = sum of the rows'
    log_prob_norm for the device parameters ``means`` (k, d), ``pc``
    (k, d, d) and ``ldw`` = log det + log weights (k); dkm_gm_estep_*."""
    so = _lib.lib()
    fn = so.dkm_gm_estep_f32 if dd.dtype == np.float32 else \
        so.dkm_gm_estep_f64
    _lib.check(fn(ptr(dd.X), dd.n, dd.d, dd.X.stride(0) if dd.n else dd.d,
                  ptr(means), ptr(pc), ptr(ldw), means.shape[0],
                  _lib.GM_UPPER if upper else 0, ptr(ws), ws.numel(),
                  ptr(resp), ptr(labels), ptr(out), stream_ptr()),
               "dkm_gm_estep")


def gm_mstep_sums(dd, resp, ws, out):
    """out (fp64, k + k d) <- [nk | resp^T X], dkm_gm_mstep_sums_*."""
    so = _lib.lib()
    fn = so.dkm_gm_mstep_sums_f32 if dd.dtype == np.float32 else \
        so.dkm_gm_mstep_sums_f64
    _lib.check(fn(ptr(dd.X), dd.n, dd.d, dd.X.stride(0) if dd.n else dd.d,
                  ptr(resp), resp.shape[1], ptr(ws), ws.numel(), ptr(out),
                  stream_ptr()), "dkm_gm_mstep_sums")


def gm_mstep_cov(dd, resp, means, ws, cov):
    """cov (k, d, d) <- sum_n r (x - mean)(x - mean)^T around the device
    ``means``, dkm_gm_mstep_cov_*."""
    so = _lib.lib()
    fn = so.dkm_gm_mstep_cov_f32 if dd.dtype == np.float32 else \
        so.dkm_gm_mstep_cov_f64
    _lib.check(fn(ptr(dd.X), dd.n, dd.d, dd.X.stride(0) if dd.n else dd.d,
                  ptr(resp), ptr(means), resp.shape[1], ptr(ws), ws.numel(),
                  ptr(cov), stream_ptr()), "dkm_gm_mstep_cov")


def add_(y, x, nonzero=None):
    """y += x; with ``nonzero`` (a device int32 element view): 1 there if any
    x != 0, else 0."""
    so = _lib.lib()
    if nonzero is None:
        _lib.check(so.dkm_add_f64(ptr(y), ptr(x), y.numel(), stream_ptr()),
                   "dkm_add_f64")
    else:
        _lib.check(so.dkm_add_f64_nz(ptr(y), ptr(x), y.numel(), ptr(nonzero),
                                     stream_ptr()), "dkm_add_f64_nz")


def add_dd_(hi, lo, x, nonzero=None):
    """(hi, lo) += x compensated (hi = the rounded running sums)."""
    so = _lib.lib()
    _lib.check(so.dkm_add_f64_dd(ptr(hi), ptr(lo), ptr(x), hi.numel(),
                                 ptr(nonzero), stream_ptr()), "dkm_add_f64_dd")


def predict(dd, C, ws, labels, mode):
    so = _lib.lib()
    k = C.shape[0]
    if dd.sparse:
        _lib.check(so.dkm_predict_csr_f64(
            ptr(dd.indptr), ptr(dd.indices), ptr(dd.data), dd.n, dd.d,
            ptr(C), k, ws.p, ws.nbytes, ptr(labels), stream_ptr()),
            "dkm_predict_csr_f64")
        return
    fn = so.dkm_predict_f32 if dd.dtype == np.float32 else so.dkm_predict_f64
    _lib.check(fn(ptr(dd.X), dd.n, dd.d, dd.X.stride(0), ptr(C), k, ws.p,
                  ws.nbytes, ptr(labels), mode, stream_ptr()),
               "dkm_predict")


def update(acc, C, sums_mode, tol, diff, flag):
    so = _lib.lib()
    k, d = C.shape
    _lib.check(so.dkm_update_centers(ptr(acc), ptr(C), k, d, sums_mode,
                                     float(tol), ptr(diff), ptr(flag),
                                     stream_ptr()), "dkm_update_centers")


def make_blobs(X, row0, n_blobs, seed, box=10.0, std=1.0, blob=None):
    so = _lib.lib()
    n, d = X.shape
    _lib.check(so.dkm_make_blobs_f64(ptr(X), int(row0), n, d, int(n_blobs),
                                     int(seed), float(box), float(std),
                                     ptr(blob), stream_ptr()),
               "dkm_make_blobs_f64")


def rechecked(ws):
    so = _lib.lib()
    out = ctypes.c_int64(0)
    _lib.check(so.dkm_screen_stats(ws.p, ctypes.byref(out), stream_ptr()),
               "dkm_screen_stats")
    return int(out.value)


def screen_counters(ws):
    """(threshold-pass tiles, tiles it decided, centre blocks screened over
    the label-sorted image, sorted-image tiles the steady-state pass handed
    to the general one) accumulated over the workspace's life."""
    so = _lib.lib()
    out = (ctypes.c_int64 * 4)()
    _lib.check(so.dkm_screen_counters(ws.p, out, stream_ptr()),
               "dkm_screen_counters")
    return tuple(int(x) for x in out)


def screen_lists(ws):
    """(re-check list, two-candidate, 3..6-candidate entries, overflowed
    samples) the last single-product screen launch left (diagnostics)."""
    so = _lib.lib()
    out = (ctypes.c_int64 * 4)()
    _lib.check(so.dkm_screen_lists(ws.p, ws.nbytes, out, stream_ptr()),
               "dkm_screen_lists")
    return tuple(int(x) for x in out)
