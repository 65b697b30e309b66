"""``RandomForestRegressor`` -- the regression forest later dislib releases
ship beside the classifier (``dislib.regression`` has none in v0.2.0, the tree
this package follows), grown on the GPU from a dense Dataset that is resident
in HBM.  The targets are the Subsets' ``labels``, one fp64
number per sample; ``predict`` writes its values into the labels.

Everything that is not about the targets is ``classification/rf.py``'s and is
imported from there: the bootstrap draws and their order from
``random_state``, ``resolve_try_features``, the counter-based feature draws
(``feature_order`` / ``mix``), the attempt slices and the node numbering, the
``threshold`` of a cut, the rank tables (``Prepared``, with zero class codes)
and the member lists (``Batch``), the first strictly smallest score among a
node's pairs (``best_of_node``) and the stable ``partition`` (with one class:
the left count is the left size).

What is new (``dkm_rfr.hip``):

* The split rule.  A node's entries of a feature are visited in (rank, sample
  index) order; after each run of equal ranks, with left weight ``ll``, left
  target sum ``SL``, node sum ``S`` and node size ``size``, the score is
  ``-(SL * SL / ll + SR * SR / rl)`` with ``SR = S - SL`` and ``rl = 1 if ll ==
  size else size - ll``, in fp64 with every operation rounded on its own.  The
  last minimum wins; a best position ``size - 1`` means no cut.  (Minimising it
  maximises the variance reduction: the sum of squares of the targets is the
  same for every cut.)
* A node is a leaf when its depth has reached ``max_depth``, when its targets
  are all equal (its minimum equals its maximum: on such a node all scores are
  equal up to rounding and a cut would be chosen by noise) or when every
  feature slice has been tried without a valid cut.  A leaf's value is the
  mean of its targets, ``sum / size``.
* The node's sum, minimum and maximum come from ``dkm_rfr_node_stats``, run on
  the roots and on the children after every partition; its sums are the ``S``
  of the next level's split search.
* ``predict`` adds the leaf values in tree order and divides by the number of
  trees (``dkm_rfr_predict_*``).

The sums are formed in a fixed order: a fit gives the same bits from run to
run.  ``distr_depth`` and ``sklearn_max`` are accepted, stored and unused.

Limits, each a loud error: dense Datasets only (``NotImplementedError`` for
CSR); one rank only (``NotImplementedError`` in a ``torch.distributed`` world
larger than 1); every Subset labelled with one finite number per sample and at
least one sample (``ValueError``); fewer than ``_lib.RF_MAX_SAMPLES`` samples;
``try_features`` within ``1..d``; finite samples; ``ValueError`` when the rank
tables, the distinct values and the targets (``rf.hbm_bytes(n, d) + 8 n``) do
not fit in free HBM.
"""
import numpy as np

from .. import _lib, _shard
from ..classification import rf

_NAME = "RandomForestRegressor"


def split_search(so, prep, yt, batch, nodes, nsum, pairs, max_size,
                 mode=_lib.RF_AUTO):
    """(score, cut) device tensors of the pairs (``dkm_rfr_split``); ``yt``
    the fp64 device targets, ``nodes`` (N, 4) and ``pairs`` (P, 2) device
    int32, ``nsum`` (N,) device fp64, ``max_size`` the largest node's size."""
    from .._device import ptr, stream_ptr, torch
    t = torch()
    P = int(pairs.shape[0])
    score = t.empty(P, dtype=t.float64, device=prep.device)
    cut = t.empty((P, 3), dtype=t.int32, device=prep.device)
    _lib.check(so.dkm_rfr_split(
        ptr(prep.rank), ptr(prep.order), prep.n, ptr(yt), ptr(batch.members),
        ptr(batch.node_of), ptr(batch.weight), ptr(nodes), ptr(nsum),
        ptr(pairs), P, int(max_size), mode, ptr(score), ptr(cut),
        stream_ptr()), "dkm_rfr_split")
    return score, cut


def node_stats(so, prep, yt, batch, nodes):
    """(N, 3) device fp64 {sum, min, max} of the nodes' targets
    (``dkm_rfr_node_stats``)."""
    from .._device import ptr, stream_ptr, torch
    t = torch()
    N = int(nodes.shape[0])
    stats = t.empty((N, 3), dtype=t.float64, device=prep.device)
    _lib.check(so.dkm_rfr_node_stats(ptr(yt), prep.n, ptr(batch.members),
                                     ptr(nodes), N, ptr(stats), stream_ptr()),
               "dkm_rfr_node_stats")
    return stats


class Forest(rf.Forest):
    """The classifier's flat node arrays; a leaf has its mean ``lvalue`` and
    its ``lsize``."""

    def __init__(self):
        rf.Forest.__init__(self, 1)
        self.lvalue = np.empty(0, np.float64)
        self.lsize = np.empty(0, np.int32)

    def close(self, g, sums, sizes):
        """Nodes g become leaves with the target sums and sizes given."""
        l0 = len(self.lvalue)
        self.lvalue = np.concatenate((self.lvalue, sums / sizes))
        self.lsize = np.concatenate((self.lsize, sizes.astype(np.int32)))
        self.child[g] = np.arange(l0, l0 + len(g), dtype=np.int32)[:, None]

    def device(self, dev):
        if self._dev is None or self._dev[0] != dev:
            from .._device import torch
            t = torch()
            self._dev = (dev, [rf._i32(self.roots, dev),
                               rf._i32(self.feature, dev),
                               t.from_numpy(self.value).to(dev),
                               rf._i32(self.child, dev),
                               t.from_numpy(self.lvalue).to(dev)])
        return self._dev[1]

    def tree_arrays(self, i):
        """Tree i alone, its nodes renumbered in creation order."""
        g = np.flatnonzero(self.tree == i)
        new = np.full(len(self.feature), -1, np.int64)
        new[g] = np.arange(len(g))
        leaf = self.feature[g] < 0
        lf = self.child[g][leaf, 0]
        child = np.where(leaf[:, None], -1, new[self.child[g]])
        leaf_of = np.full(len(g), -1, np.int64)
        leaf_of[leaf] = np.arange(len(lf))
        return dict(feature=self.feature[g], value=self.value[g], child=child,
                    leaf=leaf_of, leaf_value=self.lvalue[lf],
                    size=self.lsize[lf])


def grow(so, prep, yt, samples, seeds, first_tree, try_features, max_depth,
         forest, mode=_lib.RF_AUTO, times=None):
    """Grows the trees of one batch (bootstrap ``samples``, (T, n); feature
    seeds ``seeds``) into ``forest``, level by level with one read-back per
    level (``rf.grow`` with target sums in place of class counts)."""
    from .._device import torch
    t = torch()
    dev, n, d = prep.device, prep.n, prep.d
    batch = rf.Batch(prep, samples)
    T = batch.T
    seeds = np.asarray(seeds, dtype=np.uint64)
    g = forest.add_nodes(first_tree + np.arange(T))
    forest.roots = np.concatenate((forest.roots, g.astype(np.int32)))
    roots = np.stack((np.arange(T), np.zeros(T, np.int64),
                      np.full(T, n), np.zeros(T, np.int64)), axis=1)
    st = node_stats(so, prep, yt, batch, rf._i32(roots, dev)).cpu().numpy()
    # the frontier, ordered by tree: one entry per open node
    fr = dict(tree=np.arange(T), start=np.zeros(T, np.int64),
              size=np.full(T, n, np.int64), depth=np.zeros(T, np.int64),
              attempt=np.zeros(T, np.int64), id=np.zeros(T, np.int64),
              sum=st[:, 0].copy(), g=g)
    next_id = np.ones(T, np.int64)
    leaf = (st[:, 1] == st[:, 2]) | (0 >= max_depth)
    forest.close(fr["g"][leaf], fr["sum"][leaf], fr["size"][leaf])
    fr = {k: v[~leaf] for k, v in fr.items()}
    while len(fr["tree"]):
        N = len(fr["tree"])
        tr = fr["tree"]
        order = rf.feature_order(seeds[tr], fr["id"], d)
        a0 = fr["attempt"] * try_features
        k = np.minimum(try_features, d - a0)
        pfirst = np.concatenate(([0], np.cumsum(k)[:-1]))
        pnode = np.repeat(np.arange(N), k)
        pcol = np.arange(len(pnode)) - pfirst[pnode] + a0[pnode]
        pairs = rf._i32(np.stack((pnode, order[pnode, pcol]), axis=1), dev)
        pspan = rf._i32(np.stack((pfirst, k), axis=1), dev)
        # children's numbers: per tree, two per open node in frontier order
        first = np.searchsorted(tr, tr, side="left")
        cid = next_id[tr] + 2 * (np.arange(N) - first)
        next_id += 2 * np.bincount(tr, minlength=T)
        base = np.stack((tr, fr["start"], fr["size"]), axis=1)
        nodes = rf._i32(np.concatenate((base, fr["id"][:, None]), axis=1), dev)
        kids = rf._i32(np.concatenate((base, cid[:, None]), axis=1), dev)
        nsum = t.from_numpy(np.ascontiguousarray(fr["sum"])).to(dev)

        ev = rf._events(times)
        score, cut = split_search(so, prep, yt, batch, nodes, nsum, pairs,
                                  fr["size"].max(), mode)
        best = rf.best_of_node(so, nodes, pspan, pairs, score, cut)
        rf._mark(ev)
        rf.partition(so, prep, 1, batch, kids, best)
        # the two children of every node, in place: {tree, start, left size}
        # and {tree, start + left size, the rest} (no cut: left size 0)
        two = kids[:, None, :].repeat(1, 2, 1)
        two[:, 1, 1] += best[:, 3]
        two[:, 0, 2] = best[:, 3]
        two[:, 1, 2] -= best[:, 3]
        stats = node_stats(so, prep, yt, batch, two.reshape(2 * N, 4))
        rf._mark(ev)
        fcl = best[:, 0].clamp(min=0).long()
        lo = prep.values[prep.voff_dev[fcl] + best[:, 1]]
        hi = prep.values[prep.voff_dev[fcl] + best[:, 2]]
        back = t.cat((best.double().flatten(), stats.flatten(), lo,
                      hi)).cpu().numpy()
        rf._collect(ev, times, int(fr["size"].max()) > _lib.RFR_LDS_MAX
                    and mode != _lib.RF_LDS or mode == _lib.RF_STREAM)
        best_h = back[:4 * N].reshape(N, 4).astype(np.int64)
        st = back[4 * N:10 * N].reshape(N, 2, 3)
        lo, hi = back[10 * N:11 * N], back[11 * N:]

        cutm = best_h[:, 0] >= 0
        # nodes without a cut: the next slice of features, or a leaf
        again = ~cutm & ((fr["attempt"] + 1) * try_features < d)
        done = ~cutm & ~again
        forest.close(fr["g"][done], fr["sum"][done], fr["size"][done])
        # nodes with a cut: two children
        sp = np.flatnonzero(cutm)
        pg = fr["g"][sp]
        forest.feature[pg] = best_h[sp, 0]
        forest.value[pg] = rf.threshold(lo[sp], hi[sp])
        cg = forest.add_nodes(np.repeat(first_tree + tr[sp], 2))
        forest.child[pg] = cg.reshape(-1, 2)
        nl = best_h[sp, 3]
        cst = st[sp].reshape(-1, 3)
        ch = dict(
            tree=np.repeat(tr[sp], 2),
            start=np.stack((fr["start"][sp], fr["start"][sp] + nl), 1).ravel(),
            size=np.stack((nl, fr["size"][sp] - nl), 1).ravel(),
            depth=np.repeat(fr["depth"][sp] + 1, 2),
            attempt=np.zeros(2 * len(sp), np.int64),
            id=np.stack((cid[sp], cid[sp] + 1), 1).ravel(),
            sum=cst[:, 0].copy(), g=cg)
        leaf = (cst[:, 1] == cst[:, 2]) | (ch["depth"] >= max_depth)
        forest.close(ch["g"][leaf], ch["sum"][leaf], ch["size"][leaf])
        re = {kk: v[again] for kk, v in fr.items()}
        re["attempt"] = re["attempt"] + 1
        fr = {kk: np.concatenate((re[kk], ch[kk][~leaf])) for kk in fr}
        o = np.argsort(fr["tree"], kind="stable")
        fr = {kk: v[o] for kk, v in fr.items()}


def forest_predict(so, X, f32, forest):
    """Device fp64 (n,): the forest's mean over the rows of X."""
    from .._device import ptr, stream_ptr, torch
    t = torch()
    n, T = int(X.shape[0]), len(forest.roots)
    out = t.empty(n, dtype=t.float64, device=X.device)
    roots, feature, value, child, lvalue = forest.device(X.device)
    fn = so.dkm_rfr_predict_f32 if f32 else so.dkm_rfr_predict_f64
    _lib.check(fn(ptr(X), n, X.shape[1], X.stride(0) if n else X.shape[1],
                  ptr(roots), T, ptr(feature), ptr(value), ptr(child),
                  ptr(lvalue), ptr(out), stream_ptr()), "dkm_rfr_predict")
    return out


class RandomForestRegressor(object):
    """Random forest regression on MI355X (see the module docstring).

    Parameters are those of ``RandomForestClassifier`` without ``hard_vote``;
    ``device`` and ``profile`` are keyword-only extensions.

    Attributes
    ----------
    trees : list of dict
        Per tree and node in creation order ``feature`` (-1: a leaf),
        ``value`` (the threshold), ``child`` and ``leaf`` (its row of
        ``leaf_value``, the leaf means, and ``size``, or -1).
    times_ : dict or None
        The phases of ``fit`` in ms when ``profile`` is set.
    """

    def __init__(self, n_estimators=10, try_features='sqrt',
                 max_depth=np.inf, distr_depth='auto', sklearn_max=1e8,
                 random_state=None, *, device=None, profile=False):
        from sklearn.utils import check_random_state
        self.n_estimators = n_estimators
        self.try_features_init = try_features
        self.max_depth = max_depth
        self.distr_depth_init = distr_depth
        self.sklearn_max = sklearn_max
        self.random_state = check_random_state(random_state)
        self._device = device
        # True: fit times its phases with device events into ``times_``
        # (tools/bench_rfr.py); it synchronises after every level
        self._profile = profile
        self.trees = None
        self.times_ = None

    def fit(self, dataset):
        """Fits the forest on the ``dataset``, whose labels are the targets."""
        import time
        self.trees, self._forest = [], None
        self._checked(dataset)
        y = _targets(dataset)
        n, d = len(y), int(dataset.n_features)
        if n >= _lib.RF_MAX_SAMPLES:
            raise ValueError("%s takes fewer than %d samples, got %d"
                             % (_NAME, _lib.RF_MAX_SAMPLES, n))
        self.try_features = rf.resolve_try_features(self.try_features_init, d)
        if not 1 <= self.try_features <= d:
            raise ValueError("try_features resolves to %d with %d features"
                             % (self.try_features, d))
        so = _lib.lib()
        from .._device import _IMAGE_HEADROOM, on, preload, torch
        dd = dataset._device_data(self._device)
        t = torch()
        with on(dd.device):
            preload(dd.device)
            if not bool(t.isfinite(dd.X).all().item()):
                raise ValueError("%s takes finite samples: the Dataset holds "
                                 "NaN or infinity" % _NAME)
            free = t.cuda.mem_get_info(dd.device)[0]
            need = rf.hbm_bytes(n, d) + 8 * n
            if need + _IMAGE_HEADROOM > free:
                raise ValueError(
                    "%s keeps the sorted order, the ranks and the distinct "
                    "values of every feature and the targets resident: %d x "
                    "%d need up to %.2f GiB of HBM, and %.2f GiB are free (4 "
                    "GiB stay free)" % (_NAME, n, d, need / 2.0 ** 30,
                                        free / 2.0 ** 30))
            if self._profile:
                t.cuda.synchronize()
            t0 = time.perf_counter()
            prep = rf.Prepared(dd.X, np.zeros(n, np.int32))
            yt = t.from_numpy(y).to(dd.device)
            if self._profile:
                t.cuda.synchronize()
            self.times_ = {"prepare_ms": 1e3 * (time.perf_counter() - t0)} \
                if self._profile else None
            imax = np.iinfo(np.int32).max
            draws = [(self.random_state.randint(imax),
                      self.random_state.randint(imax))
                     for _ in range(self.n_estimators)]
            free = t.cuda.mem_get_info(dd.device)[0] - _IMAGE_HEADROOM
            per = int(max(1, min(self.n_estimators, free // (24 * n))))
            forest = Forest()
            for b in range(0, self.n_estimators, per):
                part = draws[b:b + per]
                samples = np.stack([np.random.RandomState(s).choice(
                    n, size=n, replace=True) for s, _ in part])
                grow(so, prep, yt, samples, [s for _, s in part], b,
                     self.try_features, self.max_depth, forest,
                     times=self.times_)
        self._forest, self._d, self._dev = forest, d, dd.device
        self.trees = [forest.tree_arrays(i) for i in range(self.n_estimators)]
        self.distr_depth = self.distr_depth_init

    def fit_predict(self, dataset):
        self.fit(dataset)
        self.predict(dataset)

    def _run(self, dataset):
        """(device fp64 predictions, the DeviceData) of the rows."""
        assert self.trees, 'The random forest is not fitted.'
        self._checked(dataset)
        if int(dataset.n_features) != self._d:
            raise ValueError("the forest was fitted on %d features, the "
                             "Dataset has %d" % (self._d, dataset.n_features))
        from .._device import on
        dd = dataset._device_data(self._dev)
        with on(dd.device):
            return forest_predict(_lib.lib(), dd.X, dd.dtype == np.float32,
                                  self._forest), dd

    def predict(self, dataset):
        """Writes the predicted value of every sample into the Subsets'
        labels, fp64: views of one device vector when every Subset holds a
        device tensor, else slices of one host copy."""
        from .._device import _is_torch
        out, dd = self._run(dataset)
        subsets = list(dataset)
        if not all(_is_torch(s.samples) for s in subsets):
            out = out.cpu().numpy()
        for s, (a, b) in zip(subsets, dd.subset_slices()):
            s.labels = out[a:b]
        dataset._labels = None

    def score(self, dataset):
        """R^2 of ``predict`` against the labels the Subsets hold (which stay
        as they are), in fp64 on the host."""
        true = _targets(dataset)
        pred = self._run(dataset)[0].cpu().numpy()
        res = np.sum((true - pred) ** 2)
        return 1.0 - res / np.sum((true - true.mean()) ** 2)

    @staticmethod
    def _checked(dataset):
        if dataset.sparse:
            raise NotImplementedError(
                "%s takes a dense Dataset: CSR samples are not supported"
                % _NAME)
        if _shard.active():
            raise NotImplementedError(
                "%s runs on one rank: a torch.distributed world larger than "
                "1 is not supported" % _NAME)


def _targets(dataset):
    """The Subsets' labels as one fp64 host vector."""
    parts = []
    for i, s in enumerate(dataset):
        lab = s.labels
        if lab is None:
            raise ValueError("%s takes a labelled Dataset: Subset %d has no "
                             "labels (the targets)" % (_NAME, i))
        if hasattr(lab, "cpu"):
            lab = lab.cpu().numpy()
        try:
            v = np.asarray(lab).astype(np.float64)
        except (TypeError, ValueError):
            v = None
        if v is None or v.shape != (int(s.samples.shape[0]),) or \
                not np.isfinite(v).all():
            raise ValueError("%s: the labels of Subset %d are not one finite "
                             "number per sample" % (_NAME, i))
        parts.append(v)
    if not parts or not sum(len(p) for p in parts):
        raise ValueError("%s.fit takes a Dataset with samples" % _NAME)
    return np.ascontiguousarray(np.concatenate(parts))
