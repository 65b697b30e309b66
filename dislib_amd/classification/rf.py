"""``RandomForestClassifier`` -- ``dislib.classification.RandomForestClassifier``
(dislib v0.2.0, ``dislib/classification/rf``) grown on the GPU from a dense
Dataset that is resident in HBM.

Kept exactly: the split rule of ``test_split.py`` -- every cut between
distinct values of a feature is scored with the Gini proxy ``-(sum_c L_c^2 /
|L| + sum_c R_c^2 / |R|)`` in fp64, the last position of the minimum wins, a
node whose best position is its last one has no valid cut on that feature --
and ``_compute_split``'s choice of the first strictly smallest score among the
features tried.  Kept in substance: the constructor and its defaults, the
resolution of ``try_features``, the bootstrap (per tree two
``random_state.randint(np.iinfo(np.int32).max)`` in the reference's order, the
first seeding ``RandomState(seed).choice(n, n, replace=True)``), ``max_depth``,
``hard_vote``, ``classes``, ``trees``, ``fit`` / ``fit_predict`` / ``predict``
/ ``predict_proba`` / ``score``.

What differs on purpose (tree-for-tree parity with the reference is not a
goal: by default it hands its nodes to sklearn's tree, and its own feature
draws are sequential, data dependent and depth first):

* Feature draws are counter-based, so that all nodes of a level grow in one
  launch.  A node tries the features in the order of a stable ``argsort`` over
  f of :func:`mix` (tree seed, node number, f); attempt a takes
  ``try_features`` of them from position ``a * try_features``.  The tree seed
  is the second ``randint`` of the tree.  Node numbers are handed out per
  tree, level by level: the root is 0, and the i-th open node of a level gets
  ``next + 2 i`` and ``next + 2 i + 1`` for its children, whether it splits or
  not.
* A pure node becomes a leaf at once (the reference tries every feature and
  fails on each; the tree is the same).
* The threshold is the fp64 midpoint of the two neighbouring distinct values;
  if that rounds to the upper value the lower one is stored, so ``predict``'s
  ``x <= value`` sends every training row where ``fit`` sent it.  (The
  reference computes the midpoint in the input dtype, fits with ``<`` and
  predicts with ``<=``.)
* ``predict_proba`` averages the real leaf frequencies (the reference assigns
  them into ``int64`` arrays and so truncates them to 0 / 1).
* ``distr_depth`` and ``sklearn_max`` are accepted, stored and unused.
* ``RfDataset`` is not provided: ``fit`` takes a ``Dataset``.

Limits, each a loud error: dense Datasets only (``NotImplementedError`` for
CSR); one rank only (``NotImplementedError`` in a ``torch.distributed`` world
larger than 1); finite samples only (``ValueError``); every Subset labelled;
at most ``_lib.RF_MAX_CLASSES`` classes and fewer than ``_lib.RF_MAX_SAMPLES``
samples; ``ValueError`` when the rank tables and the distinct values
(:func:`hbm_bytes`) do not fit in free HBM.
"""
import math

import numpy as np

from .. import _lib
from .._device import _IMAGE_HEADROOM, on, preload, ptr, stream_ptr, torch

_M1 = np.uint64(0x9E3779B97F4A7C15)
_M2 = np.uint64(0xBF58476D1CE4E5B9)
_M3 = np.uint64(0x94D049BB133111EB)


def mix(seed, node, f):
    """splitmix64's finalizer over ``seed * M1 + node * M2 + f * M3`` (uint64
    arrays that broadcast)."""
    with np.errstate(over="ignore"):
        z = (np.asarray(seed, np.uint64) * _M1 + np.asarray(node, np.uint64)
             * _M2 + np.asarray(f, np.uint64) * _M3)
        z = (z ^ (z >> np.uint64(30))) * _M2
        z = (z ^ (z >> np.uint64(27))) * _M3
        return z ^ (z >> np.uint64(31))


def feature_order(seed, node, d):
    """(N, d): every node's features in the order it tries them."""
    z = mix(np.asarray(seed)[:, None], np.asarray(node)[:, None],
            np.arange(d)[None, :])
    return np.argsort(z, axis=1, kind="stable").astype(np.int32)


def resolve_try_features(try_features, n_features):
    if try_features is None:
        return n_features
    if try_features == 'sqrt':
        return int(math.sqrt(n_features))
    if try_features == 'third':
        return max(1, n_features // 3)
    return int(try_features)


def threshold(lo, hi):
    """The stored value of a cut between the distinct values lo < hi."""
    with np.errstate(over="ignore"):
        mid = (np.asarray(lo, np.float64) + np.asarray(hi, np.float64)) / 2
    return np.where(mid >= hi, lo, mid)


def _i32(a, device):
    return torch().from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(
        device)


def hbm_bytes(n, d):
    """What :class:`Prepared` may hold at once: order and rank (8 bytes per
    matrix element), the distinct values (up to 8 more, when all differ) and
    the sort of one feature (the fp64 column, its sorted copy, int64 indices
    and ranks, the run flags)."""
    return 16 * n * d + 48 * n


class Prepared(object):
    """Per fit, shared by all trees: ``order`` and ``rank`` (d x n int32 on
    the device, feature-major; equal values share a rank and -0.0 == 0.0),
    the distinct values of all features in one fp64 device vector ``values``
    (feature f from ``voff[f]``) and the class codes ``y``."""

    def __init__(self, X, codes):
        t = torch()
        n, d = int(X.shape[0]), int(X.shape[1])
        self.n, self.d, self.device = n, d, X.device
        self.order = t.empty((d, n), dtype=t.int32, device=X.device)
        self.rank = t.empty((d, n), dtype=t.int32, device=X.device)
        vals, voff = [], [0]
        for f in range(d):
            col = X[:, f].to(t.float64) + 0.0
            s, idx = t.sort(col, stable=True)
            new = t.ones(n, dtype=t.bool, device=X.device)
            new[1:] = s[1:] != s[:-1]
            self.rank[f][idx] = (t.cumsum(new, 0) - 1).to(t.int32)
            self.order[f] = idx.to(t.int32)
            vals.append(s[new])
            voff.append(voff[-1] + int(vals[-1].shape[0]))
        self.values = t.cat(vals)
        self.voff = np.asarray(voff[:-1], dtype=np.int64)
        self.voff_dev = t.from_numpy(self.voff).to(X.device)
        self.y = _i32(codes, X.device)


class Batch(object):
    """The device state of the trees that grow together: the expanded member
    lists (two buffers), ``node_of`` and ``weight``, n int32 per tree each."""

    def __init__(self, prep, samples):
        t = torch()
        T, n = len(samples), prep.n
        self.T = T
        w = np.zeros((T, n), dtype=np.int32)
        for i, s in enumerate(samples):
            w[i] = np.bincount(s, minlength=n)
        self.weight = _i32(w, prep.device)
        self.node_of = _i32(np.where(w > 0, 0, -1), prep.device)
        self.members = _i32(np.sort(np.asarray(samples), axis=1), prep.device)
        self.spare = t.empty_like(self.members)


def split_search(so, prep, C, batch, nodes, ncounts, pairs, max_size,
                 mode=_lib.RF_AUTO):
    """(score, cut) device tensors of the pairs (``dkm_rf_split``); ``nodes``
    (N, 4), ``ncounts`` (N, C) and ``pairs`` (P, 2) are device int32,
    ``max_size`` the largest node's size."""
    t = torch()
    P = int(pairs.shape[0])
    score = t.empty(P, dtype=t.float64, device=prep.device)
    cut = t.empty((P, 3), dtype=t.int32, device=prep.device)
    _lib.check(so.dkm_rf_split(
        ptr(prep.rank), ptr(prep.order), prep.n, ptr(prep.y), C,
        ptr(batch.members), ptr(batch.node_of), ptr(batch.weight),
        ptr(nodes), ptr(ncounts), ptr(pairs), P, int(max_size), mode,
        ptr(score), ptr(cut), stream_ptr()), "dkm_rf_split")
    return score, cut


def best_of_node(so, nodes, pspan, pairs, score, cut):
    t = torch()
    N = int(nodes.shape[0])
    best = t.empty((N, 4), dtype=t.int32, device=nodes.device)
    _lib.check(so.dkm_rf_best(ptr(nodes), ptr(pspan), ptr(pairs), ptr(score),
                              ptr(cut), N, ptr(best), stream_ptr()),
               "dkm_rf_best")
    return best


def partition(so, prep, C, batch, nodes, best):
    """Splits the nodes that have a cut (``nodes[:, 3]``: the left child's
    number), swaps the member buffers and returns the left class counts."""
    t = torch()
    N = int(nodes.shape[0])
    lcounts = t.empty((N, C), dtype=t.int32, device=nodes.device)
    _lib.check(so.dkm_rf_partition(
        ptr(prep.rank), prep.n, ptr(prep.y), C, ptr(nodes), ptr(best), N,
        ptr(batch.members), ptr(batch.spare), ptr(batch.node_of),
        ptr(lcounts), stream_ptr()), "dkm_rf_partition")
    batch.members, batch.spare = batch.spare, batch.members
    return lcounts


class Forest(object):
    """The flat arrays of all trees: node v has ``feature[v]`` (-1: a leaf),
    ``value[v]`` and ``child[v]`` (the two children, or the leaf number
    twice); a leaf has ``freq``, ``size`` and ``mode``; ``roots`` and the
    owning ``tree`` of every node."""

    def __init__(self, C):
        self.C = C
        self.feature = np.empty(0, np.int32)
        self.value = np.empty(0, np.float64)
        self.child = np.empty((0, 2), np.int32)
        self.tree = np.empty(0, np.int32)
        self.freq = np.empty((0, C), np.int32)
        self.roots = np.empty(0, np.int32)
        self._dev = None

    def add_nodes(self, tree):
        g0 = len(self.feature)
        k = len(tree)
        self.feature = np.concatenate((self.feature, np.full(k, -1, np.int32)))
        self.value = np.concatenate((self.value, np.zeros(k)))
        self.child = np.concatenate((self.child, np.zeros((k, 2), np.int32)))
        self.tree = np.concatenate((self.tree, np.asarray(tree, np.int32)))
        return np.arange(g0, g0 + k, dtype=np.int64)

    def close(self, g, counts):
        """Nodes g become leaves with the class counts ``counts``."""
        l0 = len(self.freq)
        self.freq = np.concatenate((self.freq, counts.astype(np.int32)))
        self.child[g] = np.arange(l0, l0 + len(g), dtype=np.int32)[:, None]

    @property
    def size(self):
        return self.freq.sum(axis=1).astype(np.int32)

    @property
    def mode(self):
        return np.argmax(self.freq, axis=1).astype(np.int32)

    def device(self, dev):
        if self._dev is None or self._dev[0] != dev:
            t = torch()
            self._dev = (dev, [_i32(self.roots, dev), _i32(self.feature, dev),
                               t.from_numpy(self.value).to(dev),
                               _i32(self.child, dev), _i32(self.freq, dev),
                               _i32(self.size, dev), _i32(self.mode, dev)])
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
                    leaf=leaf_of, frequencies=self.freq[lf],
                    size=self.size[lf], mode=self.mode[lf])


def grow(so, prep, C, samples, seeds, first_tree, try_features, max_depth,
         forest, mode=_lib.RF_AUTO, times=None):
    """Grows the trees of one batch (bootstrap ``samples``, (T, n); feature
    seeds ``seeds``) into ``forest``, level by level with one read-back per
    level."""
    t = torch()
    dev, n, d = prep.device, prep.n, prep.d
    batch = Batch(prep, samples)
    T = batch.T
    codes = prep.y.cpu().numpy()
    counts = np.stack([np.bincount(codes[s], minlength=C) for s in samples])
    seeds = np.asarray(seeds, dtype=np.uint64)
    g = forest.add_nodes(first_tree + np.arange(T))
    forest.roots = np.concatenate((forest.roots, g.astype(np.int32)))
    # the frontier, ordered by tree: one entry per open node
    fr = dict(tree=np.arange(T), start=np.zeros(T, np.int64),
              size=np.full(T, n, np.int64), depth=np.zeros(T, np.int64),
              attempt=np.zeros(T, np.int64), id=np.zeros(T, np.int64),
              counts=counts.astype(np.int64), g=g)
    next_id = np.ones(T, np.int64)
    leaf = (fr["counts"].max(axis=1) == fr["size"]) | (0 >= max_depth)
    forest.close(fr["g"][leaf], fr["counts"][leaf])
    fr = {k: v[~leaf] for k, v in fr.items()}
    while len(fr["tree"]):
        N = len(fr["tree"])
        tr = fr["tree"]
        order = feature_order(seeds[tr], fr["id"], d)
        a0 = fr["attempt"] * try_features
        k = np.minimum(try_features, d - a0)
        pfirst = np.concatenate(([0], np.cumsum(k)[:-1]))
        pnode = np.repeat(np.arange(N), k)
        pcol = np.arange(len(pnode)) - pfirst[pnode] + a0[pnode]
        pairs = _i32(np.stack((pnode, order[pnode, pcol]), axis=1), dev)
        pspan = _i32(np.stack((pfirst, k), axis=1), dev)
        # children's numbers: per tree, two per open node in frontier order
        first = np.searchsorted(tr, tr, side="left")
        cid = next_id[tr] + 2 * (np.arange(N) - first)
        next_id += 2 * np.bincount(tr, minlength=T)
        base = np.stack((tr, fr["start"], fr["size"]), axis=1)
        nodes = _i32(np.concatenate((base, fr["id"][:, None]), axis=1), dev)
        kids = _i32(np.concatenate((base, cid[:, None]), axis=1), dev)
        ncounts = _i32(fr["counts"], dev)

        ev = _events(times)
        score, cut = split_search(so, prep, C, batch, nodes, ncounts, pairs,
                                  fr["size"].max(), mode)
        best = best_of_node(so, nodes, pspan, pairs, score, cut)
        _mark(ev)
        lcounts = partition(so, prep, C, batch, kids, best)
        _mark(ev)
        fcl = best[:, 0].clamp(min=0).long()
        lo = prep.values[prep.voff_dev[fcl] + best[:, 1]]
        hi = prep.values[prep.voff_dev[fcl] + best[:, 2]]
        back = t.cat((best.double().flatten(), lcounts.double().flatten(),
                      lo, hi)).cpu().numpy()
        _collect(ev, times, int(fr["size"].max()) > _lib.RF_LDS_MAX
                 and mode != _lib.RF_LDS or mode == _lib.RF_STREAM)
        best_h = back[:4 * N].reshape(N, 4).astype(np.int64)
        lc = back[4 * N:4 * N + N * C].reshape(N, C).astype(np.int64)
        lo, hi = back[4 * N + N * C:5 * N + N * C], back[5 * N + N * C:]

        cutm = best_h[:, 0] >= 0
        # nodes without a cut: the next slice of features, or a leaf
        again = ~cutm & ((fr["attempt"] + 1) * try_features < d)
        done = ~cutm & ~again
        forest.close(fr["g"][done], fr["counts"][done])
        # nodes with a cut: two children
        sp = np.flatnonzero(cutm)
        pg = fr["g"][sp]
        forest.feature[pg] = best_h[sp, 0]
        forest.value[pg] = threshold(lo[sp], hi[sp])
        cg = forest.add_nodes(np.repeat(first_tree + tr[sp], 2))
        forest.child[pg] = cg.reshape(-1, 2)
        nl = best_h[sp, 3]
        ch = dict(
            tree=np.repeat(tr[sp], 2),
            start=np.stack((fr["start"][sp], fr["start"][sp] + nl), 1).ravel(),
            size=np.stack((nl, fr["size"][sp] - nl), 1).ravel(),
            depth=np.repeat(fr["depth"][sp] + 1, 2),
            attempt=np.zeros(2 * len(sp), np.int64),
            id=np.stack((cid[sp], cid[sp] + 1), 1).ravel(),
            counts=np.stack((lc[sp], fr["counts"][sp] - lc[sp]), 1).reshape(
                -1, C),
            g=cg)
        leaf = (ch["counts"].max(axis=1) == ch["size"]) | (
            ch["depth"] >= max_depth)
        forest.close(ch["g"][leaf], ch["counts"][leaf])
        re = {kk: v[again] for kk, v in fr.items()}
        re["attempt"] = re["attempt"] + 1
        fr = {kk: np.concatenate((re[kk], ch[kk][~leaf])) for kk in fr}
        o = np.argsort(fr["tree"], kind="stable")
        fr = {kk: v[o] for kk, v in fr.items()}


def _events(times):
    if times is None:
        return None
    t = torch()
    e = [t.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    return [e, 1]


def _mark(ev):
    if ev is not None:
        ev[0][ev[1]].record()
        ev[1] += 1


def _collect(ev, times, streamed):
    if ev is None:
        return
    e = ev[0]
    e[2].synchronize()
    key = "split_stream_ms" if streamed else "split_lds_ms"
    times[key] = times.get(key, 0.0) + e[0].elapsed_time(e[1])
    times["partition_ms"] = times.get("partition_ms", 0.0) + \
        e[1].elapsed_time(e[2])


def forest_predict(so, X, f32, forest, hard):
    """Device (proba (n, C) fp64, labels int32) of the rows of X."""
    t = torch()
    n, C, T = int(X.shape[0]), forest.C, len(forest.roots)
    proba = t.empty((n, C), dtype=t.float64, device=X.device)
    labels = t.empty(n, dtype=t.int32, device=X.device)
    votes = t.empty((n, T), dtype=t.int32, device=X.device) if hard else None
    roots, feature, value, child, freq, size, mode = forest.device(X.device)
    fn = so.dkm_rf_predict_f32 if f32 else so.dkm_rf_predict_f64
    _lib.check(fn(ptr(X), n, X.shape[1], X.stride(0) if n else X.shape[1],
                  ptr(roots), T, ptr(feature), ptr(value), ptr(child),
                  ptr(freq), ptr(size), ptr(mode), C, 1 if hard else 0,
                  ptr(proba), ptr(votes), ptr(labels), stream_ptr()),
               "dkm_rf_predict")
    return proba, labels


class RandomForestClassifier(object):
    """Random forest classification on MI355X (see the module docstring).

    Parameters match ``dislib.classification.RandomForestClassifier``;
    ``device`` is a keyword-only extension.
    """

    def __init__(self, n_estimators=10, try_features='sqrt',
                 max_depth=np.inf, distr_depth='auto', sklearn_max=1e8,
                 hard_vote=False, random_state=None, *, device=None,
                 profile=False):
        from sklearn.utils import check_random_state
        self.n_estimators = n_estimators
        self.try_features_init = try_features
        self.max_depth = max_depth
        self.distr_depth_init = distr_depth
        self.sklearn_max = sklearn_max
        self.hard_vote = hard_vote
        self.random_state = check_random_state(random_state)
        self._device = device
        # True: fit times its phases with device events into ``times_``
        # (tools/bench_rf.py); it synchronises after every level
        self._profile = profile
        self.classes = None
        self.trees = None
        self.times_ = None

    def fit(self, dataset):
        """Fits the forest on the labelled ``dataset``."""
        import time

        from .. import _shard
        self.classes, self.trees, self._forest = None, [], None
        if dataset.sparse:
            raise NotImplementedError(
                "RandomForestClassifier takes a dense Dataset: CSR samples "
                "are not supported")
        if _shard.active():
            raise NotImplementedError(
                "RandomForestClassifier runs on one rank: a "
                "torch.distributed world larger than 1 is not supported")
        parts = []
        for s in dataset:
            if s.labels is None:
                raise ValueError("RandomForestClassifier.fit takes a labelled "
                                 "Dataset: a Subset has no labels")
            parts.append(np.asarray(s.labels))
        if not parts:
            raise ValueError("RandomForestClassifier.fit takes a Dataset "
                             "with samples")
        labels = np.concatenate(parts)
        classes, codes = np.unique(labels, return_inverse=True)
        n, d, C = len(labels), int(dataset.n_features), len(classes)
        if C > _lib.RF_MAX_CLASSES:
            raise ValueError("RandomForestClassifier takes at most %d "
                             "classes, got %d" % (_lib.RF_MAX_CLASSES, C))
        if n >= _lib.RF_MAX_SAMPLES:
            raise ValueError("RandomForestClassifier takes fewer than %d "
                             "samples, got %d" % (_lib.RF_MAX_SAMPLES, n))
        self.try_features = resolve_try_features(self.try_features_init, d)
        if not 1 <= self.try_features <= d:
            raise ValueError("try_features resolves to %d with %d features"
                             % (self.try_features, d))
        so = _lib.lib()
        dd = dataset._device_data(self._device)
        t = torch()
        with on(dd.device):
            preload(dd.device)
            if not bool(t.isfinite(dd.X).all().item()):
                raise ValueError("RandomForestClassifier takes finite "
                                 "samples: the Dataset holds NaN or infinity")
            free = t.cuda.mem_get_info(dd.device)[0]
            need = hbm_bytes(n, d)
            if need + _IMAGE_HEADROOM > free:
                raise ValueError(
                    "RandomForestClassifier keeps the sorted order, the "
                    "ranks and the distinct values of every feature "
                    "resident: %d x %d need up to %.2f GiB "
                    "of HBM, and %.2f GiB are free (4 GiB stay free)"
                    % (n, d, need / 2.0 ** 30, free / 2.0 ** 30))
            if self._profile:
                t.cuda.synchronize()
            t0 = time.perf_counter()
            prep = Prepared(dd.X, codes)
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
            forest = Forest(C)
            for b in range(0, self.n_estimators, per):
                part = draws[b:b + per]
                samples = np.stack([np.random.RandomState(s).choice(
                    n, size=n, replace=True) for s, _ in part])
                grow(so, prep, C, samples, [s for _, s in part], b,
                     self.try_features, self.max_depth, forest,
                     times=self.times_)
        self.classes = classes
        self._forest, self._d, self._dev = forest, d, dd.device
        self.trees = [forest.tree_arrays(i) for i in range(self.n_estimators)]
        self.distr_depth = self.distr_depth_init

    def fit_predict(self, dataset):
        self.fit(dataset)
        self.predict(dataset)

    def _run(self, dataset, hard):
        assert self.trees, 'The random forest is not fitted.'
        if dataset.sparse:
            raise NotImplementedError(
                "RandomForestClassifier takes a dense Dataset: CSR samples "
                "are not supported")
        if int(dataset.n_features) != self._d:
            raise ValueError("the forest was fitted on %d features, the "
                             "Dataset has %d" % (self._d, dataset.n_features))
        dd = dataset._device_data(self._dev)
        with on(dd.device):
            proba, labels = forest_predict(
                _lib.lib(), dd.X, dd.dtype == np.float32, self._forest, hard)
            return proba.cpu().numpy(), labels.cpu().numpy()

    def predict_proba(self, dataset):
        """Writes every sample's class probabilities (in the order of
        ``classes``) into the Subsets' labels."""
        _write_labels(dataset, self._run(dataset, False)[0])

    def predict(self, dataset):
        """Writes the predicted class of every sample into the Subsets'
        labels."""
        _write_labels(dataset, self.classes[self._run(dataset,
                                                      self.hard_vote)[1]])

    def score(self, dataset):
        """The mean accuracy of ``predict`` against the labels the Subsets
        hold (which stay as they are)."""
        true = np.concatenate([np.asarray(s.labels) for s in dataset])
        pred = self.classes[self._run(dataset, self.hard_vote)[1]]
        return np.count_nonzero(pred == true) / len(true)


def _write_labels(dataset, values):
    off = 0
    for s in dataset:
        n = int(s.samples.shape[0])
        s.labels = values[off:off + n]
        off += n
    dataset._labels = None
