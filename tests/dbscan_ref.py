"""Plain numpy statement of the DBSCAN that ``dislib_amd.cluster.DBSCAN``
computes: the reference's ``_compute_neighbours`` / ``_compute_labels``
(dislib/cluster/dbscan/classes.py:124-191) with one region, the numbering by
first appearance that its ``_compute_equivalences`` / ``_update_labels``
give, and the pinned tie rule (distance, row) where the reference's
``np.argsort`` leaves equal distances unpinned.  Not a test module.

tests/test_dbscan_host.py pins it to the goldens (the reference's own
output) on the CPU; the GPU tests compare the kernels against it.
"""
import numpy as np


def _dist(x, i):
    """_vec_matrix_euclid(x[i], x) (classes.py:153-154)."""
    return np.linalg.norm(x[i] - x, axis=1)


def dbscan_ref(x, eps, min_samples):
    """(labels int64[n], n_clusters) of the (n, d) samples ``x`` (widened to
    fp64).  Two passes that recompute the distances: nothing n x n."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    n = x.shape[0]
    core = np.zeros(n, dtype=bool)
    for i in range(n):
        core[i] = np.count_nonzero(_dist(x, i) < eps) >= min_samples

    parent = np.arange(n)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    attach = np.full(n, -1)
    for i in range(n):
        dist = _dist(x, i)
        cand = np.flatnonzero((dist < eps) & core)
        if core[i]:
            # two core samples within eps are in one component
            for j in cand[cand < i]:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
        elif cand.size:
            # a non-core sample joins its nearest core neighbour only:
            # the smallest (distance, row)
            attach[i] = cand[np.lexsort((cand, dist[cand]))[0]]

    comp = np.empty(n, dtype=np.int64)
    for i in range(n):
        if core[i]:
            comp[i] = find(i)
        elif attach[i] >= 0:
            comp[i] = find(attach[i])
        else:
            comp[i] = i               # alone
    size = np.bincount(comp, minlength=n) if n else np.zeros(0, np.int64)
    labels = np.full(n, -1, dtype=np.int64)
    number = {}
    for i in range(n):                # numbered by smallest row
        c = comp[i]
        if size[c] < min_samples:     # even when it holds a core sample
            continue
        if c not in number:
            number[c] = len(number)
        labels[i] = number[c]
    return labels, len(number)


def renumber(labels):
    """Clusters renumbered 0, 1, ... by first appearance; -1 stays."""
    labels = np.asarray(labels).astype(np.int64)
    out = np.full(labels.shape, -1, dtype=np.int64)
    number = {}
    for i, v in enumerate(labels):
        if v < 0:
            continue
        if v not in number:
            number[v] = len(number)
        out[i] = number[v]
    return out


def blobs_noise(seed, n_blob=300, n_noise=40, d=2, centers=4, std=0.25,
                box=4.0):
    """Seeded Gaussian blobs plus uniform noise, rows shuffled (the data of
    the goldens' blobs cases and of the GPU tests)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-box, box, (centers, d))
    x = c[rng.integers(0, centers, n_blob)] + std * rng.standard_normal(
        (n_blob, d))
    x = np.concatenate([x, rng.uniform(-box - 1, box + 1, (n_noise, d))])
    return np.ascontiguousarray(x[rng.permutation(len(x))])


STEAL = np.array([[0, 0], [.9, 0], [-.9, 0], [0, .95], [1.5, 0], [2, 0],
                  [2.2, 0], [-1.5, 0], [-2, 0], [-2.2, 0], [0, 1.5], [0, 2],
                  [0, 2.2]], dtype=np.float64)
STEAL_LABELS = np.array([-1, 0, 1, 2, 0, 0, 0, 1, 1, 1, 2, 2, 2])
