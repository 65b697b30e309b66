"""Golden vectors for ``DBSCAN``, produced by the REFERENCE itself:
``dislib.cluster.DBSCAN.fit`` (``dislib/cluster/dbscan/base.py``) run the way
``gen_golden_neighbors.py`` runs its cases -- imported under the sequential
PyCOMPSs stub of ``gen_golden.py``.

The reference's ``_compute_labels`` assigns ndarray rows into a scipy
``lil_matrix``, which the installed scipy's ``connected_components`` refuses
(``TypeError: Expected list, got numpy.ndarray``).  It runs once
``_compute_neighbours`` returns every neighbour array as a ``list`` of ints,
so this script wraps that function at run time (a monkeypatch; nothing of the
reference is copied).

Per case the inputs are stored, and for every constructor setting of
``SETTINGS`` (``name__settings``) the labels and ``n_clusters`` the reference returned.  Before
writing, the script asserts that every setting of a case gives the labels of
``n_regions=1`` after renumbering by first appearance: the grid parameters
only partition the reference's work, and ``dislib_amd.cluster.DBSCAN``
returns the ``n_regions=1`` labels for all of them.  It refuses to write the
file otherwise (pick another seed for a case that trips it).

Run in the development container only:
``python tests/golden/gen_golden_dbscan.py``.  Writes ``dbscan_ref.npz``.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

# (n_regions, max_samples or -1, dimensions padded with -1; all -1 = None)
SETTINGS = [(1, -1, -1, -1), (1, 70, -1, -1), (2, -1, -1, -1),
            (3, 50, -1, -1), (4, -1, 1, -1)]
# the 10-feature case: the reference builds n_regions ** len(dimensions)
# regions and compares every pair of them (3 ** 10 = 59049 regions never
# finish), so its n_regions = 2 and 3 settings divide two features only
SETTINGS_D10 = [(1, -1, -1, -1), (1, 70, -1, -1), (2, -1, 0, 1),
                (3, 50, 0, 1), (4, -1, 1, -1)]


def cases():
    import numpy as np
    sys.path.insert(0, os.path.dirname(HERE))
    import dbscan_ref as ref
    blobs = ref.blobs_noise(7)
    rng = np.random.default_rng(11)
    c10 = rng.uniform(-3, 3, (3, 10))
    d10 = c10[rng.integers(0, 3, 300)] + 0.3 * rng.standard_normal((300, 10))
    # (name, x, subset_size, eps, min_samples)
    return [
        ("doc", np.array([[1, 2], [2, 2], [2, 3], [8, 7], [8, 8], [25, 80]]),
         2, 3.0, 2),
        ("blobs", blobs, 100, 0.3, 5),
        ("blobs_ms1", blobs, 100, 0.2, 1),
        ("steal", ref.STEAL, 5, 1.0, 4),
        ("d10", d10, 75, 1.6, 5),
    ]


def generate():
    import numpy as np
    from dislib.cluster import DBSCAN
    from dislib.cluster.dbscan import classes
    from dislib.data import load_data
    sys.path.insert(0, os.path.dirname(HERE))
    import dbscan_ref as ref

    inner = classes._compute_neighbours

    def as_lists(*args, **kw):
        neigh, core = inner(*args, **kw)
        return [[int(j) for j in v] for v in neigh], core
    classes._compute_neighbours = as_lists

    out = {}
    for name, x, sub, eps, ms in cases():
        settings = SETTINGS_D10 if name == "d10" else SETTINGS
        out[name + "__x"] = x
        out[name + "__meta"] = np.array([sub, eps, ms], dtype=np.float64)
        out[name + "__settings"] = np.array(settings, dtype=np.int64)
        first = None
        for s, (nr, mx, *dims) in enumerate(settings):
            dims = [c for c in dims if c >= 0]
            ds = load_data(x, subset_size=sub)
            est = DBSCAN(eps=eps, min_samples=ms, n_regions=nr,
                         max_samples=None if mx < 0 else mx,
                         dimensions=dims or None)
            est.fit(ds)
            labels = np.concatenate([np.asarray(b.labels).astype(np.int64)
                                     for b in ds])
            out["%s__labels_s%d" % (name, s)] = labels
            out["%s__ncl_s%d" % (name, s)] = np.array(est.n_clusters)
            if first is None:
                first = labels
            assert np.array_equal(ref.renumber(labels),
                                  ref.renumber(first)), \
                "%s: setting %r differs from n_regions=1" % (name,
                                                             settings[s])
            assert est.n_clusters == len(set(labels[labels >= 0].tolist()))
        print("dbscan", name, x.shape, "clusters", int(first.max()) + 1,
              "noise", int((first < 0).sum()))
    assert np.array_equal(out["steal__labels_s0"], ref.STEAL_LABELS)
    np.savez_compressed(os.path.join(HERE, "dbscan_ref.npz"), **out)
    print("wrote dbscan_ref.npz")


def main():
    try:
        import dislib  # noqa: F401
        import pycompss  # noqa: F401
        ok = True
    except ImportError:
        ok = False
    if ok:
        generate()
        return
    if not os.path.isdir(REF):
        print("reference not present; golden vectors are committed -- skip")
        return
    sys.path.insert(0, HERE)
    from gen_golden import SHIM
    shim = tempfile.mkdtemp(prefix="dkm_shim_")
    for rel, body in SHIM.items():
        p = os.path.join(shim, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w") as f:
            f.write(body)
    env = dict(os.environ, PYTHONPATH=shim + ":" + REF,
               PYTHONDONTWRITEBYTECODE="1")
    sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)],
                             env=env, cwd=REF))


if __name__ == "__main__":
    main()
