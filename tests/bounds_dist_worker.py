"""One rank of a multi-process KMeans fit with per-row bounds, started by
tests/test_gpu_bounds.py through torch.distributed.run (not a test module).

Every rank builds the same dataset (``oracle.make_blobs_rows``), takes its
contiguous block of Subsets (``shard_dataset``), runs the product
``KMeans.fit_predict`` with gloo on cuda:0 and writes its centres, labels,
row count and the ``dkm_bounds_counters`` of its own workspace (the bounds
are rank-local) to ``<out>.<rank>.npz``.

  python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1
      --master-port P tests/bounds_dist_worker.py --case NAME --out PREFIX
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (d, k, max_iter, Subset sizes)
CASES = {
    # ragged Subsets, shards that are no multiple of the 32-row tile
    "ragged": (32, 37, 10, [7001, 2999, 5003, 4998, 6000, 4000]),
    # one Subset over two ranks: a rank with no rows joins every all-reduce
    "empty": (32, 10, 8, [9001]),
}


def data(case):
    from oracle import kmeans_oracle as orc
    d, k, _, sizes = CASES[case]
    x, _ = orc.make_blobs_rows(0, sum(sizes), d, k, 3)
    return np.ascontiguousarray(x)


def dataset(case, x):
    from dislib_amd.data import Dataset, Subset
    full = Dataset(n_features=x.shape[1], sparse=False)
    lo = 0
    for s in CASES[case][3]:
        full.append(Subset(x[lo:lo + s]))
        lo += s
    return full


def fit(case, ds):
    """fit_predict on ``ds``; (centres, the fit's _Lloyd state)."""
    import dislib_amd.cluster.kmeans as km_mod
    made = []
    orig = km_mod._Lloyd

    class Rec(orig):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    km_mod._Lloyd = Rec
    try:
        _, k, iters, _ = CASES[case]
        km = km_mod.KMeans(n_clusters=k, max_iter=iters, tol=0.0,
                           random_state=0)
        km.fit_predict(ds)
    finally:
        km_mod._Lloyd = orig
    return np.asarray(km.centers), made[0]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--case", required=True)
    p.add_argument("--out", required=True)
    a = p.parse_args()
    import torch
    import torch.distributed as dist
    rank = int(os.environ["RANK"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    from dislib_amd import _shard, shard_dataset
    ds = shard_dataset(dataset(a.case, data(a.case)))
    cen, st = fit(a.case, ds)
    lab = ds.labels_int32()
    np.savez("%s.%d.npz" % (a.out, rank), centers=cen,
             nrows=np.array(st.dd.n), bounding=np.array(bool(st.bounding)),
             counters=np.array(st.bounds_counters() if st.dd.n else
                               (0, 0, 0, 0)),
             labels=lab if lab is not None else np.zeros(0, np.int32))
    dist.barrier()
    _shard.finalize()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
