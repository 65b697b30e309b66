"""One rank of a multi-process KMeans(sums="reference") fit on the GPU,
started by tests/test_gpu_ordered_dist.py (not a test module).

Every rank loads golden F13's samples (6000 x 4 in 120 Subsets of 50 rows),
takes its contiguous block of Subsets (``shard_dataset``) and fits once per
requested arity with gloo on cuda:0; it writes its centres and labels to
``<out>.<rank>.npz``.  Started without torch.distributed.run (no RANK in the
environment) it is the single-process fit of the whole Dataset.

  python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1
      --master-port P tests/ordered_dist_worker.py --arity 50,2 --out PREFIX
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--arity", required=True)
    p.add_argument("--out", required=True)
    a = p.parse_args()
    import torch
    import torch.distributed as dist
    multi = "RANK" in os.environ
    rank = int(os.environ.get("RANK", 0))
    torch.cuda.set_device(0)
    if multi:
        dist.init_process_group("gloo")
    from dislib_amd import _shard, shard_dataset
    from dislib_amd.cluster import KMeans
    from dislib_amd.data import load_data
    with np.load(os.path.join(ROOT, "tests", "golden", "f13_arity.npz")) as z:
        x = z["x"]
    out = {}
    for arity in [int(v) for v in a.arity.split(",")]:
        ds = shard_dataset(load_data(x, subset_size=50))
        km = KMeans(n_clusters=6, max_iter=4, tol=0, arity=arity,
                    random_state=13, sums="reference")
        km.fit_predict(ds)
        out["centers_a%d" % arity] = km.centers
        out["labels_a%d" % arity] = ds.labels_int32()
        out["subsets_a%d" % arity] = np.array(len(ds))
    np.savez("%s.%d.npz" % (a.out, rank), **out)
    if multi:
        dist.barrier()
        _shard.finalize()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
