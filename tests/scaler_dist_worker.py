"""One rank of a multi-process StandardScaler.fit_transform on the GPU,
started by tests/test_gpu_scaler_dist.py (not a test module).

Every rank rebuilds the inputs of the goldens s02 (fp64, 120 Subsets of 50
rows) and s03 (fp32, 6 Subsets of 500), takes its contiguous block of
Subsets (``shard_dataset``) and runs, with gloo on cuda:0, the reference
mode (s02 with arity 50 and 2, s03 with arity 50) and the fast mode; it
writes ``mean_``, ``var_`` and its shard's scaled rows to
``<out>.<rank>.npz``.  RANK, WORLD_SIZE, MASTER_ADDR and MASTER_PORT come
from the environment; without RANK it is the single-process run.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = (("s02", "reference", 50), ("s02", "reference", 2),
        ("s03", "reference", 50), ("s02", "fast", 50), ("s03", "fast", 50))


def run_all():
    """{key: array} of every run on this rank's shard."""
    from dislib_amd import shard_dataset
    from dislib_amd.data import Dataset, Subset
    from dislib_amd.preprocessing import StandardScaler
    from tests import scaler_ref as sr
    out = {}
    for name, sums, arity in RUNS:
        (_, x, sizes, _), = sr.inputs(name)
        ds = Dataset(n_features=x.shape[1])
        for block in sr.split(x, sizes):
            ds.append(Subset(block))
        ds = shard_dataset(ds)
        sc = StandardScaler(arity=arity, sums=sums)
        sc.fit_transform(ds)
        key = "%s_%s_a%d_" % (name, sums, arity)
        out[key + "mean"], out[key + "var"] = sc.mean_, sc.var_
        out[key + "y"] = np.concatenate([s.samples for s in ds])
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", required=True)
    a = p.parse_args()
    import torch
    import torch.distributed as dist
    multi = "RANK" in os.environ
    rank = int(os.environ.get("RANK", 0))
    torch.cuda.set_device(0)
    if multi:
        dist.init_process_group("gloo")
    np.savez("%s.%d.npz" % (a.out, rank), **run_all())
    if multi:
        from dislib_amd import _shard
        dist.barrier()
        _shard.finalize()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
