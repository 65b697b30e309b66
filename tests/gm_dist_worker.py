"""One rank of a multi-process GaussianMixture.fit_predict on the GPU,
started by tests/test_gpu_gm_dist.py (not a test module).

Every rank rebuilds the inputs of the goldens gm_a (k-means initialisation)
and gm_b (random initialisation, 17 features, 5 components), takes its
contiguous block of Subsets (``shard_dataset``) and fits with gloo on
cuda:0; it writes the parameters, ``n_iter``, ``lower_bound_`` and its
shard's labels to ``<out>.<rank>.npz``.  RANK, WORLD_SIZE, MASTER_ADDR and
MASTER_PORT come from the environment; without RANK it is the
single-process run.
"""
import argparse
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = ("gm_a", "gm_b")
ATTRS = ("weights_", "means_", "covariances_", "precisions_cholesky_")


def run_all():
    """{key: array} of every run on this rank's shard."""
    from dislib_amd import shard_dataset
    from dislib_amd.cluster import GaussianMixture
    from dislib_amd.data import Dataset, Subset
    from tests import gm_ref as gr
    out = {}
    for name in RUNS:
        inp = gr.inputs(name)
        ds = Dataset(n_features=inp["x"].shape[1])
        for block in gr.split(inp["x"], inp["sizes"]):
            ds.append(Subset(block))
        ds = shard_dataset(ds)
        gm = GaussianMixture(**inp["kw"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gm.fit_predict(ds)
        for a in ATTRS:
            out[name + "_" + a] = getattr(gm, a)
        out[name + "_n_iter"] = np.array(gm.n_iter)
        out[name + "_converged"] = np.array(gm.converged_)
        out[name + "_lower_bound"] = np.array(gm.lower_bound_)
        out[name + "_labels"] = np.concatenate([s.labels for s in ds])
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
