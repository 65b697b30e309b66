"""Time KMeans(sums="reference") against the default sums="fast" on
device-made blobs, and the ordered-sums call on its own:

  python tools/bench_ordered.py [--shape NAME ...] [--steps 6] [--reps 3]
                                [--limit 600] [--scale 1.0]

Per shape (the bench headline: 100M x 32 fp64, k = 100, Subsets of 1M rows;
"c3": 25M x 64 fp64, k = 1000, Subsets of 1M rows) it records

* ms per Lloyd step in reference and in fast mode, as alternating fits
  (reference, fast, reference, ...; iteration 0 left out: the median of the
  later steps of every fit, then the best fit of each mode);
* the dkm_ordered_sums_* call on the fit's last labels and the rate at which
  the whole call (grouping included) gets through X in TB/s, and its
  grouping part as an upper bound: the same call on a one-column copy of X
  with the same labels and Subsets (the grouping kernels do not read X; the
  one-column chains still gather one value per row, so the difference of
  the two times is NOT the chains' time on the full rows);
* dkm_merge_tree.

Every shape runs in a child process of its own under a time limit
(--limit seconds): the parent never opens the GPU, and a child that runs
over is ended instead of waited for.  One JSON line per shape.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    # name: (n, d, k, subset)
    "headline": (100_000_000, 32, 100, 1_000_000),
    "c3": (25_000_000, 64, 1000, 1_000_000),
}


def _timed(torch, fn, reps):
    out = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r:
            out.append(1e3 * (time.perf_counter() - t0))
    return min(out)


def child(a):
    import torch
    from dislib_amd import _device, _shard
    from dislib_amd.cluster.kmeans import _Lloyd, _init_centers
    from dislib_amd.data import Dataset, Subset
    n, d, k, subset = SHAPES[a.child]
    n = max(subset // 8, int(n * a.scale))
    subset = min(subset, n)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    X = torch.empty((n, d), dtype=torch.float64, device=dev)
    _device.make_blobs(X, 0, k, seed=0, box=10.0, std=1.0)
    ds = Dataset(n_features=d)
    for i in range(0, n, subset):
        ds.append(Subset(X[i:i + subset]))
    dd = ds._device_data(dev)
    C0 = _init_centers(d, False, k, 0)
    per = {"reference": [], "fast": []}
    st = None
    for rep in range(a.reps):
        for sums in ("reference", "fast"):
            dd.drop_images()
            del st
            st = _Lloyd(ds, C0, 0.0, False, "auto", dev, sums=sums)
            ts = []
            for _ in range(a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st.step()
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            per[sums].append(statistics.median(ts[1:]))
            print(a.child, rep, sums, ["%.2f" % t for t in ts], flush=True)
    # the ordered-sums call alone, on the labels of a reference-mode fit
    del st
    dd.drop_images()
    st = _Lloyd(ds, C0, 0.0, False, "auto", dev, sums="reference")
    st.step()
    st.step()
    osum, labels = st.osum, st.labels
    t_all = _timed(torch, lambda: _device.ordered_sums(dd, labels, osum),
                   a.reps)
    t_merge = _timed(torch, lambda: _device.merge_tree(osum, st.acc, False),
                     a.reps)
    # one column of X, the same rows, labels and Subsets
    ds1 = Dataset(n_features=1)
    x1 = X[:, :1].contiguous()
    for i in range(0, n, subset):
        ds1.append(Subset(x1[i:i + subset]))
    dd1 = ds1._device_data(dev)
    o1 = _device.OrderedSums(dd1, k, 0, len(dd1.sizes),
                             *_shard.merge_schedule(len(dd1.sizes), 50))
    t_grp = _timed(torch, lambda: _device.ordered_sums(dd1, labels, o1),
                   a.reps)
    print(json.dumps({
        "shape": a.child, "n": n, "d": d, "k": k, "subsets": len(dd.sizes),
        "steps": a.steps, "reps": a.reps,
        "reference_ms_per_step": round(min(per["reference"]), 3),
        "fast_ms_per_step": round(min(per["fast"]), 3),
        "reference_ms_all_fits": [round(v, 3) for v in per["reference"]],
        "fast_ms_all_fits": [round(v, 3) for v in per["fast"]],
        "ordered_sums_ms": round(t_all, 3),
        "grouping_ms_upper_bound": round(t_grp, 3),
        "ordered_sums_X_TBps": round(n * d * 8 / t_all * 1e-9, 3),
        "merge_tree_ms": round(t_merge, 3)}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", nargs="*", default=sorted(SHAPES))
    p.add_argument("--steps", type=int, default=6)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--limit", type=int, default=600)
    p.add_argument("--scale", type=float, default=1.0,
                   help="fraction of each shape's rows (a quick look)")
    p.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        return child(a)
    for name in a.shape:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name,
               "--steps", str(a.steps), "--reps", str(a.reps), "--scale",
               str(a.scale)]
        try:
            r = subprocess.run(cmd, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print("%s: ended at its %d s limit; stopping" % (name, a.limit),
                  flush=True)
            return 1
        if r.returncode != 0:
            # a faulted or aborted child: start nothing more on the GPU
            print("%s: exit status %d; stopping" % (name, r.returncode),
                  flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
