"""Time the two paths of a bounds call at the same active share
(the crossover constant BOUNDS_LIST_FRAC).

    python tools/bounds_crossover.py [--n 100000000] [--stds 1,1.6,2,2.4]

For each blob spread the headline fit (d = 32, k = 100) runs twice from the
same initial centres: with DKM_BOUNDS_LIST_FRAC=1 (the active rows always
screened as a list) and =0 (always every row from the image).  Labels are
identical either way, so iteration i of both fits starts from the same state
and the same active share; the tool prints that share and both wall times
per iteration, one JSON line each.  A wider spread keeps more rows active.
"""
import argparse
import json
import os
import time

import torch

from dislib_amd import _device
from dislib_amd.cluster.kmeans import _Lloyd, _init_centers
from dislib_amd.data import Dataset, Subset


def fit(ds, C0, steps, n, dev):
    ds._device_data(dev).drop_images()
    st = _Lloyd(ds, C0, 0.0, True, "auto", dev)
    rows, prev = [], (0, 0, 0, 0)
    for it in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        c = st.bounds_counters()
        rows.append((round((c[1] - prev[1]) / n, 5), round(ms, 3),
                     c[0] - prev[0]))
        prev = c
    return rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=100_000_000)
    p.add_argument("--d", type=int, default=32)
    p.add_argument("--k", type=int, default=100)
    p.add_argument("--steps", type=int, default=12)
    p.add_argument("--stds", default="1,1.6,2,2.4")
    a = p.parse_args()
    dev = torch.device("cuda")
    X = torch.empty((a.n, a.d), dtype=torch.float64, device=dev)
    C0 = _init_centers(a.d, False, a.k, 0)
    for std in [float(s) for s in a.stds.split(",")]:
        _device.make_blobs(X, 0, a.k, seed=0, box=10.0, std=std)
        ds = Dataset(n_features=a.d, sparse=False)
        for i in range(0, a.n, 1_000_000):
            ds.append(Subset(X[i:i + 1_000_000]))
        res = {}
        for frac in ("1", "0"):
            os.environ["DKM_BOUNDS_LIST_FRAC"] = frac
            fit(ds, C0, a.steps, a.n, dev)            # warm-up
            res[frac] = fit(ds, C0, a.steps, a.n, dev)
        for it, (li, im) in enumerate(zip(res["1"], res["0"])):
            if li[2]:
                print(json.dumps({"std": std, "iteration": it,
                                  "active_frac": li[0],
                                  "active_frac_image_run": im[0],
                                  "list_ms": li[1], "image_ms": im[1]}))
    os.environ.pop("DKM_BOUNDS_LIST_FRAC", None)


if __name__ == "__main__":
    main()
