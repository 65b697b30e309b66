"""Per-iteration bounds counters of the headline fit.

    python tools/bounds_iters.py [--n 100000000] [--d 32] [--k 100] [--steps 20]

Runs bench.py's headline fit (on-device make_blobs, np.random.seed(0)
initial centres, tol = 0) and prints, per iteration, the wall time and what
dkm_bounds_counters gained: rows active, rows skipped, and whether the
active rows were screened as a list or every row from the image, the rows
the exact re-check took (the gain of rechecked()) and the rows it gave
bounds to (dkm_bounds_settled; DKM_BOUNDS_SETTLE=0 turns that off).
"""
import argparse
import json
import time

import torch

from dislib_amd import _device
from dislib_amd.cluster.kmeans import _Lloyd, _init_centers
from dislib_amd.data import Dataset, Subset


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=100_000_000)
    p.add_argument("--d", type=int, default=32)
    p.add_argument("--k", type=int, default=100)
    p.add_argument("--steps", type=int, default=20)
    a = p.parse_args()
    dev = torch.device("cuda")
    X = torch.empty((a.n, a.d), dtype=torch.float64, device=dev)
    _device.make_blobs(X, 0, a.k, seed=0, box=10.0, std=1.0)
    ds = Dataset(n_features=a.d, sparse=False)
    for i in range(0, a.n, 1_000_000):
        ds.append(Subset(X[i:i + 1_000_000]))
    C0 = _init_centers(a.d, False, a.k, 0)
    for rep in range(2):          # the first fit warms up
        ds._device_data(dev).drop_images()
        st = _Lloyd(ds, C0, 0.0, True, "auto", dev)
        rows, prev = [], (0, 0, 0, 0)
        st.prepare()      # writes the workspace header the counters read
        prev_r, prev_s = st.rechecked(), st.bounds_settled()
        for it in range(a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.step()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            c = st.bounds_counters()
            rows.append({"iteration": it, "ms": round(ms, 3),
                         "bounds_pass": c[0] - prev[0],
                         "active": c[1] - prev[1],
                         "skipped": c[2] - prev[2],
                         "active_frac": round((c[1] - prev[1]) / a.n, 5),
                         "list_screen": c[3] - prev[3],
                         "rechecked": st.rechecked() - prev_r,
                         "settled": st.bounds_settled() - prev_s})
            prev = c
            prev_r, prev_s = st.rechecked(), st.bounds_settled()
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
