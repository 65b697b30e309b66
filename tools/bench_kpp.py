"""Time ``dislib_amd.cluster.kmeans_plusplus`` at C2's shape (d = 32,
k = 100, fp64 blobs generated on the device) against two yardsticks measured
in the same run, and compare the fits the two ``init`` rules lead to.

* the byte floor of a round: one read of X, one write of
  dc (8 L bytes per row), the commit's read of one dc column and a read and
  a write of mind (24 bytes per row), over the HBM bandwidth of a device copy
  of X (``Tensor.copy_``: 16 d bytes per row);
* a plain torch composition of the same rule (same draws, same indices).

Timings are host clocks around whole calls, which end in a device-to-host
read; the median of ``--reps`` calls after a warm-up call, the candidates
alternating.  Then, on standardised blobs, ``KMeans`` with ``init="random"``
against ``"k-means++"``: Lloyd iterations to convergence and final inertia.
One JSON line each.

  python tools/bench_kpp.py [--n 10000000] [--reps 5] [--fit-n 1000000]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, K = 32, 100


def torch_kpp(X, k, seed, L):
    """The rule of kmeans_plusplus in torch ops (fp64)."""
    import numpy as np
    import torch
    n = X.shape[0]
    rs = np.random.RandomState(seed)
    idx = [int(rs.randint(n))]
    U = torch.from_numpy(rs.uniform(size=(k - 1, L))).to(X.device)
    mind = ((X - X[idx[0]]) ** 2).sum(1)
    out = torch.empty(k, dtype=torch.int64, device=X.device)
    out[0] = idx[0]
    for t in range(1, k):
        rows = torch.searchsorted(torch.cumsum(mind, 0), U[t - 1] * mind.sum())
        rows = rows.clamp_(max=n - 1)
        cand = torch.stack([torch.minimum(mind, ((X - X[r]) ** 2).sum(1))
                            for r in rows])
        best = cand.sum(1).argmin()
        mind = cand[best]
        out[t] = rows[best]
    return out.cpu().numpy()


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def dataset(X, subset=1_000_000):
    from dislib_amd.data import Dataset, Subset
    ds = Dataset(n_features=X.shape[1])
    for i in range(0, X.shape[0], subset):
        ds.append(Subset(X[i:i + subset]))
    return ds


def inertia(X, centers):
    import torch
    C = torch.from_numpy(centers).to(X.device)
    tot = 0.0
    for i in range(0, X.shape[0], 1 << 18):
        tot += float((torch.cdist(X[i:i + (1 << 18)], C) ** 2).min(1)[0].sum())
    return tot


def main():
    import numpy as np
    import torch
    from dislib_amd import _device
    from dislib_amd.cluster import KMeans, kmeans_plusplus

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit-n", type=int, default=1_000_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kpp.py needs a ROCm GPU")
    n, L = args.n, 2 + int(np.log(K))
    X = torch.empty((n, D), dtype=torch.float64, device="cuda")
    _device.make_blobs(X, 0, K, seed=0, box=10.0, std=1.0)
    ds = dataset(X)
    ds._device_data("cuda")
    Y = torch.empty_like(X)
    cands = {"kpp": lambda: kmeans_plusplus(ds, K, random_state=0)[1],
             "torch": lambda: torch_kpp(X, K, 0, L),
             "copy": lambda: (Y.copy_(X), torch.cuda.synchronize())}
    got = {k: fn() for k, fn in cands.items()}           # warm-up
    times = {k: [] for k in cands}
    for _ in range(args.reps):
        for k, fn in cands.items():
            times[k].append(timed(fn)[0])
    med = {k: float(np.median(v)) for k, v in times.items()}
    bw = 16.0 * D * n / med["copy"]
    round_bytes = n * (8.0 * D + 8.0 * L + 24.0)
    floor = (K - 1) * round_bytes / bw
    print(json.dumps({
        "n": n, "d": D, "k": K, "trials": L,
        "kpp_ms": med["kpp"] * 1e3, "torch_ms": med["torch"] * 1e3,
        "kpp_min_max_ms": [min(times["kpp"]) * 1e3, max(times["kpp"]) * 1e3],
        "rounds_per_s": (K - 1) / med["kpp"],
        "copy_GBps": bw * 1e-9, "byte_floor_ms": floor * 1e3,
        "share_of_byte_floor": floor / med["kpp"],
        "x_torch": med["kpp"] / med["torch"],
        "same_indices_as_torch": bool(np.array_equal(got["kpp"],
                                                     got["torch"]))}),
        flush=True)
    del Y, ds
    # the fits: standardised blobs, as the README's recipe produces them
    Z = X[:args.fit_n]
    Z = ((Z - Z.mean(0)) / Z.std(0, unbiased=False)).contiguous()
    del X
    for init in ("random", "k-means++"):
        zs = dataset(Z)
        km = KMeans(n_clusters=K, max_iter=300, random_state=0, init=init)
        dt, _ = timed(lambda: km.fit(zs))
        print(json.dumps({"fit_n": Z.shape[0], "init": init,
                          "lloyd_iterations": km.n_iter, "fit_s": dt,
                          "inertia": inertia(Z, km.centers)}), flush=True)


if __name__ == "__main__":
    main()
