"""Time ``dislib_amd.decomposition.PCA.fit`` in fp64 at (n = 4M, d = 32) and
(n = 1M, d = 256) against yardsticks measured in the same run (DESIGN.md
3.24):

* a two-pass torch fp64 scatter on the same resident matrix,
  ``m = X.mean(0); (X - m).T @ (X - m)``;
* the HBM bandwidth of a device copy of X (``Tensor.copy_``: 16 d bytes per
  row), against which the Gram pass's one read of X (8 d bytes per row) is
  set at d = 32;
* the 78.6 TF/s f64 MFMA peak, against which the useful flops of the upper
  triangle, n (d + 1)(d + 2), are set at d = 256.

``fit`` and the torch scatter are host clocks around whole calls that end in
a device-to-host read or a synchronise; ``gram`` is the Gram launch pair
alone between device events.  Medians of ``--reps`` calls after a warm-up
call, the candidates alternating.  One JSON line per shape.

  python tools/bench_pca.py [--reps 7]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(4_000_000, 32), (1_000_000, 256)]
PEAK_F64_MFMA = 78.6e12      # MI355X, dense fp64 matrix flop/s


def main():
    import numpy as np
    import torch
    from dislib_amd import _device
    from dislib_amd.data import Dataset, Subset
    from dislib_amd.decomposition import PCA

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pca.py needs a ROCm GPU")
    for n, d in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        X = torch.randn((n, d), dtype=torch.float64, device="cuda",
                        generator=g)
        X *= torch.linspace(1.0, 3.0, d, dtype=torch.float64, device="cuda")
        X += 5.0
        ds = Dataset(n_features=d)
        ds.append(Subset(X))
        dd = ds._device_data("cuda")
        Y = torch.empty_like(X)
        ws, pivot = _device.pca_workspace(dd), _device.pca_pivot(dd)
        pca = PCA()

        def two_pass():
            m = X.mean(0)
            xc = X - m
            S = xc.T @ xc
            torch.cuda.synchronize()
            return m, S

        def gram():
            a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            a.record()
            _device.pca_gram(dd, pivot, ws)
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e-3

        def clock(fn):
            t0 = time.perf_counter()
            fn()
            return time.perf_counter() - t0

        cands = {"fit": lambda: clock(lambda: pca.fit(ds)),
                 "torch": lambda: clock(two_pass), "gram": gram,
                 "copy": lambda: clock(lambda: (Y.copy_(X),
                                                torch.cuda.synchronize()))}
        for fn in cands.values():                        # warm-up
            fn()
        times = {k: [] for k in cands}
        for _ in range(args.reps):
            for k, fn in cands.items():
                times[k].append(fn())
        med = {k: float(np.median(v)) for k, v in times.items()}
        m, S = two_pass()
        cov = (S / (n - 1)).cpu().numpy()
        lam = np.linalg.eigvalsh(cov)[::-1]
        bw = 16.0 * d * n / med["copy"]
        print(json.dumps({
            "n": n, "d": d, "chunks": _device.pca_chunks(n, d),
            "fit_ms": med["fit"] * 1e3, "torch_two_pass_ms": med["torch"] * 1e3,
            "gram_kernels_ms": med["gram"] * 1e3,
            "gram_min_max_ms": [min(times["gram"]) * 1e3,
                                max(times["gram"]) * 1e3],
            "fit_over_torch": med["fit"] / med["torch"],
            "gram_over_torch": med["gram"] / med["torch"],
            "copy_GBps": bw * 1e-9,
            "gram_read_GBps": 8.0 * d * n / med["gram"] * 1e-9,
            "gram_share_of_copy_bandwidth": 8.0 * d * n / med["gram"] / bw,
            "gram_share_of_f64_mfma_peak":
                n * (d + 1.0) * (d + 2.0) / med["gram"] / PEAK_F64_MFMA,
            "max_rel_eigenvalue_difference_to_torch": float(
                np.abs(pca.explained_variance_ - lam).max() / lam[0])}),
            flush=True)
        del X, Y, ds, dd, ws


if __name__ == "__main__":
    main()
