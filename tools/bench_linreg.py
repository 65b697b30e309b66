"""Time ``dislib_amd.regression.LinearRegression.fit`` in fp64 at (n = 10M,
d = 32) and (n = 4M, d = 96) against yardsticks measured in the same run
(DESIGN.md 3.25):

* the byte floor of one read of X: 8 n d bytes over the bandwidth of a device
  copy of X (``Tensor.copy_``: 16 d bytes per row);
* ``dkm_pca_gram_f64`` on the same Dataset: what forming the normal equations
  would cost;
* ``torch.linalg.lstsq`` on the device.

``fit`` and torch's lstsq are host clocks around whole calls that end in a
device-to-host read or a synchronise; ``tsqr`` and ``gram`` are the kernel
launches alone between device events.  Medians of ``--reps`` calls after a
warm-up call, the candidates alternating.  One JSON line per shape.

  python tools/bench_linreg.py [--reps 7]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(10_000_000, 32), (4_000_000, 96)]


def main():
    import numpy as np
    import torch
    from dislib_amd import _device
    from dislib_amd.data import Dataset, Subset
    from dislib_amd.regression import LinearRegression

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", type=int, default=len(SHAPES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linreg.py needs a ROCm GPU")
    for n, d in SHAPES[:args.shapes]:
        g = torch.Generator(device="cuda").manual_seed(0)
        X = torch.randn((n, d), dtype=torch.float64, device="cuda",
                        generator=g)
        X *= torch.linspace(1.0, 3.0, d, dtype=torch.float64, device="cuda")
        X += 5.0
        beta = torch.linspace(-1.0, 1.0, d, dtype=torch.float64,
                              device="cuda")
        yd = X @ beta + 2.0 + 0.1 * torch.randn(
            n, dtype=torch.float64, device="cuda", generator=g)
        ds = Dataset(n_features=d)
        ds.append(Subset(X, labels=yd.cpu().numpy()))
        dd = ds._device_data("cuda")
        Y = torch.empty_like(X)
        ws = _device.tsqr_workspace(dd, d + 2)
        pws, pivot = _device.pca_workspace(dd), _device.pca_pivot(dd)
        lr = LinearRegression()

        def events(fn):
            a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e-3

        def clock(fn):
            t0 = time.perf_counter()
            fn()
            return time.perf_counter() - t0

        def torch_lstsq():
            A = torch.cat([torch.ones((n, 1), dtype=torch.float64,
                                      device="cuda"), X], 1)
            return torch.linalg.lstsq(A, yd[:, None]).solution.cpu()

        cands = {"fit": lambda: clock(lambda: lr.fit(ds)),
                 "tsqr": lambda: events(lambda: _device.tsqr(dd, yd, 1, ws)),
                 "gram": lambda: events(
                     lambda: _device.pca_gram(dd, pivot, pws)),
                 "torch": lambda: clock(torch_lstsq),
                 "copy": lambda: clock(lambda: (Y.copy_(X),
                                                torch.cuda.synchronize()))}
        for fn in cands.values():                        # warm-up
            fn()
        times = {k: [] for k in cands}
        for _ in range(args.reps):
            for k, fn in cands.items():
                times[k].append(fn())
        med = {k: float(np.median(v)) for k, v in times.items()}
        # the coefficients against the fp64 normal equations of the centred
        # columns (this data is well conditioned, so they are a fair check)
        xc, yc = X - X.mean(0), yd - yd.mean()
        ne = torch.linalg.solve(xc.T @ xc, xc.T @ yc).cpu().numpy()
        sol = torch_lstsq().numpy()[1:, 0]
        bw = 16.0 * d * n / med["copy"]
        print(json.dumps({
            "n": n, "d": d, "ranges": _device.tsqr_ranges(n),
            "fit_ms": med["fit"] * 1e3, "tsqr_kernels_ms": med["tsqr"] * 1e3,
            "tsqr_min_max_ms": [min(times["tsqr"]) * 1e3,
                                max(times["tsqr"]) * 1e3],
            "pca_gram_kernels_ms": med["gram"] * 1e3,
            "torch_lstsq_ms": med["torch"] * 1e3,
            "copy_GBps": bw * 1e-9,
            "byte_floor_ms": 8.0 * d * n / bw * 1e3,
            "tsqr_over_byte_floor": med["tsqr"] * bw / (8.0 * d * n),
            "tsqr_over_gram": med["tsqr"] / med["gram"],
            "fit_over_torch": med["fit"] / med["torch"],
            "max_rel_coef_difference_to_normal_equations": float(
                np.abs(lr.coef_ - ne).max() / np.abs(ne).max()),
            "torch_lstsq_max_rel_coef_difference_to_normal_equations": float(
                np.abs(sol - ne).max() / np.abs(ne).max())}),
            flush=True)
        del X, Y, yd, xc, yc, ds, dd, ws, pws


if __name__ == "__main__":
    main()
