"""Time one loss-and-gradient evaluation of ``dislib_amd.classification.
LogisticRegression`` in fp64 at (n = 10M, d = 32, K = 10) and (n = 4M,
d = 128, K = 2) against yardsticks measured in the same run:

* the byte floor of one read of X: 8 n d bytes over the bandwidth of a device
  copy of X (``Tensor.copy_``: 16 d bytes per row);
* the torch composition on the same resident matrix: ``X @ W^T + b``,
  ``log_softmax`` (``logsigmoid`` for two classes), ``(P - Y)^T @ X``;
* a whole ``fit`` against scikit-learn's ``lbfgs`` fit of the same data on
  the host (its BLAS on the machine's threads; ``--no-sklearn`` skips it).

``eval`` and ``torch`` are the launches alone between device events; ``fit``,
``copy`` and scikit-learn are host clocks around whole calls that end in a
device-to-host read or a synchronise.  Medians of ``--reps`` calls after a
warm-up call, the candidates alternating; the minimum and maximum of ``eval``
are reported with it.  One JSON line per shape.

  python tools/bench_logreg.py [--reps 7]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(10_000_000, 32, 10), (4_000_000, 128, 2)]


def main():
    import numpy as np
    import torch
    from dislib_amd import _device
    from dislib_amd.classification import LogisticRegression
    from dislib_amd.data import Dataset, Subset

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", type=int, default=len(SHAPES))
    ap.add_argument("--no-sklearn", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_logreg.py needs a ROCm GPU")
    f64 = torch.float64
    for n, d, K in SHAPES[:args.shapes]:
        g = torch.Generator(device="cuda").manual_seed(0)
        X = torch.randn((n, d), dtype=f64, device="cuda", generator=g)
        truth = torch.randn((K, d), dtype=f64, device="cuda", generator=g)
        noise = -torch.log(-torch.log(torch.rand(
            (n, K), dtype=f64, device="cuda", generator=g)))
        codes = (X @ truth.T + noise).argmax(1).to(torch.int32)
        del noise
        labels = codes.cpu().numpy()
        ds = Dataset(n_features=d)
        ds.append(Subset(X, labels=labels))
        dd = ds._device_data("cuda")
        cols = 1 if K == 2 else K
        W = 0.1 * torch.randn((cols, d + 1), dtype=f64, device="cuda",
                              generator=g)
        ws = _device.logreg_workspace(dd, cols)
        out = torch.empty(1 + W.numel(), dtype=f64, device="cuda")
        Y = torch.empty_like(X)
        idx = codes.long()
        lr = LogisticRegression()

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

        def composition():
            Z = torch.addmm(W[:, d], X, W[:, :d].T)
            if cols == 1:
                sign = 1.0 - 2.0 * idx.to(f64)          # -1 for class 1
                loss = -torch.nn.functional.logsigmoid(-sign * Z[:, 0]).sum()
                R = torch.sigmoid(Z)
                R[:, 0] -= idx.to(f64)
            else:
                L = torch.log_softmax(Z, 1)
                loss = -L.gather(1, idx[:, None]).sum()
                R = L.exp_()
                R.scatter_add_(1, idx[:, None], torch.full(
                    (n, 1), -1.0, dtype=f64, device="cuda"))
            return torch.cat([loss[None], torch.cat(
                [R.T @ X, R.sum(0)[:, None]], 1).reshape(-1)])

        cands = {"eval": lambda: events(lambda: _device.logreg_lossgrad(
                     dd, codes, W, 1, ws, out)),
                 "torch": lambda: events(composition),
                 "fit": lambda: clock(lambda: lr.fit(ds)),
                 "copy": lambda: clock(lambda: (Y.copy_(X),
                                                torch.cuda.synchronize()))}
        for fn in cands.values():                        # warm-up
            fn()
        times = {k: [] for k in cands}
        for _ in range(args.reps):
            for k, fn in cands.items():
                times[k].append(fn())
        med = {k: float(np.median(v)) for k, v in times.items()}
        ref = composition()
        diff = float(((out - ref).abs() / ref.abs().clamp_min(1.0)).max())
        bw = 16.0 * d * n / med["copy"]
        res = {
            "n": n, "d": d, "classes": K, "chunks": _device.logreg_chunks(n),
            "tile_rows": _device.logreg_tile_rows(d),
            "eval_ms": med["eval"] * 1e3,
            "eval_min_max_ms": [min(times["eval"]) * 1e3,
                                max(times["eval"]) * 1e3],
            "torch_composition_ms": med["torch"] * 1e3,
            "copy_GBps": bw * 1e-9,
            "byte_floor_ms": 8.0 * d * n / bw * 1e3,
            "eval_over_byte_floor": med["eval"] * bw / (8.0 * d * n),
            "eval_over_torch": med["eval"] / med["torch"],
            "max_rel_difference_to_torch": diff,
            "fit_ms": med["fit"] * 1e3, "fit_iterations": lr.n_iter_}
        if not args.no_sklearn:
            from sklearn.linear_model import LogisticRegression as SkLogReg
            xh = X.cpu().numpy()
            sk = SkLogReg(solver="lbfgs")
            res["sklearn_fit_ms"] = clock(lambda: sk.fit(xh, labels)) * 1e3
            res["sklearn_iterations"] = int(sk.n_iter_[0])
            res["fit_over_sklearn"] = res["fit_ms"] / res["sklearn_fit_ms"]
            res["max_coef_difference_to_sklearn"] = float(
                np.abs(lr.coef_ - sk.coef_).max())
            del xh
        print(json.dumps(res), flush=True)
        del X, Y, ds, dd, ws, codes, idx, truth


if __name__ == "__main__":
    main()
