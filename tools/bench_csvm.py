"""Measure the CascadeSVM kernels (never asserted in a test).

At n rows (default 2^17) of d in {16, 128} features, rbf, fp64:

* the kernel rows of one working set (``dkm_svm_rows_f64``, q = 128 against
  the whole matrix as one node) against the f64 MFMA peak and against torch
  (``matmul`` + ``exp`` on the gathered rows, fp64);
* one node solve (``csvm.solve_node``, ``--node`` rows) against
  ``sklearn.svm.SVC`` on the host's CPUs: the same rows, kernel, C and tol;
* ``decision_function`` (``dkm_svm_decision_f64``, ``--sv`` support rows)
  against the torch composition.

Medians of ``--rounds`` alternating rounds (ours, theirs, ours, ...), each a
timed stream-synchronised call after one untimed call.  Prints one JSON line
per d."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F64_MFMA = 78.6e12      # MI355X, matrix fp64 FLOP/s


def timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(ours, theirs, rounds, torch):
    ours(), theirs()
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(ours, torch))
        b.append(timed(theirs, torch))
    return float(np.median(a)), float(np.median(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 17)
    ap.add_argument("--node", type=int, default=8192)
    ap.add_argument("--sv", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--dims", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--no-sklearn", action="store_true")
    args = ap.parse_args()
    import torch
    from dislib_amd import _lib
    from dislib_amd._device import ptr, stream_ptr
    from dislib_amd.classification import csvm
    so = _lib.lib()
    q = _lib.SVM_QMAX
    for d in args.dims:
        rng = np.random.default_rng(d)
        n = args.n
        x = rng.standard_normal((n, d))
        y = np.where(x[:, 0] + 0.5 * rng.standard_normal(n) > 0, 1.0, -1.0)
        gamma = 1.0 / d
        X = torch.from_numpy(x).cuda()
        xn = csvm.norms(so, X, False)
        rows = torch.arange(n, dtype=torch.int32, device="cuda")
        ws = torch.from_numpy(rng.permutation(n)[:q].astype(np.int32)).cuda()
        K = torch.empty((q, n), dtype=torch.float64, device="cuda")

        def ours_rows():
            _lib.check(so.dkm_svm_rows_f64(
                ptr(X), n, d, d, ptr(rows), n, ptr(ws), q, ptr(xn),
                _lib.SVM_RBF, gamma, ptr(K), n, stream_ptr()), "rows")

        def torch_rows():
            a = X[ws.long()]
            dot = a @ X.T
            return torch.exp(-gamma * (xn[ws.long()][:, None] + xn[None, :]
                                       - 2.0 * dot))
        t_rows, t_rows_torch = alternate(ours_rows, torch_rows, args.rounds,
                                         torch)

        ns = args.sv
        sv = torch.from_numpy(rng.permutation(n)[:ns].astype(np.int32)).cuda()
        coef = torch.from_numpy(rng.standard_normal(ns)).cuda()
        out = torch.empty(n, dtype=torch.float64, device="cuda")

        def ours_dec():
            _lib.check(so.dkm_svm_decision_f64(
                ptr(X), n, d, d, ptr(X), 0, n, d, ptr(sv), ns, ptr(coef), 0.5,
                ptr(xn), ptr(xn), _lib.SVM_RBF, gamma, ptr(out),
                stream_ptr()), "decision")

        def torch_dec():
            a = X[sv.long()]
            k = torch.exp(-gamma * (xn[:, None] + xn[sv.long()][None, :]
                                    - 2.0 * (X @ a.T)))
            return k @ coef + 0.5
        t_dec, t_dec_torch = alternate(ours_dec, torch_dec, args.rounds,
                                       torch)

        m = min(args.node, n)
        nrows = rows[:m].contiguous()
        yd = torch.from_numpy(y[:m]).cuda()
        stats = {}
        csvm.solve_node(so, X, False, nrows, yd, xn, _lib.SVM_RBF, gamma, 1.0,
                        stats=stats)
        t_solve = timed(lambda: csvm.solve_node(
            so, X, False, nrows, yd, xn, _lib.SVM_RBF, gamma, 1.0), torch)
        t_svc = None
        if not args.no_sklearn:
            from sklearn.svm import SVC
            t0 = time.perf_counter()
            SVC(C=1.0, kernel="rbf", gamma=gamma, tol=1e-3,
                cache_size=4000).fit(x[:m], y[:m])
            t_svc = time.perf_counter() - t0
        print(json.dumps(dict(
            n=n, d=d, q=q,
            rows_s=t_rows, rows_torch_s=t_rows_torch,
            rows_mfma_peak_share=2.0 * q * n * d / t_rows / PEAK_F64_MFMA,
            decision_sv=ns, decision_s=t_dec, decision_torch_s=t_dec_torch,
            node=m, node_solve_s=t_solve, node_outer=stats.get("outer"),
            node_svc_s=t_svc)))


if __name__ == "__main__":
    main()
