"""Time one ALS half-step (dkm_als.hip) pass by pass on a seeded random
ratings matrix, next to two yardsticks: the half-step's flop count at the f64
MFMA peak, and a torch composition of the same solve on the same data
(padded gather -> ``bmm`` -> ``torch.linalg.cholesky`` -> ``cholesky_solve``).

    python tools/bench_als.py [--n 1048576] [--m 65536] [--nnz 64]
                              [--nf 32 100] [--reps 3]
                              [--out profiles/als/bench.json]

Prints one JSON line per n_f: the median seconds of the device transpose
(torch), the row means, the update with fp32 factors, the squared error over
all rows and the torch composition (in row batches that fit its padded
gather), the update's flops (2 nnz n_f^2 for the Gram matrices plus n_f^3 / 3
per non-empty row for the factorisations) and its fraction of the f64 MFMA
peak, and the largest difference between the two solutions.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F64_MFMA = 78.6e12      # MI355X, dense fp64 matrix flop/s


def data(t, n, m, nnz, seed):
    """CSR (n x m): row lengths uniform in [1, 2 nnz - 1], random columns
    (duplicates within a row are possible and harmless here), ratings
    1-5."""
    g = t.Generator(device="cuda").manual_seed(seed)
    lens = t.randint(1, 2 * nnz, (n,), generator=g, device="cuda")
    indptr = t.zeros(n + 1, dtype=t.int64, device="cuda")
    indptr[1:] = t.cumsum(lens, 0)
    total = int(indptr[-1].item())
    indices = t.randint(0, m, (total,), generator=g, device="cuda",
                        dtype=t.int32)
    vals = t.randint(1, 6, (total,), generator=g,
                     device="cuda").to(t.float64)
    return indptr, indices, vals


def timed(t, fn, reps):
    out = []
    for _ in range(reps):
        t.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def torch_half_step(t, csr, X, lambda_, batch):
    """The same normal equations by torch, ``batch`` rows at a time."""
    n_f = X.shape[1]
    X64 = X.to(t.float64)
    out = t.empty((csr.n_rows, n_f), dtype=t.float32, device=X.device)
    lens = csr.indptr[1:] - csr.indptr[:-1]
    eye = t.eye(n_f, dtype=t.float64, device=X.device)
    for a in range(0, csr.n_rows, batch):
        b = min(a + batch, csr.n_rows)
        ln = lens[a:b]
        width = int(ln.max().item())
        pos = t.arange(width, device=X.device)[None, :]
        mask = pos < ln[:, None]
        e = (csr.indptr[a:b, None] + pos).clamp_(max=csr.nnz - 1)
        rows = X64[csr.indices[e].long()] * mask[:, :, None]
        r = csr.data[e] * mask
        gram = t.bmm(rows.transpose(1, 2), rows) + \
            (lambda_ * ln.to(t.float64))[:, None, None] * eye
        v = t.bmm(rows.transpose(1, 2), r[:, :, None])
        chol = t.linalg.cholesky(gram)
        out[a:b] = t.cholesky_solve(v, chol)[:, :, 0].to(t.float32)
    return out


def run(n, m, nnz, n_f, reps):
    import torch as t
    from dislib_amd import _device, _lib
    from dislib_amd.recommendation import als
    so = _lib.lib()
    _device.preload(t.device("cuda", t.cuda.current_device()))
    csr = als._Csr(*data(t, n, m, nnz, 1), n, m)
    g = t.Generator(device="cuda").manual_seed(2)
    X = t.rand((m, n_f), generator=g, device="cuda", dtype=t.float32)
    U = t.rand((n, n_f), generator=g, device="cuda", dtype=t.float32)
    res = {"n": n, "m": m, "nnz": csr.nnz, "n_f": n_f, "reps": reps,
           "device": t.cuda.get_device_name()}
    res["transpose_s"] = timed(t, lambda: als.csr_transpose(csr), reps)
    res["row_means_s"] = timed(t, lambda: als.row_means(so, csr), reps)
    als.update(so, csr, X, 0.065)                      # warm-up
    res["update_s"] = timed(t, lambda: als.update(so, csr, X, 0.065), reps)
    res["sse_s"] = timed(
        t, lambda: als.sse(so, csr, U, X, 0, n, 0), reps)
    flops = 2.0 * csr.nnz * n_f * n_f + n * n_f ** 3 / 3.0
    res["update_flops"] = flops
    res["mfma_peak_s"] = flops / PEAK_F64_MFMA
    res["update_frac_of_peak"] = res["mfma_peak_s"] / res["update_s"]
    batch = max(1, min(n, (1 << 28) // (2 * nnz * n_f + n_f * n_f)))
    torch_half_step(t, csr, X, 0.065, batch)           # warm-up
    res["torch_s"] = timed(
        t, lambda: torch_half_step(t, csr, X, 0.065, batch), reps)
    res["torch_batch_rows"] = batch
    res["update_over_torch"] = res["update_s"] / res["torch_s"]
    res["max_abs_diff"] = float((als.update(so, csr, X, 0.065) -
                                 torch_half_step(t, csr, X, 0.065,
                                                 batch)).abs().max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--m", type=int, default=1 << 16)
    ap.add_argument("--nnz", type=int, default=64)
    ap.add_argument("--nf", type=int, nargs="+", default=[32, 100])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    results = []
    for n_f in a.nf:
        res = run(a.n, a.m, a.nnz, n_f, a.reps)
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
