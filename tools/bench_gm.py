"""Time one GaussianMixture EM iteration on a resident Dataset, pass by pass,
against its two yardsticks:

  python tools/bench_gm.py [--shape NAME ...] [--reps 5] [--limit 300]
                           [--scale 1.0]

Per shape (n = 2^20 fp64 rows; "d16k8", "d16k32", "d64k8", "d64k32";
device-made blobs) it records the median over ``--reps`` alternating rounds
(every variant once per round, in turn) of

* the E-step (``dkm_gm_estep_*``), the M-step sums (``dkm_gm_mstep_sums_*``),
  the M-step covariances (``dkm_gm_mstep_cov_*``) and the host share of an
  iteration: the two device-to-host copies, numpy / scipy on K d and K d^2
  values (Cholesky, triangular solve) and the parameter uploads;
* yardstick 1, the same three passes written with ``torch.matmul`` /
  ``torch.logsumexp`` in fp64 on the same matrix (K matmuls per pass, as
  the reference does per Subset);
* yardstick 2, the bytes an iteration must move: X read three times, resp
  written once and read twice, as a time at the rate of a device-to-device
  copy of X timed in the same rounds.

Every shape runs in a child process of its own under a time limit
(--limit seconds): the parent never opens the GPU.  One JSON line per shape.
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

N = 1 << 20
SHAPES = {"d16k8": (16, 8), "d16k32": (16, 32), "d64k8": (64, 8),
          "d64k32": (64, 32)}


def child(a):
    import math

    import numpy as np
    import torch

    from dislib_amd import _device
    from dislib_amd.cluster.gm import GaussianMixture, _EM
    from dislib_amd.data import load_data
    d, K = SHAPES[a.child]
    n = max(1024, int(N * a.scale))
    torch.cuda.set_device(0)
    X = torch.empty((n, d), dtype=torch.float64, device="cuda")
    _device.make_blobs(X, 0, K, 7, box=6.0, std=2.5)
    ds = load_data(X, subset_size=n // 8)
    dd = ds._device_data()

    # a model one iteration into a random initialisation
    gm = GaussianMixture(n_components=K, init_params='random',
                         random_state=0, max_iter=1)
    em = _EM(dd, K)
    rs = np.random.RandomState(0)
    resp0 = torch.from_numpy(rs.dirichlet(np.ones(K), n)).cuda()
    em.resp.copy_(resp0)
    gm.reg_covar = 1e-6
    em.m_step(gm)
    mu, pc = gm.means_, gm.precisions_cholesky_
    ldw = np.sum(np.log(pc.reshape(K, -1)[:, ::d + 1]), 1) + \
        np.log(gm.weights_)
    dmu, dpc, dldw = (em._dev(v) for v in (mu, pc, ldw))
    head = em.head
    Xc = torch.empty_like(X)

    def host_share():
        h = head.cpu().numpy()
        nk = h[1:1 + K] + 10 * np.finfo(np.float64).eps
        means = h[1 + K:].reshape(K, d) / nk[:, None]
        em._dev(means)
        cov = em.cov.cpu().numpy()
        for k in range(K):
            cov[k] /= nk[k]
            cov[k].flat[::d + 1] += 1e-6
        from dislib_amd.cluster.gm import _compute_precision_cholesky
        p = _compute_precision_cholesky(cov)
        em._dev(p)
        return p

    cst = d * math.log(2 * math.pi)

    def torch_estep():
        lp = torch.empty((n, K), dtype=torch.float64, device="cuda")
        for k in range(K):
            y = torch.matmul(X, dpc[k]) - torch.matmul(dmu[k], dpc[k])
            lp[:, k] = (y * y).sum(1)
        wlp = -.5 * (cst + lp) + dldw
        lse = torch.logsumexp(wlp, 1)
        return torch.exp(wlp - lse[:, None]), lse.sum()

    def torch_sums():
        return em.resp.sum(0), torch.matmul(em.resp.T, X)

    def torch_cov():
        out = torch.empty((K, d, d), dtype=torch.float64, device="cuda")
        for k in range(K):
            diff = X - dmu[k]
            out[k] = torch.matmul(em.resp[:, k] * diff.T, diff)
        return out

    variants = {
        "estep": lambda: _device.gm_estep(dd, dmu, dpc, dldw, True, em.ws,
                                          em.resp, None, em.lpn[:1]),
        "mstep_sums": lambda: _device.gm_mstep_sums(dd, em.resp, em.ws,
                                                    head[1:]),
        "mstep_cov": lambda: _device.gm_mstep_cov(dd, em.resp, dmu, em.ws,
                                                  em.cov),
        "host": host_share,
        "copy": lambda: Xc.copy_(X),
        "torch_estep": torch_estep,
        "torch_sums": torch_sums,
        "torch_cov": torch_cov,
    }
    times = {k: [] for k in variants}
    for r in range(a.reps + 1):          # round 0 warms up
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            dt = 1e3 * (time.perf_counter() - t0)
            del out
            if r:
                times[name].append(dt)
    med = {k: statistics.median(v) for k, v in times.items()}
    ours = med["estep"] + med["mstep_sums"] + med["mstep_cov"]
    tor = med["torch_estep"] + med["torch_sums"] + med["torch_cov"]
    copy_rate = 2 * n * d * 8 / med["copy"]            # bytes per ms
    floor = (3 * n * d * 8 + 3 * n * K * 8) / copy_rate
    flops = {"estep": n * K * d * (d + 1.0),           # upper triangle
             "mstep_sums": 2.0 * n * K * (d + 1),
             "mstep_cov": n * K * d * (d + 1.0)}
    res = {"shape": a.child, "n": n, "d": d, "k": K, "rounds": a.reps,
           "ms": {k: round(v, 3) for k, v in med.items()},
           "ms_all": {k: [round(x, 3) for x in v] for k, v in times.items()},
           "kernels_ms": round(ours, 3), "torch_ms": round(tor, 3),
           "kernels_over_torch": {
               "estep": round(med["estep"] / med["torch_estep"], 3),
               "mstep_sums": round(med["mstep_sums"] / med["torch_sums"], 3),
               "mstep_cov": round(med["mstep_cov"] / med["torch_cov"], 3),
               "iteration": round(ours / tor, 3)},
           "bytes_floor_ms": round(floor, 3),
           "kernels_over_floor": round(ours / floor, 2),
           "host_share": round(med["host"] / (ours + med["host"]), 3),
           "tflops": {k: round(v / med[k] / 1e9, 2)
                      for k, v in flops.items()}}
    print("RESULT " + json.dumps(res), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--limit", type=int, default=300)
    p.add_argument("--scale", type=float, default=1.0)
    p.add_argument("--child")
    a = p.parse_args()
    if a.child:
        child(a)
        return 0
    for name in a.shape or list(SHAPES):
        try:
            r = subprocess.run(
                [sys.executable, os.path.abspath(__file__), "--child", name,
                 "--reps", str(a.reps), "--scale", str(a.scale)],
                capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"shape": name, "error": "time limit"}))
            return 1
        lines = [ln for ln in r.stdout.splitlines()
                 if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            print(json.dumps({"shape": name, "error": r.stderr[-2000:]}))
            return 1
        print(lines[-1][7:], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
