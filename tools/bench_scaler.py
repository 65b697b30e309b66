"""Time StandardScaler on a resident Dataset against its two yardsticks:

  python tools/bench_scaler.py [--shape NAME ...] [--reps 5] [--limit 500]
                               [--scale 1.0] [--membench tools/membench]

Per shape ("headline": 100M x 32 fp64 in 100 Subsets; "f32": 25M x 64 fp32
in 25 Subsets; device-made blobs) it records the median over ``--reps``
alternating rounds (every variant once per round, in turn) of

* ``fit``, ``transform`` and ``fit_transform`` with sums="fast", and ``fit``
  with sums="reference" (fewer rounds: it is slow by definition);
* yardstick 1, the bytes each call must move: ``fit`` reads X twice,
  ``transform`` reads X and writes Y.  Their rate in TB/s, and as a fraction
  of (a) the device-to-device copy of the same matrix (``Y.copy_(X)``: one
  read and one write) timed in the same rounds and (b) the best contiguous
  read rate ``tools/membench`` prints for the shape's fp64 footprint when
  its binary is given (membench times reads only);
* yardstick 2, the torch expressions a user would otherwise write on the
  same matrix: ``X.mean(0)``, ``((X - m) ** 2).mean(0)`` and
  ``(X - m) / v.sqrt()``, and the peak HBM they allocate beside X.

Every shape runs in a child process of its own under a time limit
(--limit seconds): the parent never opens the GPU.  One JSON line per shape.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    # name: (n, d, dtype, Subsets)
    "headline": (100_000_000, 32, "float64", 100),
    "f32": (25_000_000, 64, "float32", 25),
}


def _make(torch, n, d, dtype):
    from dislib_amd import _device
    X = torch.empty((n, d), dtype=getattr(torch, dtype), device="cuda")
    step = 5_000_000
    for r0 in range(0, n, step):
        m = min(step, n - r0)
        blk = torch.empty((m, d), dtype=torch.float64, device="cuda")
        _device.make_blobs(blk, r0, 16, 7)
        X[r0:r0 + m] = blk
    return X


def child(a):
    import torch
    from dislib_amd.data import load_data
    from dislib_amd.preprocessing import StandardScaler
    n, d, dtype, subsets = SHAPES[a.child]
    n = max(subsets, int(n * a.scale) // subsets * subsets)
    torch.cuda.set_device(0)
    X = _make(torch, n, d, dtype)
    isz = X.element_size()

    def fresh():
        ds = load_data(X, subset_size=n // subsets)
        ds._device_data()
        return ds

    fitted = StandardScaler()
    fitted.fit(fresh())
    Ycopy = torch.empty_like(X)

    def run_fit(sums):
        ds = fresh()
        return lambda: StandardScaler(sums=sums).fit(ds)

    def run_transform():
        ds = fresh()
        return lambda: fitted.transform(ds)

    def run_fit_transform():
        ds = fresh()
        return lambda: StandardScaler().fit_transform(ds)

    def torch_fit():
        m = X.mean(0)
        return m, ((X - m) ** 2).mean(0)

    tm, tv = torch_fit()

    variants = {
        "fit_fast": lambda: run_fit("fast"),
        "transform": run_transform,
        "fit_transform": run_fit_transform,
        "copy": lambda: (lambda: Ycopy.copy_(X)),
        "torch_fit": lambda: torch_fit,
        "torch_transform": lambda: (lambda: (X - tm) / tv.sqrt()),
        "fit_reference": lambda: run_fit("reference"),
    }
    times = {k: [] for k in variants}
    peaks = {}
    for r in range(a.reps + 1):          # round 0 warms up
        for name, prep in variants.items():
            if name == "fit_reference" and r > max(1, a.reps // 2):
                continue
            fn = prep()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            dt = 1e3 * (time.perf_counter() - t0)
            peaks[name] = torch.cuda.max_memory_allocated() - base
            del out, fn
            if r:
                times[name].append(dt)
    med = {k: statistics.median(v) for k, v in times.items()}
    gb = n * d * isz / 1e9
    rate = {"fit_fast": 2 * gb / med["fit_fast"],
            "fit_reference": 2 * gb / med["fit_reference"],
            "transform": 2 * gb / med["transform"],
            "copy": 2 * gb / med["copy"]}            # TB/s (GB per ms)
    res = {"shape": a.child, "n": n, "d": d, "dtype": dtype,
           "subsets": subsets, "rounds": a.reps,
           "ms": {k: round(v, 3) for k, v in med.items()},
           "ms_all": {k: [round(x, 3) for x in v] for k, v in times.items()},
           "tb_per_s": {k: round(v, 3) for k, v in rate.items()},
           "fraction_of_copy": {k: round(rate[k] / rate["copy"], 3)
                                for k in ("fit_fast", "transform")},
           "peak_bytes_beside_x": peaks,
           "fast_over_torch": {
               "fit": round(med["fit_fast"] / med["torch_fit"], 3),
               "transform": round(med["transform"] / med["torch_transform"],
                                  3)},
           "reference_over_fast_fit": round(
               med["fit_reference"] / med["fit_fast"], 1)}
    print("RESULT " + json.dumps(res), flush=True)


def membench_read(binary, n, d, isz):
    """Best contiguous read rate (TB/s) membench prints for rows of 32 or
    64 fp64 covering the same bytes; None without the binary."""
    if not binary or not os.path.exists(binary):
        return None
    dd = 32 if d * isz // 8 <= 32 else 64
    rows = n * d * isz // (8 * dd)
    r = subprocess.run([binary, str(rows), str(dd)], capture_output=True,
                       text=True, timeout=120)
    if r.returncode != 0:
        return None
    best = [float(v) for v in re.findall(r"contig [\d.]+ ms (\d+) GB/s",
                                         r.stdout)]
    return max(best) / 1e3 if best else None


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--limit", type=int, default=500)
    p.add_argument("--scale", type=float, default=1.0)
    p.add_argument("--membench", default=os.path.join(ROOT, "tools",
                                                      "membench"))
    p.add_argument("--child")
    a = p.parse_args()
    if a.child:
        child(a)
        return 0
    for name in a.shape or list(SHAPES):
        n, d, dtype, subsets = SHAPES[name]
        n = max(subsets, int(n * a.scale) // subsets * subsets)
        isz = 4 if dtype == "float32" else 8
        read = membench_read(a.membench, n, d, isz)
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
        res = json.loads(lines[-1][7:])
        res["membench_read_tb_per_s"] = read
        if read:
            res["fraction_of_membench_read"] = {
                "fit_fast": round(res["tb_per_s"]["fit_fast"] / read, 3)}
        print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
