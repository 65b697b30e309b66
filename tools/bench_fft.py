"""Time ``dislib_amd.fft.fft`` on device tensors against two yardsticks that
are measured in the same run:

* the byte floor of the plan: passes x 32 B per point (each pass reads and
  writes every complex128 once) over the HBM bandwidth of a device copy of
  the same size (``Tensor.copy_``: 32 B per point as well);
* ``torch.fft.fft`` on the same tensor.

Shapes: n = 2^10 and 2^12 with batches that fill the GPU (2^24 points),
n = 2^20 and 2^24 with batch 1.  Every timing is the median of ``--reps``
windows of ``--iters`` calls between device events, after a warm-up; the
three candidates alternate inside a repetition.  One JSON line per shape.

  python tools/bench_fft.py [--reps 7] [--iters 20] [--shapes n:batch,...]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1 << 10, 1 << 14), (1 << 12, 1 << 12), (1 << 20, 1), (1 << 24, 1)]


def window(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), \
        torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def main():
    import numpy as np
    import torch
    from dislib_amd import _device
    from dislib_amd.fft import fft

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fft.py needs a ROCm GPU")
    shapes = SHAPES if not args.shapes else [
        tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]
    for n, batch in shapes:
        g = torch.Generator(device="cuda").manual_seed(n)
        x = torch.randn((batch, n, 2), dtype=torch.float64, device="cuda",
                        generator=g)
        x = torch.view_as_complex(x)
        y = torch.empty_like(x)
        cands = {"fft": lambda: fft(x, rows=True),
                 "torch": lambda: torch.fft.fft(x, dim=1),
                 "copy": lambda: y.copy_(x)}
        ref = cands["torch"]()
        err = float((cands["fft"]() - ref).abs().max() / ref.abs().max())
        for fn in cands.values():                      # warm-up
            window(fn, 3)
        times = {k: [] for k in cands}
        for _ in range(args.reps):
            for k, fn in cands.items():
                times[k].append(window(fn, args.iters))
        med = {k: float(np.median(v)) for k, v in times.items()}
        passes = len(_device.fft_plan(n))
        points = n * batch
        bw = 32.0 * points / med["copy"]
        floor = passes * 32.0 * points / bw
        print(json.dumps({
            "n": n, "batch": batch, "plan": _device.fft_plan(n),
            "fft_ms": med["fft"] * 1e3, "torch_fft_ms": med["torch"] * 1e3,
            "copy_ms": med["copy"] * 1e3, "copy_GBps": bw * 1e-9,
            "byte_floor_ms": floor * 1e3,
            "x_byte_floor": med["fft"] / floor,
            "x_torch_fft": med["fft"] / med["torch"],
            "fft_min_max_ms": [min(times["fft"]) * 1e3,
                               max(times["fft"]) * 1e3],
            "max_rel_diff_vs_torch": err}), flush=True)


if __name__ == "__main__":
    main()
