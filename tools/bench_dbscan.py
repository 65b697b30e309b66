"""Time the passes of DBSCAN (dkm_dbscan.hip) on seeded blobs plus noise,
with the tile prune on and off, next to the yardstick of its pair loop: the
existing ``dkm_radius_count_f64`` with Q = X at the same shape in the same
process (the same pair arithmetic, almost nothing written).

    python tools/bench_dbscan.py [--n 1000000] [--d 2 8] [--reps 3]
                                 [--out profiles/dbscan/bench.json]

Prints one JSON line per shape: the median seconds of the ordering (torch),
the core, link and finalize calls with the prune on and off, the yardstick,
``core_off / yardstick`` (DESIGN.md 3.18 asks for <= 1.15) and the prune's
on / off ratios.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def data(t, n, d, seed):
    """90 % blobs (std 0.5 in a box of +-20) and 10 % uniform noise."""
    g = t.Generator(device="cuda").manual_seed(seed)
    nb = n - n // 10
    c = (t.rand((64, d), generator=g, device="cuda", dtype=t.float64) - 0.5) * 40
    idx = t.randint(0, 64, (nb,), generator=g, device="cuda")
    x = c[idx] + 0.5 * t.randn((nb, d), generator=g, device="cuda",
                               dtype=t.float64)
    noise = (t.rand((n - nb, d), generator=g, device="cuda",
                    dtype=t.float64) - 0.5) * 44
    x = t.cat([x, noise])
    return x[t.randperm(n, generator=g, device="cuda")].contiguous()


def timed(t, fn, reps):
    out = []
    for _ in range(reps):
        t.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def run(n, d, eps, ms, reps):
    import torch as t
    from dislib_amd import _device, _lib
    from dislib_amd._device import ptr, stream_ptr
    from dislib_amd.cluster import dbscan as mod
    so = _lib.lib()
    _device.preload(t.device("cuda", t.cuda.current_device()))
    X = data(t, n, d, 1)
    res = {"n": n, "d": d, "eps": eps, "min_samples": ms, "reps": reps,
           "device": t.cuda.get_device_name()}
    state = {}

    def order():
        perm = mod._cell_order(X, eps, list(range(d)))
        state["orig"] = perm.to(t.int32)
        state["Xs"] = X.index_select(0, perm)
    res["order_s"] = timed(t, order, reps)
    Xs, orig = state["Xs"], state["orig"]
    wsb = int(so.dkm_dbscan_workspace_bytes(n, d))
    ws = t.empty(wsb, dtype=t.uint8, device="cuda")
    wp = ctypes.c_void_p(ws.data_ptr())
    core = t.empty(n, dtype=t.int32, device="cuda")
    parent = t.empty(n, dtype=t.int32, device="cuda")
    attach = t.empty(n, dtype=t.int32, device="cuda")
    labels = t.empty(n, dtype=t.int32, device="cuda")
    ncl = t.zeros(1, dtype=t.int32, device="cuda")
    counts = t.empty(n, dtype=t.int64, device="cuda")

    def yard():
        _lib.check(so.dkm_radius_count_f64(
            ptr(Xs), n, d, ptr(Xs), n, d, d, eps, ptr(counts), stream_ptr()),
            "radius_count")
    yard()                                   # warm-up
    res["yardstick_s"] = timed(t, yard, reps)
    for tag, flags in (("on", 0), ("off", _lib.DBSCAN_NOPRUNE)):
        def corep():
            _lib.check(so.dkm_dbscan_core_f64(
                ptr(Xs), n, d, d, eps, ms, flags, wp, wsb, ptr(core),
                stream_ptr()), "core")

        def link():
            _lib.check(so.dkm_dbscan_link_f64(
                ptr(Xs), n, d, d, eps, flags, wp, wsb, ptr(core), ptr(orig),
                ptr(parent), ptr(attach), stream_ptr()), "link")

        def fin():
            _lib.check(so.dkm_dbscan_finalize(
                n, ms, wp, wsb, ptr(core), ptr(orig), ptr(parent),
                ptr(attach), ptr(labels), ptr(ncl), stream_ptr()), "finalize")
        corep()                              # warm-up
        res["core_%s_s" % tag] = timed(t, corep, reps)
        res["link_%s_s" % tag] = timed(t, link, reps)
        link()                               # a fresh forest for finalize
        res["finalize_%s_s" % tag] = timed(t, fin, 1)
        res["n_clusters_%s" % tag] = int(ncl.item())
        res["noise_%s" % tag] = int((labels < 0).sum().item())
        res["core_rows_%s" % tag] = int(core.sum().item())
        state[tag] = labels.clone()
    res["labels_equal"] = bool(t.equal(state["on"], state["off"]))
    res["core_off_over_yardstick"] = res["core_off_s"] / res["yardstick_s"]
    res["core_on_over_off"] = res["core_on_s"] / res["core_off_s"]
    res["link_on_over_off"] = res["link_on_s"] / res["link_off_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--eps", type=float, nargs="+", default=None,
                    help="one eps per --d (default 0.1 for d = 2, else 0.8)")
    ap.add_argument("--min-samples", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    eps = a.eps or [0.1 if d == 2 else 0.8 for d in a.d]
    rows = []
    for d, e in zip(a.d, eps):
        r = run(a.n, d, e, a.min_samples, a.reps)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
