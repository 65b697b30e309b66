"""Measure RandomForestClassifier (never asserted in a test).

``fit`` and ``predict`` on ``--n`` x ``--d`` samples of ``--classes`` classes
(sklearn's ``make_classification``, seeded) against sklearn's
``RandomForestClassifier`` with 16 jobs on the host's CPUs: the same
``n_estimators``, ``max_features='sqrt'`` and bootstrap.  Our fit is split
into preparation (sort and rank of every feature), split search by regime
(the levels with a node above ``RF_LDS_MAX`` count as streamed) and
partition, from device events around the launches of every level; the rest
of the fit is host work and the per-level read-back (``profile=True``; a
fit without it is timed as well, ``fit_plain_ms``).  ``predict`` is timed over
``--predict-reps`` back-to-back ``score`` calls on ``--n`` rows that end in a
device synchronise.  One untimed round first, then ``--rounds`` alternating
rounds; prints one JSON line of medians with ``<key>_min`` / ``<key>_max``."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--trees", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--predict-reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    from sklearn.datasets import make_classification
    from sklearn.ensemble import RandomForestClassifier as SkRF

    from dislib_amd.classification import RandomForestClassifier
    from dislib_amd.data import load_data
    assert torch.cuda.is_available(), "bench_rf needs the GPU"
    x, y = make_classification(2 * a.n, a.d, n_informative=a.d // 2,
                               n_classes=a.classes, random_state=0)
    xt, yt, x, y = x[a.n:], y[a.n:], x[:a.n], y[:a.n]
    train = load_data(x, subset_size=a.n // 4 + 1, y=y)
    train._device_data()
    rows = []
    for r in range(a.rounds + 1):
        fits = []
        for profile in (False, True):
            est = RandomForestClassifier(n_estimators=a.trees, random_state=r,
                                         profile=profile)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            est.fit(train)
            torch.cuda.synchronize()
            fits.append(time.perf_counter() - t0)
        plain, fit = fits
        test = load_data(xt, subset_size=len(xt), y=yt)
        test._device_data()
        est.score(test)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.predict_reps):
            acc = est.score(test)
        torch.cuda.synchronize()
        pred = (time.perf_counter() - t0) / a.predict_reps
        sk = SkRF(n_estimators=a.trees, max_features='sqrt', n_jobs=16,
                  random_state=r)
        t0 = time.perf_counter()
        sk.fit(x, y)
        sk_fit = time.perf_counter() - t0
        t0 = time.perf_counter()
        sk_acc = sk.score(xt, yt)
        sk_pred = time.perf_counter() - t0
        if r:                                   # round 0 is the warm-up
            rows.append(dict(est.times_, fit_ms=1e3 * fit,
                             fit_plain_ms=1e3 * plain,
                             predict_ms=1e3 * pred, acc=acc,
                             sk_fit_ms=1e3 * sk_fit,
                             sk_predict_ms=1e3 * sk_pred, sk_acc=sk_acc,
                             nodes=len(est._forest.feature)))
    keys = sorted(set().union(*rows))
    out = {}
    for k in keys:
        v = [r.get(k, 0.0) for r in rows]
        out.update({k: float(np.median(v)), k + "_min": float(min(v)),
                    k + "_max": float(max(v))})
    out.update(n=a.n, d=a.d, classes=a.classes, trees=a.trees,
               rounds=a.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
