"""Measure RandomForestRegressor (never asserted in a test).

One profiled ``fit`` on ``--n`` x ``--d`` samples of Friedman #1 (sklearn's
``make_friedman1``, seeded, ``--d`` >= 5) after one untimed fit, against
sklearn's ``RandomForestRegressor`` with 16 jobs on the host's CPUs: the same
``n_estimators`` and features per split.  Prints one JSON line: ``times_``
(preparation, split search by regime -- the levels with a node above
``RFR_LDS_MAX`` count as streamed -- and partition with the node statistics,
from device events), the whole fit, sklearn's fit and both held-out R^2."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--trees", type=int, default=10)
    a = ap.parse_args()
    import torch
    from sklearn.datasets import make_friedman1
    from sklearn.ensemble import RandomForestRegressor as SkRF

    from dislib_amd.classification.rf import resolve_try_features
    from dislib_amd.data import load_data
    from dislib_amd.regression import RandomForestRegressor
    assert torch.cuda.is_available(), "bench_rfr needs the GPU"
    x, y = make_friedman1(a.n + a.n // 4, a.d, noise=1.0, random_state=0)
    xt, yt, x, y = x[a.n:], y[a.n:], x[:a.n], y[:a.n]
    train = load_data(x, subset_size=a.n // 4 + 1, y=y)
    train._device_data()
    for profile in (False, True):               # the first fit is the warm-up
        est = RandomForestRegressor(n_estimators=a.trees, random_state=0,
                                    profile=profile)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        est.fit(train)
        torch.cuda.synchronize()
        fit = time.perf_counter() - t0
    r2 = est.score(load_data(xt, subset_size=len(xt), y=yt))
    sk = SkRF(n_estimators=a.trees, n_jobs=16, random_state=0,
              max_features=resolve_try_features('sqrt', a.d))
    t0 = time.perf_counter()
    sk.fit(x, y)
    sk_fit = time.perf_counter() - t0
    print(json.dumps(dict(est.times_, fit_ms=1e3 * fit, r2=r2,
                          sk_fit_ms=1e3 * sk_fit, sk_r2=sk.score(xt, yt),
                          nodes=len(est._forest.feature), n=a.n, d=a.d,
                          trees=a.trees)))


if __name__ == "__main__":
    main()
