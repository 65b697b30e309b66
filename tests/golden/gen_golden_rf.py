"""Golden vectors for ``RandomForestClassifier``, produced by the REFERENCE
itself, imported under the sequential PyCOMPSs stub of ``gen_golden.py`` (as
``gen_golden_csvm.py`` does); nothing of the reference is copied.

``rf_ref.npz`` holds

* ``<case>__values`` / ``__y`` / ``__meta`` = [n_classes] and the reference's
  own ``test_split`` result ``__score`` / ``__value`` for small node cases, in
  fp64 and (``_f32``) fp32;
* ``acc``: the probe accuracy of the yardstick forest for ``random_state``
  0..9 on ``make_classification(1200, 12, n_informative=6, n_classes=3,
  random_state=0)``, 900 rows to fit (three Subsets of 300) and 300 to probe,
  ``n_estimators=10``; ``acc_source``: which yardstick ran -- the reference's
  ``RandomForestClassifier``, or sklearn's ``RandomForestClassifier(
  n_estimators=10, max_features='sqrt')`` if the reference forest cannot run
  under the stub.

Run in the development container only:
``python tests/golden/gen_golden_rf.py``.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def node_cases():
    import numpy as np
    rng = np.random.RandomState(7)
    c = {}
    c["single"] = ([1.5], [0], 2)
    c["pair"] = ([2.0, 1.0], [1, 0], 2)
    c["pure"] = (rng.rand(9), [1] * 9, 3)
    c["constant"] = ([3.0] * 8, [0, 1, 0, 1, 1, 0, 2, 2], 3)
    c["distinct"] = (rng.permutation(65).astype(float), rng.randint(0, 3, 65),
                     3)
    c["runs"] = (rng.randint(0, 4, 257).astype(float), rng.randint(0, 3, 257),
                 3)
    c["equal_proportions"] = ([0., 0., 1., 1., 2., 2.], [0, 1, 0, 1, 0, 1], 2)
    c["two_minima"] = ([0., 1., 2., 3.], [0, 1, 1, 0], 2)
    c["signed_zero"] = ([-0.0, 0.0, 1.0, -1.0], [0, 0, 1, 1], 2)
    c["many_classes"] = (rng.randint(0, 20, 300).astype(float),
                         rng.randint(0, 32, 300), 32)
    return c


def generate():
    import numpy as np
    from sklearn.datasets import make_classification
    from dislib.classification.rf.test_split import test_split
    out = {}
    for name, (v, y, nc) in node_cases().items():
        for tag, dt in (("", np.float64), ("_f32", np.float32)):
            v_ = np.asarray(v, dtype=dt)
            y_ = np.asarray(y, dtype=np.int64)
            score, value = test_split(np.arange(len(y_)), y_, v_, nc)
            k = name + tag
            out[k + "__values"] = v_
            out[k + "__y"] = y_
            out[k + "__meta"] = np.array([nc])
            out[k + "__score"] = np.float64(score)
            out[k + "__value"] = np.float64(value)
    x, y = make_classification(1200, 12, n_informative=6, n_classes=3,
                               random_state=0)
    acc, source = [], "reference"
    try:
        from dislib.classification import RandomForestClassifier
        from dislib.data import Dataset, Subset
        for seed in range(10):
            ds = Dataset(n_features=12)
            for a in range(0, 900, 300):
                ds.append(Subset(x[a:a + 300], y[a:a + 300]))
            probe = Dataset(n_features=12)
            probe.append(Subset(x[900:], y[900:]))
            est = RandomForestClassifier(n_estimators=10, random_state=seed)
            est.fit(ds)
            acc.append(float(est.score(probe)))
    except Exception as e:             # the stub cannot run the forest
        print("reference forest failed under the stub:", repr(e))
        from sklearn.ensemble import RandomForestClassifier as SkRF
        acc, source = [], "sklearn"
        for seed in range(10):
            est = SkRF(n_estimators=10, max_features='sqrt',
                       random_state=seed).fit(x[:900], y[:900])
            acc.append(float(est.score(x[900:], y[900:])))
    out["acc"] = np.array(acc)
    out["acc_source"] = np.array(source)
    print("rf yardstick", source, acc)
    np.savez_compressed(os.path.join(HERE, "rf_ref.npz"), **out)
    print("wrote rf_ref.npz")


def main():
    try:
        import dislib  # noqa: F401
        import pycompss  # noqa: F401
        ok = True
    except ImportError:
        ok = False
    if ok:
        generate()
        return
    if not os.path.isdir(REF):
        print("reference not present; golden vectors are committed -- skip")
        return
    sys.path.insert(0, HERE)
    from gen_golden import SHIM
    shim = tempfile.mkdtemp(prefix="dkm_shim_")
    for rel, body in SHIM.items():
        p = os.path.join(shim, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w") as f:
            f.write(body)
    env = dict(os.environ, PYTHONPATH=shim + ":" + REF,
               PYTHONDONTWRITEBYTECODE="1")
    sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)],
                             env=env, cwd=REF))


if __name__ == "__main__":
    main()
