"""Generate the StandardScaler goldens s01 .. s07 by running the REFERENCE
``dislib.preprocessing.StandardScaler`` (dislib v0.2.0).

Run in the development container only:
``python tests/golden/gen_golden_scaler.py``

Like ``gen_golden.py`` it runs the reference in PyCOMPSs sequential
semantics through that file's stub package (``SHIM``); no reference source
is copied: this script imports it and records its outputs as ``.npz`` data.
The inputs are built by ``tests/scaler_ref.py`` (``inputs``), which the
tests share; an input that a fixed seed or another golden regenerates is
stored as its sha256.  ``mean_`` and ``var_`` are stored in full; the scaled
matrix in full when it has at most 4096 elements or holds a NaN, otherwise
as its sha256.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from gen_golden import REF, SHIM, sha  # noqa: E402

SMALL = 4096


def generate():
    import numpy as np
    from dislib.data import Dataset, Subset
    from dislib.preprocessing import StandardScaler

    from tests import scaler_ref as sr

    def dataset(x, sizes):
        ds = Dataset(n_features=x.shape[1])
        for block in sr.split(x, sizes):
            ds.append(Subset(block))
        return ds

    def scaled(ds):
        return np.concatenate([s.samples for s in ds])

    def record(out, key, y):
        if y.size <= SMALL or np.isnan(y).any():
            out[key + "y"] = y
        else:
            out[key + "y_sha"] = np.array(sha(y))
        out[key + "y_dtype"] = np.array(str(y.dtype))

    for name in ("s01", "s02", "s03", "s04", "s05", "s06"):
        out = {}
        for key, x, sizes, arities in sr.inputs(name):
            out[key + "x_sha"] = np.array(sha(x))
            out[key + "sizes"] = np.array(sizes)
            for arity in arities:
                k = key if len(arities) == 1 else "%sa%d_" % (key, arity)
                ds = dataset(x, sizes)
                sc = StandardScaler(arity=arity)
                with np.errstate(all="ignore"):
                    sc.fit_transform(ds)
                out[k + "mean"], out[k + "var"] = sc.mean_, sc.var_
                record(out, k, scaled(ds))
        if name == "s02":
            # the tree is not a formality: the two arities give other bits
            assert not (np.array_equal(out["a50_mean"], out["a2_mean"]) and
                        np.array_equal(out["a50_var"], out["a2_var"])), \
                "s02: both trees give the same bits -- pick another input"
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
        print("wrote", name)

    # s07 -- s01's fp64 statistics on an fp32 Dataset: fp64 output
    (_, x, sizes, _), = sr.inputs("s07")
    sc = StandardScaler(arity=50)
    sc.fit(dataset(x, sizes))
    x32, sizes32 = sr.s07_input()
    ds = dataset(x32, sizes32)
    sc.transform(ds)
    out = {"x_sha": np.array(sha(x32)), "sizes": np.array(sizes32),
           "mean": sc.mean_, "var": sc.var_}
    record(out, "", scaled(ds))
    np.savez_compressed(os.path.join(HERE, "s07.npz"), **out)
    print("wrote s07")


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
