"""Golden vectors for ``CascadeSVM``, produced by the REFERENCE itself:
``dislib.classification.CascadeSVM`` (``dislib/classification/csvm/base.py``)
run the way ``gen_golden_als.py`` runs its cases -- imported under the
sequential PyCOMPSs stub of ``gen_golden.py``.

The reference trains every node with ``sklearn.svm.SVC`` (libsvm), whose
solution is only defined up to its stopping tolerance.  So every case runs
three times, by monkeypatching the ``SVC`` name in the reference's module
(nothing of the reference is copied): as is, with ``shrinking=False`` and with
``tol=1e-6``.  ``_create_ids`` is patched as well, to hand out the global row
numbers in place of ``uuid4`` values, so that the support vectors can be named
by row; ``_lagrangian_fast`` is wrapped to record the ``W`` sequence.

Stored once per dataset (``data_<name>__x``, ``__y``, ``__probe``) and per
case (``<case>__key``): ``data`` (the dataset's name), ``sizes`` (rows per
Subset), ``meta`` = [fp32 input, arity, max_iter, tol, rbf, C, gamma (-1 =
"auto"), check_convergence, label shift], and of the run as is:
``iterations``, ``converged``, ``w``, the probe decision values ``dec`` and
labels ``pred``; over the three runs: ``dec_spread`` (the largest probe
decision difference), ``w_gap`` (the largest relative ``W`` difference at a
common iteration), ``clear_sv`` (rows that are support vectors with ``alpha >=
0.01 C`` in all three) and ``clear_nonsv`` (rows with ``y f(x) >= 1 + 10
dec_spread`` in all three).

The script refuses to write the file when, in any case, the three runs
disagree on ``iterations`` or ``converged``; some iteration's ``|dW / W|``
lies within ``100 x w_gap`` of ``tol``, both relative: ``| |dW / W| - tol | <=
100 w_gap tol`` (cases with ``tol <= 0`` are exempt: ``|dW / W| < tol`` is
false whatever ``W`` is); or more than 10 % of the probe rows have
``|decision| < 10 x dec_spread``.  The cases were picked for that.

Run in the development container only:
``python tests/golden/gen_golden_csvm.py``.  Writes ``csvm_ref.npz``.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def datasets():
    import numpy as np
    from sklearn.datasets import make_blobs, make_classification
    out = {}
    x, y = make_classification(600, 12, n_informative=6, class_sep=0.8,
                               flip_y=0.05, random_state=0)
    out["cls"] = (x, y)
    for seed in (0, 1):
        out["blobs%d" % seed] = make_blobs(600, 8, centers=2,
                                           cluster_std=4.0, random_state=seed)
    p1, p2, p3, p4 = [1, 2], [2, 1], [-1, -2], [-2, -1]
    out["toy"] = (np.array([p1, p4, p3, p2], dtype=np.float64),
                  np.array([0, 1, 1, 0]))
    a1, a2, a3, a4 = [0, 2], [0, 1], [0, -2], [0, -1]
    out["toyaxis"] = (np.array([a1, a4, a3, a2], dtype=np.float64),
                      np.array([0, 1, 1, 0]))
    out["dup"] = (np.array([[0, 1], [1, 1], [0, 1], [1, 2], [0, 0], [2, 2],
                            [2, 1], [1, 0]], dtype=np.float64),
                  np.array([1, 0, 1, 0, 1, 0, 0, 1]))
    probes = {}
    for name, (x, y) in out.items():
        rng = np.random.default_rng(len(name) + x.shape[0])
        if x.shape[0] > 100:
            pick = rng.choice(x.shape[0], 200, replace=False)
            probes[name] = x[pick] + 0.3 * rng.standard_normal((200,
                                                                x.shape[1]))
        else:
            probes[name] = np.concatenate(
                [x, [[1, 1], [-1, -1], [1, 0], [-1, 0]]]).astype(np.float64)
    return out, probes


def cases():
    big = dict(cascade_arity=2, max_iter=8, tol=1e-3, c=1)
    toy = dict(cascade_arity=3, max_iter=10, tol=1e-4, c=2, gamma=0.1)
    # (name, dataset, subset sizes, fp32, label shift, constructor arguments)
    return [
        ("rbf_auto", "cls", [100] * 6, 0, 0, dict(big, kernel="rbf")),
        ("lin_b0", "blobs0", [100] * 6, 0, 0, dict(big, kernel="linear")),
        ("lin_b1", "blobs1", [100] * 6, 0, 0, dict(big, kernel="linear")),
        ("nonfinite", "blobs0", [100] * 6, 0, 0,
         dict(kernel="rbf", gamma=0.5)),
        ("arity3_s7", "cls", [90] * 6 + [60], 0, 0,
         dict(big, kernel="rbf", cascade_arity=3)),
        ("noconv", "cls", [100] * 6, 0, 0,
         dict(big, kernel="rbf", check_convergence=False, max_iter=1)),
        ("labels12", "cls", [100] * 6, 0, 1, dict(big, kernel="rbf")),
        ("rbf_auto_f32", "cls", [100] * 6, 1, 0, dict(big, kernel="rbf")),
        ("toy_predict", "toy", [2, 2], 0, 0,
         dict(toy, kernel="linear", check_convergence=False)),
        ("toy_score", "toy", [2, 2], 0, 0, dict(toy, kernel="rbf")),
        ("toy_decision", "toyaxis", [2, 2], 0, 0,
         dict(toy, kernel="rbf", check_convergence=False)),
        ("duplicates", "dup", [2] * 4, 0, 0, dict(c=1, max_iter=100, tol=0)),
    ]


def generate():
    import numpy as np
    from sklearn.svm import SVC
    import dislib.classification.csvm.base as base
    from dislib.classification import CascadeSVM
    from dislib.data import Dataset, Subset

    counter = [0]

    def create_ids(subset):
        n = subset.samples.shape[0]
        counter[0] += n
        return np.arange(counter[0] - n, counter[0])
    base._create_ids = create_ids

    inner_w = CascadeSVM._lagrangian_fast

    def lagr(self, *a, **k):
        with np.errstate(over="ignore", invalid="ignore"):
            w = inner_w(self, *a, **k)
        self._ws.append(float(w))
        return w
    CascadeSVM._lagrangian_fast = lagr

    variants = [("as is", {}), ("shrinking=False", dict(shrinking=False)),
                ("tol=1e-6", dict(tol=1e-6))]
    data, probes = datasets()
    out, problems = {}, []
    for name, (x, y) in data.items():
        out["data_%s__x" % name] = x
        out["data_%s__y" % name] = y.astype(np.int64)
        out["data_%s__probe" % name] = probes[name]
    for name, dname, sizes, f32, shift, kw in cases():
        x, y = data[dname]
        x = x.astype(np.float32) if f32 else x
        y = y + shift
        probe = probes[dname].astype(x.dtype)
        runs = []
        for _, extra in variants:
            base.SVC = (lambda extra: lambda **p: SVC(**dict(p, **extra)))(
                extra)
            counter[0] = 0
            ds = Dataset(n_features=x.shape[1])
            off = 0
            for s in sizes:
                ds.append(Subset(x[off:off + s], y[off:off + s]))
                off += s
            est = CascadeSVM(**kw)
            est._ws = []
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                est.fit(ds)
            clf = est._clf
            c = float(kw.get("c", 1))
            ids = np.asarray(est._feedback_ids)
            ypm = np.where(y == clf.classes_[1], 1.0, -1.0)
            runs.append(dict(
                iterations=est.iterations, converged=bool(est.converged),
                w=np.array(est._ws, dtype=np.float64),
                dec=clf.decision_function(probe),
                pred=clf.predict(probe),
                sv=set(ids[np.abs(clf.dual_coef_[0]) >= 0.01 * c].tolist()),
                margin=ypm * clf.decision_function(x),
                n_sv=len(ids)))
        base.SVC = SVC
        r0 = runs[0]
        if not all(r["iterations"] == r0["iterations"] and
                   r["converged"] == r0["converged"] for r in runs):
            problems.append(
                "%s: the three runs disagree on iterations / converged: %r"
                % (name, [(r["iterations"], r["converged"]) for r in runs]))
            continue
        spread = max(np.abs(r["dec"] - r0["dec"]).max() for r in runs)
        spread = max(spread, np.abs(runs[1]["dec"] - runs[2]["dec"]).max())
        w_gap = 0.0
        for a in range(3):
            for b in range(a + 1, 3):
                wa, wb = runs[a]["w"], runs[b]["w"]
                ok = np.isfinite(wa) & np.isfinite(wb)
                assert np.array_equal(np.isfinite(wa), np.isfinite(wb))
                if ok.any():
                    w_gap = max(w_gap, float(np.max(
                        np.abs(wa[ok] - wb[ok]) / np.abs(wa[ok]))))
        tol = float(kw.get("tol", 1e-3))
        w = r0["w"]
        margin = np.inf
        if tol > 0:
            for i in range(1, len(w)):
                if w[i - 1] and np.isfinite(w[i]) and np.isfinite(w[i - 1]):
                    margin = min(margin, abs(abs((w[i] - w[i - 1]) / w[i - 1])
                                             - tol))
        if not margin > 100 * w_gap * tol:
            problems.append(
                "%s: an iteration's |dW / W| is within %g of tol = %g, w_gap "
                "is %g" % (name, margin, tol, w_gap))
        band = np.mean(np.abs(r0["dec"]) < 10 * spread)
        if not band <= 0.10:
            problems.append(
                "%s: %.0f %% of the probe rows lie within 10 x dec_spread = "
                "%g of the boundary" % (name, 100 * band, 10 * spread))
        clear_sv = set.intersection(*[r["sv"] for r in runs])
        clear_non = np.flatnonzero(np.all(
            [r["margin"] >= 1 + 10 * spread for r in runs], axis=0))
        gamma = kw.get("gamma", "auto")
        out[name + "__data"] = np.array(dname)
        out[name + "__sizes"] = np.array(sizes, dtype=np.int64)
        out[name + "__meta"] = np.array(
            [f32, kw.get("cascade_arity", 2), kw.get("max_iter", 5), tol,
             kw.get("kernel", "rbf") == "rbf", kw.get("c", 1),
             -1.0 if gamma == "auto" else gamma,
             kw.get("check_convergence", True), shift], dtype=np.float64)
        out[name + "__iterations"] = np.array(r0["iterations"])
        out[name + "__converged"] = np.array(r0["converged"])
        out[name + "__w"] = r0["w"]
        out[name + "__dec"] = np.asarray(r0["dec"], dtype=np.float64)
        out[name + "__pred"] = np.asarray(r0["pred"], dtype=np.int64)
        out[name + "__dec_spread"] = np.array(spread)
        out[name + "__w_gap"] = np.array(w_gap)
        out[name + "__clear_sv"] = np.array(sorted(clear_sv), dtype=np.int64)
        out[name + "__clear_nonsv"] = clear_non.astype(np.int64)
        out[name + "__n_sv"] = np.array(r0["n_sv"])
        print("csvm", name, "iterations", r0["iterations"], "converged",
              r0["converged"], "n_sv", [r["n_sv"] for r in runs],
              "dec_spread %.3g" % spread, "w_gap %.3g" % w_gap,
              "margin %.3g" % margin, "band %.1f %%" % (100 * band),
              "clear sv / non-sv", len(clear_sv), len(clear_non),
              "W", [r["w"][:4] for r in runs])
    if problems:
        print("\n".join(problems))
        sys.exit("csvm_ref.npz not written")
    np.savez_compressed(os.path.join(HERE, "csvm_ref.npz"), **out)
    print("wrote csvm_ref.npz")


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
