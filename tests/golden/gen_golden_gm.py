"""Generate the GaussianMixture goldens gm_a .. gm_g by running the REFERENCE
``dislib.cluster.GaussianMixture`` (dislib v0.2.0).

Run in the development container only:
``python tests/golden/gen_golden_gm.py``

Like ``gen_golden.py`` it runs the reference in PyCOMPSs sequential
semantics through that file's stub package (``SHIM``, which also restores
``logsumexp``); ``np.infty`` (removed in numpy 2) is aliased in this process
before the import.  No reference source is copied: this script imports it
and records its outputs as ``.npz`` data.  The inputs are built by
``tests/gm_ref.py`` (``inputs``), which the tests share; their sha256 is
stored.

Recorded per case: the four parameter arrays, ``n_iter``, ``converged_``,
``lower_bound_``, the labels of ``fit_predict`` and of a ``predict`` on
held-out rows, the per-iteration ``diff`` trace (from ``verbose=True``), the
largest covariance condition number, the responsibilities' top-two gap per
row (fitted and held-out rows) and, for a k-means initialisation, the
k-means centres.  The conditions every golden input meets are asserted
here and re-checked by tests/test_gm_host.py.
"""
import contextlib
import io
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from gen_golden import REF, SHIM, sha  # noqa: E402


def generate():
    import warnings

    import numpy as np
    if not hasattr(np, "infty"):
        np.infty = np.inf
    from dislib.cluster import GaussianMixture
    from dislib.data import Dataset, Subset

    from tests import gm_ref as gr

    def dataset(x, sizes):
        ds = Dataset(n_features=x.shape[1])
        for block in gr.split(x, sizes):
            ds.append(Subset(block))
        return ds

    def resp_of(gm, ds):
        _, resp = gm._e_step(ds)
        return np.concatenate([r.samples for r in resp])

    for name in gr.CASES:
        inp = gr.inputs(name)
        x, sizes, kw = inp["x"], inp["sizes"], inp["kw"]
        ds = dataset(x, sizes)
        gm = GaussianMixture(verbose=True, **kw)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gm.fit_predict(ds)
        text = buf.getvalue().split("GaussianMixture EM algorithm start")[1]
        trace = np.array([float(v) for v in re.findall(
            r"Convergence crit\. = (\S+)", text)])
        tol = gm.tol
        gap = gr.top_two_gap(resp_of(gm, ds))
        test = dataset(inp["x_test"], inp["test_sizes"])
        gm.predict(test)
        gap_test = gr.top_two_gap(resp_of(gm, test))
        cond = gr.max_cond(gm.covariances_)
        out = dict(
            x_sha=np.array(sha(x)), x_test_sha=np.array(sha(inp["x_test"])),
            sizes=np.array(sizes), weights=np.asarray(gm.weights_),
            means=np.asarray(gm.means_), covariances=gm.covariances_,
            precisions_cholesky=gm.precisions_cholesky_,
            n_iter=np.array(gm.n_iter), converged=np.array(gm.converged_),
            lower_bound=np.array(gm.lower_bound_),
            labels=ds.labels.astype(np.int64),
            predict_labels=test.labels.astype(np.int64), trace=trace,
            cond=np.array(cond), gap=gap, gap_test=gap_test)
        if kw.get("init_params", "kmeans") == "kmeans":
            out["kmeans_centers"] = gm.kmeans.centers
        # the conditions on a golden input
        assert len(trace) == (gm.n_iter if gm.converged_ else gm.max_iter)
        assert np.abs(trace - tol).min() >= 1e-6, (name, trace)
        for g in (gap, gap_test):
            assert (g < gr.GAP).mean() <= 0.005, (name, (g < gr.GAP).mean())
        if name not in gr.NO_CHOL:
            assert cond <= 1e3, (name, cond)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
        print("wrote %s: n_iter %d converged %s cond %.3g min|diff-tol| %.3g "
              "near-ties %d" % (name, gm.n_iter, gm.converged_, cond,
                                np.abs(trace - tol).min(),
                                int((gap < gr.GAP).sum())))


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
