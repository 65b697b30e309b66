"""Golden vectors for ``ALS``, produced by the REFERENCE itself:
``dislib.recommendation.ALS.fit`` (``dislib/recommendation/als/base.py``) run
the way ``gen_golden_dbscan.py`` runs its cases -- imported under the
sequential PyCOMPSs stub of ``gen_golden.py``.

Three things in the reference do not run on the installed numpy and scipy;
they are patched at run time (monkeypatches; nothing of the reference is
copied):

* ``np.NaN`` (``als/base.py:168``) is gone from numpy 2: ``np.NaN = np.nan``;
* ``_merge_split_subsets`` (``data/classes.py:423``) stacks a generator of
  single matrices, which the installed scipy refuses with ``TypeError``: it
  is replaced by the equivalent ``vstack(list(split)).transpose()``;
* ``scipy.sparse.linalg`` is imported before the fit (``base.py:240`` uses
  ``sparse.linalg`` without importing it).

Iterations are counted by wrapping ``ALS._update`` (two calls each) and the
RMSE sequence is recorded by wrapping ``ALS._has_converged``.  The reference's
own test data (``sample_movielens_ratings.csv``) is a Git-LFS pointer, so the
cases are synthetic: the docstring example, a 40-user x 60-item matrix about
25 % filled with ratings 1-5 under several settings, and a variant with an
empty user, an empty item and two stored zeros.  ``random_state=0`` is left
out: it does not seed (``base.py:151``).

Per case (``name__key``): the ratings with items as rows (``r``, dense, and
``r_stored``, the mask of stored entries), ``meta`` = [subset_size, n_f,
lambda, tol, max_iter, check_convergence, seed], ``test`` when the fit took
one, and the reference's ``users``, ``items``, ``n_iter``, ``converged``,
``rmses``; for the cases of ``TRANSPOSED`` also the Subsets of the
reference's ``dataset.transpose()`` (``t<i>``, dense).

The script refuses to write the file if, in any case, some iteration's
``|rmse - last_rmse|`` lies within 100 x the case's measured RMSE gap of
``tol`` (the gap: the largest difference, over the case's iterations, between
the reference's RMSE and that of the exact-solve restatement
``tests/als_ref.py``): ``n_iter`` and ``converged`` must not be left to
rounding.  The tolerances and seeds of the 40 x 60 cases were picked for
that -- ``cg`` leaves the RMSE some 1e-5 off, so a fit that creeps up to
``tol = 1e-4`` over tens of iterations cannot satisfy it; pick another seed
for a case that trips it.

Run in the development container only:
``python tests/golden/gen_golden_als.py``.  Writes ``als_ref.npz``.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

TRANSPOSED = ("doc", "m_f8_s4", "holes_f8_s4")


def ratings(seed, holes=False):
    """(items x users CSR, users x items CSR test matrix): 60 items, 40
    users, about 25 % filled, ratings 1-5."""
    import numpy as np
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    dense = rng.integers(1, 6, (60, 40)) * (rng.random((60, 40)) < 0.25)
    test = rng.integers(1, 6, (40, 60)) * (rng.random((40, 60)) < 0.1)
    if holes:
        dense[:, 7] = 0           # an empty user
        dense[11, :] = 0          # an empty item
    r = sp.csr_matrix(dense.astype(np.float64))
    if holes:                     # two stored zeros
        nz = np.flatnonzero(r.data)
        r.data[nz[5]] = 0.0
        r.data[nz[-9]] = 0.0
    return r, sp.csr_matrix(test.astype(np.float64))


def cases():
    import numpy as np
    import scipy.sparse as sp
    doc = sp.csr_matrix(np.array([[0, 0, 5], [3, 0, 5], [3, 1, 2]],
                                 dtype=np.float64)).transpose().tocsr()
    r, test = ratings(3)
    rh, _ = ratings(5, holes=True)
    kw = dict(lambda_=0.065, tol=1e-4, max_iter=100, check_convergence=True)
    # (name, items x users, subset_size, test, constructor arguments)
    return [
        ("doc", doc, 1, None, dict(kw, n_f=100, tol=0.01, random_state=666)),
        ("m_f8_s1", r, 60, None, dict(kw, n_f=8, tol=0.05, random_state=21)),
        ("m_f8_s4", r, 15, None, dict(kw, n_f=8, tol=0.02, random_state=4)),
        ("m_f32_s4", r, 15, None,
         dict(kw, n_f=32, tol=0.05, random_state=28)),
        ("m_f100_s1", r, 60, None,
         dict(kw, n_f=100, tol=0.05, random_state=12)),
        ("m_f8_s1_test", r, 60, test,
         dict(kw, n_f=8, tol=0.02, random_state=2)),
        ("m_f32_s4_test", r, 15, test,
         dict(kw, n_f=32, tol=0.05, random_state=18)),
        ("m_f8_s4_noconv", r, 15, None,
         dict(kw, n_f=8, random_state=12, check_convergence=False,
              max_iter=3)),
        ("m_f8_s4_long", r, 15, None,
         dict(kw, n_f=8, random_state=12, check_convergence=False,
              max_iter=30)),
        ("m_f32_s4_maxiter", r, 15, None,
         dict(kw, n_f=32, random_state=13, tol=1e-9, max_iter=4)),
        ("holes_f8_s4", rh, 15, None,
         dict(kw, n_f=8, tol=0.02, random_state=15)),
    ]


def generate():
    import warnings
    import numpy as np
    import scipy.sparse as sp
    import scipy.sparse.linalg  # noqa: F401  (base.py:240)
    np.NaN = np.nan
    import dislib.data.classes as classes
    from dislib.data import Subset, load_data
    from dislib.recommendation import ALS
    sys.path.insert(0, os.path.dirname(HERE))
    import als_ref as ref

    def merge(sparse, *split):
        stack_f = sp.vstack if sparse else np.vstack
        return Subset(samples=stack_f(list(split)).transpose())
    classes._merge_split_subsets = merge

    inner_update, inner_conv = ALS._update, ALS._has_converged

    def update(self, *a, **k):
        self._calls += 1
        return inner_update(self, *a, **k)

    def conv(self, last_rmse, rmse):
        self._rmses.append(float(rmse))
        return inner_conv(self, last_rmse, rmse)
    ALS._update, ALS._has_converged = update, conv

    out = {}
    for name, r, sub, test, kw in cases():
        ds = load_data(x=r, subset_size=sub)
        est = ALS(**kw)
        est._calls, est._rmses = 0, []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")     # the mean of an empty item
            est.fit(ds, test=test)
        stored = np.zeros(r.shape, dtype=bool)
        coo = r.tocoo()                         # keeps the stored zeros
        stored[coo.row, coo.col] = True
        out[name + "__r"] = r.toarray()
        out[name + "__r_stored"] = stored
        out[name + "__meta"] = np.array(
            [sub, kw["n_f"], kw["lambda_"], kw["tol"], kw["max_iter"],
             int(kw["check_convergence"]), kw["random_state"]],
            dtype=np.float64)
        if test is not None:
            out[name + "__test"] = test.toarray()
        assert est.users.dtype == np.float32 == est.items.dtype
        assert est._calls % 2 == 0
        out[name + "__users"] = est.users
        out[name + "__items"] = est.items
        out[name + "__n_iter"] = np.array(est._calls // 2)
        out[name + "__converged"] = np.array(bool(est.converged))
        out[name + "__rmses"] = np.array(est._rmses, dtype=np.float64)
        if name in TRANSPOSED:
            for i, s in enumerate(load_data(x=r, subset_size=sub)
                                  .transpose()):
                out["%s__t%d" % (name, i)] = s.samples.toarray()
        seq = np.concatenate([[np.inf], est._rmses])
        steps = np.abs(np.diff(seq)) if len(seq) > 1 else np.zeros(0)
        margin = np.abs(steps - kw["tol"]).min() if len(steps) else np.inf
        mine = ref.als_ref(r, len(ds), kw["n_f"], kw["lambda_"], kw["tol"],
                           kw["max_iter"], kw["check_convergence"],
                           kw["random_state"], test)
        k = min(len(mine.rmses), len(est._rmses))
        gap = np.abs(np.array(mine.rmses[:k]) -
                     np.array(est._rmses[:k])).max() if k else 0.0
        assert margin > 100 * gap, \
            "%s: an iteration's |d rmse| is within %g of tol, the RMSE " \
            "gap is %g" % (name, margin, gap)
        print("als", name, r.shape, "n_iter", est._calls // 2, "converged",
              bool(est.converged), "margin %.3g" % margin,
              "gap %.3g" % gap)
    doc = out["doc__users"][0].dot(out["doc__items"].T)
    print("doc predict_user(0) =", doc)    # the reference's test_predict
    assert 2.75 < doc[0] < 3.25 and doc[1] < 1 and doc[2] > 4.5
    np.savez_compressed(os.path.join(HERE, "als_ref.npz"), **out)
    print("wrote als_ref.npz")


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
