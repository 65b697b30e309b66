"""GaussianMixture over two ranks (gloo, both on cuda:0): both ranks end
with byte-identical parameters, within the whole-class tolerances of the
goldens, and their concatenated labels are the single-process labels outside
the near-tie rows.

The single-process run is made here; the two ranks are two child processes,
each under its own ``timeout``: three processes hold the GPU."""
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import gm_ref as gr
from tests.conftest import load_golden
from tests.gm_dist_worker import ATTRS, RUNS
from tests.test_gm_host import PARAMS, close, keep

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "gm_dist_worker.py")
WORLD = 2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    from dislib_amd import _lib
    assert _lib.lib().dkm_build_flags() == 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def single():
    from tests import gm_dist_worker
    return gm_dist_worker.run_all()


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("w2") / "gm")
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(_free_port()), WORLD_SIZE=str(WORLD))
    limit = [shutil.which("timeout"), "-k", "10", "150"]
    assert limit[0], "coreutils timeout not found"
    procs = [subprocess.Popen(
        limit + [sys.executable, WORKER, "--out", out],
        env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE,
        stderr=subprocess.STDOUT, text=True) for r in range(WORLD)]
    logs = [p.communicate()[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    return [dict(np.load("%s.%d.npz" % (out, r))) for r in range(WORLD)]


@pytest.mark.parametrize("name", RUNS)
def test_two_ranks_agree_and_match_the_golden(name, single, ranks):
    g = load_golden(name)
    a, b = ranks
    for key in a:
        if key.startswith(name) and not key.endswith("_labels"):
            assert a[key].tobytes() == b[key].tobytes(), key
    for r in ranks:
        assert r[name + "_n_iter"] == g["n_iter"]
        assert r[name + "_converged"] == g["converged"]
        for p, attr in zip(PARAMS, ATTRS):
            tol = 1e-9 * (float(g["cond"]) if p == "precisions_cholesky"
                          else 1.0)
            assert close(r[name + "_" + attr], g[p], tol), p
        assert abs(r[name + "_lower_bound"] - g["lower_bound"]) <= \
            1e-9 * abs(g["lower_bound"])
    assert all(len(r[name + "_labels"]) for r in ranks)   # both hold a shard
    labels = np.concatenate([r[name + "_labels"] for r in ranks])
    assert labels.dtype == np.int64
    k = keep(g)
    assert np.array_equal(labels[k], single[name + "_labels"][k])
    assert np.array_equal(labels[k], g["labels"][k])
