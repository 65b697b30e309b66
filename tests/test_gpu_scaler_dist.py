"""StandardScaler over two ranks (gloo, both on cuda:0): in the reference
mode every rank's ``mean_``, ``var_`` and its shard's scaled rows are
byte-identical to the single-process run (the partials of all ranks' Subsets
are all-reduced -- adding +0.0 is exact -- and every rank walks the same
tree); the fast mode stays within its tolerances.

The single-process run is made here; the two ranks are two child processes,
each under its own ``timeout``: three processes hold the GPU."""
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "scaler_dist_worker.py")
WORLD = 2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def single():
    from tests import scaler_dist_worker
    return scaler_dist_worker.run_all()


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("w2") / "scaler")
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


def _rows(ranks, key):
    return np.concatenate([r[key] for r in ranks])


@pytest.mark.parametrize("key", ["s02_reference_a50_", "s02_reference_a2_",
                                 "s03_reference_a50_"])
def test_reference_mode_bytes_equal_the_single_process(key, single, ranks):
    name = key[:3]
    g = load_golden(name)
    gk = key[4:].replace("reference_", "") if name == "s02" else ""
    for r in ranks:
        for stat in ("mean", "var"):
            assert r[key + stat].dtype == single[key + stat].dtype
            assert r[key + stat].tobytes() == single[key + stat].tobytes()
            assert r[key + stat].tobytes() == g[gk + stat].tobytes()
    assert all(len(r[key + "y"]) for r in ranks)      # both hold a shard
    y = _rows(ranks, key + "y")
    assert y.dtype == single[key + "y"].dtype
    assert y.tobytes() == single[key + "y"].tobytes()


def test_fast_mode_fp64_within_tolerance(ranks):
    g = load_golden("s02")
    gm, gv = g["a50_mean"], g["a50_var"]
    std = np.sqrt(gv)
    x = load_golden("f13_arity")["x"]
    z = (x - gm) / std
    for r in ranks:
        m, v = r["s02_fast_a50_mean"], r["s02_fast_a50_var"]
        assert (np.abs(m - gm) <= 1e-9 * np.maximum(np.abs(gm), std)).all()
        assert (np.abs(v - gv) <= 1e-9 * np.maximum(np.abs(gv), std)).all()
    y = _rows(ranks, "s02_fast_a50_y")
    assert (np.abs(y - z) <= 1e-9 * np.maximum(np.abs(z), 1.0)).all()


def test_fast_mode_fp32_within_tolerance(ranks):
    """The bounds of test_gpu_scaler.test_fast_mode_fp32_against_fp64_numpy."""
    from tests import scaler_ref as sr
    x = load_golden("f10_fp32")["x"]
    m64, v64 = sr.fit_fp64(x)
    sd = np.sqrt(v64)
    z = (x.astype(np.float64) - m64) / sd
    for r in ranks:
        m, v = r["s03_fast_a50_mean"], r["s03_fast_a50_var"]
        assert m.dtype == v.dtype == np.float32
        assert (np.abs(m - m64) <= 2.0 ** -22 * np.maximum(np.abs(m64),
                                                          sd)).all()
        assert (np.abs(v - v64) <= 2.0 ** -22 * v64).all()
    y = _rows(ranks, "s03_fast_a50_y")
    assert y.dtype == np.float32
    assert (np.abs(y - z) <= 2.0 ** -24 * (np.abs(m64) / sd +
                                           4 * np.abs(z))).all()
