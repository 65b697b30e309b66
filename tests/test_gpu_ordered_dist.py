"""KMeans(sums="reference") over several ranks: world 2 and world 4 (gloo,
every rank on cuda:0) over golden F13's 120 Subsets give centres
byte-identical to the single-process fit and to the reference's golden
centres, for arity 50 and 2 -- the partials of all ranks' Subsets are
all-reduced (adding +0.0 is exact) and every rank walks the same tree.

Each launch is its own subprocess under its own timeout; at most four
worker processes hold the GPU at a time."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "ordered_dist_worker.py")
ARITIES = (50, 2)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(out, world):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable]
    if world > 1:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1",
                "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                "--master-port", str(_free_port())]
    cmd += [WORKER, "--arity", ",".join(str(a) for a in ARITIES), "--out",
            out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [dict(np.load("%s.%d.npz" % (out, i))) for i in range(world)]


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    return _run(str(tmp_path_factory.mktemp("w1") / "f13"), 1)[0]


def test_single_process_equals_golden(single):
    g = load_golden("f13_arity")
    for a in ARITIES:
        assert np.array_equal(single["centers_a%d" % a], g["centers_a%d" % a])
        assert np.array_equal(single["labels_a%d" % a], g["labels_a%d" % a])
    # the tree is not a formality: the two arities give other bits
    assert not np.array_equal(g["centers_a50"], g["centers_a2"])


@pytest.mark.parametrize("world", [2, 4])
def test_world_n_bytes_equal_single_process_and_golden(world, single,
                                                       tmp_path):
    g = load_golden("f13_arity")
    res = _run(str(tmp_path / "f13"), world)
    assert sum(int(r["subsets_a50"]) for r in res) == 120
    for a in ARITIES:
        for r in res:
            cen = r["centers_a%d" % a]
            assert cen.tobytes() == single["centers_a%d" % a].tobytes()
            assert cen.tobytes() == g["centers_a%d" % a].tobytes()
        lab = np.concatenate([r["labels_a%d" % a] for r in res])
        assert np.array_equal(lab, g["labels_a%d" % a])
