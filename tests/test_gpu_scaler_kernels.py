"""GPU tests of the kernels of dkm_scale.hip through the C ABI at the edges
tests/test_gpu_scaler.py leaves out, with its yardsticks (``check_chains``,
``check_stats``, ``check_scaling``: the chains and the scaling equal numpy's
bit for bit, the fast statistics within 2 (n + 3) 2^-53 sum|terms|):

rows of more than 256 column pieces (two and three column chunks, a last
chunk of one piece and of 256), more than 256 blocks and the grid cap of
2048, more columns than the final sum's grid, the vector path's gate with
X and Y qualifying separately, and Y = X.

The shapes are those of tests/kernel_edge_shapes.py;
tests/test_kernel_plans_host.py shows that each reaches its branch."""
import numpy as np
import pytest

from dislib_amd import _device
from tests import kernel_edge_shapes as es
from tests.test_gpu_scaler import (_padded, check_chains, check_scaling,
                                   check_stats, scale_pairings)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def _name(v):
    return v.__name__ if isinstance(v, type) else None


def _data(n, d, dtype, seed):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal((n, d)) * 3.0 +
            rs.uniform(-4, 4, d)).astype(dtype)


@pytest.mark.parametrize("dtype,d,pad", [c[:3] for c in es.CHUNKS],
                         ids=_name)
def test_two_and_three_column_chunks(dtype, d, pad):
    sizes = es.scale_chunk_sizes(dtype, d, pad)
    x = _data(sum(sizes), d, dtype, d + pad)
    X = _padded(x, d + pad)
    assert X.data_ptr() % 16 == 0
    check_chains(x, X, sizes)
    check_stats(x, X)
    check_scaling(x, X)


@pytest.mark.parametrize("dtype,d,n", [b[:3] for b in es.BLOCKS], ids=_name)
def test_257_and_600_blocks(dtype, d, n):
    assert _device.scale_grid(n, d) in (257, 600)
    x = _data(n, d, dtype, n)
    for pad in (0, 1):                      # the vector and the scalar path
        X = _padded(x, d + pad)
        check_stats(x, X)
        check_scaling(x, X)


@pytest.mark.parametrize("dtype,d,n", es.CAPPED, ids=_name)
def test_the_grid_cap(dtype, d, n):
    assert _device.scale_grid(n, d) == _device.SCALE_GRID_CAP
    x = _data(n, d, dtype, n)
    X = _padded(x, d)
    check_stats(x, X)
    check_scaling(x, X, pairings=scale_pairings(dtype)[:1])


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("d,n", es.WIDE)
def test_more_columns_than_the_final_sums_grid(d, n, dtype):
    x = _data(n, d, dtype, d)
    for pad in (0, 1):
        X = _padded(x, d + pad)
        check_chains(x, X, [n // 2, n - n // 2])
        check_stats(x, X)
        check_scaling(x, X)


# (X's padding, X's offset, Y's padding, Y's offset): each alone takes the
# vector path from the call
GATE = {"y_stride": (0, 0, 1, 0), "x_stride": (1, 0, 0, 0),
        "x_base": (0, 1, 0, 0), "y_base": (0, 0, 0, 1)}


@pytest.mark.parametrize("case", sorted(GATE))
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_the_vector_gate_needs_both_x_and_y(dtype, case):
    d, n = 32, 700
    xpad, xoff, ypad, yoff = GATE[case]
    x = _data(n, d, dtype, 32)
    X = _padded(x, d + xpad, xoff)
    assert X.data_ptr() % 16 == xoff * x.itemsize
    check_scaling(x, X, ypad=ypad, yoff=yoff)
    check_stats(x, X)


def test_the_vector_gate_mixed_pairing_odd_ldy():
    """fp32 samples with fp64 statistics: X takes 16-B pieces, Y is 16-B
    aligned, but its odd stride puts every other row 8 B off."""
    d, n = 32, 700
    x = _data(n, d, np.float32, 33)
    check_scaling(x, _padded(x, d), ypad=1,
                  pairings=scale_pairings(np.float32)[1:])
    check_scaling(x, _padded(x, d), ypad=2,
                  pairings=scale_pairings(np.float32)[1:])


@pytest.mark.parametrize("d,pad", [(32, 0), (32, 1), (1028, 0), (257, 1)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_in_place_gives_the_same_bytes(dtype, d, pad):
    n = 3 * _device.SCALE_GRID_UNIT // d + 5
    x = _data(n, d, dtype, d + pad)
    check_scaling(x, _padded(x, d + pad), in_place=True,
                  pairings=scale_pairings(dtype)[:1])
