"""GPU parity of the dense assignment kernels on fp32 samples, and on strided
or misaligned rows of both sample types.

Every dense kernel is a template over the sample type: the fp32 and fp64
forms differ in their row loads (float4 x 2 against double2 x 4), in the
stride that makes a row a 16-B vector row (ldx % 4 against ldx % 2) and in
their ABI symbols.  The tests run both forms on data on which every partial
sum is exact (tests/dense_f32_ref.py), so labels, counts and sums are
compared with ``array_equal``: against the oracle and between the two types.

The C ABI tests put the matrix into a padded buffer with a row stride
ldx > d or a base that is not 16-B aligned: a kernel that addresses rows with
d instead of ldx or reads a padding column shows up as a wrong label, a
wrong or NaN sum, or rows sent to the exact re-check that the screen should
have decided.

Not covered: WHICH path plan_screen takes for a stride.  A gate that used
the fp64 divisor for fp32 rows (ldx = 34 taken as a vector row) issues 16-B
loads at 8-B aligned addresses, which gfx950 serves correctly, so no value
changes; the ldx = 34 case checks that the path taken is correct, not that
it is the scalar one.  Asserting the gate needs the plan exposed (a counter
such as dkm_screen_counters').
"""
import functools

import numpy as np
import pytest

from oracle import kmeans_oracle as orc
from tests import dense_f32_ref as ref
from tests.test_gpu_nonfinite import MODES as NF_MODES
from tests.test_gpu_nonfinite import SHAPES as NF_SHAPES
from tests.test_gpu_nonfinite import _blobs, _same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SCREENS = ["screen32", "bf16x3", "bf16"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------------------
# fp32 == fp64 == oracle, bit for bit, through _device
# ---------------------------------------------------------------------------
# (n, d, k), the smallest shapes that reach each kernel family; the kernel
# named is what launch_screen's plan (plan_screen, dkm_dense.hip) and assign
# select for contiguous rows.  "exact" mode runs k_exact_reg for d <= 64 with
# the centres in LDS (k d 8 B <= 80 KB) and k_exact_gen otherwise; k = 1 is
# not screen_ok, so every mode runs the exact kernel there.
GRID_SHAPES = [
    # exact register tiles (MAXD 8, 8, 8) and the generic kernel (d > 64)
    (70, 3, 1), (4097, 1, 2), (4000, 7, 5), (600, 300, 5),
    # resident k_screen, 32 < d <= 128: non-VEC NKS 2, VEC NKS 2, non-VEC
    # NKS 4; (5000, 13, 17): d <= 32 with d % 8 != 0, non-VEC NKS 1
    (3000, 50, 10), (5000, 13, 17), (3000, 64, 40), (2000, 100, 12),
    # d <= 32, d % 8 == 0: k_screen_w32 in bf16x3 / auto (the full-sums
    # call builds the split image, the delta call streams it through the
    # hinted threshold pass and sums its moved-row list), k_screen_b2 over
    # the single image in bf16, resident VEC k_screen NKS 1 in screen32;
    # d = 24: no power of two
    (5000, 32, 100), (4000, 8, 9), (3000, 16, 250), (3000, 24, 30),
    # d <= 32, d % 8 != 0: never w32 or single product, non-VEC k_screen
    (3000, 17, 37), (3000, 30, 100),
    # sums (and mostly fragments) beyond LDS: the screens write labels, the
    # sums come from them (k_label_sums / sorted sums).  (3000, 64, 1000):
    # CHUNK k_screen in screen32, k_screen_c32 + the re-screen (CHUNK
    # k_screen with the two-candidate list + k_cand2) in bf16x3, k_screen_b2
    # + k_cand2 + k_candn + the re-screen in bf16 / auto; (2000, 128, 700)
    # and (6000, 16, 5000): VEC CHUNK k_screen NKS 4 / NKS 1 in every screen
    # mode (the bf16 centres exceed the single product's LDS); (3000, 33,
    # 1500): non-VEC CHUNK NKS 2; (2000, 32, 600): resident fragments,
    # k_screen_w32 over the image in bf16x3, k_screen_b2 in bf16 / auto;
    # (4200, 16, 4000): k_screen_b1 in bf16 / auto (the centres fit its LDS,
    # not k_screen_b2's)
    (3000, 64, 1000), (2000, 128, 700), (3000, 33, 1500), (6000, 16, 5000),
    (2000, 32, 600), (4200, 16, 4000),
    # d > 128: the GEMM screen (k_gemm_split VEC only for d % 8 == 0),
    # one partial sample tile, k < 4, one stage of padding
    (1500, 257, 600), (70, 160, 9), (800, 300, 3), (1000, 129, 8),
]


@pytest.mark.parametrize("mode", ref.MODE_NAMES)
@pytest.mark.parametrize("n,d,k", GRID_SHAPES)
def test_grid_f32_f64_oracle_bit_equal(n, d, k, mode):
    """partial_sum (building the sample image where the screen takes one),
    assign_delta (streaming it), partial_sum over a poisoned label buffer and
    predict, with the samples as fp32 and as fp64: labels, counts and sums
    equal the oracle's and each other, bit for bit."""
    g = ref.grid_case(n, d, k)
    got = {}
    for dt in (np.float32, np.float64):
        run = ref.DeviceRun(g.samples(dt), g.C)
        # the label buffer holds the previous labels: the single-product
        # screens read it as their threshold pass's hint
        got[dt, "partial"] = run.call("partial", mode, g.prev)
        got[dt, "delta"] = run.call("delta", mode, g.prev)
        got[dt, "poisoned"] = run.call("partial", mode)
        got[dt, "predict"] = run.call("predict", mode)
    for (dt, kind), (lab, sums, cnt, _) in got.items():
        what = (np.dtype(dt).name, kind)
        assert np.array_equal(lab, g.labels), what
        if kind == "predict":
            continue
        want_s, want_c = (g.delta[:, :d], g.delta[:, d]) if kind == "delta" \
            else (g.sums, g.counts)
        assert np.array_equal(cnt, want_c), what
        assert np.array_equal(sums, want_s), what
    for kind in ("partial", "delta", "poisoned", "predict"):
        a, b = got[np.float32, kind], got[np.float64, kind]
        for u, v in zip(a[:3], b[:3]):
            assert np.array_equal(u, v), kind


# ---------------------------------------------------------------------------
# strided rows and misaligned bases through the C ABI
# ---------------------------------------------------------------------------
# (dtype, d, ldx, off, k); n = 3000.  plan_screen's vector rows need
# d % 8 == 0, ldx % (16 / sizeof) == 0 and a 16-B aligned base.
STRIDED = [
    (np.float32, 32, 32, 1, 100),     # base misaligned by 4 B: not vector
    (np.float32, 32, 34, 0, 100),     # ldx % 4 != 0: not vector for fp32
                                      # (values only: see the docstring)
    (np.float32, 32, 36, 0, 100),     # strided, vector
    (np.float32, 24, 28, 0, 100),     # strided, vector, d no power of two
    (np.float32, 7, 9, 0, 100),       # d % 8 != 0
    (np.float32, 64, 65, 0, 1000),    # CHUNK / single product, not vector
    (np.float32, 64, 68, 0, 1000),    # CHUNK / c32 / b2, strided vector
    (np.float32, 160, 161, 0, 40),    # GEMM split, not vector
    (np.float32, 160, 164, 0, 40),    # GEMM split, strided vector
    (np.float64, 32, 33, 0, 100),     # ldx % 2 != 0: not vector
    (np.float64, 32, 34, 0, 100),     # strided, vector
    (np.float64, 32, 32, 1, 100),     # base misaligned by 8 B
    (np.float64, 64, 66, 0, 1000),    # CHUNK / c32 / b2, strided vector
    (np.float64, 160, 161, 0, 40),    # GEMM split, not vector
]


@pytest.mark.parametrize("pad", [np.nan, 2.0 ** 15], ids=["nan", "big"])
@pytest.mark.parametrize("mode", ["exact", "bf16x3", "bf16"])
@pytest.mark.parametrize("dt,d,ldx,off,k", STRIDED, ids=[
    "%s-d%d-ldx%d-off%d-k%d" % (np.dtype(s[0]).name, s[1], s[2], s[3], s[4])
    for s in STRIDED])
def test_strided_rows_through_the_abi(dt, d, ldx, off, k, mode, pad):
    """The padding holds NaN, or a large finite value (2^15, exact in both
    types: read into a sum or a product it gives a wrong value where a NaN
    would only send the row to the exact path)."""
    n = 3000
    g = ref.grid_case(n, d, k)
    run = ref.StridedRun(g.samples(dt), ldx, off, g.C, pad)
    # A padding value read into a row's norm does not change the label: a
    # NaN sends the row to the exact re-check, a finite one widens the
    # screen's bound.  So the re-checked rows are bounded too, where the
    # screen is bf16x3 arithmetic: bf16x3 mode, and bf16 mode on rows that
    # are not 16-B vector rows (plan_screen then runs the bf16x3 screen;
    # d > 128 keeps the single product).  The rows a centre was drawn from
    # lie 0.1 sqrt(d) from it and the data's spread from every other one, a
    # gap far beyond the bf16x3 bound: the screen decides them itself.
    vector = d % 8 == 0 and off == 0 and \
        ldx % (16 // np.dtype(dt).itemsize) == 0
    bounded = mode == "bf16x3" or (mode == "bf16" and d <= 128 and
                                   not vector)
    lab, sums, cnt, nre = run.call("partial", mode)
    assert np.array_equal(lab, g.labels)
    assert np.array_equal(cnt, g.counts)
    assert np.array_equal(sums, g.sums)
    assert not bounded or nre <= n - k // 2
    lab, sums, cnt, nre = run.call("delta", mode, g.prev)
    assert np.array_equal(lab, g.labels)
    assert np.array_equal(cnt, g.delta[:, d])
    assert np.array_equal(sums, g.delta[:, :d])
    assert not bounded or nre <= n - k // 2
    lab, _, _, nre = run.call("predict", mode)
    assert np.array_equal(lab, g.labels)
    assert not bounded or nre <= n - k // 2
    assert run.untouched()


# ---------------------------------------------------------------------------
# fp32 magnitudes and ties (labels; the oracle on the fp32 array)
# ---------------------------------------------------------------------------
MAG_SHAPES = [(32, 100), (64, 1000), (160, 20)]
MAG_N = 2000


def _labels_all_modes(x, C, modes=ref.MODE_NAMES):
    """{mode: (partial labels, predict labels, rechecked)} of fp32 x."""
    assert x.dtype == np.float32
    run = ref.DeviceRun(x, C)
    out = {}
    for mode in modes:
        lab, _, cnt, nre = run.call("partial", mode)
        assert cnt.sum() == x.shape[0], mode
        plab, _, _, _ = run.call("predict", mode)
        out[mode] = (lab, plab, nre)
    return out


def _check_labels(x, C, modes=ref.MODE_NAMES):
    rl = orc.predict_labels(x, C)
    for mode, (lab, plab, _) in _labels_all_modes(x, C, modes).items():
        assert np.array_equal(lab, rl), mode
        assert np.array_equal(plab, rl), mode
    return rl


def _log_uniform(rng, lo, hi, shape):
    mag = 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), shape)
    return mag * rng.choice([-1.0, 1.0], shape)


@pytest.mark.parametrize("d,k", MAG_SHAPES)
def test_f32_rows_whose_fp32_squares_overflow(d, k):
    """|x| in [1e19, 3e38]: x^2 overflows fp32 (the screens' |x|^2 and
    products are +inf or NaN) while every fp64 distance is finite."""
    rng = np.random.default_rng(500 + d)
    x = _log_uniform(rng, 1e19, 3e38, (MAG_N, d)).astype(np.float32)
    assert np.isfinite(x).all()
    pick = rng.choice(MAG_N, k, replace=False)
    C = x[pick].astype(np.float64) * (1 + 0.01 * rng.standard_normal((k, d)))
    assert np.isfinite(orc.dense_distances(x[:50], C)).all()
    rl = _check_labels(x, C)
    assert len(np.unique(rl)) > k // 2


@pytest.mark.parametrize("d,k", MAG_SHAPES)
def test_f32_subnormal_rows(d, k):
    """fp32 subnormal and near-subnormal rows (1e-45 .. 1e-37), centres at
    the same scale: an fp32 |x|^2 or product is 0."""
    rng = np.random.default_rng(600 + d)
    x = _log_uniform(rng, 1e-45, 1e-37, (MAG_N, d)).astype(np.float32)
    assert (np.abs(x[x != 0]) < np.finfo(np.float32).tiny).any()
    pick = rng.choice(MAG_N, k, replace=False)
    C = x[pick].astype(np.float64) * (1 + 0.01 * rng.standard_normal((k, d)))
    rl = _check_labels(x, C)
    assert len(np.unique(rl)) > k // 2


def test_f32_mixed_magnitudes_in_every_tile():
    """Rows of scale 1e-30, 1 and 1e30 interleaved, so that every 32-row
    tile of every screen holds all three."""
    rng = np.random.default_rng(700)
    n, d, k = 3000, 32, 99
    scale = np.array([1e-30, 1.0, 1e30])[np.arange(n) % 3]
    x = (rng.standard_normal((n, d)) * scale[:, None]).astype(np.float32)
    pick = np.arange(k) * 30 + np.arange(k) % 3   # k / 3 of each scale
    assert len(np.unique(pick % 3)) == 3
    C = x[pick].astype(np.float64) * (1 + 0.01 * rng.standard_normal((k, d)))
    rl = _check_labels(x, C)
    for s in range(3):                         # each scale keeps its centres
        assert len(np.unique(rl[s::3])) > k // 6


def _mirror(rng, n=5000, d=16):
    """Centres 0 and 1 mirror images in coordinate 0 (fp32 values): a sample
    with x_0 = 0 is exactly equidistant from both."""
    C = rng.standard_normal((4, d)).astype(np.float32).astype(np.float64)
    C[1] = C[0].copy()
    C[1][0] = -C[0][0]
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[:, 0] = 0.0
    return x, C


def test_f32_exact_ties_take_the_first_index():
    x, C = _mirror(np.random.default_rng(3))
    rl = orc.predict_labels(x, C)
    assert (rl == 0).any() and not (rl == 1).any()
    res = _labels_all_modes(x, C)
    for mode, (lab, plab, nre) in res.items():
        assert np.array_equal(lab, rl), mode
        assert np.array_equal(plab, rl), mode
        if mode in SCREENS:
            assert nre > 0, mode


@pytest.mark.parametrize("step", ["subnormal", "ulp"])
def test_f32_one_ulp_near_ties(step):
    """The mirror construction with x_0 = +-m 2^-149 (the smallest fp32
    steps off the plane: below fp64's resolution of the distances, a tie
    for the oracle too) and x_0 = +- one fp32 ulp of 1 (2^-23: a distance
    gap of about 1e-7 relative, decided in fp64, far below the bf16 and
    fp32 screens' bounds)."""
    rng = np.random.default_rng(11)
    x, C = _mirror(rng)
    n = x.shape[0]
    sign = rng.choice([-1.0, 1.0], n)
    if step == "subnormal":
        x0 = sign * rng.integers(1, 4, n) * 2.0 ** -149
    else:
        x0 = sign * 2.0 ** -23
    x[:, 0] = x0.astype(np.float32)
    assert np.array_equal(x[:, 0].astype(np.float64), x0)
    rl = _check_labels(x, C)
    if step == "ulp":
        assert (rl == 0).any() and (rl == 1).any()


def _poison_rows_f32(rng, x, m):
    """m rows each of: a NaN, a +inf, a -inf, +inf and -inf together, and a
    row of 3e38 (finite fp64 distances; fp32 squares overflow)."""
    n, d = x.shape
    bad = rng.choice(n, 5 * m, replace=False)
    cols = rng.integers(0, d, 5 * m)
    x[bad[:m], cols[:m]] = np.nan
    x[bad[m:2 * m], cols[m:2 * m]] = np.inf
    x[bad[2 * m:3 * m], cols[2 * m:3 * m]] = -np.inf
    x[bad[3 * m:4 * m], 0] = np.inf
    x[bad[3 * m:4 * m], d - 1] = -np.inf
    x[bad[4 * m:]] = 3e38
    return bad


@functools.lru_cache(maxsize=None)
def _nonfinite_case(n, d, k):
    rng, x, C = _blobs(n, d, k, n + d + k)
    x = x.astype(np.float32)
    _poison_rows_f32(rng, x, 12)
    with np.errstate(invalid="ignore"):
        rl, rs, rc = orc.partial_sum(x.astype(np.float64), C)
        assert np.array_equal(rl, orc.predict_labels(x, C))
    return x, C, rl, rs, rc


@pytest.mark.parametrize("mode", NF_MODES)
@pytest.mark.parametrize("n,d,k", NF_SHAPES)
def test_f32_nonfinite_samples(mode, n, d, k):
    """test_gpu_nonfinite.test_nonfinite_samples on fp32 samples: np.argmin's
    rules on NaN / inf rows, sums with NaN / inf where the oracle's have
    them."""
    x, C, rl, rs, rc = _nonfinite_case(n, d, k)
    run = ref.DeviceRun(x, C)
    lab, sums, cnt, _ = run.call("partial", mode)
    assert np.array_equal(lab, rl)
    assert np.array_equal(cnt, rc.astype(np.float64))
    _same(sums, rs, 1e-12)
    plab, _, _, _ = run.call("predict", mode)
    assert np.array_equal(plab, rl)
    prev = rl.copy()
    prev[::5] = (prev[::5] + 1) % k
    dl, _, _, _ = run.call("delta", mode, prev)
    assert np.array_equal(dl, rl)
