"""CPU tests of sums="reference": the merge schedule that dkm_merge_tree
walks (``_shard.merge_schedule``), replayed in numpy, against the oracle's
``merge_tree`` (reference base.py:137-141, 184-191) bit for bit, and the
validation of the ``sums`` keyword."""
import numpy as np
import pytest

from dislib_amd import _shard
from dislib_amd.cluster import KMeans
from oracle import kmeans_oracle as orc


def replay(partials, schedule, n_ops, n_slots, n_f32):
    """dkm_merge_tree in numpy: ``partials`` (S, len) fp64 (fp32 values
    widened); the first ``n_f32`` elements fold in fp32, the rest in fp64."""
    S, ln = partials.shape
    if n_ops == 0:
        assert S == 1
        return partials[0].copy()
    scratch = np.full((max(n_slots, 1), ln), np.nan)
    acc = None
    p = 0

    def at(i):
        return partials[i] if i < S else scratch[i - S]
    for _ in range(n_ops):
        dst, cnt = int(schedule[p]), int(schedule[p + 1])
        src = [int(v) for v in schedule[p + 2:p + 2 + cnt]]
        p += 2 + cnt
        lo = at(src[0])[:n_f32].astype(np.float32)
        hi = at(src[0])[n_f32:].copy()
        for s in src[1:]:
            lo = lo + at(s)[:n_f32].astype(np.float32)
            hi = hi + at(s)[n_f32:]
        r = np.concatenate([lo.astype(np.float64), hi])
        if dst < 0:
            acc = r
        else:
            assert 0 <= dst < n_slots
            scratch[dst] = r
    assert p == len(schedule) and acc is not None
    return acc


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("arity", [2, 3, 50])
@pytest.mark.parametrize("S", [1, 2, 49, 50, 51, 120, 2501])
def test_schedule_replay_equals_oracle_merge_tree(S, arity, dtype):
    k, d = 3, 2
    rng = np.random.default_rng(S * 100 + arity)
    sums = (rng.standard_normal((S, k, d)) *
            10.0 ** rng.uniform(-8, 8, (S, k, d))).astype(dtype)
    counts = rng.integers(0, 1 << 40, (S, k)).astype(np.int64)
    want_s, want_c = orc.merge_tree(
        [(sums[i], counts[i]) for i in range(S)], arity)
    assert want_s.dtype == dtype
    if S >= 49:   # the order matters for these values
        back = orc.merge_tree([(sums[i], counts[i])
                               for i in range(S)][::-1], arity)[0]
        assert not np.array_equal(want_s, back)
    sched, n_ops, n_slots = _shard.merge_schedule(S, arity)
    assert sched.dtype == np.int32
    flat = np.concatenate([sums.reshape(S, -1).astype(np.float64),
                           counts.astype(np.float64)], axis=1)
    got = replay(flat, sched, n_ops, n_slots,
                 k * d if dtype == np.float32 else 0)
    assert np.array_equal(got[:k * d].reshape(k, d),
                          want_s.astype(np.float64))
    assert np.array_equal(got[k * d:], want_c.astype(np.float64))
    # a slot is reused once folded: the scratch stays near S / arity buffers
    assert n_slots <= (S + arity - 1) // arity + 1


def test_arity_below_two_never_terminates_in_the_reference():
    with pytest.raises(ValueError, match="arity"):
        _shard.merge_schedule(2, 1)
    with pytest.raises(ValueError, match="arity"):
        _shard.merge_schedule(3, 0)
    sched, n_ops, n_slots = _shard.merge_schedule(1, 1)   # nothing to merge
    assert (len(sched), n_ops, n_slots) == (0, 0, 0)


def test_sums_keyword_validation():
    assert KMeans()._sums == "fast"
    assert KMeans(sums="reference")._sums == "reference"
    for bad in ("exact", "Reference", None, 1):
        with pytest.raises(ValueError, match="fast.*reference"):
            KMeans(sums=bad)
    with pytest.raises(TypeError):
        KMeans(8, 10, 1e-4, 50, None, False, "auto", None, "reference")
