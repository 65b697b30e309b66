"""CPU tests of tests/csr_ref.py: every generator of the CSR kernel tests is
held to the condition test_gpu_csr_kernels.py relies on, against the
oracle's sklearn-order arithmetic."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import kmeans_oracle as orc
from tests import csr_ref as ref

# (k, d): distinct column pairs (d = 40 has no room for disjoint supports
# beyond k = 3), disjoint supports, a sliced shape
SHAPES = [(2, 40), (9, 40), (257, 40), (65, 2000), (65, 65537)]


@pytest.mark.parametrize("k,d", [(1, 40)] + SHAPES)
def test_own_rows_are_surely_decided_and_every_centre_wins(k, d):
    n = 2 * k + 3
    ptr, ind, dat, C = ref.own_rows(k, d, n, k)
    assert len(ptr) == n + 1 and dat.min() < 0 < dat.max()
    assert np.array_equal(ref.bf16_round(dat), dat)
    assert np.array_equal(ref.bf16_round(C.data), C.data)
    labels, _, counts = ref.expected(ptr, ind, dat, d, C)
    assert np.array_equal(labels, np.arange(n) % k)
    assert (counts > 0).all()
    decided, undecided = ref.classify(ptr, ind, dat, d, C)
    assert decided.all() and not undecided.any()
    if k * ref.N_SUP <= d:                 # pairwise disjoint supports
        G = sp.lil_matrix(abs(C) @ abs(C).T)
        G.setdiag(0)
        assert sp.csr_matrix(G).count_nonzero() == 0


@pytest.mark.parametrize("k,d", SHAPES)
def test_twin_rows_tie_exactly_and_take_the_lower_index(k, d):
    n = 150
    h = (k + 1) // 2
    ptr, ind, dat, C = ref.twin_rows(k, d, n, k)
    Cd = C.toarray() if d <= 2000 else None
    if Cd is not None:
        assert np.array_equal(Cd[h:], Cd[:k - h])
    dist = ref.distances(ptr, ind, dat, d, C)
    labels, _, _ = ref.expected(ptr, ind, dat, d, C, dist)
    assert (labels < h).all()
    assert np.array_equal(labels, np.arange(n) % (k - h))
    rows = np.arange(n)
    assert np.array_equal(dist[rows, labels], dist[rows, labels + h])
    assert (dist[rows, labels] == dist.min(axis=1)).all()
    decided, undecided = ref.classify(ptr, ind, dat, d, C)
    assert undecided.all()


@pytest.mark.parametrize("k,d,offset", [(64, 2000, 32), (65, 65537, 64),
                                        (129, 65537, 64)])
@pytest.mark.parametrize("descending", [False, True])
def test_near_twin_rows_label_both_members(k, d, offset, descending):
    n = 300
    ptr, ind, dat, C = ref.near_twin_rows(k, d, n, 0, offset,
                                          descending=descending)
    pairs = ref.near_twin_pairs(k, offset)
    assert all(hi - lo == offset for lo, hi in pairs)
    labels, _, _ = ref.expected(ptr, ind, dat, d, C)
    lo = np.array([pairs[i % len(pairs)][0] for i in range(n)])
    assert ((labels == lo) | (labels == lo + offset)).all()
    high = labels == lo + offset
    assert n // 4 <= high.sum() <= n - n // 8, high.sum()
    # the bf16 table orders some pairs the other way round, both ways: rows
    # a merge that kept only one slice's scores would label wrongly
    s = ref.table_scores(ptr, ind, dat, d, C)
    rows = np.arange(n)
    gap = s[rows, lo] - s[rows, lo + offset]       # > 0: the table says high
    tol = 1e-5 * np.abs(s[rows, lo])
    assert ((gap > tol) & ~high).sum() >= 5
    assert ((gap < -tol) & high).sum() >= 5
    if descending:
        assert all((np.diff(ind[a:b]) < 0).all()
                   for a, b in zip(ptr[:-1], ptr[1:]))


def test_length_rows_have_the_given_lengths_and_stored_zeros():
    lengths = list(range(27)) + [32, 33, 40, 64, 65]
    ptr, ind, dat = ref.length_rows(lengths, 70, 0, zeros=True)
    assert np.array_equal(np.diff(ptr), lengths)
    assert (dat == 0).any() and dat.min() < 0 < dat.max()
    for a, b in zip(ptr[:-1], ptr[1:]):
        assert len(set(ind[a:b])) == b - a and ind[a:b].max(initial=0) < 70
    for k in (1, 2, 3, 5, 130):
        C = ref.dense_int_centres(k, 70, k)
        labels, _, _ = ref.expected(ptr, ind, dat, 70, C)
        assert labels[0] == 0               # the empty row: first of the tie
        _, undecided = ref.classify(ptr, ind, dat, 70, C)
        assert undecided[0] == (k > 1)


def test_expected_agrees_with_the_oracle_partial_sum():
    rng = np.random.default_rng(0)
    n, d, k = 200, 50, 9
    lengths = rng.integers(0, 20, n)
    ptr, ind, dat = ref.length_rows(lengths, d, 1, zeros=True)
    C = ref.dense_int_centres(k, d, 2)
    xs = ref.as_csr(ptr, ind, dat, d)
    assert xs.nnz == len(dat)               # stored zeros kept
    rl, rs, rc = orc.partial_sum(xs, C, sparse=True)
    labels, sums, counts = ref.expected(ptr, ind, dat, d, C)
    assert np.array_equal(labels, rl)
    assert np.array_equal(counts, rc)
    assert np.array_equal(sums.toarray(), rs)
    prev = labels.copy()
    prev[::4] = (prev[::4] + 1) % k
    prev[1::4] = -1
    prev[2::4] = k + 5
    ds, dc = ref.expected_delta(ptr, ind, dat, d, k, labels, prev)
    want = np.zeros((k, d + 1))
    xd = xs.toarray()
    for i in np.nonzero(prev != labels)[0]:
        want[labels[i], :d] += xd[i]
        want[labels[i], d] += 1
        if 0 <= prev[i] < k:
            want[prev[i], :d] -= xd[i]
            want[prev[i], d] -= 1
    assert np.array_equal(ds.toarray(), want[:, :d])
    assert np.array_equal(dc, want[:, d])


def test_bound_restatement_against_hand_values():
    # an empty row: A = 0, B = 2 (2 u c2 + 8 w c2) + 2^-100
    c2 = 9.0
    want = 2 * (2.0 ** -24 * 2 * c2 + 4 * 2.0 ** -53 * 2 * c2) + 2.0 ** -100
    assert ref.screen_bound(0.0, 0, 3.0) == want
    # dominated by the bf16 table term 2^-6 A
    b = ref.screen_bound(16.0, 10, 5.0)
    assert 2.0 ** -6 * 20 < b < 2.0 ** -6 * 20 * 1.001
