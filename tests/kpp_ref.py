"""The k-means++ rule of ``dislib_amd.cluster.kmeans_plusplus`` restated in
``np.longdouble``: direct squared differences, a sequential cumsum,
``searchsorted(side='left')`` clipped to n - 1, first-minimum argmin."""
import numpy as np

LD = np.longdouble


def sqdist(x, c):
    """|x_i - c|^2 per row of x, in longdouble."""
    df = x.astype(LD) - c.astype(LD)
    return (df * df).sum(axis=1)


def sample(mind, targets):
    """min(searchsorted(cumsum(mind), targets, 'left'), n - 1), the cumsum."""
    cs = np.cumsum(mind.astype(LD))
    return np.minimum(np.searchsorted(cs, targets, side="left"),
                      len(mind) - 1), cs


def kpp_ref(x, k, random_state=None, n_local_trials=None):
    """(indices, margin): the chosen rows, and the smallest distance, relative
    to the potential, of a target from a cumsum boundary or of the best trial
    potential from the second best (exact ties aside) over all rounds."""
    n = len(x)
    rs = np.random.RandomState(random_state)
    L = n_local_trials or 2 + int(np.log(k))
    idx = [int(rs.randint(n))]
    U = rs.uniform(size=(k - 1, L))
    mind = sqdist(x, x[idx[0]])
    margin = np.inf
    for t in range(1, k):
        pot = mind.sum()
        targets = U[t - 1].astype(LD) * pot
        rows, cs = sample(mind, targets)
        cand = np.stack([np.minimum(mind, sqdist(x, x[r])) for r in rows])
        pots = np.sort(cand.sum(axis=1))
        gaps = [np.abs(cs[:, None] - targets[None, :]).min()]
        if L > 1 and pots[1] != pots[0]:
            gaps.append(pots[1] - pots[0])
        if pot > 0:
            margin = min(margin, float(min(gaps) / pot))
        best = int(np.argmin(cand.sum(axis=1)))
        mind = cand[best]
        idx.append(int(rows[best]))
    return np.array(idx, dtype=np.int64), margin
