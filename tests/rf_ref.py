"""A plain numpy restatement of ``dislib_amd.classification.rf``: the split
rule of the reference's ``test_split``, the counter-based feature draws, the
level loop and the prediction.  Written for clarity, one node at a time."""
from collections import Counter

import numpy as np

M1, M2, M3 = (np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9),
              np.uint64(0x94D049BB133111EB))


def split(values, y, n_classes):
    """(score, position, lower value, upper value) of a node whose members
    (bootstrap repeats listed) have feature ``values`` and classes ``y``.
    Position ``len(y) - 1``: no valid cut."""
    size = len(y)
    o = np.argsort(values, kind="stable")
    v, ys = np.asarray(values)[o], np.asarray(y)[o]
    left = np.zeros(n_classes, dtype=np.int64)
    right = np.bincount(ys, minlength=n_classes).astype(np.int64)
    best, pos = np.inf, -1
    for i in range(size):
        left[ys[i]] += 1
        right[ys[i]] -= 1
        if i + 1 < size and v[i + 1] == v[i]:
            continue
        ll, rl = np.float64(i + 1), np.float64(max(size - i - 1, 1))
        s = -(np.float64(np.sum(left * left)) / ll +
              np.float64(np.sum(right * right)) / rl)
        if s <= best:
            best, pos = s, i
    return best, pos, v[pos], v[min(pos + 1, size - 1)]


def threshold(lo, hi):
    mid = (np.float64(lo) + np.float64(hi)) / 2
    return np.float64(lo) if mid >= hi else mid


def feature_order(seed, node, d):
    with np.errstate(over="ignore"):
        z = np.uint64(seed) * M1 + np.uint64(node) * M2 + \
            np.arange(d, dtype=np.uint64) * M3
        z = (z ^ (z >> np.uint64(30))) * M2
        z = (z ^ (z >> np.uint64(27))) * M3
        z = z ^ (z >> np.uint64(31))
    return np.argsort(z, kind="stable")


def grow_tree(x, y, n_classes, sample, seed, try_features, max_depth):
    """One tree as the arrays of ``RandomForestClassifier.trees``: per node
    in creation order ``feature`` (-1: a leaf), ``value``, ``child`` and
    ``leaf`` (its row of ``frequencies``, or -1)."""
    x = np.asarray(x, dtype=np.float64)
    d = x.shape[1]
    nodes = [{}]
    level = [dict(v=0, mem=np.sort(sample), id=0, depth=0, attempt=0)]
    next_id = 1

    def is_leaf(e):
        c = np.bincount(y[e["mem"]], minlength=n_classes)
        if c.max() == len(e["mem"]) or e["depth"] >= max_depth:
            nodes[e["v"]]["freq"] = c
            return True
        return False

    level = [e for e in level if not is_leaf(e)]
    while level:
        nxt_again, nxt_kids = [], []
        for i, e in enumerate(level):
            feats = feature_order(seed, e["id"], d)[
                e["attempt"] * try_features:(e["attempt"] + 1) * try_features]
            best = (np.inf, None)
            for f in feats:
                r = split(x[e["mem"], f], y[e["mem"]], n_classes)
                if r[0] < best[0]:
                    best = (r[0], (f,) + r[1:])
            f, pos, lo, hi = best[1]
            if pos == len(e["mem"]) - 1:
                if (e["attempt"] + 1) * try_features < d:
                    nxt_again.append(dict(e, attempt=e["attempt"] + 1))
                else:
                    nodes[e["v"]]["freq"] = np.bincount(
                        y[e["mem"]], minlength=n_classes)
                continue
            go = x[e["mem"], f] <= lo
            kids = []
            for k, m in enumerate((e["mem"][go], e["mem"][~go])):
                nodes.append({})
                kids.append(dict(v=len(nodes) - 1, mem=m, depth=e["depth"] + 1,
                                 id=next_id + 2 * i + k, attempt=0))
            nodes[e["v"]].update(feature=int(f), value=threshold(lo, hi),
                                 child=(kids[0]["v"], kids[1]["v"]))
            nxt_kids += [k for k in kids if not is_leaf(k)]
        next_id += 2 * len(level)
        level = nxt_again + nxt_kids
    leaves = [v for v, nd in enumerate(nodes) if "freq" in nd]
    leaf = np.full(len(nodes), -1)
    leaf[leaves] = np.arange(len(leaves))
    return dict(
        feature=np.array([nd.get("feature", -1) for nd in nodes]),
        value=np.array([nd.get("value", 0.0) for nd in nodes]),
        child=np.array([nd.get("child", (-1, -1)) for nd in nodes]),
        leaf=leaf, frequencies=np.array([nodes[v]["freq"] for v in leaves]))


def forest(x, y, n_classes, n_estimators, try_features, max_depth,
           random_state):
    rs = np.random.RandomState(random_state)
    imax = np.iinfo(np.int32).max
    draws = [(rs.randint(imax), rs.randint(imax))
             for _ in range(n_estimators)]
    n = len(y)
    return [grow_tree(x, y, n_classes, np.random.RandomState(a).choice(
        n, size=n, replace=True), b, try_features, max_depth)
        for a, b in draws]


def predict(trees, x, n_classes):
    """(proba, soft labels, hard labels) of the rows of ``x``."""
    x = np.asarray(x, dtype=np.float64)
    proba = np.zeros((len(x), n_classes))
    soft = np.zeros(len(x), dtype=np.int64)
    hard = np.zeros(len(x), dtype=np.int64)
    for r, row in enumerate(x):
        votes = []
        for t in trees:
            v = 0
            while t["feature"][v] >= 0:
                v = t["child"][v][0 if row[t["feature"][v]] <= t["value"][v]
                                  else 1]
            freq = t["frequencies"][t["leaf"][v]]
            proba[r] += freq / np.float64(freq.sum())
            votes.append(int(np.argmax(freq)))
        soft[r] = np.argmax(proba[r])
        hard[r] = Counter(votes).most_common(1)[0][0]
    return proba / len(trees), soft, hard
