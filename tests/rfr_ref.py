"""A plain numpy restatement of ``dislib_amd.regression.forest``, one node at
a time, with ``rf_ref``'s feature draws and threshold."""
import numpy as np

from tests.rf_ref import feature_order, threshold


def scores(values, y, dtype=np.float64):
    """(scores in (value, member) order, ``inf`` inside a run of equal values;
    the sorted values), computed in ``dtype``."""
    size = len(y)
    o = np.argsort(values, kind="stable")
    v, ys = np.asarray(values)[o], np.asarray(y, dtype=dtype)[o]
    S, SL = ys.sum(dtype=dtype), dtype(0)
    out = np.full(size, np.inf, dtype=dtype)
    for i in range(size):
        SL = SL + ys[i]
        if i + 1 < size and v[i + 1] == v[i]:
            continue
        SR = S - SL
        ll, rl = dtype(i + 1), dtype(max(size - i - 1, 1))
        out[i] = -(SL * SL / ll + SR * SR / rl)
    return out, v


def split(values, y):
    """(score, position, lower, upper value) of the last minimum."""
    s, v = scores(values, y)
    pos = len(s) - 1 - int(np.argmin(s[::-1]))
    return s[pos], pos, v[pos], v[min(pos + 1, len(s) - 1)]


def grow_tree(x, y, sample, seed, try_features, max_depth):
    """One tree as the arrays of ``RandomForestRegressor.trees``."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    d = x.shape[1]
    nodes = [{}]
    level = [dict(v=0, mem=np.sort(sample), id=0, depth=0, attempt=0)]
    next_id = 1

    def is_leaf(e, force=False):
        t = y[e["mem"]]
        if force or t.min() == t.max() or e["depth"] >= max_depth:
            nodes[e["v"]]["leaf"] = (t.sum() / len(t), len(t))
            return True
        return False

    level = [e for e in level if not is_leaf(e)]
    while level:
        nxt_again, nxt_kids = [], []
        for i, e in enumerate(level):
            a = e["attempt"]
            best = (np.inf, None)
            for f in feature_order(seed, e["id"], d)[a * try_features:
                                                     (a + 1) * try_features]:
                r = split(x[e["mem"], f], y[e["mem"]])
                if r[0] < best[0]:
                    best = (r[0], (f,) + r[1:])
            f, pos, lo, hi = best[1]
            if pos == len(e["mem"]) - 1:
                if (a + 1) * try_features < d:
                    nxt_again.append(dict(e, attempt=a + 1))
                else:
                    is_leaf(e, True)
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
    leaves = [nd["leaf"] for nd in nodes if "leaf" in nd]
    leaf = np.full(len(nodes), -1)
    leaf[["leaf" in nd for nd in nodes]] = np.arange(len(leaves))
    return dict(
        feature=np.array([nd.get("feature", -1) for nd in nodes]),
        value=np.array([nd.get("value", 0.0) for nd in nodes]),
        child=np.array([nd.get("child", (-1, -1)) for nd in nodes]),
        leaf=leaf, leaf_value=np.array([m for m, _ in leaves]),
        size=np.array([s for _, s in leaves]))


def forest(x, y, n_estimators, try_features, max_depth, random_state):
    rs = np.random.RandomState(random_state)
    imax = np.iinfo(np.int32).max
    draws = [(rs.randint(imax), rs.randint(imax))
             for _ in range(n_estimators)]
    return [grow_tree(x, y, np.random.RandomState(a).choice(
        len(y), size=len(y), replace=True), b, try_features, max_depth)
        for a, b in draws]


def predict(trees, x):
    """The leaf values added in tree order, divided by the trees."""
    out = np.zeros(len(x))
    for r, row in enumerate(np.asarray(x, dtype=np.float64)):
        for t in trees:
            v = 0
            while t["feature"][v] >= 0:
                v = t["child"][v][int(row[t["feature"][v]] > t["value"][v])]
            out[r] += t["leaf_value"][t["leaf"][v]]
    return out / len(trees)
