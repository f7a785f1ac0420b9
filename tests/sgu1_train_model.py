"""The SGU1 training contract (include/sgmm.h above
sgmm_sgu1_task) in numpy, independent of the kernel and written twice:

``fit`` builds the histograms of a whole level at once (exact integer
bincounts over (feature, node, bin) keys, prefix sums, one vectorised score
array per level); ``fit_bruteforce`` works node by node from the rows
themselves -- it compares the raw feature values with every cut and sums the
quantised gradients of the rows on each side, no bins and no histograms.  The
two agree bit for bit whenever every feature has at most ``max_bin`` distinct
values (then the cuts are the data values and both see the same candidates);
the rows of the finished tree are routed by walking it on the raw values in
both, as SGU1Forest.predict does.

Also here: ``make_cuts`` (the cut rule), ``base_score`` and ``write_json``
(xgboost's JSON model layout)."""
import json
import math

import numpy as np

NF = 20
PARAMS = dict(max_depth=4, min_child_weight=4.0, eta=0.01, reg_lambda=1.0, reg_alpha=0.01, gamma=0.0, max_bin=256,
              n_estimators=1000, early_stopping_rounds=20)
RT_EPS = 1e-6  # xgboost's kRtEps


def make_cuts(X, max_bin=256):
    """Cuts of every feature from the training rows X [n, 20] (float32): the sorted distinct
    non-NaN values v (-0 and +0 one value); v[1:] when len(v) <= max_bin, otherwise
    v[ceil(k len(v) / max_bin)] for k = 1 .. max_bin - 1."""
    out = []
    for f in range(NF):
        x = np.asarray(X[:, f], np.float32)
        v = np.unique(x[~np.isnan(x)] + np.float32(0.0))
        if len(v) <= max_bin:
            out.append(v[1:].copy())
        else:
            k = np.arange(1, max_bin, dtype=np.int64)
            out.append(v[(k * len(v) + max_bin - 1) // max_bin].copy())
    return out


def base_score(y):
    y = np.asarray(y, np.float32)
    return np.float32(math.fsum(float(v) for v in y) / len(y))


def _soft(G, alpha):
    return np.where(G > alpha, G - alpha, np.where(G < -alpha, G + alpha, 0.0))


def _gain(Q, H, s, P):
    T = _soft(np.ldexp(np.asarray(Q, np.int64).astype(np.float64), -s), P["reg_alpha"])
    return T * T / (np.asarray(H, np.float64) + P["reg_lambda"])


def _weight(Q, H, s, P):
    T = float(_soft(np.ldexp(np.float64(int(Q)), -s), P["reg_alpha"]))
    return -T / (float(H) + P["reg_lambda"])


def _exact_bincount(key, q, size):
    """sum of int64 q (|q| <= 2^40, at most 2^20 of them) per key: two float64 bincounts of 20-bit halves."""
    lo = (q & ((1 << 20) - 1)).astype(np.float64)
    hi = (q >> 20).astype(np.float64)
    return (np.bincount(key, hi, size).astype(np.int64) << 20) + np.bincount(key, lo, size).astype(np.int64)


class _Tree:
    def __init__(self, Q0, H0):
        self.left, self.right, self.feat, self.dl = [-1], [-1], [0], [0]
        self.value, self.bw, self.lc = [np.float32(0)], [np.float32(0)], [np.float32(0)]
        self.Q, self.H = [int(Q0)], [int(H0)]

    def split(self, node, f, thr, dl, score, QL, HL, s, P):
        k = len(self.left)
        self.left[node], self.right[node], self.feat[node], self.dl[node] = k, k + 1, int(f), int(dl)
        self.value[node] = np.float32(thr)
        self.bw[node] = np.float32(_weight(self.Q[node], self.H[node], s, P))
        with np.errstate(over="ignore"):  # a score past float32 is +inf, as the device's cast
            self.lc[node] = np.float32(score)
        for Q, H in ((QL, HL), (self.Q[node] - QL, self.H[node] - HL)):
            self.left.append(-1), self.right.append(-1), self.feat.append(0), self.dl.append(0)
            self.value.append(np.float32(0)), self.bw.append(np.float32(0)), self.lc.append(np.float32(0))
            self.Q.append(int(Q)), self.H.append(int(H))

    def finish(self, s, P):
        for node in range(len(self.left)):
            if self.left[node] == -1 and s is not None:
                v = np.float32(P["eta"] * _weight(self.Q[node], self.H[node], s, P))
                self.value[node] = self.bw[node] = v
        return self


def walk(tree, X):
    """Leaf node id of every row of X [n, 20] (raw values: x < thr left, NaN the default side)."""
    left, right, feat = np.asarray(tree.left), np.asarray(tree.right), np.asarray(tree.feat)
    thr, dl = np.asarray(tree.value, np.float32), np.asarray(tree.dl).astype(bool)
    pos = np.zeros(len(X), np.int64)
    while True:
        inner = left[pos] != -1
        if not inner.any():
            return pos
        x = X[np.arange(len(X)), feat[pos]]
        go_left = np.where(np.isnan(x), dl[pos], x < thr[pos])
        pos = np.where(inner, np.where(go_left, left[pos], right[pos]), pos)


def _accept(score, P):
    return score > -np.inf and score > P["gamma"] and score > RT_EPS


def grow_hist(X, q, s, cuts, P):
    """Level by level: one histogram over (feature, node, bin) of all the level's rows."""
    n = len(X)
    miss = np.isnan(X)
    bins = np.stack([np.searchsorted(cuts[f], X[:, f], side="right") for f in range(NF)], axis=1)
    bins = np.where(miss, 256, bins).astype(np.int64)
    ncut = np.array([len(c) for c in cuts])
    tree = _Tree(q.sum(), n)
    pos = np.zeros(n, np.int64)
    lo, hi = 0, 1
    for _ in range(P["max_depth"]):
        if lo == hi:
            break
        nn = hi - lo
        idx = np.nonzero((pos >= lo) & (pos < hi))[0]
        key = ((np.arange(NF)[None, :] * nn + (pos[idx] - lo)[:, None]) * 257 + bins[idx]).ravel()
        hs = _exact_bincount(key, np.repeat(q[idx], NF), NF * nn * 257).reshape(NF, nn, 257)
        hc = np.bincount(key, minlength=NF * nn * 257).reshape(NF, nn, 257)
        PQ, PH = np.cumsum(hs[:, :, :256], axis=2), np.cumsum(hc[:, :, :256], axis=2)
        MQ, MH = hs[:, :, 256], hc[:, :, 256]
        NQ, NH = np.array(tree.Q[lo:hi], np.int64), np.array(tree.H[lo:hi], np.int64)
        QL = np.stack([PQ, PQ + MQ[:, :, None]], axis=3)  # [f, node, cut, default_left]
        HL = np.stack([PH, PH + MH[:, :, None]], axis=3)
        QR, HR = NQ[None, :, None, None] - QL, NH[None, :, None, None] - HL
        valid = (np.arange(256)[None, None, :, None] < ncut[:, None, None, None]) \
            & (HL >= P["min_child_weight"]) & (HR >= P["min_child_weight"]) \
            & np.stack([np.ones_like(MH, bool), MH > 0], axis=2)[:, :, None, :]
        with np.errstate(all="ignore"):
            score = (_gain(QL, HL, s, P) + _gain(QR, HR, s, P)) - _gain(NQ, NH, s, P)[None, :, None, None]
        score = np.where(valid, score, -np.inf)
        nxt = hi
        for k in range(nn):
            flat = score[:, k].reshape(-1)  # (feature, cut, default_left): argmax takes the first maximum
            c = int(np.argmax(flat))
            if not _accept(flat[c], P):
                continue
            f, j, dl = c // 512, (c // 2) % 256, c % 2
            tree.split(lo + k, f, cuts[f][j], dl, flat[c], int(QL[f, k, j, dl]), int(HL[f, k, j, dl]), s, P)
            rows = idx[pos[idx] == lo + k]
            go_left = np.where(miss[rows, f], bool(dl), bins[rows, f] <= j)
            pos[rows] = np.where(go_left, nxt, nxt + 1)
            nxt += 2
        lo, hi = hi, nxt
    return tree.finish(s, P)


def grow_bruteforce(X, q, s, cuts, P):
    """Node by node from the rows: every (feature, cut, missing side) against the raw values."""
    alpha, lam, mcw = P["reg_alpha"], P["reg_lambda"], P["min_child_weight"]

    def gain(Q, H):  # one value at a time, in the contract's operation order
        G = math.ldexp(float(int(Q)), -s)
        T = G - alpha if G > alpha else (G + alpha if G < -alpha else 0.0)
        return T * T / (float(H) + lam)

    tree = _Tree(q.sum(), len(X))
    members = {0: np.arange(len(X))}
    level = [0]
    for _ in range(P["max_depth"]):
        nxt_level = []
        for node in level:
            rows = members.pop(node)
            qn = q[rows]
            NQ, NH = int(qn.sum()), len(rows)
            assert (NQ, NH) == (tree.Q[node], tree.H[node])
            gN = gain(NQ, NH)
            best = (-np.inf, None)
            for f in range(NF):
                x = X[rows, f]
                nan = np.isnan(x)
                for j, cut in enumerate(cuts[f]):
                    below = x < cut  # NaN compares false
                    for dl in ((0, 1) if nan.any() else (0,)):
                        L = below | nan if dl else below
                        HL = int(L.sum())
                        if not (HL >= mcw and NH - HL >= mcw):
                            continue
                        QL = int(qn[L].sum())
                        sc = (gain(QL, HL) + gain(NQ - QL, NH - HL)) - gN
                        if sc > best[0]:  # strict: the first of equal scores stays
                            best = (sc, (f, j, dl, QL, HL, L))
            if best[1] is None or not _accept(best[0], P):
                continue
            f, j, dl, QL, HL, L = best[1]
            k = len(tree.left)
            tree.split(node, f, cuts[f][j], dl, best[0], QL, HL, s, P)
            members[k], members[k + 1] = rows[L], rows[~L]
            nxt_level += [k, k + 1]
        level = nxt_level
    return tree.finish(s, P)


def _exponent(m):
    """e with 2^(e-1) <= m < 2^e for a positive float32 (subnormals included)."""
    return int(np.frexp(np.float32(m))[1])


def rmse_metric(pred, y):
    r = np.asarray(pred, np.float32) - np.asarray(y, np.float32)
    mr = np.abs(r).max()
    if mr == 0:
        return 0.0
    s2 = 20 - _exponent(mr)
    v = np.rint(np.ldexp(r.astype(np.float64), s2)).astype(np.int64)
    return math.sqrt(math.ldexp(float(int((v * v).sum())), -2 * s2) / len(r))


def _fit(grow, X_train, y_train, X_val, y_val, params):
    P = dict(PARAMS)
    P.update(params)
    Xt, yt = np.ascontiguousarray(X_train, np.float32), np.asarray(y_train, np.float32).ravel()
    nv = 0 if X_val is None else len(X_val)
    Xv = np.ascontiguousarray(X_val, np.float32) if nv else np.zeros((0, NF), np.float32)
    yv = np.asarray(y_val, np.float32).ravel() if nv else np.zeros(0, np.float32)
    if P["early_stopping_rounds"] and not nv:
        raise ValueError("early stopping needs validation rows")
    cuts = make_cuts(Xt, P["max_bin"])
    base = base_score(yt)
    pt, pv = np.full(len(Xt), base, np.float32), np.full(nv, base, np.float32)
    trees, hist = [], []
    best_it, best = -1, np.inf
    for t in range(P["n_estimators"]):
        g = pt - yt
        m = np.abs(g).max()
        if m == 0:
            tree = _Tree(0, len(Xt)).finish(None, P)  # one +0 leaf
        else:
            s = 40 - _exponent(m)
            q = np.rint(np.ldexp(g.astype(np.float64), s)).astype(np.int64)
            tree = grow(Xt, q, s, cuts, P)
        trees.append(tree)
        val = np.asarray(tree.value, np.float32)
        pt = pt + val[walk(tree, Xt)]
        if nv:
            pv = pv + val[walk(tree, Xv)]
            hist.append(rmse_metric(pv, yv))
            if hist[-1] < best:
                best, best_it = hist[-1], t
            elif P["early_stopping_rounds"] and t - best_it >= P["early_stopping_rounds"]:
                break
    cat = lambda name, dt: np.concatenate([np.asarray(getattr(t, name), dt) for t in trees]) if trees else np.zeros(0, dt)
    return dict(left=cat("left", np.int32), right=cat("right", np.int32), feat=cat("feat", np.int32),
                value=cat("value", np.float32), default_left=cat("dl", np.uint8), base_weight=cat("bw", np.float32),
                loss_change=cat("lc", np.float32), sum_hessian=cat("H", np.float32),
                tree_off=np.concatenate([[0], np.cumsum([len(t.left) for t in trees])]).astype(np.int64),
                base_score=base, val_rmse=np.array(hist, np.float64), n_trees=len(trees), best_iteration=best_it,
                best_score=best if best_it >= 0 else float("nan"), pred_train=pt, pred_val=pv, cuts=cuts, params=P)


def fit(X_train, y_train, X_val=None, y_val=None, **params):
    return _fit(grow_hist, X_train, y_train, X_val, y_val, params)


def fit_bruteforce(X_train, y_train, X_val=None, y_val=None, **params):
    return _fit(grow_bruteforce, X_train, y_train, X_val, y_val, params)


FOREST_KEYS = ("left", "right", "feat", "value", "default_left", "base_weight", "loss_change", "sum_hessian", "tree_off")


def same_fit(a, b):
    """Byte equality of two fits (forest, history, best round and score)."""
    for k in FOREST_KEYS + ("val_rmse",):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return False
    return (a["n_trees"], a["best_iteration"]) == (b["n_trees"], b["best_iteration"]) and \
        np.float64(a["best_score"]).tobytes() == np.float64(b["best_score"]).tobytes() and \
        np.float32(a["base_score"]).tobytes() == np.float32(b["base_score"]).tobytes()


def _f32_list(a):
    return [float(str(v)) for v in np.asarray(a, np.float32)]  # the shortest decimal that reads back to the float32


def write_json(fit_result, path, feature_names):
    """xgboost's JSON model (the layout of Booster.save_model, version [3, 1, 3])."""
    r = fit_result
    off = r["tree_off"]
    trees = []
    for t in range(len(off) - 1):
        a, b = int(off[t]), int(off[t + 1])
        left, right = r["left"][a:b], r["right"][a:b]
        parents = np.full(b - a, 2147483647, np.int64)
        for k in range(b - a):
            if left[k] != -1:
                parents[left[k]] = parents[right[k]] = k
        trees.append({
            "base_weights": _f32_list(r["base_weight"][a:b]), "categories": [], "categories_nodes": [],
            "categories_segments": [], "categories_sizes": [],
            "default_left": [int(v) for v in r["default_left"][a:b]], "id": t,
            "left_children": [int(v) for v in left], "loss_changes": _f32_list(r["loss_change"][a:b]),
            "parents": [int(v) for v in parents], "right_children": [int(v) for v in right],
            "split_conditions": _f32_list(r["value"][a:b]), "split_indices": [int(v) for v in r["feat"][a:b]],
            "split_type": [0] * (b - a), "sum_hessian": _f32_list(r["sum_hessian"][a:b]),
            "tree_param": {"num_deleted": "0", "num_feature": str(NF), "num_nodes": str(b - a),
                           "size_leaf_vector": "1"}})
    mant, exp = np.format_float_scientific(np.float32(r["base_score"]), unique=True).split("e")
    attributes = {"scikit_learn": '{"_estimator_type": "regressor"}'}
    if r["best_iteration"] >= 0:
        attributes.update(best_iteration=str(int(r["best_iteration"])), best_score=repr(float(r["best_score"])))
    doc = {"learner": {
        "attributes": attributes, "feature_names": list(feature_names), "feature_types": ["int" if n == "f_hour" else "float" for n in feature_names],
        "gradient_booster": {"model": {
            "cats": {"enc": [], "feature_segments": [], "sorted_idx": []},
            "gbtree_model_param": {"num_parallel_tree": "1", "num_trees": str(len(trees))},
            "iteration_indptr": list(range(len(trees) + 1)), "tree_info": [0] * len(trees), "trees": trees},
            "name": "gbtree"},
        "learner_model_param": {"base_score": f"[{mant.rstrip('.')}E{int(exp)}]", "boost_from_average": "1",
                                "num_class": "0", "num_feature": str(NF), "num_target": "1"},
        "objective": {"name": "reg:squarederror", "reg_loss_param": {"scale_pos_weight": "1"}}},
        "version": [3, 1, 3]}
    with open(path, "w") as fh:
        json.dump(doc, fh)
