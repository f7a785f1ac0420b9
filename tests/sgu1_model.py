"""Independent numpy model of SGU1 on the device, for the
tests and for tests/golden/gen_golden_sgu1.py.

``forest_predict`` is xgboost's CPU predictor for reg:squarederror restated
over the original node arrays: pointer chasing from the root, ``x < thr`` goes
left, NaN takes the node's default side, and the float32 prediction starts at
base_score and adds one leaf per tree in tree order.  It shares no layout with
the kernel (no complete trees, no packing).  ``roll_mean`` restates pandas'
sliding Kahan roll_mean, ``slope_closed`` the kernel's closed-form slope and
``slope_exact`` the least-squares slope in exact rational arithmetic.
"""
from fractions import Fraction

import numpy as np

FEATURES = tuple([f"f_trades_{p}" for p in (1, 2, 3, 5, 10)] + [f"f_vwap_{r}" for r in (1, 3, 5)] +
                 [f"f_slope_{s}" for s in (1, 3, 5)] + [f"f_lag_rr_{k}" for k in (1, 2, 3, 4, 5)] +
                 ["f_spread", "f_vol_imb", "f_total_vol", "f_hour"])
EV_COLS = ("trade_time", "askprice1", "bidprice1", "p_buy_max", "p_sell_min", "v_buy_sum", "v_sell_sum", "vol_sum",
           "trade_count", "vwap_num")


def forest_depth(left, right, tree_off):
    """Longest root-to-leaf path of the forest (by recursion over the children)."""
    def d(base, n):
        return 0 if left[base + n] == -1 else 1 + max(d(base, left[base + n]), d(base, right[base + n]))
    return max([d(int(o), 0) for o in tree_off[:-1]], default=0)


def forest_predict(left, right, feat, value, default_left, tree_off, base_score, X, n_trees=None, depth=None):
    """X: float32 [n, 20].  Returns (pred float32 [n], leaf int32 [n, n_trees]); leaf is the
    position 0 .. 2^depth - 1 the walk ends at in a complete tree of ``depth`` (the forest's own
    by default, at least 1): the path's turns (right = 1) as bits, and a leaf reached above
    that depth counted as the rightmost position below it."""
    X = np.asarray(X, np.float32)
    n, T = X.shape[0], len(tree_off) - 1
    nt = T if n_trees is None else n_trees
    D = max(forest_depth(left, right, tree_off), 1) if depth is None else depth
    pred = np.full(n, np.float32(base_score), np.float32)
    leaf = np.zeros((n, nt), np.int32)
    rows = np.arange(n)
    for t in range(nt):
        base = int(tree_off[t])
        node = np.zeros(n, np.int64)
        path = np.zeros(n, np.int64)
        steps = np.zeros(n, np.int64)
        while True:
            live = left[base + node] != -1
            if not live.any():
                break
            f, thr = feat[base + node], value[base + node].astype(np.float32)
            x = X[rows, np.where(live, f, 0)]
            go_left = np.where(np.isnan(x), default_left[base + node] != 0, x < thr)
            nxt = np.where(go_left, left[base + node], right[base + node])
            node = np.where(live, nxt, node)
            path = np.where(live, 2 * path + (~go_left), path)
            steps = steps + live
        pred = (pred + value[base + node].astype(np.float32)).astype(np.float32)  # float32, tree order
        leaf[:, t] = ((path + 1) << (D - steps)) - 1
    return pred, leaf


def roll_mean(v, w, stats=None):
    """Series(v).rolling(w, min_periods=1).mean() for NaN-free v, bit for bit: pandas keeps
    one running sum per series with separate Kahan compensations for the values it adds and
    the values it removes; a window of one is set up afresh at every index.

    ``stats``: a dict that receives, per index, which override of calc_mean decided the value
    and changed its bits -- ``same`` (all values of the window equal, and sum / nobs is another
    number or a zero of the other sign), ``clamp_nonneg`` (no negative value, a negative mean)
    and ``clamp_neg`` (all negative, a positive mean) -- and ``neg``, the window's count of
    values with the sign bit set."""
    v = np.asarray(v, np.float64)
    out = np.empty(len(v))
    if stats is not None:
        stats.update(same=np.zeros(len(v), bool), clamp_nonneg=np.zeros(len(v), bool),
                     clamp_neg=np.zeros(len(v), bool), neg=np.zeros(len(v), np.int64))
    s = c_add = c_rm = 0.0
    nobs = neg = same = 0
    prev = v[0] if len(v) else 0.0
    for i in range(len(v)):
        if w == 1 or i == 0:
            s = c_add = c_rm = 0.0
            nobs = neg = same = 0
            prev = v[i]
        elif i >= w:
            x = v[i - w]
            y = -x - c_rm
            t = s + y
            c_rm = t - s - y
            s = t
            nobs -= 1
            neg -= int(np.signbit(x))
        x = v[i]
        y = x - c_add
        t = s + y
        c_add = t - s - y
        s = t
        nobs += 1
        neg += int(np.signbit(x))
        same = same + 1 if x == prev else 1
        prev = x
        r = s / nobs
        if stats is not None:
            stats["neg"][i] = neg
            if same >= nobs:
                stats["same"][i] = r != prev or np.signbit(r) != np.signbit(prev)
            else:
                stats["clamp_nonneg"][i], stats["clamp_neg"][i] = neg == 0 and r < 0, neg == nobs and r > 0
        if same >= nobs:
            r = prev
        elif neg == 0 and r < 0:
            r = 0.0
        elif neg == nobs and r > 0:
            r = 0.0
        out[i] = r
    return out


def slope_closed(y):
    """Least-squares slope of y (1 to 5 float64 values) against 0 .. m-1, on differences."""
    y = [np.float64(a) for a in y]
    m = len(y)
    if m < 2:
        return np.float64(0.0)
    if m == 2:
        return y[1] - y[0]
    if m == 3:
        return (y[2] - y[0]) / np.float64(2.0)
    if m == 4:
        return (np.float64(3.0) * (y[3] - y[0]) + (y[2] - y[1])) / np.float64(10.0)
    return (np.float64(2.0) * (y[4] - y[0]) + (y[3] - y[1])) / np.float64(10.0)


def slope_exact(y):
    """The same slope in exact rational arithmetic (Fraction)."""
    y = [Fraction(float(a)) for a in y]
    m = len(y)
    if m < 2:
        return Fraction(0)
    xm = Fraction(m - 1, 2)
    num = sum((Fraction(i) - xm) * a for i, a in enumerate(y))
    den = sum((Fraction(i) - xm) ** 2 for i in range(m))
    return num / den


def window_slopes(mid, s):
    """Per table row r (after shift(1) and the back-fill): the window of mids f_slope_s is
    computed from -- mids max(r-1, 0) - m + 1 .. max(r-1, 0), m = min(s, max(r-1, 0) + 1)."""
    out = []
    for r in range(len(mid)):
        p = max(r - 1, 0)
        m = min(s, p + 1)
        out.append(np.asarray(mid[p - m + 1:p + 1], np.float64))
    return out


def bar_mids(ev):
    """Closing mid of every 19-event bar of one day's event bars."""
    n = len(ev["trade_time"])
    last = np.arange(0, n - 19, 19) + 18
    return (np.asarray(ev["askprice1"], np.float64)[last] + np.asarray(ev["bidprice1"], np.float64)[last]) / 2.0


def feature_table(ev, stats=None):
    """SGU1DataPro.gen_dataset(19) of one day's event bars by the rules of DESIGN §9 row f6
    (numpy's pairwise sums from oracle/bundle_oracle.py, roll_mean and slope_closed above):
    float64 [rows, 21], the 20 features then label; no row below 6 bars.

    ``stats``: a dict that receives the per-bar intermediates -- ``branch`` (1 .. 4, the arm of
    the label's NaN fallback), ``x`` (the label before rounding), ``vwap``, ``hour`` and
    ``roll`` ({window: the stats of roll_mean})."""
    import bundle_oracle as bo
    col = {c: np.asarray(ev[c], np.int64 if c == "trade_time" else np.float64) for c in EV_COLS}
    starts = list(range(0, len(col["trade_time"]) - 19, 19))
    nb = len(starts)
    if nb < 6:
        return np.zeros((0, 21))
    nansum = lambda a: bo.pairwise_sum(np.where(np.isnan(a), 0.0, a))
    tr, vwap, mid, lab, spread, imb, vol, hour, xs, branch = (np.empty(nb) for _ in range(10))
    for b, a in enumerate(starts):
        g = {c: v[a:a + 19] for c, v in col.items()}
        bmax, smin = bo.nanmax(g["p_buy_max"]), bo.nanmin(g["p_sell_min"])
        am, bm = bo.skipna_mean(g["askprice1"]), bo.skipna_mean(g["bidprice1"])
        if not np.isnan(bmax) and not np.isnan(smin):
            x, branch[b] = bmax - smin, 1
        elif not np.isnan(smin):
            x, branch[b] = am - smin, 2
        elif not np.isnan(bmax):
            x, branch[b] = bmax - bm, 3
        else:
            x, branch[b] = am - bm, 4
        xs[b] = x
        lab[b] = np.rint(np.float64(x) * 1e4) / 1e4
        v = nansum(g["vol_sum"])
        tr[b], vol[b] = nansum(g["trade_count"]), v
        vwap[b] = nansum(g["vwap_num"]) / (v + 1e-9)
        mid[b] = (g["askprice1"][18] + g["bidprice1"][18]) / 2.0
        imb[b] = (nansum(g["v_buy_sum"]) - nansum(g["v_sell_sum"])) / (v + 1e-9)
        spread[b] = g["askprice1"][0] - g["bidprice1"][0]
        hour[b] = g["trade_time"][0] // 10000000
    p = np.maximum(np.arange(nb) - 1, 0)  # shift(1), row 0 back-filled from row 1
    out = np.empty((nb, 21))
    for j, w in enumerate((1, 2, 3, 5, 10)):
        out[:, j] = [tr[max(q - w + 1, 0):q + 1].sum() for q in p]
    roll = {w: {} for w in (1, 3, 5)}
    for j, w in enumerate((1, 3, 5)):
        out[:, 5 + j] = roll_mean(vwap, w, roll[w] if stats is not None else None)[p]
        out[:, 8 + j] = [slope_closed(y) for y in window_slopes(mid, w)]
    for L in range(1, 6):
        out[:, 10 + L] = lab[np.maximum(np.arange(nb) - L, 0)]
    out[:, 16], out[:, 17], out[:, 18], out[:, 19], out[:, 20] = spread[p], imb[p], vol[p], hour, lab
    if stats is not None:
        stats.update(branch=branch.astype(np.int64), x=xs, vwap=vwap, hour=hour.astype(np.int64), roll=roll)
    return out


# ---- hand-built forests shared by the CPU and GPU tests

def forest_arrays(trees):
    """trees: per tree a list of nodes -- (left, right, feat, thr, default_left) for a split,
    (-1, -1, 0, leaf_value, 0) for a leaf.  Returns the six node arrays."""
    flat = [n for t in trees for n in t]
    off = np.concatenate([[0], np.cumsum([len(t) for t in trees])]).astype(np.int64)
    return (np.array([n[0] for n in flat], np.int32), np.array([n[1] for n in flat], np.int32),
            np.array([n[2] for n in flat], np.int32), np.array([n[3] for n in flat], np.float32),
            np.array([n[4] for n in flat], np.uint8), off)


def leaf(v):
    return (-1, -1, 0, v, 0)


def edge_forest():
    """Three trees worked out by hand (base_score 0.25, complete depth 2):
      tree 0  x0 < 1.5 (NaN left) ? 10 : (x1 < 0.0 (NaN right) ? 20 : 30)
      tree 1  x2 < 1e-40 (a float32 subnormal; NaN right) ? 1 : 2      -- leaves at depth 1
      tree 2  the single leaf 0.5                                         -- a leaf at depth 0
    Returns (arrays, base_score, X float32 [5, 20], pred, leaf positions)."""
    arrays = forest_arrays([
        [(1, 2, 0, 1.5, 1), leaf(10.0), (3, 4, 1, 0.0, 0), leaf(20.0), leaf(30.0)],
        [(1, 2, 2, 1e-40, 0), leaf(1.0), leaf(2.0)],
        [leaf(0.5)]])
    nan, inf = np.nan, np.inf
    X = np.zeros((5, 20), np.float32)
    X[:, :3] = [[1.5, -0.0, 0.0],      # x == thr goes right; -0.0 < 0.0 is false: 30; 0 < 1e-40: 1
                [nan, 7.0, nan],       # NaN left: 10; NaN right: 2
                [inf, -inf, 1e-40],    # right, -inf < 0: 20; x == the subnormal threshold: 2
                [-inf, 0.0, 5e-41],    # left: 10; a smaller subnormal: 1
                [2.0, nan, -1.0]]      # right, NaN right: 30; 1
    pred = np.array([31.75, 12.75, 22.75, 11.75, 31.75], np.float32)
    # positions in the complete depth-2 tree; a shallow leaf counts as the rightmost below it
    pos = np.array([[3, 1, 3], [1, 3, 3], [2, 3, 3], [1, 1, 3], [3, 1, 3]], np.int32)
    return arrays, np.float32(0.25), X, pred, pos


def order_forest():
    """Four single-leaf trees whose float32 sum depends on the order: sequentially
    ((0 + 1e8) + 1) - 1e8 + 1 = 1, pairwise (1e8 + 1) + (-1e8 + 1) = 0."""
    return forest_arrays([[leaf(1e8)], [leaf(1.0)], [leaf(-1e8)], [leaf(1.0)]]), np.float32(0.0), np.float32(1.0)


def random_forest(rng, n_trees, depth, p_leaf=0.3):
    """Unbalanced random trees, the deepest path of the first tree exactly ``depth`` long;
    thresholds from a small grid so that rows drawn from the same grid hit x == thr."""
    trees = []
    for t in range(n_trees):
        nodes = []

        def grow(d, force):
            i = len(nodes)
            nodes.append(None)
            if d == depth or (not force and rng.random() < p_leaf):
                nodes[i] = leaf(float(np.float32(rng.normal())))
                return i
            l = grow(d + 1, force)
            r = grow(d + 1, False)
            nodes[i] = (l, r, int(rng.integers(0, 20)), float(rng.integers(-3, 4)) / 2.0, int(rng.integers(0, 2)))
            return i

        grow(0, t == 0)
        trees.append(nodes)
    return forest_arrays(trees)


def random_rows(rng, n):
    X = (rng.integers(-4, 5, (n, 20)) / 2.0).astype(np.float32)
    X[rng.random((n, 20)) < 0.05] = np.nan
    return X
