"""Inputs of the SGU1 training tests, shared by the CPU tests of the model
(tests/test_sgu1_train_model.py, which assert that the model really reaches
the edge a case is built for) and the GPU tests (tests/test_gpu_sgu1_train.py,
which compare the device with the model on the same input, byte for byte).

A case is (X [n, 20], y [n], rows_train, rows_val, params) or, with the
validation rows in a table of their own, (X, y, rows_train, rows_val, params,
X_val, y_val).  ``case(name)`` builds one, ``model(name)`` is the model's fit
of it; both are computed once per process and must be left unchanged."""
import functools

import numpy as np

import sgu1_train_model as tm

SMALL = dict(tm.PARAMS, n_estimators=16, early_stopping_rounds=3, eta=0.3)
SCALES = (-140, -100, -7, 0, 30, 100, 124)  # -7: the nearest scale to -6 at which the 1e-6 rule removes a split
SMALL_SCALE = -7
# At 2^-140 every gradient and residual has at most 12 bits, so each quantisation is exact at any
# scale and an exponent off by one in the subnormal range changes no result.  At 2^-130 all
# labels are still subnormal but the residuals carry more than the metric's 20 bits: there it shows.
SUBNORMAL_SCALE = -130
MAX_BINS = (2, 3, 255, 256)
PLANTED_COLS = (0, 2, 5, 7, 11, 19)


def grid(rng, n):
    """The background: nine values -2 .. 2 per column, 3 % NaN."""
    X = (rng.integers(-4, 5, (n, 20)) / 2).astype(np.float32)
    X[rng.random((n, 20)) < 0.03] = np.nan
    return X


def edge_table(rng, n):
    """Rows that take every branch of the trainer: column 1 all NaN, column 2 with NaNs that
    belong left under x0 < 0 and right otherwise, column 3 constant, column 4 continuous
    (more than 256 distinct values from 257 rows on), columns 5 and 6 identical, the rest a
    small grid with a few NaNs."""
    X = grid(rng, n)
    X[:, 0] = rng.integers(-2, 3, n)
    X[:, 1] = np.nan
    X[:, 2] = np.where(rng.random(n) < 0.3, np.nan, rng.integers(0, 4, n)).astype(np.float32)
    X[:, 3] = 1.25
    X[:, 4] = rng.normal(size=n).astype(np.float32)
    X[:, 6] = X[:, 5]
    x2 = X[:, 2]
    low = X[:, 0] < 0
    y = np.where(low, np.where(np.isnan(x2) | (x2 < 2), -2.0, 2.0), np.where(np.isnan(x2) | (x2 >= 2), 3.0, 0.0)) \
        + np.where(X[:, 5] < 0, 1.0, 0.0) + 0.5 * X[:, 4] + 0.2 * rng.normal(size=n)
    return X, y.astype(np.float32)


def split_rows(n_train, n_val):
    """Index lists with gaps between them, as the days of a feature table leave."""
    rt = 2 + np.arange(n_train)
    rv = 2 + n_train + 3 + np.arange(n_val)
    return rt, rv, 2 + n_train + 3 + n_val + 1


@functools.lru_cache(maxsize=None)
def edge():
    X, y = edge_table(np.random.default_rng(1), 420)
    rt, rv, _ = split_rows(300, 110)
    return X, y, rt, rv


def planted(variant):
    """Six independent +-1 columns decide the label, so a depth-6 tree splits on all of them:
    full levels.  Variant 1: powers of two and lambda 0 (every split halves what is left);
    variant 2: near-equal coefficients under lambda 1 (a large node mean would suppress
    splits)."""
    rng = np.random.default_rng(20 + variant)
    n = 1100
    X = grid(rng, n)
    B = (rng.integers(0, 2, (n, 6)) * 2 - 1).astype(np.float32)
    X[:, PLANTED_COLS] = B
    c = {1: [32, 16, 8, 4, 2, 1], 2: [1.5, 1.4, 1.3, 1.2, 1.1, 1.0]}[variant]
    y = (B.astype(np.float64) @ np.array(c) + 0.05 * rng.normal(size=n)).astype(np.float32)
    return X, y, np.arange(1000), 1000 + np.arange(100)


def planted_params(variant, depth):
    return dict(SMALL, max_depth=depth, min_child_weight=1.0, eta=0.3, n_estimators=4,
                reg_lambda={1: 0.0, 2: 1.0}[variant])


ROUNDING_SEED = 3  # of seeds 0 .. 3, 1 and 3 leave a root child whose sum float64 cannot hold; 3 leaves it on a tie
N_BIG, N_TIE, N_WHOLE = 30000, 2000, 769


def rounding_table():
    """Round-0 gradients that rint has to round, ties among them, and node sums past 2^53.

    base_score is exactly 0 (the labels come in pairs +-), so g = -y in round 0.  30 000
    pairs +-v, v = 1 + j / 1024: the largest |g| lies in [1, 2), s = 39, and a child that
    holds the rows of one sign sums to about 30 000 * 1.2 * 2^39 = 2^54.1.  2 000 pairs +-d
    with d an odd multiple of 2^-40 below 2^-33: d 2^39 is a half-integer, an exact tie;
    769 pairs with d a multiple of 2^-39, which no rounding moves.  Column 0 is the label's
    sign for the +-v rows and a random sign for the tiny rows; column 1 is 3 on the tiny
    rows, outside the grid, so that below the root split a level-1 split sets them apart:
    their leaf holds the sum of rounded ties alone, and its value shows every unit of it
    (beside 2^54 a unit is less than the float64 rounding of the sum)."""
    rng = np.random.default_rng(ROUNDING_SEED)
    v = 1.0 + rng.integers(0, 410, N_BIG) / 1024.0
    d = np.concatenate([np.ldexp(2.0 * rng.integers(0, 64, N_TIE) + 1.0, -40),
                        np.ldexp(rng.integers(1, 64, N_WHOLE).astype(np.float64), -39)])
    y = np.concatenate([v, -v, d, -d])
    n, tiny = len(y), np.abs(y) < 1.0
    X = grid(rng, n)
    X[:, 0] = np.where(tiny, rng.integers(0, 2, n) * 2.0 - 1.0, np.sign(y))
    X[tiny, 1] = 3.0
    perm = rng.permutation(n)
    y32 = y[perm].astype(np.float32)
    assert (y32.astype(np.float64) == y[perm]).all()  # every label is a float32
    return X[perm], y32, np.arange(n), np.arange(64)


ROUNDING_PARAMS = dict(SMALL, max_depth=2, n_estimators=2, early_stopping_rounds=0, reg_alpha=0.0)


def inf_table():
    """The edge table with +inf and -inf in column 4 (about 10 % each, the labels shifted by
    +-4 on those rows, so that the split at the infinite cut pays) and random signs on the
    zeros of column 5."""
    X, y, rt, rv = edge()
    rng = np.random.default_rng(31)
    X, y = X.copy(), y.copy()
    u = rng.random(len(X))
    X[u < 0.1, 4], X[u > 0.9, 4] = np.inf, -np.inf
    y[u < 0.1] += 4.0
    y[u > 0.9] -= 4.0
    zero = X[:, 5] == 0
    X[zero, 5] = np.where(rng.random(zero.sum()) < 0.5, -0.0, 0.0).astype(np.float32)
    X[:, 6] = X[:, 5]
    return X, y, rt, rv


def cuts_table():
    """Columns with exactly 256 and 257 distinct values, +-0 as one value, an all-NaN column
    and a short column with both infinities."""
    X = np.zeros((300, 20), np.float32)
    X[:, 0] = np.minimum(np.arange(300), 255)
    X[:, 1] = np.minimum(np.arange(300), 256)
    X[:, 2] = np.where(np.arange(300) % 2, -0.0, 0.0)
    X[:, 3] = np.nan
    X[:7, 4] = [3, np.nan, 1, 2, 2, np.inf, -np.inf]
    return X


def second_table():
    """Validation rows from a table of their own, with another leading dimension."""
    X2, y2 = edge_table(np.random.default_rng(7), 57)
    return X2, y2, np.array([50, 3, 3, 56, 0] + list(range(10, 40)))


@functools.lru_cache(maxsize=None)
def case(name):
    kind, *args = name.split(":")
    if kind == "depth":  # A
        X, y, rt, rv = edge()
        return X, y, rt, rv, dict(SMALL, max_depth=int(args[0]), min_child_weight=2.0)
    if kind == "planted":  # B: variant, depth
        return planted(int(args[0])) + (planted_params(int(args[0]), int(args[1])),)
    if kind == "scale":  # C
        X, y, rt, rv = edge()
        return X, np.ldexp(y, int(args[0])), rt, rv, dict(SMALL, reg_alpha=0.0, min_child_weight=2.0)
    if kind == "rounding":  # D
        return rounding_table() + (ROUNDING_PARAMS,)
    if kind == "inf":  # E; SGU1(n_estimators=16, early_stopping_rounds=3, learning_rate=0.3) has these parameters
        return inf_table() + (dict(SMALL),)
    if kind == "max_bin":
        X, y, rt, rv = edge()
        return X, y, rt, rv, dict(SMALL, max_bin=int(args[0]), min_child_weight=2.0)
    X, y, rt, rv = edge()  # F
    if kind == "second_table":
        X2, y2, rv2 = second_table()
        return X, y, rt, rv2, dict(SMALL), X2, y2
    if kind == "one_val_row":
        return X, y, rt, rv[:1], dict(SMALL)
    if kind == "bootstrap":
        return X, y, np.random.default_rng(41).choice(rt, len(rt)), rv, dict(SMALL, min_child_weight=2.0)
    if kind == "mcw2.5":
        return X, y, rt, rv, dict(SMALL, min_child_weight=2.5)
    if kind == "mcw0":
        return X, y, rt, rv, dict(SMALL, min_child_weight=0.0, reg_lambda=1.0, max_depth=6)
    raise KeyError(name)


ROWS_AND_TABLES = ("second_table", "one_val_row", "bootstrap", "mcw2.5", "mcw0")


def model_fit(X, y, rt, rv, p, X_val=None, y_val=None, fit=tm.fit):
    """The model on a case: it sees the gathered rows X[rt], not the index lists."""
    Xv, yv = (X, y) if X_val is None else (X_val, y_val)
    return fit(X[rt], y[rt], Xv[rv] if len(rv) else None, yv[rv] if len(rv) else None, **p)


@functools.lru_cache(maxsize=None)
def model(name):
    return model_fit(*case(name))


def level_widths(fit, t):
    """Nodes per depth of tree t (index d: the nodes at depth d)."""
    a, b = int(fit["tree_off"][t]), int(fit["tree_off"][t + 1])
    left, right = fit["left"][a:b], fit["right"][a:b]
    depth = np.zeros(b - a, np.int64)
    for k in range(b - a):  # children have larger ids than their parent
        if left[k] != -1:
            depth[left[k]] = depth[right[k]] = depth[k] + 1
    return np.bincount(depth), depth
