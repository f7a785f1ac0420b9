"""Edge days of the SGU1 feature table, shared by the CPU
tests of the model (tests/test_sgu1_model.py, which assert that a day really
reaches the branch it is built for and that pandas agrees with the model on
it) and the GPU tests (tests/test_gpu_sgu1.py, which hold k_sgu1_features to
the model on the same day, byte for byte).

A day is a dict of the sm.EV_COLS columns (19 * bars + 1 events) for
EventBarsGPU.from_bars.  ``day(name)`` builds one, ``table(name)`` is the
model's (table, stats) of it, ``turns()`` the list of days of the joint
launch; all are computed once per process and must be left unchanged.

Everything comes from seeded default_rng streams; nothing is read from a file.
"""
import functools

import numpy as np

import sgu1_model as sm

EVENTS = 19
DAYS = ("rolling", "ties", "cast", "hours", "full")
TURNS = (6, 7, 1023, 5, 1024, 1025, 0, 2048, 2049)  # bars per day of the joint launch; 0: a day without events
FLT_MAX = float(np.finfo(np.float32).max)

# Stretches of one sign and a wide dynamic range on which pandas' Kahan sum ends on the other
# side of zero: (seed, sign, window that clamps).  Found by a search over seeds with the
# stretches in this order at the head of the series (the running sum and its compensations
# carry over from all that precedes); test_edge_days_reach_their_edges holds them to it.
CLAMPS = ((137, 1, 3), (201632, -1, 3), (226674, 1, 5), (227768, -1, 5))
CLAMP_LEN = 40
# The same with three values in ten replaced by -0.0, so that a window holds a -0.0 where the
# sum ends on the wrong side: signbit counts it as negative (pandas), x < 0 does not, and the
# clamp decides the other way.  They follow the CLAMPS stretches.
SIGNED_ZERO_CLAMPS = ((7923, 1, 3), (7961, 1, 5), (20194, -1, 3), (20214, -1, 5))


def wide(seed, n=CLAMP_LEN):
    rng = np.random.default_rng(seed)
    return rng.random(n) * 10.0 ** rng.integers(-8, 17, n)


def wide_signed_zero(seed, sign, n=CLAMP_LEN):
    rng = np.random.default_rng(seed)
    v = rng.random(n) * 10.0 ** rng.integers(-8, 17, n)
    return np.where(rng.random(n) < 0.3, -0.0, sign * v)


def rolling_targets(seed, nb=None):
    """vwap targets that take every branch of pandas' calc_mean: the clamp stretches, runs of
    1-6 equal values, signed values, 1e16 cancellations, runs of +-0.0, and the ends of the
    float64 range.  One cycle of the pieces when nb is None, else cycles cut to nb bars."""
    rng = np.random.default_rng(seed)
    out, n = [], 0
    while nb is None or n < nb:
        p = [s * wide(k) for k, s, _ in CLAMPS] + [wide_signed_zero(k, s) for k, s, _ in SIGNED_ZERO_CLAMPS]
        p.append(np.repeat(np.round(rng.normal(3.5, 0.01, 70), 3), rng.integers(1, 7, 70)))
        p.append(rng.normal(0, 1, 90))
        p.append(np.concatenate([[1e16, 1.0, -1e16], rng.random(12) * 1e-3, [0.0] * 7, [1e16, 1.0, -1e16],
                                 [0.0] * 6, rng.random(5), [-1e16, -1.0, 1e16], [0.0] * 4]))
        p.append(np.repeat(rng.choice([-0.0, 0.0, 1e-3], 30, p=[0.5, 0.3, 0.2]), rng.integers(1, 5, 30)))
        p.append(np.array([1e300, 1e-300, 5e-324, 1e300, 1e300, 1e300, 5e-324, 5e-324, 5e-324, 5e-324, 1e-300,
                           1e-300, -1e300, -1e-300, -5e-324, -5e-324, -5e-324, 1e300, -1e300, 5e-324, 0.0, 3.5]))
        out += p
        n += sum(len(a) for a in p)
        if nb is None:
            break
    v = np.concatenate(out)
    return v if nb is None else v[:nb]


def quotes(rng, n):
    """Ordinary quotes: positive, finite, about 3.0 on a 1e-3 grid."""
    bid = 3.0 + 1e-3 * np.abs(np.cumsum(rng.integers(-2, 3, n)) % 400 - 200)
    return bid + 1e-3 * rng.integers(1, 3, n), bid


def plant(seed, target, branch, vol=None, buy_max=None, sell_min=None, first_time=None):
    """Event bars of len(target) bars with per-bar values planted.

    vol_sum of a bar is NaN except one event holding vol (1.0 by default) and vwap_num NaN
    except one event holding the target, so vwap = target / (vol + 1e-9) and equal targets
    give bit-equal vwaps; a target of -0.0 fills all 19 vwap_num with -0.0, since a NaN
    counts as +0.0 in the sum and would erase the sign.  branch (1 .. 4 per bar) selects the
    arm of the label's NaN fallback: p_buy_max / p_sell_min hold one value or none (buy_max /
    sell_min plant that value, else a price near the bid).  first_time plants the trade_time of
    a bar's first event.  Quotes stay ordinary."""
    rng = np.random.default_rng(seed)
    target, branch = np.asarray(target, np.float64), np.asarray(branch)
    nb = len(target)
    n = EVENTS * nb + 1
    ask, bid = quotes(rng, n)
    nan = np.where(rng.random(n) < 0.2, np.nan, 1.0)
    buy, sell = rng.integers(0, 30, n) * 100.0 * nan, rng.integers(0, 30, n) * 100.0 * nan
    ev = {"trade_time": 93000000 + 1000 * np.arange(n, dtype=np.int64), "askprice1": ask, "bidprice1": bid,
          "p_buy_max": np.full(n, np.nan), "p_sell_min": np.full(n, np.nan), "v_buy_sum": buy, "v_sell_sum": sell,
          "vol_sum": np.full(n, np.nan), "trade_count": rng.integers(1, 9, n) * nan, "vwap_num": np.full(n, np.nan)}
    first = EVENTS * np.arange(nb)
    at = lambda: first + rng.integers(0, EVENTS, nb)  # one event of every bar
    ev["vol_sum"][at()] = 1.0 if vol is None else np.asarray(vol, np.float64)
    ev["vwap_num"][at()] = target
    for b in np.nonzero((target == 0) & np.signbit(target))[0]:
        ev["vwap_num"][first[b]:first[b] + EVENTS] = -0.0
    price = np.round(bid[first] + 1e-3 * rng.integers(-1, 3, nb), 3)
    bm = price if buy_max is None else np.asarray(buy_max, np.float64)
    sm_ = price - 1e-3 * rng.integers(0, 3, nb) if sell_min is None else np.asarray(sell_min, np.float64)
    i, j = at(), at()
    ev["p_buy_max"][i] = np.where((branch == 1) | (branch == 3), bm, np.nan)
    ev["p_sell_min"][j] = np.where((branch == 1) | (branch == 2), sm_, np.nan)
    if first_time is not None:
        ev["trade_time"][first] = np.asarray(first_time, np.int64)
    return ev


def rolling_style(seed, nb=None):
    target = rolling_targets(seed, nb)
    return plant(seed + 1000, target, np.random.default_rng(seed + 2000).integers(1, 5, len(target)))


def tie_inputs():
    """(branch, buy_max, sell_min, k) of bars whose label input times 1e4 is exactly k + 0.5.

    Branch 1: x = buy_max - sell_min with sell_min 0.0 (348 of k = 0 .. 399 are exact) and 0.5
    (13 of 400).  Branches 2 and 3 (x = mean ask - sell_min, x = buy_max - mean bid) take the
    free price from a search against the day's own quote means: see ties_day.  Branch 4
    (mean ask - mean bid) has no tie: on the 1e-3 grid 19 * x * 1e4 is ten times an integer,
    never 19 * (k + 0.5), and none of 20 000 bars of these quotes rounded onto one."""
    rows = []
    for s in (0.0, 0.5):
        for k in range(400):
            b = (k + 0.5) / 1e4 + s
            if (b - s) * 1e4 == k + 0.5:
                rows.append((1, b, s, k))
    return rows


def ties_day():
    rows = tie_inputs()
    n1 = len(rows)
    nb = n1 + 400
    branch = np.array([1] * n1 + [2, 3] * 200)
    bm, sl = np.full(nb, np.nan), np.full(nb, np.nan)
    bm[:n1], sl[:n1] = [r[1] for r in rows], [r[2] for r in rows]
    ev = plant(11, np.full(nb, 3.5), branch, buy_max=np.where(np.isnan(bm), 0.0, bm),
               sell_min=np.where(np.isnan(sl), 0.0, sl))
    # branches 2 and 3: the free price that puts x on a tie with this bar's quote mean, if one exists
    import bundle_oracle as bo
    for b in range(n1, nb):
        a = EVENTS * b
        col, other = ("p_sell_min", "askprice1") if branch[b] == 2 else ("p_buy_max", "bidprice1")
        mean = bo.skipna_mean(ev[other][a:a + EVENTS])
        at = a + int(np.nonzero(~np.isnan(ev[col][a:a + EVENTS]))[0][0])
        for k in range(b % 7, 400, 7):
            p = mean - (k + 0.5) / 1e4 if branch[b] == 2 else mean + (k + 0.5) / 1e4
            x = mean - p if branch[b] == 2 else p - mean
            if x * 1e4 == k + 0.5:
                ev[col][at] = p
                break
        else:
            ev[col][at] = np.round(mean, 3)
    return ev


def divisor_for(want):
    """target with target / (1 + 1e-9) == want exactly (vol = 1.0)."""
    t = np.float64(want) * (1.0 + 1e-9)
    for _ in range(8):
        for c in (t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf)):
            if c / (1.0 + 1e-9) == want:
                return float(c)
        t = np.nextafter(t, np.inf if t / (1.0 + 1e-9) < want else -np.inf)
    raise ValueError(want)


CAST_VALUES = (2.0 ** 128, FLT_MAX * (1 + 2.0 ** -25), FLT_MAX + 2.0 ** 103, 2.0 ** -126 * (1 - 2.0 ** -24),
               2.0 ** -149, 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -52), 2.0 ** -151, 1 + 2.0 ** -24,
               1 + 3 * 2.0 ** -24, 2.0 ** -126 * (1 - 2.0 ** -23), 2.0 ** -127, 3 * 2.0 ** -150, 1e39, 1e-46)


def cast_day():
    """f_total_vol holds every CAST_VALUES entry (vol_sum planted, vwap ordinary), then f_vwap_1
    holds each and its negative (vol 1.0, the target divided back exactly)."""
    c = np.array(CAST_VALUES)
    vol = np.concatenate([c, np.ones(2 * len(c)), [1.0, 1.0, 1.0]])
    target = np.concatenate([np.full(len(c), 3.5), [divisor_for(v) for v in c], [-divisor_for(v) for v in c],
                             [3.5, -3.5, 3.5]])
    return plant(21, target, np.random.default_rng(22).integers(1, 5, len(vol)), vol=vol)


HOURS = (93000000, 95959999, 99999999, 100000000, 100000001, 113000000, 130000000, 145959999, 9999999, 10000000,
         0, 2 ** 31 + 93000000, 2 ** 40 + 7, 145959999)


def hours_day():
    nb = len(HOURS)
    return plant(31, np.full(nb, 3.5), np.ones(nb, np.int64), first_time=HOURS)


@functools.lru_cache(maxsize=None)
def day(name):
    if name == "rolling":
        return rolling_style(1)
    if name == "ties":
        return ties_day()
    if name == "cast":
        return cast_day()
    if name == "hours":
        return hours_day()
    if name == "full":
        return rolling_style(7, 4096)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def turns():
    """The days of the joint launch, TURNS bars each, rolling-style from 1023 bars on; the last
    bar of the 1025- and of the 2049-bar day (the only bar of its turn through the workgroup)
    takes fallback arm 4 and 3."""
    days = []
    for k, nb in enumerate(TURNS):
        if nb == 0:
            days.append({c: np.zeros(0, np.int64 if c == "trade_time" else np.float64) for c in sm.EV_COLS})
            continue
        target = rolling_targets(40 + k, nb)
        branch = np.random.default_rng(60 + k).integers(1, 5, nb)
        if nb in (1025, 2049):
            branch[-1] = 4 if nb == 1025 else 3
        days.append(plant(80 + k, target, branch))
    return days


@functools.lru_cache(maxsize=None)
def table(name):
    """(feature_table, stats) of day(name), or of turns()[int(name)]."""
    stats = {}
    ev = turns()[int(name)] if name.isdigit() else day(name)
    return sm.feature_table(ev, stats), stats
