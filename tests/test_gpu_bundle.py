"""GPU tests of the bundle builder: libsgmm.so's
event-bar / SGU2-window / step-bundle kernels against the reference's own
outputs (tests/golden/g6_bundle.npz) and against oracle/bundle_oracle.py on
seeded synthetic days with the edge cases the reference's data can hold; the
branches only dirty data reaches (NaN quotes, floored bars, forward fill,
nan_to_num, the bars-per-day guard, more than one x-block of step samples)
against tests/golden/g11_bundle_edges.npz and the oracle.
Bit-exact throughout (float64 columns, float32 windows)."""
import numpy as np
import pandas as pd
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

NAMES = ("s1", "s2", "mid", "ask", "bid", "buy_max", "sell_min")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.astype(np.float64), b.astype(np.float64), equal_nan=True)


@pytest.fixture(scope="module")
def g6(golden):
    return golden("g6_bundle.npz")


def golden_days(g6):
    from sgmm_amd.bundle import _filter_sort
    days = []
    for k in range(len(g6["dates"])):
        snap = pd.DataFrame({c[len(f"d{k}_snap_"):]: g6[c] for c in g6 if c.startswith(f"d{k}_snap_")})
        tick = pd.DataFrame({c[len(f"d{k}_tick_"):]: g6[c] for c in g6 if c.startswith(f"d{k}_tick_")})
        days.append(_filter_sort(snap, tick))
    return days


def test_event_bars_match_reference(sgmm, g6):
    from sgmm_amd.bundle import EV_COLS, event_bars
    ev = event_bars(golden_days(g6))
    for k in range(len(g6["dates"])):
        day = ev.day(k)
        for c in EV_COLS:
            assert same(day[c], g6[f"d{k}_ev_{c}"]), (k, c)


def test_sgu2_windows_match_reference(sgmm, g6):
    from sgmm_amd.bundle import event_bars
    wins = event_bars(golden_days(g6)).windows()
    for k, (X, y) in enumerate(wins):
        assert str(X.dtype) == "torch.float32"
        assert np.array_equal(X.cpu().numpy(), g6[f"d{k}_sgu2_X"]), k
        assert np.array_equal(y.cpu().numpy(), g6[f"d{k}_sgu2_y"]), k


class M1:
    def predict(self, X):
        return np.asarray(X.iloc[:, 0].values, dtype=np.float32)


class M2:
    def predict(self, X):
        return np.asarray(X[:, -1, 0], dtype=np.float32).reshape(-1, 1)


class Identity:
    def transform(self, X):
        return X


def test_load_signals_bundle_matches_reference(sgmm, g6, tmp_path):
    """The drop-in load_signals_bundle on parquet files (the reference's own
    layout data/{symbol}/{snap,tick}/{date}.parquet) with the fixture's
    stand-in models, against the reference's 7-tuple."""
    from sgmm_amd.bundle import load_signals_bundle
    dates = [str(d) for d in g6["dates"]]
    for k, d in enumerate(dates):
        for kind in ("snap", "tick"):
            p = tmp_path / "data" / "SYN" / kind
            p.mkdir(parents=True, exist_ok=True)
            pd.DataFrame({c[len(f"d{k}_{kind}_"):]: g6[c] for c in g6 if c.startswith(f"d{k}_{kind}_")}) \
                .to_parquet(p / f"{d}.parquet")
    f0 = iter([g6[f"d{k}_sgu1_f0"] for k in range(len(dates))])

    def sgu1_features(bars):  # the fixture pins SGU1's first feature column (days in order)
        v = next(f0)
        return pd.DataFrame({"f0": v, "label": np.zeros(len(v))})

    out = load_signals_bundle("SYN", dates, M1(), M2(), Identity(), sgu1_features=sgu1_features,
                              data_root=str(tmp_path))
    for name, a in zip(NAMES, out):
        assert same(a, g6[f"bundle_{name}"]), name


def synthetic(seed, n_snap, n_tick, t_lo=93000000):
    rng = np.random.default_rng(seed)
    st = np.sort(rng.integers(t_lo, t_lo + 6_000_000, n_snap)).astype(np.int64)
    bid = 3.4 + 0.001 * np.cumsum(rng.choice([-1, 0, 0, 1], n_snap))
    ask = bid + 0.001 * rng.choice([1, 1, 1, 2], n_snap)
    bv = rng.integers(1, 5, n_snap) * 100.0
    av = rng.integers(1, 5, n_snap) * 100.0
    rep = rng.random(n_snap) < 0.4
    for i in range(1, n_snap):
        if rep[i]:
            bid[i], ask[i], bv[i], av[i] = bid[i - 1], ask[i - 1], bv[i - 1], av[i - 1]
    tt = np.sort(rng.integers(t_lo - 100_000, t_lo + 6_100_000, n_tick)).astype(np.int64)
    tt[1::5] = tt[0:-1:5]
    tt = np.sort(tt)
    side = rng.choice([-1, 1], n_tick).astype(np.int32)
    price = np.round(3.4 + 0.01 * rng.standard_normal(n_tick), 3)
    price[rng.random(n_tick) < 0.01] = np.nan
    vol = rng.integers(1, 30, n_tick) * 100.0
    snap = {"trade_time": st, "bidprice1": bid, "askprice1": ask, "bidvol1": bv, "askvol1": av}
    tick = {"trade_time": tt, "Price": price, "Volume": vol, "side": side}
    return snap, tick


def edge_days():
    days = [synthetic(1, 5000, 20000), synthetic(2, 3000, 0), synthetic(3, 1, 7), synthetic(4, 400, 3),
            synthetic(5, 2100, 9000, t_lo=93000000)]
    s, t = synthetic(6, 600, 2000)
    for c in ("bidprice1", "askprice1", "bidvol1", "askvol1"):
        s[c][:] = s[c][0]  # one event all day
    days.append((s, t))
    s, t = synthetic(7, 700, 1500)
    t["trade_time"] = t["trade_time"] + 10_000_000  # every trade after the last snapshot
    days.append((s, t))
    s, t = synthetic(8, 19 * 12 + 1, 500)  # exactly 12 bars boundary
    for c in ("bidprice1",):
        s[c] = 3.0 + 0.001 * np.arange(len(s[c]))  # every row an event
    days.append((s, t))
    return days


@pytest.fixture(scope="module")
def edge():
    import bundle_oracle as bo
    days = edge_days()
    return days, [bo.event_bars(s, t) for s, t in days]


def test_event_bars_match_oracle_edge_cases(sgmm, edge):
    from sgmm_amd.bundle import EV_COLS, event_bars
    days, want = edge
    ev = event_bars(days)
    for k, w in enumerate(want):
        got = ev.day(k)
        assert len(got["trade_time"]) == len(w["trade_time"]), k
        for c in EV_COLS:
            assert same(got[c], w[c]), (k, c)


def test_windows_and_steps_match_oracle_edge_cases(sgmm, edge):
    import bundle_oracle as bo
    from sgmm_amd.bundle import event_bars
    days, want = edge
    ev = event_bars(days)
    wins = ev.windows()
    n_samples, parts = [], []
    for k, w in enumerate(want):
        X, y = bo.sgu2_windows(bo.bar_mids(w))
        gx, gy = wins[k]
        assert gx.shape[0] == (X.shape[0] if X.ndim == 3 else 0), k
        if X.ndim == 3:
            assert np.array_equal(gx.cpu().numpy(), X) and np.array_equal(gy.cpu().numpy(), y), k
        total = (len(w["trade_time"]) + 18) // 19
        ns = [0, total, max(total - 3, 0), total + 5][k % 4]
        n_samples.append(ns)
        if ns > 0:  # n_samples 0 = a skipped day (agent_trainer.py:33-41)
            sig = np.zeros(ns, np.float32)
            p = bo.step_bundle(w, sig, sig)
            parts.append(p[2:])
    (mid, ask, bid, bmax, smin), n_steps = ev.steps(n_samples)
    assert int(n_steps.sum()) == mid.shape[0]
    for j, g in enumerate((mid, ask, bid, bmax, smin)):
        want_j = np.concatenate([p[j] for p in parts]) if parts else np.zeros(0)
        assert same(g.cpu().numpy(), want_j), j


def test_bundle_many_days_one_launch(sgmm, g6):
    """All days of a request go through one launch per kernel: 64 copies of
    the golden days give 64 copies of the reference's event bars."""
    from sgmm_amd.bundle import EV_COLS, event_bars
    days = golden_days(g6)
    ev = event_bars(days * 16)
    for r in range(16):
        for k in range(len(days)):
            day = ev.day(r * len(days) + k)
            for c in EV_COLS:
                assert same(day[c], g6[f"d{k}_ev_{c}"]), (r, k, c)


# ---- dirty data: tests/golden/g11_bundle_edges.npz (gen_golden_bundle_edges.py) ----

@pytest.fixture(scope="module")
def g11(golden):
    return golden("g11_bundle_edges.npz")


@pytest.fixture(scope="module")
def dirty(g11):
    """(tags, days as handed to HFTMarketBase, the oracle's event bars)."""
    import bundle_oracle as bo
    tags = [str(t) for t in g11["tags"]]
    days = []
    for k in range(len(tags)):
        snap = {c[len(f"d{k}_snap_"):]: g11[c] for c in g11 if c.startswith(f"d{k}_snap_")}
        tick = {c[len(f"d{k}_tick_"):]: g11[c] for c in g11 if c.startswith(f"d{k}_tick_")}
        days.append((snap, tick))
    return tags, days, [bo.event_bars(s, t) for s, t in days]


def test_dirty_days_event_bars(sgmm, g11, dirty):
    from sgmm_amd.bundle import EV_COLS, event_bars
    tags, days, want = dirty
    ev = event_bars(days)
    for k, tag in enumerate(tags):
        got = ev.day(k)
        for c in EV_COLS:
            assert same(got[c], g11[f"d{k}_ev_{c}"]), (tag, c, "reference")
            assert same(got[c], want[k][c]), (tag, c, "oracle")


def test_dirty_days_windows(sgmm, g11, dirty):
    """Forward fill, the leading NaN bar, the 1e-5 floor and the skip-NaN mean
    fallbacks against the reference's gen_dataset(19, 10) and the oracle."""
    import bundle_oracle as bo
    from sgmm_amd.bundle import event_bars
    tags, days, want = dirty
    wins = event_bars(days).windows()
    for k, tag in enumerate(tags):
        gx, gy = (t.cpu().numpy() for t in wins[k])
        ref_X, ref_y = g11[f"d{k}_sgu2_X"], g11[f"d{k}_sgu2_y"]
        X, y = bo.sgu2_windows(bo.bar_mids(want[k]))
        assert gy.shape == ref_y.shape == y.shape, tag
        assert gx.dtype == np.float32 and gx.shape == (len(ref_y), 10, 1), tag
        if len(ref_y):
            assert np.array_equal(gx, ref_X) and np.array_equal(gy, ref_y), (tag, "reference")
            assert np.array_equal(gx, X) and np.array_equal(gy, y), (tag, "oracle")
    n_win = {t: len(wins[k][1]) for k, t in enumerate(tags)}
    assert [n_win[t] for t in ("d_bars11", "d_bars12", "d_bars13")] == [0, 1, 2]
    a = wins[tags.index("a_floor")][0].cpu().numpy()
    assert np.abs(a).max() > 1e5  # a bar floored to 1e-5 and the return that leaves it


@pytest.mark.parametrize("n_samples", [1, 2, None])
def test_dirty_days_steps(sgmm, dirty, n_samples):
    """1, 2 and all sampled events of every day (the e_* days hold 19k, 19k + 1
    and 19k + 18 events) against agent_trainer's step loop in the oracle."""
    import bundle_oracle as bo
    from sgmm_amd.bundle import event_bars
    tags, days, want = dirty
    ev = event_bars(days)
    totals = [(len(w["trade_time"]) + 18) // 19 for w in want]
    assert [totals[tags.index(t)] for t in ("e_19k", "e_19k1", "e_19k18")] == [15, 16, 16]
    ns = [n_samples or t for t in totals]
    parts = [bo.step_bundle(w, np.zeros(n, np.float32), np.zeros(n, np.float32))[2:] for w, n in zip(want, ns)]
    got, n_steps = ev.steps(ns)
    assert n_steps.tolist() == [n - 1 for n in ns]
    for j, g in enumerate(got):
        assert same(g.cpu().numpy(), np.concatenate([p[j] for p in parts])), j


def test_infinite_bar_becomes_flt_max(sgmm, dirty):
    """nan_to_num's +inf -> FLT_MAX store needs a bar mid beyond float32, which
    the reference fixture cannot hold (its parity domain ends far below), so
    this is pinned by the oracle alone: the traded extremes of one bar are
    overwritten on the device with 1e39 and k_bar_windows runs on those columns."""
    import bundle_oracle as bo
    from sgmm_amd.bundle import event_bars
    tags, days, _ = dirty
    ev = event_bars([days[tags.index("e_19k18")]])
    for c in ("p_buy_max", "p_sell_min"):
        ev.cols[c][19 * 12:19 * 13] = 1e39
    (gx, gy), = ev.windows()
    with np.errstate(over="ignore", invalid="ignore"):
        X, y = bo.sgu2_windows(bo.bar_mids(ev.day(0)))
    assert np.array_equal(gx.cpu().numpy(), X) and np.array_equal(gy.cpu().numpy(), y)
    assert (X == np.finfo(np.float32).max).any() and (y == np.finfo(np.float32).max).any()
    assert np.all(np.isfinite(X)) and not (X == -np.finfo(np.float32).max).any()


def all_events_day(n):
    """Every snapshot row an event, one trade per 50 rows at that row's time:
    the event bars are the snapshot itself with the as-of trade beside it."""
    rng = np.random.default_rng(n)
    t = 93000000 + np.arange(n, dtype=np.int64)
    bid = 3.0 + 0.001 * np.cumsum(rng.integers(1, 3, n))
    ask = bid + 0.001 * rng.integers(1, 3, n)
    vol = rng.integers(1, 5, n) * 100.0
    snap = {"trade_time": t, "bidprice1": bid, "askprice1": ask, "bidvol1": vol, "askvol1": vol}
    at = np.arange(0, n, 50)
    side = rng.choice([-1, 1], len(at)).astype(np.int32)
    price = np.round(bid[at] + 0.001 * side, 3)
    tv = rng.integers(1, 30, len(at)) * 100.0
    tick = {"trade_time": t[at], "Price": price, "Volume": tv, "side": side}
    j = np.arange(n) // 50
    nan = np.full(len(at), np.nan)
    ev = {"trade_time": t, "askprice1": ask, "bidprice1": bid,
          "p_buy_max": np.where(side == 1, price, nan)[j], "p_sell_min": np.where(side == -1, price, nan)[j],
          "v_buy_sum": np.where(side == 1, tv, 0.0)[j], "v_sell_sum": np.where(side == -1, tv, 0.0)[j],
          "vol_sum": tv[j], "trade_count": np.ones(n), "vwap_num": (price * tv)[j]}
    return (snap, tick), ev


def test_day_of_4096_bars(sgmm):
    """The most bars a day may hold (19 * 4096 + 1 events): windows against the
    oracle, and all 4 097 samples through k_step_bundle, 16 x-blocks of 256."""
    import bundle_oracle as bo
    from sgmm_amd.bundle import EV_COLS, event_bars
    n = 19 * 4096 + 1
    day, want = all_events_day(n)
    ev = event_bars([day])
    got = ev.day(0)
    for c in EV_COLS:
        assert same(got[c], want[c]), c
    (gx, gy), = ev.windows()
    X, y = bo.sgu2_windows(bo.bar_mids(want))
    assert X.shape == (4096 - 11, 10, 1)
    assert np.array_equal(gx.cpu().numpy(), X) and np.array_equal(gy.cpu().numpy(), y)
    total = (n + 18) // 19
    assert total == 4097
    sig = np.zeros(total, np.float32)
    parts = bo.step_bundle(want, sig, sig)[2:]
    steps, n_steps = ev.steps([total])
    assert n_steps.tolist() == [4096]
    for j, g in enumerate(steps):
        assert same(g.cpu().numpy(), parts[j]), j


def test_day_of_4097_bars_is_refused(sgmm):
    """One bar more than the LDS arrays hold: windows() raises, and the kernel
    itself, launched past the host check, returns before indexing -- it marks
    the day with -1 and writes no window."""
    import ctypes
    import torch
    from sgmm_amd import _lib
    from sgmm_amd._lib import ptr, stream_ptr
    from sgmm_amd.bundle import event_bars
    n = 19 * 4097 + 1
    day, _ = all_events_day(n)
    ev = event_bars([day])
    assert int(ev.n_events[0]) == n
    with pytest.raises(_lib.SgmmError):
        ev.windows()
    sentinel = -1234.5
    X = torch.full((n // 19 + 1, 10), sentinel, dtype=torch.float32, device="cuda")
    y = torch.full((n // 19 + 1,), sentinel, dtype=torch.float32, device="cuda")
    nw = torch.zeros(1, dtype=torch.int32, device="cuda")
    win_off = torch.zeros(2, dtype=torch.int64, device="cuda")
    rc = ev.L.sgmm_bar_windows(ctypes.byref(ev.bars), 1, ptr(ev._in["snap_off"]), ptr(win_off), ptr(X), ptr(y),
                               ptr(nw), 0, stream_ptr())
    assert rc == 0
    assert nw.cpu().tolist() == [-1]
    assert bool((X == sentinel).all()) and bool((y == sentinel).all())
