"""The bundle-builder oracle (oracle/bundle_oracle.py) against the reference's
outputs on synthetic days (tests/golden/g6_bundle.npz) and on days with dirty
data -- NaN quotes, non-positive trade prices, window-count and sample-count
boundaries (tests/golden/g11_bundle_edges.npz, gen_golden_bundle_edges.py)."""
import numpy as np
import pytest

import bundle_oracle as bo


def day_inputs(d, k):
    snap = {c[len(f"d{k}_snap_"):]: d[c] for c in d if c.startswith(f"d{k}_snap_")}
    tick = {c[len(f"d{k}_tick_"):]: d[c] for c in d if c.startswith(f"d{k}_tick_")}
    keep = (snap["trade_time"] >= 93000000) & (snap["askprice1"] > 0) & (snap["bidprice1"] > 0)
    snap = {c: v[keep] for c, v in snap.items()}  # agent_trainer.py:27 (inputs are already time-sorted)
    return snap, tick


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def g6(golden):
    return golden("g6_bundle.npz")


def test_event_bars_match_reference(g6):
    for k in range(len(g6["dates"])):
        ev = bo.event_bars(*day_inputs(g6, k))
        for c in bo.EV_COLS:
            assert same(ev[c], g6[f"d{k}_ev_{c}"]), (k, c)


def test_sgu2_windows_match_reference(g6):
    for k in range(len(g6["dates"])):
        ev = {c: g6[f"d{k}_ev_{c}"] for c in bo.EV_COLS}
        X, y = bo.sgu2_windows(bo.bar_mids(ev))
        assert np.array_equal(X, g6[f"d{k}_sgu2_X"]) and np.array_equal(y, g6[f"d{k}_sgu2_y"]), k


def test_step_bundle_matches_load_signals_bundle(g6):
    parts = []
    for k in range(len(g6["dates"])):
        ev = {c: g6[f"d{k}_ev_{c}"] for c in bo.EV_COLS}
        X, _ = bo.sgu2_windows(bo.bar_mids(ev))
        s1 = g6[f"d{k}_sgu1_f0"].astype(np.float32)  # the stand-in m1 of the fixture
        s2 = X[:, -1, 0].astype(np.float32)          # the stand-in m2
        parts.append(bo.step_bundle(ev, s1, s2))
    for j, name in enumerate(("s1", "s2", "mid", "ask", "bid", "buy_max", "sell_min")):
        assert same(np.concatenate([p[j] for p in parts]), g6[f"bundle_{name}"]), name


@pytest.fixture(scope="module")
def g11(golden):
    return golden("g11_bundle_edges.npz")


def test_dirty_days_match_reference(g11):
    """Event bars and SGU2 windows of the g11 days, bit for bit.  The NaN-quote
    days (b_*, c_*) need Series.mean's skip-NaN semantics in bar_mids: a mean
    that is NaN as soon as one quote is NaN gives other windows on all five."""
    tags = [str(t) for t in g11["tags"]]
    assert sum(t[0] in "bc" for t in tags) >= 4
    nan_bars = floored = 0
    for k, tag in enumerate(tags):
        snap = {c[len(f"d{k}_snap_"):]: g11[c] for c in g11 if c.startswith(f"d{k}_snap_")}
        tick = {c[len(f"d{k}_tick_"):]: g11[c] for c in g11 if c.startswith(f"d{k}_tick_")}
        ev = bo.event_bars(snap, tick)
        for c in bo.EV_COLS:
            assert same(ev[c], g11[f"d{k}_ev_{c}"]), (tag, c)
        m = bo.bar_mids(ev)
        nan_bars += int(np.isnan(m).sum())
        floored += int((m < 1e-5).sum())
        X, y = bo.sgu2_windows(m)
        want_X, want_y = g11[f"d{k}_sgu2_X"], g11[f"d{k}_sgu2_y"]
        assert X.shape == want_X.shape and np.array_equal(X, want_X), tag
        assert y.shape == want_y.shape and np.array_equal(y, want_y), tag
    assert nan_bars > 0 and floored > 0  # the forward fill and the 1e-5 floor ran
    assert [len(g11[f"d{tags.index(t)}_sgu2_y"]) for t in ("d_bars11", "d_bars12", "d_bars13")] == [0, 1, 2]
