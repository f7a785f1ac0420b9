"""GPU tests of SGU1 on the device: sgmm_sgu1_features
against the reference's own SGU1DataPro.gen_dataset(19) tables
(tests/golden/g14_sgu1.npz, gen_golden_sgu1.py), sgmm_sgu1_predict against the
independent evaluator of tests/sgu1_model.py, and load_signals_bundle with
the table and the forest on the device.

Bit-exact throughout, except f_slope_3 / f_slope_5: the reference's
np.polyfit (LAPACK SVD) cannot be pinned bit for bit, so the kernel's closed
form and the reference are both held within 4 * 2^-52 * max|mid| of the exact
(fractions.Fraction) least-squares slope of the window's float64 mids -- the
closed forms take at most 4 roundings of intermediates <= 8 * max|mid| and a
division by 10.  Measured on an MI355X over the fixture days: kernel worst
0.0004 * 2^-52 * max|mid| (differences of neighbouring mids are exact),
reference worst 1.54 * 2^-52 * max|mid|.  Where the exact slope vanishes (a flat
or a symmetric window) the kernel gives exactly +0.0 (or the last-bit noise
of the mids) and polyfit +-1e-16: the one place the float32 matrices differ
(30 slope entries of the fixture), asserted to be confined to slopes below
one ulp of the mids.

The fixture days leave most value-dependent branches of the feature kernel
untaken; the generated edge days of tests/sgu1_feature_cases.py (which
tests/test_sgu1_model.py holds to pandas on the CPU) carry them through it and
are compared with the model byte for byte, the sign of a zero included.
Kernel variants run once on an MI355X against these tests: without the "all
equal" override of the rolling mean the rolling, ties, hours, turns and full
days fail, without the two clamps the rolling, turns and full days, with
floor(x * 1e4 + 0.5) for rint the ties, turns and full days, and with float32
denormals flushed the cast day; none of the first three failed a test of the
fixture days."""
import ctypes
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import sgu1_feature_cases as fc
import sgu1_model as sm
from conftest import has_gpu

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

ARR = ("left", "right", "feat", "value", "default_left", "tree_off")
NAMES = ("s1", "s2", "mid", "ask", "bid", "buy_max", "sell_min")
SLOPES = (9, 10)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.astype(np.float64), b.astype(np.float64), equal_nan=True)


def same_bytes(a, b):
    """Equal shape, type and bytes: array_equal would hide the sign of a zero."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def cast32(F):
    """numpy's float64 -> float32 cast (to nearest even; inf past FLT_MAX + half an ulp)."""
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(F, np.float64).astype(np.float32)


@pytest.fixture(scope="module")
def g14(golden):
    return golden("g14_sgu1.npz")


@pytest.fixture(scope="module")
def g6(golden):
    return golden("g6_bundle.npz")


def fixture_bars(g14):
    return [{c: g14[f"d{k}_ev_{c}"] for c in sm.EV_COLS} for k in range(len(g14["tags"]))]


@pytest.fixture(scope="module")
def table(sgmm, g14):
    """Every fixture day through one launch: (EventBarsGPU, per-day F64 [rows, 20], X, label)."""
    from sgmm_amd.bundle import EventBarsGPU
    ev = EventBarsGPU.from_bars(fixture_bars(g14))
    views = ev.sgu1_table()
    days = []
    for d, (X, label) in enumerate(views):
        a, n = int(ev.sgu1_row_off[d]), int(ev.sgu1_n_rows[d])
        days.append((ev.sgu1_F64[:, a:a + n].cpu().numpy().T, X.cpu().numpy().T, label.cpu().numpy()))
    return ev, days


def test_feature_table_matches_reference(g14, table):
    ev, days = table
    for k, tag in enumerate(g14["tags"]):
        want = g14[f"d{k}_table"]
        F64, X, label = days[k]
        assert F64.shape == (len(want), 20) and X.shape == (len(want), 20) and label.shape == (len(want),), tag
        assert X.dtype == np.float32 and F64.dtype == np.float64
        if not len(want):
            continue
        for j in range(20):
            if j not in SLOPES:
                assert np.array_equal(F64[:, j], want[:, j]), (tag, sm.FEATURES[j])
                assert np.array_equal(X[:, j], want[:, j].astype(np.float32)), (tag, sm.FEATURES[j])
        assert np.array_equal(label, want[:, 20]), tag
        assert np.array_equal(X, F64.astype(np.float32)), tag  # float64 rounded to nearest even, f_hour int -> float
        # the same rules in numpy: every column bit for bit, the closed-form slopes included
        assert np.array_equal(F64, sm.feature_table(fixture_bars(g14)[k])[:, :20]), tag
    assert [len(days[list(g14["tags"]).index(t)][0]) for t in ("bars5", "bars6", "events19", "events20")] == [0, 6, 0, 0]
    assert ev.sgu1_n_rows.tolist() == [len(g14[f"d{k}_table"]) for k in range(len(g14["tags"]))]


def test_slopes_within_bound_of_exact(g14, table):
    _, days = table
    worst_k = worst_r = 0.0
    flat = cast_diff = 0
    for k, tag in enumerate(g14["tags"]):
        want, (F64, X, _) = g14[f"d{k}_table"], days[k]
        if not len(want):
            continue
        mid = sm.bar_mids(fixture_bars(g14)[k])
        for s, j in ((3, 9), (5, 10)):
            for r, y in enumerate(sm.window_slopes(mid, s)):
                exact, unit = sm.slope_exact(y), 2.0 ** -52 * float(np.abs(y).max())
                ek = abs(float(Fraction(float(F64[r, j])) - exact)) / unit
                er = abs(float(Fraction(float(want[r, j])) - exact)) / unit
                worst_k, worst_r = max(worst_k, ek), max(worst_r, er)
                assert ek <= 4 and er <= 4, (tag, j, r, ek, er)
                if np.all(y == y[0]):  # a flat window: exactly +0.0
                    flat += 1
                    assert F64[r, j] == 0.0 and not np.signbit(F64[r, j]) and not np.signbit(X[r, j]), (tag, j, r)
                if X[r, j] != np.float32(want[r, j]):  # only where the slope vanishes
                    cast_diff += 1
                    assert abs(float(exact)) <= unit, (tag, j, r, float(exact))
        assert np.all(F64[:, 8] == 0.0) and not np.signbit(F64[:, 8]).any()  # f_slope_1
    print(f"worst |slope - exact| / (2^-52 max|mid|): kernel {worst_k:.4f}, reference {worst_r:.4f}; "
          f"{flat} flat windows, {cast_diff} float32 casts differ")
    assert flat > 0 and cast_diff > 0


def test_frame_is_the_references(g14, table):
    ev, _ = table
    df = ev.sgu1_frame(0)
    assert tuple(df.columns) == sm.FEATURES + ("label",)
    assert df["f_hour"].dtype == np.int64 and all(df[c].dtype == np.float64 for c in df.columns if c != "f_hour")
    want = g14["d0_table"]
    assert np.array_equal(df["f_hour"].to_numpy(), want[:, 19].astype(np.int64))
    for j, c in enumerate(df.columns):
        if j not in SLOPES:
            assert np.array_equal(df[c].to_numpy(np.float64), want[:, j]), c
    assert len(ev.sgu1_frame(4)) == 0 and tuple(ev.sgu1_frame(4).columns) == sm.FEATURES + ("label",)


def test_one_launch_equals_day_by_day(g14, table):
    from sgmm_amd.bundle import EventBarsGPU
    _, days = table
    for k, bars in enumerate(fixture_bars(g14)):
        one = EventBarsGPU.from_bars([bars])
        (X, label), = one.sgu1_table()
        assert np.array_equal(X.cpu().numpy().T, days[k][1]) and np.array_equal(label.cpu().numpy(), days[k][2]), k
        a, n = 0, int(one.sgu1_n_rows[0])
        assert np.array_equal(one.sgu1_F64[:, a:a + n].cpu().numpy().T, days[k][0]), k


# ---------------------------------------------------------------- the edge days (sgu1_feature_cases.py)

def launch(bars):
    """One launch: (EventBarsGPU, per day (F64 [rows, 20], X [rows, 20], label [rows]))."""
    from sgmm_amd.bundle import EventBarsGPU
    ev = EventBarsGPU.from_bars(bars)
    days = []
    for d, (X, label) in enumerate(ev.sgu1_table()):
        a, n = int(ev.sgu1_row_off[d]), int(ev.sgu1_n_rows[d])
        days.append((ev.sgu1_F64[:, a:a + n].cpu().numpy().T, X.cpu().numpy().T, label.cpu().numpy()))
    return ev, days


def assert_day_is_the_models(got, want, tag):
    """The float64 table, the label and the float32 matrix, byte for byte, column by column."""
    F64, X, label = got
    assert F64.shape == (len(want), 20) and X.shape == (len(want), 20) and label.shape == (len(want),), tag
    assert F64.dtype == np.float64 and X.dtype == np.float32 and label.dtype == np.float64
    want32 = cast32(want[:, :20])
    for j in range(20):
        bad = np.nonzero(F64[:, j].view(np.uint64) != want[:, j].view(np.uint64))[0]
        assert not len(bad), (tag, sm.FEATURES[j], len(bad), bad[:5], F64[bad[:5], j], want[bad[:5], j])
        bad = np.nonzero(X[:, j].view(np.uint32) != want32[:, j].view(np.uint32))[0]
        assert not len(bad), (tag, sm.FEATURES[j], "float32", len(bad), bad[:5], X[bad[:5], j], want32[bad[:5], j])
    assert same_bytes(label, want[:, 20]), tag
    assert same_bytes(F64, want[:, :20]) and same_bytes(X, want32), tag


@pytest.mark.parametrize("name", ["rolling", "ties", "cast", "hours"])
def test_edge_day_is_the_models(sgmm, name):
    """Each edge day through the kernel: calc_mean's three overrides and the signbit count
    (rolling), rint on exact ties (ties), the float32 cast at overflow, subnormals, underflow
    and halfway cases (cast), the integer division of trade_time (hours)."""
    want, _ = fc.table(name)
    ev, days = launch([fc.day(name)])
    assert ev.sgu1_n_rows.tolist() == [len(want)]
    assert_day_is_the_models(days[0], want, name)
    if name == "rolling":  # the closed-form slopes against the exact least-squares slope
        mid = sm.bar_mids(fc.day(name))
        for s, j in ((3, 9), (5, 10)):
            for r, y in enumerate(sm.window_slopes(mid, s)):
                bound = 4 * 2.0 ** -52 * float(np.abs(y).max())
                assert abs(float(Fraction(float(days[0][0][r, j])) - sm.slope_exact(y))) <= bound, (j, r)
    if name == "hours":
        df = ev.sgu1_frame(0)
        assert df["f_hour"].dtype == np.int64
        assert df["f_hour"].tolist() == [t // 10 ** 7 for t in fc.HOURS]


def test_turns_in_one_launch_and_alone(sgmm):
    """6, 7, 1023, 1024, 1025, 2048 and 2049 bars in one launch, a 5-bar and an empty day
    between them: every day is the model's, and a day launched alone has the same bytes."""
    bars = fc.turns()
    ev, days = launch(bars)
    assert ev.sgu1_n_rows.tolist() == [nb if nb >= 6 else 0 for nb in fc.TURNS]
    for k, nb in enumerate(fc.TURNS):
        if nb < 6:
            assert days[k][0].shape == (0, 20) and days[k][2].shape == (0,)
            continue
        assert_day_is_the_models(days[k], fc.table(str(k))[0], nb)
        _, alone = launch([bars[k]])
        assert all(same_bytes(a, b) for a, b in zip(alone[0], days[k])), nb


def sentinel_launch(bars, want, whole=()):
    """One launch with gaps between the days and behind the last: rows outside
    row_off[d] .. +n_rows[d] stay untouched in X, F64 and label, for every feature; without F64
    the float32 matrix has the same bytes.  want: per day the table [rows, 21]; the days listed
    in ``whole`` are held to it on every column, byte for byte."""
    import torch
    from sgmm_amd._lib import check, ptr, stream_ptr
    from sgmm_amd.bundle import EventBarsGPU
    ev = EventBarsGPU.from_bars(bars)
    n = [len(w) for w in want]
    gap = 3
    row_off = np.concatenate([[gap], gap + np.cumsum([v + gap for v in n])]).astype(np.int64)
    ld = int(row_off[-1]) + 5
    S = -1234.5
    outs = []
    for with_f64 in (True, False):
        X = torch.full((20, ld), S, dtype=torch.float32, device="cuda")
        F = torch.full((20, ld), S, dtype=torch.float64, device="cuda")
        lab = torch.full((ld,), S, dtype=torch.float64, device="cuda")
        nr = torch.full((len(bars) + 2,), -77, dtype=torch.int32, device="cuda")
        ro = torch.from_numpy(row_off).to("cuda")
        check(ev.L.sgmm_sgu1_features(ctypes.byref(ev.bars), len(bars), ptr(ev._in["snap_off"]), ptr(ro), 4096, ld,
                                      ptr(X), ptr(lab), ptr(F) if with_f64 else None, ptr(nr), stream_ptr()),
              "sgmm_sgu1_features")
        X, F, lab, nr = X.cpu().numpy(), F.cpu().numpy(), lab.cpu().numpy(), nr.cpu().numpy()
        assert nr.tolist() == n + [-77, -77]
        inside = np.zeros(ld, bool)
        for d in range(len(bars)):
            rows = slice(row_off[d], row_off[d] + n[d])
            inside[rows] = True
            if n[d]:
                assert np.array_equal(lab[rows], want[d][:, 20])
                assert np.array_equal(X[0, rows], want[d][:, 0].astype(np.float32))
            if d in whole:
                assert same_bytes(lab[rows], want[d][:, 20]), d
                assert same_bytes(X[:, rows].T, cast32(want[d][:, :20])), (d, with_f64)
                assert not with_f64 or same_bytes(F[:, rows].T, want[d][:, :20]), d
        assert np.all(X[:, ~inside] == S) and np.all(lab[~inside] == S)
        assert np.all(X[:, inside] != S) and np.all(lab[inside] != S)
        assert np.all(F[:, ~inside] == S) and (np.all(F[:, inside] != S) if with_f64 else np.all(F == S))
        outs.append(X)
    assert np.array_equal(outs[0], outs[1]) and outs[0].tobytes() == outs[1].tobytes()


def test_sentinels_behind_every_output(sgmm, g14):
    """Rows outside row_off[d] .. +n_rows[d] stay untouched in X, F64 and label, for every
    feature; without F64 the float32 matrix is the same."""
    bars = fixture_bars(g14)
    sentinel_launch(bars, [g14[f"d{k}_table"] for k in range(len(bars))])


def test_sentinels_with_an_edge_day_among_the_fixture_days(sgmm, g14):
    """The same launch with the rolling day between the fixture days: strides and gaps with
    signed zeros, 1e300 and subnormal vwaps, with and without F64."""
    bars = fixture_bars(g14)
    want = [g14[f"d{k}_table"] for k in range(len(bars))]
    bars.insert(2, fc.day("rolling"))
    want.insert(2, fc.table("rolling")[0])
    sentinel_launch(bars, want, whole=(2,))


def all_events_bars(nb, seed=0):
    """Event bars of nb bars (19 * nb + 1 events), trades on most events."""
    rng = np.random.default_rng(seed)
    n = 19 * nb + 1
    bid = 3.0 + 0.001 * np.cumsum(rng.integers(-2, 3, n))
    ask = bid + 0.001 * rng.integers(1, 3, n)
    nan = np.where(rng.random(n) < 0.2, np.nan, 1.0)
    vol = rng.integers(1, 30, n) * 100.0
    buy = rng.integers(0, 30, n) * 100.0
    price = np.round(bid + 0.001 * rng.integers(-1, 3, n), 3)
    return {"trade_time": 93000000 + 1000 * np.arange(n, dtype=np.int64), "askprice1": ask, "bidprice1": bid,
            "p_buy_max": price * np.where(rng.random(n) < 0.5, nan, np.nan), "p_sell_min": (price - 0.001) * nan,
            "v_buy_sum": np.minimum(buy, vol) * nan, "v_sell_sum": (vol - np.minimum(buy, vol)) * nan,
            "vol_sum": vol * nan, "trade_count": rng.integers(1, 9, n) * nan, "vwap_num": price * vol * nan}


def test_more_bars_than_threads(sgmm):
    """1 100 bars: every per-bar loop of the 1 024-thread workgroup takes a second turn."""
    from sgmm_amd.bundle import EventBarsGPU
    bars = all_events_bars(1100, seed=3)
    ev = EventBarsGPU.from_bars([bars])
    (X, label), = ev.sgu1_table()
    want = sm.feature_table(bars)
    assert ev.sgu1_n_rows.tolist() == [1100]
    assert np.array_equal(ev.sgu1_F64[:, :1100].cpu().numpy().T, want[:, :20])
    assert np.array_equal(label.cpu().numpy(), want[:, 20])
    assert np.array_equal(X.cpu().numpy().T, want[:, :20].astype(np.float32))


def test_bars_per_day_guard(sgmm):
    """4 096 bars are the most a day may hold; one more reports -1 and writes nothing, also
    when the kernel is launched past the host check."""
    import torch
    from sgmm_amd import _lib
    from sgmm_amd._lib import ptr, stream_ptr
    from sgmm_amd.bundle import EventBarsGPU
    ev = EventBarsGPU.from_bars([all_events_bars(4096), all_events_bars(7, seed=1)])
    ev.sgu1_table()
    assert ev.sgu1_n_rows.tolist() == [4096, 7]
    # a full day of edge values: the last LDS slot of every per-bar array, 4096-step serial chains
    ev, days = launch([fc.day("full")])
    assert ev.sgu1_n_rows.tolist() == [4096]
    assert_day_is_the_models(days[0], fc.table("full")[0], "full")
    ev = EventBarsGPU.from_bars([all_events_bars(4097)])
    with pytest.raises(_lib.SgmmError):
        ev.sgu1_table()
    S = -1234.5
    X = torch.full((20, 4200), S, dtype=torch.float32, device="cuda")
    lab = torch.full((4200,), S, dtype=torch.float64, device="cuda")
    nr = torch.zeros(1, dtype=torch.int32, device="cuda")
    ro = torch.zeros(2, dtype=torch.int64, device="cuda")
    rc = ev.L.sgmm_sgu1_features(ctypes.byref(ev.bars), 1, ptr(ev._in["snap_off"]), ptr(ro), 0, 4200, ptr(X),
                                 ptr(lab), None, ptr(nr), stream_ptr())
    assert rc == 0 and nr.cpu().tolist() == [-1]
    assert bool((X == S).all()) and bool((lab == S).all())


# ---------------------------------------------------------------- the forest

@pytest.fixture(scope="module")
def real(sgmm, g14):
    from sgmm_amd.gate_units import SGU1Forest
    f = SGU1Forest.from_arrays(*[g14[f"forest_{n}"] for n in ARR], g14["forest_base_score"],
                               int(g14["forest_best_iteration"]))
    X = np.concatenate([g14[f"d{k}_table"][:, :20] for k in range(4)]).astype(np.float32)
    return f, X


def test_real_forest_on_fixture_rows(g14, real):
    f, X = real
    assert (f.n_trees, len(f.tree_off) - 1, f.depth) == (278, 298, 4)
    got = f.predict(X)
    assert got.dtype == np.float32 and np.array_equal(got, g14["pred_best"])
    assert np.array_equal(f.predict(X, n_trees=298), g14["pred_all"])
    leaf = f.pred_leaf(X, n_trees=298)
    assert leaf.dtype == np.int32 and np.array_equal(leaf, g14["leaf"])
    assert np.array_equal(f.pred_leaf(X), g14["leaf"][:, :278])
    assert np.array_equal(f.predict(pd.DataFrame(X.astype(np.float64), columns=list(sm.FEATURES))), g14["pred_best"])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1000])
def test_row_counts(g14, real, n):
    f, X = real
    idx = np.arange(n) % len(X)
    got, leaf = f.predict(X[idx]), f.pred_leaf(X[idx])
    assert got.shape == (n,) and leaf.shape == (n, 278)
    assert np.array_equal(got, g14["pred_best"][idx]) and np.array_equal(leaf, g14["leaf"][idx, :278])


def test_hand_built_forests(sgmm):
    from sgmm_amd.gate_units import SGU1Forest
    arrays, base, X, pred, pos = sm.edge_forest()
    f = SGU1Forest.from_arrays(*arrays, base)
    assert f.depth == 2 and f.n_trees == 3
    assert np.array_equal(f.predict(X), pred) and np.array_equal(f.pred_leaf(X), pos)
    arrays, base, want = sm.order_forest()
    f = SGU1Forest.from_arrays(*arrays, base)
    assert f.predict(np.zeros((3, 20), np.float32)).tolist() == [want] * 3  # sequential float32 sum
    assert f.predict(np.zeros((3, 20)), n_trees=0).tolist() == [0.0] * 3     # base_score alone


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5, 6])
def test_depths(sgmm, depth):
    from sgmm_amd.gate_units import SGU1Forest
    rng = np.random.default_rng(100 + depth)
    arrays = sm.random_forest(rng, 37, depth)  # 37: two groups of 16 trees (SGMM_FOREST_ILP) and a tail of 5
    X = sm.random_rows(rng, 300)
    f = SGU1Forest.from_arrays(*arrays, 0.5)
    assert f.depth == depth
    pred, leaf = sm.forest_predict(*arrays, np.float32(0.5), X)
    assert np.array_equal(f.predict(X), pred) and np.array_equal(f.pred_leaf(X), leaf)


def test_groups_and_tail_in_a_second_chunk(sgmm):
    """701 trees at depth 4 over 65 rows: an LDS chunk of 666 trees, then 35 -- two full groups
    of 16 and a tail of 3 inside the second chunk, and an odd count, so the uint2 tail copy runs
    at a non-zero blob offset."""
    from sgmm_amd.gate_units import SGU1Forest
    rng = np.random.default_rng(701)
    arrays = sm.random_forest(rng, 701, 4)
    X = sm.random_rows(rng, 65)
    f = SGU1Forest.from_arrays(*arrays, 0.5)
    assert f.depth == 4 and f._blob.shape == (701, 46)
    pred, leaf = sm.forest_predict(*arrays, np.float32(0.5), X)
    assert np.array_equal(f.predict(X), pred) and np.array_equal(f.pred_leaf(X), leaf)


@pytest.mark.parametrize("depth,n_trees", [(4, 1000), (6, 230)])
def test_forest_larger_than_lds(sgmm, depth, n_trees):
    """Blobs past 160 KiB are walked in LDS-sized chunks of trees with the partial sum carried
    over: the same bits as the model evaluating the forest in one piece."""
    from sgmm_amd.gate_units import SGU1Forest
    rng = np.random.default_rng(depth)
    arrays = sm.random_forest(rng, n_trees, depth, p_leaf=0.15)
    f = SGU1Forest.from_arrays(*arrays, -1.25)
    assert f._blob.nbytes > 160 * 1024
    assert f._blob.nbytes == f_bytes(depth, n_trees)
    X = sm.random_rows(rng, 300)
    pred, leaf = sm.forest_predict(*arrays, np.float32(-1.25), X)
    assert np.array_equal(f.predict(X), pred) and np.array_equal(f.pred_leaf(X), leaf)


def f_bytes(depth, n_trees):
    from sgmm_amd import _lib
    return _lib.load().sgmm_sgu1_forest_bytes(depth, n_trees)


def test_garbage_blob_runs(sgmm, real):
    """Random words where thresholds, features and leaves should be: the 5-bit feature mask and
    the 32-column staging keep every index in bounds.  The result is not compared."""
    import torch
    from sgmm_amd.gate_units import SGU1Forest
    f, X = real
    g = SGU1Forest.from_arrays(*[getattr(f, n) for n in ARR], f.base_score)
    g._blob = np.random.default_rng(0).integers(0, 2 ** 32, g._blob.shape, dtype=np.uint64).astype(np.uint32)
    out, leaf = g.predict(X), g.pred_leaf(X)
    torch.cuda.synchronize()
    assert out.shape == (len(X),) and leaf.min() >= 0 and leaf.max() < 16


def test_unsupported_depth_and_bad_arguments(sgmm, real):
    import torch
    from sgmm_amd import _lib
    from sgmm_amd._lib import ptr, stream_ptr
    f, X = real
    L = _lib.load()
    Xd = torch.zeros((20, 8), dtype=torch.float32, device="cuda")
    out = torch.zeros(8, dtype=torch.float32, device="cuda")
    blob = f._device_blob(Xd.device)
    call = lambda depth, nt, nbytes: L.sgmm_sgu1_predict(ptr(blob), nbytes, depth, nt, 0.0, ptr(Xd), 8, 8, ptr(out),
                                                         None, stream_ptr())
    assert call(7, 10, blob.numel() * 4) == -4  # SGMM_ERR_UNSUPPORTED
    assert call(0, 10, blob.numel() * 4) == -1
    assert call(4, 299, blob.numel() * 4) == -1  # more trees than the blob holds
    assert call(4, 298, blob.numel() * 4) == 0
    assert L.sgmm_sgu1_forest_bytes(4, 601) == 601 * 184 and L.sgmm_sgu1_forest_bytes(7, 1) == 0


# ---------------------------------------------------------------- end to end

class M1:
    def predict(self, X):
        return np.asarray(X.iloc[:, 0].values, dtype=np.float32)


class M2:
    def predict(self, X):
        return np.asarray(X[:, -1, 0], dtype=np.float32).reshape(-1, 1)


class Identity:
    def transform(self, X):
        return X


@pytest.fixture(scope="module")
def parquet_root(g6, tmp_path_factory):
    root = tmp_path_factory.mktemp("sgu1_bundle")
    for k, d in enumerate(str(d) for d in g6["dates"]):
        for kind in ("snap", "tick"):
            p = root / "data" / "SYN" / kind
            p.mkdir(parents=True, exist_ok=True)
            pd.DataFrame({c[len(f"d{k}_{kind}_"):]: g6[c] for c in g6 if c.startswith(f"d{k}_{kind}_")}) \
                .to_parquet(p / f"{d}.parquet")
    return str(root)


def test_bundle_with_forest_on_device(sgmm, g6, g14, real, parquet_root):
    """s1 is the model's prediction on the kernel's own float32 matrix, aligned as
    agent_trainer.py:47-61 (the last n = min(len(s1), len(s2)) rows, the final one dropped)."""
    from sgmm_amd.bundle import _filter_sort, event_bars, load_signals_bundle
    f, _ = real
    dates = [str(d) for d in g6["dates"]]
    out = load_signals_bundle("SYN", dates, f, M2(), Identity(), data_root=parquet_root)
    days = []
    for k in range(len(dates)):
        snap = pd.DataFrame({c[len(f"d{k}_snap_"):]: g6[c] for c in g6 if c.startswith(f"d{k}_snap_")})
        tick = pd.DataFrame({c[len(f"d{k}_tick_"):]: g6[c] for c in g6 if c.startswith(f"d{k}_tick_")})
        days.append(_filter_sort(snap, tick))
    ev = event_bars(days)
    want = []
    for k, (X, _) in enumerate(ev.sgu1_table()):
        pred, _ = sm.forest_predict(*[g14[f"forest_{n}"] for n in ARR], g14["forest_base_score"],
                                    X.cpu().numpy().T, n_trees=278)
        n = min(len(pred), len(g6[f"d{k}_sgu2_y"]))
        want.append(pred[-n:][:-1])
    assert out[0].dtype == np.float32 and np.array_equal(out[0], np.concatenate(want))
    for name, a in list(zip(NAMES, out))[1:]:
        assert same(a, g6[f"bundle_{name}"]), name


def test_bundle_with_host_model_and_device_table(sgmm, g6, parquet_root):
    from sgmm_amd.bundle import load_signals_bundle
    out = load_signals_bundle("SYN", [str(d) for d in g6["dates"]], M1(), M2(), Identity(), data_root=parquet_root)
    for name, a in zip(NAMES, out):
        assert same(a, g6[f"bundle_{name}"]), name


def test_bundle_with_callable_is_unchanged(sgmm, g6, parquet_root):
    from sgmm_amd.bundle import load_signals_bundle
    dates = [str(d) for d in g6["dates"]]
    f0 = iter([g6[f"d{k}_sgu1_f0"] for k in range(len(dates))])

    def sgu1_features(bars):
        v = next(f0)
        return pd.DataFrame({"f0": v, "label": np.zeros(len(v))})

    out = load_signals_bundle("SYN", dates, M1(), M2(), Identity(), sgu1_features=sgu1_features,
                              data_root=parquet_root)
    for name, a in zip(NAMES, out):
        assert same(a, g6[f"bundle_{name}"]), name
