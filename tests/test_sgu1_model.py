"""SGU1 on the device, the host side: the independent
forest evaluator of tests/sgu1_model.py on forests worked out by hand, the
xgboost JSON loader and the complete-tree packer of gate_units.SGU1Forest,
and the restatements of pandas' rolling mean and of the slope that the
feature kernel transcribes.  Fixtures: tests/golden/g14_sgu1.npz and
g14_sgu1_model.json (gen_golden_sgu1.py)."""
import json
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import sgu1_feature_cases as fc
import sgu1_model as sm
from conftest import GOLDEN

ARR = ("left", "right", "feat", "value", "default_left", "tree_off")


@pytest.fixture(scope="module")
def g14(golden):
    return golden("g14_sgu1.npz")


def test_evaluator_on_hand_built_forest():
    arrays, base, X, pred, pos = sm.edge_forest()
    got, leaf = sm.forest_predict(*arrays, base, X)
    assert got.dtype == np.float32 and np.array_equal(got, pred)
    assert np.array_equal(leaf, pos)
    assert sm.forest_depth(arrays[0], arrays[1], arrays[5]) == 2
    got2, leaf2 = sm.forest_predict(*arrays, base, X, n_trees=2)  # a prefix of the trees
    assert np.array_equal(got2, pred - np.float32(0.5)) and np.array_equal(leaf2, pos[:, :2])


def test_evaluator_sums_sequentially_in_float32():
    arrays, base, want = sm.order_forest()
    got, _ = sm.forest_predict(*arrays, base, np.zeros((1, 20), np.float32))
    assert got[0] == want
    v = arrays[3]
    assert np.float32(np.float32(v[0] + v[1]) + np.float32(v[2] + v[3])) != want  # pairwise gives other bits


def packed_walk(D, blob, X):
    """The complete-tree walk over a packed blob, in numpy: (pred without base, positions)."""
    T, NI = blob.shape[0], (1 << D) - 1
    pos = np.zeros((len(X), T), np.int32)
    val = np.zeros((len(X), T), np.float32)
    for t in range(T):
        k = np.zeros(len(X), np.int64)
        for _ in range(D):
            thr, word = blob[t, 2 * k].view(np.float32), blob[t, 2 * k + 1]
            x = X[np.arange(len(X)), word & 31]
            left = np.where(np.isnan(x), (word >> 31) != 0, x < thr)
            k = 2 * k + np.where(left, 1, 2)
        pos[:, t] = k - NI
        val[:, t] = blob[t, NI + k].view(np.float32)
    return val, pos


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5, 6])
def test_packer_round_trips(sgmm, depth):
    from sgmm_amd.gate_units import pack_forest
    rng = np.random.default_rng(depth)
    arrays = sm.random_forest(rng, 30, depth)
    X = sm.random_rows(rng, 200)
    D, blob = pack_forest(*arrays)
    assert D == depth == sm.forest_depth(arrays[0], arrays[1], arrays[5])
    assert blob.dtype == np.uint32 and blob.shape == (30, 3 * (1 << D) - 2)
    val, pos = packed_walk(D, blob, X)
    _, leaf = sm.forest_predict(*arrays, 0.0, X)
    assert np.array_equal(pos, leaf)
    for t in range(30):  # the same leaf value, tree by tree
        one = [a[arrays[5][t]:arrays[5][t + 1]] for a in arrays[:5]] + [np.array([0, arrays[5][t + 1] - arrays[5][t]])]
        want, _ = sm.forest_predict(*one, 0.0, X)
        assert np.array_equal(val[:, t], want), t


def test_packer_on_edge_forest_and_single_leaves(sgmm):
    from sgmm_amd.gate_units import pack_forest
    arrays, base, X, pred, pos = sm.edge_forest()
    D, blob = pack_forest(*arrays)
    assert D == 2
    val, got = packed_walk(D, blob, X)
    assert np.array_equal(got, pos)
    acc = np.full(len(X), base, np.float32)
    for t in range(3):
        acc = acc + val[:, t]
    assert np.array_equal(acc, pred)
    D, blob = pack_forest(*sm.order_forest()[0])  # a forest of single leaves packs at depth 1
    assert D == 1 and np.array_equal(blob[:, 2:].view(np.float32), [[1e8] * 2, [1.0] * 2, [-1e8] * 2, [1.0] * 2])


def test_packer_rejects_bad_forests(sgmm):
    from sgmm_amd.gate_units import pack_forest
    lf = sm.leaf(1.0)
    with pytest.raises(ValueError):  # child out of range
        pack_forest(*sm.forest_arrays([[(1, 5, 0, 0.0, 0), lf, lf]]))
    with pytest.raises(ValueError):  # one child only
        pack_forest(*sm.forest_arrays([[(1, -1, 0, 0.0, 0), lf]]))
    with pytest.raises(ValueError):  # a cycle never reaches a leaf
        pack_forest(*sm.forest_arrays([[(1, 2, 0, 0.0, 0), (0, 2, 0, 0.0, 0), lf]]))
    with pytest.raises(ValueError):  # feature outside the table
        pack_forest(*sm.forest_arrays([[(1, 2, 20, 0.0, 0), lf, lf]]))
    with pytest.raises(ValueError):  # depth 7
        pack_forest(*sm.random_forest(np.random.default_rng(0), 2, 7))


def test_loader_reads_xgboost_json(sgmm, g14):
    from sgmm_amd.gate_units import SGU1_FEATURES, SGU1Forest
    f = SGU1Forest().load(GOLDEN / "g14_sgu1_model.json")
    assert SGU1_FEATURES == sm.FEATURES
    n = int(g14["forest_tree_off"][40])
    assert np.array_equal(f.tree_off, g14["forest_tree_off"][:41])
    for name in ARR[:5]:
        got, want = getattr(f, name), g14[f"forest_{name}"][:n]
        assert got.dtype == want.dtype and np.array_equal(got, want), name
    assert f.base_score.dtype == np.float32 and f.base_score == g14["forest_base_score"]
    assert f.best_iteration == 37 and f.n_trees == 38 and f.depth == 4
    g = SGU1Forest.from_arrays(*[g14[f"forest_{n}"] for n in ARR], g14["forest_base_score"],
                               int(g14["forest_best_iteration"]))
    assert g.n_trees == 278 and g.depth == 4 and g._blob.shape == (298, 46)


def test_loader_rejects_what_it_cannot_walk(sgmm, tmp_path):
    from sgmm_amd.gate_units import SGU1Forest
    model = json.loads((GOLDEN / "g14_sgu1_model.json").read_text())

    def broken(edit):
        m = json.loads(json.dumps(model))
        edit(m["learner"])
        p = tmp_path / "m.json"
        p.write_text(json.dumps(m))
        return p

    def categorical(L):
        L["gradient_booster"]["model"]["trees"][3]["split_type"][0] = 1

    def targets(L):
        L["learner_model_param"]["num_target"] = "2"

    def objective(L):
        L["objective"]["name"] = "reg:logistic"

    def deep(L):  # hang a chain of 7 splits under tree 0
        t = L["gradient_booster"]["model"]["trees"][0]
        n = len(t["left_children"])
        for k in ("left_children", "right_children", "split_indices", "split_conditions", "default_left"):
            t[k] = list(t[k])
        leafs = [i for i in range(n) if t["left_children"][i] == -1]
        cur = leafs[0]
        for _ in range(7):
            a = len(t["left_children"])
            for k, v in (("left_children", [-1, -1]), ("right_children", [-1, -1]), ("split_indices", [0, 0]),
                         ("split_conditions", [0.0, 0.0]), ("default_left", [0, 0])):
                t[k] += v
            t["left_children"][cur], t["right_children"][cur] = a, a + 1
            cur = a

    for edit in (categorical, targets, objective, deep):
        with pytest.raises(ValueError):
            SGU1Forest().load(broken(edit))


def rolling_inputs():
    rng = np.random.default_rng(5)
    walk = 3.49 + 1e-3 * np.cumsum(rng.integers(-2, 3, 3000))
    rep = np.repeat(np.round(rng.normal(3.5, 0.01, 400), 3), rng.integers(1, 6, 400))  # runs of equal values
    zeros = np.where(rng.random(1500) < 0.4, 0.0, rng.random(1500) * 4)
    signed = rng.normal(0, 1, 1500)
    tiny = np.concatenate([[1e16, 1.0, -1e16], rng.random(50), [0.0] * 7])
    return dict(walk=walk, rep=rep, zeros=zeros, signed=signed, tiny=tiny)


@pytest.mark.parametrize("w", [1, 3, 5])
def test_roll_mean_equals_pandas(w):
    fresh_differs = 0
    for name, v in rolling_inputs().items():
        want = pd.Series(v).rolling(w, min_periods=1).mean().to_numpy()
        got = sm.roll_mean(v, w)
        assert np.array_equal(got, want), (name, w, int((got != want).sum()))
        fresh = np.array([v[max(i - w + 1, 0):i + 1].mean() for i in range(len(v))])
        fresh_differs += int((fresh != want).sum())
    assert w == 1 or fresh_differs > 0  # a fresh window mean is not what pandas computes


# ---------------------------------------------------------------- the edge days (sgu1_feature_cases.py)

EDGE_DAYS = fc.DAYS + tuple(str(k) for k, nb in enumerate(fc.TURNS) if nb >= 6)


def shown(a):
    """Per-bar values that reach the table: shift(1) drops the last bar's."""
    return a[:-1]


def halfway(v):
    """+1 / -1 where the float64 v lies exactly between two neighbouring float32 values and the
    cast moves it away from / towards zero, else 0."""
    with np.errstate(over="ignore"):
        f = np.asarray(v, np.float64).astype(np.float32)
    out = np.zeros(len(f), np.int64)
    for i, (a, b) in enumerate(zip(np.asarray(v, np.float64), f)):
        if a == b or not np.isfinite(a):
            continue
        # the float32 neighbour on the other side of a, with 2^128 standing in for inf
        with np.errstate(over="ignore"):
            other = np.nextafter(b, np.float32(0 if abs(b) > abs(a) else np.copysign(np.inf, a)))
        lo, hi = sorted((Fraction(2) ** 128 * int(np.sign(x)) if np.isinf(x) else Fraction(float(x)))
                        for x in (b, other))
        if Fraction(float(a)) - lo == hi - Fraction(float(a)):
            out[i] = 1 if abs(float(b)) > abs(a) else -1
    return out


def test_edge_days_reach_their_edges():
    """Conditions on the generators, from the model's intermediates: a day that misses one is
    changed, never the count.  Measured: rolling (778 bars) 181 / 61 overriding all-equal rows
    at windows 3 / 5, clamps 5 + 22 / 5 + 5, 185-206 bars per label arm, 78 vwaps of -0.0."""
    _, st = fc.table("rolling")
    assert len(st["vwap"]) < 1000
    for w in (3, 5):
        r = st["roll"][w]
        assert shown(r["same"]).sum() >= 20, w
        assert shown(r["clamp_nonneg"]).sum() >= 1 and shown(r["clamp_neg"]).sum() >= 1, w
    for i, (_, sign, w) in enumerate(fc.CLAMPS):  # every stretch kept for a clamp hits it
        hit = st["roll"][w]["clamp_nonneg" if sign > 0 else "clamp_neg"]
        assert hit[fc.CLAMP_LEN * i + w:fc.CLAMP_LEN * (i + 1)].any(), i
    assert np.bincount(st["branch"], minlength=5)[1:].min() >= 100
    assert shown((st["vwap"] == 0) & np.signbit(st["vwap"])).sum() >= 4
    v = st["vwap"]
    assert (v > 9e299).any() and (v < -9e299).any() and np.isin([5e-324, -5e-324], v).all()
    assert ((v > 0) & (v < 2e-300)).sum() >= 4

    tab, st = fc.table("ties")
    k = np.floor(st["x"] * 1e4)
    tie = st["x"] * 1e4 == k + 0.5
    assert (tie & (k % 2 == 0)).sum() >= 4 and (tie & (k % 2 == 1)).sum() >= 4
    assert (tab[tie, 20] != np.floor(st["x"][tie] * 1e4 + 0.5) / 1e4).sum() >= 4
    for arm in (1, 2, 3):  # a tie of each parity in every arm that can have one (none in arm 4: fc.tie_inputs)
        assert (tie & (st["branch"] == arm) & (k % 2 == 0)).sum() >= 4, arm
        assert (tie & (st["branch"] == arm) & (k % 2 == 1)).sum() >= 4, arm

    tab, _ = fc.table("cast")
    for cols in ((18,), (5,), (5, 18)):
        F = tab[:, cols].ravel()
        with np.errstate(over="ignore"):
            X = F.astype(np.float32)
        h = halfway(F)
        classes = dict(inf=np.isinf(X) & np.isfinite(F), subnormal=(X != 0) & (np.abs(X) < 2.0 ** -126),
                       zero=(X == 0) & (F != 0), half_away=h == 1, half_towards=h == -1)
        for name, m in classes.items():
            assert m.sum() >= 2, (cols, name)
    with np.errstate(over="ignore"):
        assert (np.isneginf(tab[:, 5].astype(np.float32)) & np.isfinite(tab[:, 5])).sum() >= 2

    _, st = fc.table("hours")
    assert st["hour"].tolist() == [t // 10 ** 7 for t in fc.HOURS]
    assert {9, 10, 14, 0, 1}.issubset(st["hour"].tolist()) and st["hour"].max() > 2 ** 31 // 10 ** 7

    for k, nb in enumerate(fc.TURNS):
        if nb not in (1025, 2049):
            continue
        _, st = fc.table(str(k))
        assert len(st["vwap"]) == nb
        # the one bar of the last turn shows its label only: an arm no 1100- or 4096-bar day of
        # all_events_bars reaches
        assert st["branch"][-1] == (4 if nb == 1025 else 3)
        if nb == 2049:  # a whole second turn: every arm, signed and -0.0 vwaps
            assert set(st["branch"][1024:2048].tolist()) == {1, 2, 3, 4}
            v = st["vwap"][1024:2048]
            assert (v < 0).any() and ((v == 0) & np.signbit(v)).any()
    _, st = fc.table("full")
    assert len(st["vwap"]) == 4096 and set(st["branch"][3072:].tolist()) == {1, 2, 3, 4}


@pytest.mark.parametrize("name", EDGE_DAYS)
def test_edge_days_equal_pandas(name):
    """pandas (2.3.3 when written) is the reference of the rolling means, the rounding and the
    hour on every edge day: bytes, since array_equal hides the sign of zero."""
    tab, st = fc.table(name)
    ev = fc.turns()[int(name)] if name.isdigit() else fc.day(name)
    assert len(tab) == len(st["vwap"]) >= 6
    fill = lambda s: s.shift(1).ffill().bfill().to_numpy()
    for j, w in enumerate((1, 3, 5)):
        want = fill(pd.Series(st["vwap"]).rolling(w, min_periods=1).mean())
        assert tab[:, 5 + j].tobytes() == want.tobytes(), (name, w, int((tab[:, 5 + j] != want).sum()))
    label = np.round(st["x"], 4)
    assert tab[:, 20].tobytes() == label.tobytes()
    for L in range(1, 6):
        assert tab[:, 10 + L].tobytes() == pd.Series(label).shift(L).ffill().bfill().to_numpy().tobytes(), L
    first = np.asarray(ev["trade_time"])[::19][:len(tab)]
    assert tab[:, 19].tobytes() == (first // 10 ** 7).astype(np.float64).tobytes()


def roll_mean_mutant(v, w, mutation):
    """sm.roll_mean with one rule changed: 'same', 'clamp_nonneg', 'clamp_neg' drop that
    override, 'less_than_zero' counts x < 0 in place of signbit(x), 'one_compensation' shares
    one Kahan compensation between adding and removing."""
    v = np.asarray(v, np.float64)
    out = np.empty(len(v))
    isneg = (lambda x: x < 0) if mutation == "less_than_zero" else np.signbit
    shared = mutation == "one_compensation"
    s = c_add = c_rm = 0.0
    nobs = neg = same = 0
    prev = v[0]
    for i in range(len(v)):
        if w == 1 or i == 0:
            s = c_add = c_rm = 0.0
            nobs = neg = same = 0
            prev = v[i]
        elif i >= w:
            x = v[i - w]
            y = -x - (c_add if shared else c_rm)
            t = s + y
            c = t - s - y
            c_add, c_rm = (c, c_rm) if shared else (c_add, c)
            s = t
            nobs -= 1
            neg -= int(isneg(x))
        x = v[i]
        y = x - c_add
        t = s + y
        c_add = t - s - y
        s = t
        nobs += 1
        neg += int(isneg(x))
        same = same + 1 if x == prev else 1
        prev = x
        r = s / nobs
        if same >= nobs and mutation != "same":
            r = prev
        elif same >= nobs:
            pass
        elif neg == 0 and r < 0 and mutation != "clamp_nonneg":
            r = 0.0
        elif neg == nobs and r > 0 and mutation != "clamp_neg":
            r = 0.0
        out[i] = r
    return out


def test_model_notices_the_mutations():
    """Each rule of the rolling mean and of the rounding, changed in a copy, changes the table of
    the day built for it; the unchanged copy does not."""
    tab, st = fc.table("rolling")
    p = np.maximum(np.arange(len(tab)) - 1, 0)
    for j, w in ((6, 3), (7, 5)):
        assert roll_mean_mutant(st["vwap"], w, None)[p].tobytes() == tab[:, j].tobytes()
        for m in ("same", "clamp_nonneg", "clamp_neg", "less_than_zero", "one_compensation"):
            got = roll_mean_mutant(st["vwap"], w, m)[p]
            assert got.tobytes() != tab[:, j].tobytes(), (w, m)
    # without the -0.0 bars x < 0 and signbit agree: those bars are what holds the rule
    v = np.where(st["vwap"] == 0, 0.0, st["vwap"])
    assert roll_mean_mutant(v, 3, "less_than_zero").tobytes() == sm.roll_mean(v, 3).tobytes()
    tab, st = fc.table("ties")
    y = st["x"] * 1e4
    half_away = np.copysign(np.floor(np.abs(y) + 0.5), y) / 1e4
    assert (half_away != tab[:, 20]).sum() >= 4
    assert ((np.floor(y + 0.5) / 1e4) != tab[:, 20]).sum() >= 4


def test_slope_closed_form_against_exact_fractions(g14):
    rng = np.random.default_rng(9)
    worst = 0.0
    cases = [rng.normal(3.5, 0.01, m) for m in (1, 2, 3, 4, 5) for _ in range(400)]
    cases += [np.round(rng.normal(3.5, 0.003, m), 4) for m in (2, 3, 4, 5) for _ in range(400)]
    cases += [rng.normal(0, 1, m) * 10.0 ** rng.integers(-8, 9) for m in (2, 3, 4, 5) for _ in range(200)]
    for y in cases:
        got, exact = sm.slope_closed(y), sm.slope_exact(y)
        bound = 4 * 2.0 ** -52 * float(np.abs(y).max())
        err = abs(float(Fraction(float(got)) - exact))
        assert err <= bound, (y, got, float(exact))
        worst = max(worst, err / bound * 4)
    for m in (1, 2, 3, 4, 5):  # a flat window: exactly +0.0
        s = sm.slope_closed(np.full(m, 3.4915))
        assert s == 0.0 and not np.signbit(s)
    assert sm.slope_exact([1.0, 2.0, 4.0]) == Fraction(3, 2) and sm.slope_exact([5.0]) == 0
    assert sm.slope_exact([0.0, 1.0, 0.0, 3.0, 1.0]) == Fraction(2, 5)  # polyfit's value, by hand
    print(f"worst closed-form slope error: {worst:.3f} * 2^-52 * max|y|")


def test_feature_table_rules_reproduce_the_reference(g14):
    """The rules the kernel transcribes, in numpy (sgu1_model.feature_table), on every fixture
    day: 18 columns and the label bit for bit; the slopes of both sides within
    4 * 2^-52 * max|mid| of the exact slope of the window."""
    rows = {}
    for k, tag in enumerate(g14["tags"]):
        ev = {c: g14[f"d{k}_ev_{c}"] for c in sm.EV_COLS}
        got, want = sm.feature_table(ev), g14[f"d{k}_table"]
        rows[str(tag)] = len(want)
        assert got.shape == want.shape, tag
        if not len(want):
            continue
        for j in range(21):
            if j not in (9, 10):
                assert np.array_equal(got[:, j], want[:, j]), (tag, j)
        mid = sm.bar_mids(ev)
        for s, j in ((3, 9), (5, 10)):
            for r, y in enumerate(sm.window_slopes(mid, s)):
                exact, bound = sm.slope_exact(y), 4 * 2.0 ** -52 * float(np.abs(y).max())
                assert abs(float(Fraction(got[r, j]) - exact)) <= bound, (tag, j, r)
                assert abs(float(Fraction(want[r, j]) - exact)) <= bound, (tag, j, r)
    assert [rows[t] for t in ("bars5", "bars6", "events19", "events20")] == [0, 6, 0, 0]


def test_fixture_predictions_are_the_evaluators(g14):
    arrays = [g14[f"forest_{n}"] for n in ARR]
    X = np.concatenate([g14[f"d{k}_table"][:, :20] for k in range(4)]).astype(np.float32)
    pred, leaf = sm.forest_predict(*arrays, g14["forest_base_score"], X[:40], n_trees=278)
    assert np.array_equal(pred, g14["pred_best"][:40]) and np.array_equal(leaf, g14["leaf"][:40, :278])


def test_forest_equals_xgboost(sgmm, g14):
    """For anyone who has xgboost: SGU1Forest.predict against Booster.predict, bit for bit."""
    xgb = pytest.importorskip("xgboost")
    from conftest import has_gpu
    if not has_gpu():
        pytest.skip("needs a HIP device")
    from sgmm_amd.gate_units import SGU1Forest
    X = np.concatenate([g14[f"d{k}_table"][:, :20] for k in range(4)]).astype(np.float32)
    booster = xgb.Booster()
    booster.load_model(str(GOLDEN / "g14_sgu1_model.json"))
    want = booster.predict(xgb.DMatrix(X, feature_names=list(sm.FEATURES)), iteration_range=(0, 38))
    got = SGU1Forest().load(GOLDEN / "g14_sgu1_model.json").predict(X)
    assert np.array_equal(got, want)
