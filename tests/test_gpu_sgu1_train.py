"""GPU tests of SGU1 training on the device: sgmm_sgu1_train
against the numpy model of tests/sgu1_train_model.py.  Byte equality
throughout -- forest, node statistics, history, best round and score, running
predictions: every sum over rows is an integer sum and the float64 split
search has one operation order, so there is no tolerance to state."""
import json

import numpy as np
import pandas as pd
import pytest

import sgu1_model as sm
import sgu1_train_cases as sc
import sgu1_train_model as tm
from conftest import has_gpu
from sgu1_train_cases import SMALL, edge_table, model_fit, split_rows

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

FOREST = ("left", "right", "feat", "value", "default_left", "tree_off")


def device_fits(cases):
    """cases: (X [n, 20], y [n], rows_train, rows_val, params) or, with the validation rows in
    a table of their own, (X, y, rows_train, rows_val, params, X_val, y_val) -> run_sgu1_fits'
    results, one launch."""
    import torch
    from sgmm_amd import gate_units as gu
    specs, up = [], {}

    def dev(a):
        if id(a) not in up:
            up[id(a)] = torch.from_numpy(np.ascontiguousarray(a.T)).to("cuda")
        return up[id(a)]

    for X, y, rt, rv, p, *val in cases:
        Xv, yv = val if val else (X, y)
        specs.append(dict(X_train=dev(X), y_train=dev(y), rows_train=rt, X_val=dev(Xv), y_val=dev(yv), rows_val=rv,
                          params=p))
    return gu.run_sgu1_fits(specs)


def assert_same(got, want, what=""):
    for k in tm.FOREST_KEYS + ("val_rmse", "pred_train", "pred_val"):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, k, a[:8], b[:8])
    assert tm.same_fit(got, want), (what, got["n_trees"], want["n_trees"], got["best_iteration"], want["best_iteration"],
                                    got["best_score"], want["best_score"])


@pytest.fixture(scope="module")
def big(sgmm):
    return edge_table(np.random.default_rng(0), 2049 + 700 + 6)


@pytest.mark.parametrize("n_train", [1, 3, 7, 8, 63, 64, 65, 1025, 2049])
def test_row_counts(big, n_train):
    """3 rows cannot split at min_child_weight 4 (single-leaf trees), 8 is the first size
    that can; 1 025 and 2 049 cross the workgroup's row stride."""
    X, y = big
    n_val = max(2, min(n_train // 3, 700))
    rt, rv, ld = split_rows(n_train, n_val)
    assert ld <= len(X)
    want = model_fit(X, y, rt, rv, SMALL)
    got, = device_fits([(X, y, rt, rv, SMALL)])
    assert_same(got, want, n_train)
    if n_train < 8:
        assert len(want["left"]) == want["n_trees"]
    if n_train >= 63:
        assert len(want["left"]) > want["n_trees"]


@pytest.fixture(scope="module")
def edge(sgmm):
    return sc.edge()


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5, 6])
def test_depths_and_edge_columns(edge, depth):
    """One task per launch: the launch's largest max_depth picks k_sgu1_train<depth>."""
    X, y, rt, rv = edge
    p = dict(SMALL, max_depth=depth, min_child_weight=2.0)
    assert sc.case(f"depth:{depth}")[4] == p
    want = sc.model(f"depth:{depth}")
    got, = device_fits([(X, y, rt, rv, p)])
    assert_same(got, want, depth)
    inner = want["left"] != -1
    used = set(want["feat"][inner].tolist())
    assert not used & {1, 3, 6}  # no cut in an all-NaN or a constant column; of two equal columns the lower wins
    assert len(want["cuts"][1]) == 0 and len(want["cuts"][3]) == 0 and len(want["cuts"][4]) == 255
    assert len(np.unique(X[rt, 4])) > 256
    sizes = np.diff(want["tree_off"])
    assert sizes.max() <= 2 ** (depth + 1) - 1 and (depth > 1 or (sizes == 3).all())
    if depth >= 4:
        assert sizes.max() > 2 ** depth - 1  # some tree reaches the last level
        assert {4, 5} <= used
        f2 = inner & (want["feat"] == 2)
        assert set(want["default_left"][f2].tolist()) == {0, 1}  # the NaNs of column 2 go either way


def test_alpha_above_every_gradient(edge):
    X, y, rt, rv = edge
    p = dict(SMALL, reg_alpha=1e9, early_stopping_rounds=0, n_estimators=3)
    want = model_fit(X, y, rt, rv, p)
    got, = device_fits([(X, y, rt, rv, p)])
    assert_same(got, want)
    assert got["left"].tolist() == [-1] * 3 and (got["value"] == 0).all() and (got["sum_hessian"] == 300).all()
    assert got["pred_train"].tobytes() == np.full(300, want["base_score"], np.float32).tobytes()


def test_gamma_prunes(edge):
    X, y, rt, rv = edge
    free = model_fit(X, y, rt, rv, SMALL)
    p = dict(SMALL, gamma=20.0)
    want = model_fit(X, y, rt, rv, p)
    got, = device_fits([(X, y, rt, rv, p)])
    assert_same(got, want)
    kept = want["loss_change"][want["left"] != -1]
    assert want["n_trees"] < len(want["left"]) < len(free["left"]) and (kept > 20.0).all()
    assert (free["loss_change"][free["left"] != -1] <= 20.0).any()


def test_equal_labels(edge):
    """m = 0 in every round: +0 leaves, rmse 0 at round 0 and never strictly lower."""
    X, y, rt, rv = edge
    y = np.full_like(y, 2.5)
    want = model_fit(X, y, rt, rv, SMALL)
    got, = device_fits([(X, y, rt, rv, SMALL)])
    assert_same(got, want)
    assert got["n_trees"] == 4 and got["best_iteration"] == 0 and got["best_score"] == 0.0
    assert got["left"].tolist() == [-1] * 4 and not np.signbit(got["value"]).any() and (got["value"] == 0).all()


def test_no_validation_rows(edge):
    X, y, rt, _ = edge
    p = dict(SMALL, early_stopping_rounds=0, n_estimators=5)
    rv = np.zeros(0, np.int64)
    want = model_fit(X, y, rt, rv, p)
    got, = device_fits([(X, y, rt, rv, p)])
    assert_same(got, want)
    assert got["n_trees"] == 5 and got["best_iteration"] == -1 and np.isnan(got["best_score"])
    assert len(got["val_rmse"]) == 0 and len(got["pred_val"]) == 0


def test_stopping_fires_and_never_fires(edge):
    X, y, rt, rv = edge
    noise = y.copy()
    noise[rv] = np.random.default_rng(3).normal(size=len(rv)).astype(np.float32)  # nothing to learn
    fires = dict(SMALL, eta=0.5, min_child_weight=1.0)
    never = dict(SMALL, eta=0.05)
    want_f, want_n = model_fit(X, noise, rt, rv, fires), model_fit(X, y, rt, rv, never)
    got_f, got_n = device_fits([(X, noise, rt, rv, fires), (X, y, rt, rv, never)])
    assert_same(got_f, want_f, "fires")
    assert_same(got_n, want_n, "never")
    assert got_f["n_trees"] == got_f["best_iteration"] + 3 + 1 < 16
    assert got_n["n_trees"] == 16 and got_n["best_iteration"] == 15


def test_permuted_rows_give_the_same_bytes(edge):
    """The order of the rows changes nothing: integer sums, an exactly rounded base score."""
    X, y, rt, rv = edge
    rng = np.random.default_rng(4)
    pt, pv = rng.permutation(len(rt)), rng.permutation(len(rv))
    a, b = device_fits([(X, y, rt, rv, SMALL), (X, y, rt[pt], rv[pv], SMALL)])
    assert tm.same_fit(a, b)
    assert a["pred_train"][pt].tobytes() == b["pred_train"].tobytes()
    assert a["pred_val"][pv].tobytes() == b["pred_val"].tobytes()
    # and a table whose rows lie elsewhere
    perm = rng.permutation(len(X))
    inv = np.argsort(perm)
    c, = device_fits([(X[perm], y[perm], inv[rt], inv[rv], SMALL)])
    assert tm.same_fit(a, c) and a["pred_train"].tobytes() == c["pred_train"].tobytes()


def test_five_mixed_tasks_in_one_launch(big, edge):
    Xb, yb = big
    X, y, rt, rv = edge
    rtb, rvb, _ = split_rows(1025, 300)
    cases = [(X, y, rt, rv, dict(SMALL, max_depth=6, min_child_weight=1.0)),
             (Xb, yb, rtb, rvb, dict(SMALL, max_depth=2, eta=0.1, reg_alpha=0.5)),
             (X, y, rt[:50], rv[:0], dict(SMALL, max_depth=4, early_stopping_rounds=0, n_estimators=7)),
             (Xb, yb, rtb[:8], rvb[:2], dict(SMALL, max_depth=1)),
             (X, y, rt, rv, dict(SMALL, max_depth=5, reg_lambda=0.0, max_bin=16, gamma=1.0))]
    together = device_fits(cases)
    for k, case in enumerate(cases):
        alone, = device_fits([case])
        assert tm.same_fit(together[k], alone), k
        assert together[k]["pred_train"].tobytes() == alone["pred_train"].tobytes(), k
        assert_same(together[k], model_fit(*case), k)


def test_saved_model_predicts_the_trainers_predictions(edge, tmp_path):
    from sgmm_amd import gate_units as gu
    X, y, rt, rv = edge
    m = gu.SGU1(n_estimators=16, early_stopping_rounds=3, learning_rate=0.3)
    m.train(X[rt], y[rt], X[rv], y[rv])
    want = model_fit(X, y, rt, rv, dict(SMALL, min_child_weight=4.0))
    assert_same(m.fit_, want)
    assert m.best_iteration == want["best_iteration"] and m.best_score == want["best_score"]
    assert m.evals_result["validation_0"]["rmse"] == want["val_rmse"].tolist()
    p = tmp_path / "sgu1.json"
    m.save(str(p))
    with open(p) as fh:
        doc = json.load(fh)
    assert doc == gu.sgu1_json(want)
    f = gu.SGU1Forest(str(p))
    total = len(f.tree_off) - 1
    assert total == want["n_trees"] and f.n_trees == want["best_iteration"] + 1
    assert f.predict(X[rt], n_trees=total).tobytes() == m.fit_["pred_train"].tobytes()
    assert f.predict(X[rv], n_trees=total).tobytes() == m.fit_["pred_val"].tobytes()
    # predict() stops at the best round, as XGBRegressor does after early stopping
    pred, _ = sm.forest_predict(*[want[k] for k in FOREST], want["base_score"], X[rv], n_trees=f.n_trees)
    assert m.predict(X[rv]).tobytes() == pred.tobytes()
    again = gu.SGU1()
    again.load(str(p))
    assert again.predict(X[rv]).tobytes() == pred.tobytes()


# ---------------------------------------------------------------- the cases of tests/sgu1_train_cases.py
#
# What each input reaches in the model (level widths, infinite loss changes, ties, sums past
# 2^53, ...) is asserted without a GPU in tests/test_sgu1_train_model.py; here the device
# has to give the model's bytes on it.

def check_cases(names):
    """The named cases in one launch against the model."""
    got = device_fits([sc.case(n) for n in names])
    for n, g in zip(names, got):
        assert_same(g, sc.model(n), n)
    return got


@pytest.mark.parametrize("depth", [6, 5])
def test_full_levels(sgmm, depth):
    """Depth 6: 32 nodes at level 5, one feature per pass, feature 19 in the 20th and last --
    and every tree of both tables splits on it there.  Depth 5: 16 nodes at level 4, two
    features per pass."""
    check_cases([f"planted:1:{depth}", f"planted:2:{depth}"])


def test_label_scales_in_one_launch(sgmm):
    """2^-140 (subnormal labels, the subnormal branch of the exponent) to 2^124 (s = 40 - e
    negative, loss_change +inf in float32); the model's fits at 2^30, 2^100 and 2^124 are
    those of 2^0 times the power of two exactly, so the device is held to that too."""
    got = check_cases([f"scale:{k}" for k in sc.SCALES])
    by_k = dict(zip(sc.SCALES, got))
    assert np.isinf(by_k[124]["loss_change"]).any() and np.isinf(by_k[100]["loss_change"]).any()
    assert by_k[-140]["left"].tolist() == [-1] * 4 and by_k[-100]["left"].tolist() == [-1] * 4
    assert by_k[-140]["value"].tobytes() == sc.model("scale:-140")["value"].tobytes()
    assert by_k[124]["pred_val"].tobytes() == np.ldexp(by_k[0]["pred_val"], 124).tobytes()
    assert by_k[124]["val_rmse"].tobytes() == np.ldexp(by_k[0]["val_rmse"], 124).tobytes()
    assert 0 < (by_k[sc.SMALL_SCALE]["left"] != -1).sum() < (by_k[0]["left"] != -1).sum()


def test_largest_label_scale_alone(sgmm):
    got, = check_cases(["scale:124"])
    assert np.isfinite(got["pred_train"]).all() and np.abs(got["pred_train"]).max() > 2.0 ** 124


def test_subnormal_labels_that_the_metric_rounds(sgmm):
    """2^-130: all labels subnormal and residuals of more than 20 bits, where the exponent of
    a subnormal decides what the metric rounds to (at 2^-140 everything is exact)."""
    got, = check_cases([f"scale:{sc.SUBNORMAL_SCALE}"])
    assert got["n_trees"] == 4 and (got["val_rmse"] > 0).all() and (got["val_rmse"] < 2.0 ** -126).all()


def test_rounding_ties_and_sums_past_2_53(sgmm):
    """65 538 rows in one workgroup: rint on exact ties, a child sum of 2^54.1 that float64
    has to round, and a leaf of the tiny rows alone whose value shows each unit of its sum."""
    got, = check_cases(["rounding"])
    assert got["n_trees"] == 2 and got["left"][4] == -1 and got["value"][4] != 0


def test_infinite_and_zero_thresholds_through_save_and_predict(sgmm, tmp_path):
    """+-inf and +-0 feature values: trained thresholds at +inf and at +0, and the saved model
    read back into the forest kernel gives the trainer's running predictions."""
    from sgmm_amd import gate_units as gu
    X, y, rt, rv, p = sc.case("inf")
    want = sc.model("inf")
    got, = check_cases(["inf"])
    inner = got["left"] != -1
    assert np.isinf(got["value"][inner]).any() and not np.signbit(got["value"][inner & (got["value"] == 0)]).any()
    m = gu.SGU1(n_estimators=16, early_stopping_rounds=3, learning_rate=0.3)
    assert gu.sgu1_fit_params(m.params) == {k: p[k] for k in gu.sgu1_fit_params(m.params)}
    m.train(X[rt], y[rt], X[rv], y[rv])
    assert_same(m.fit_, want)
    path = tmp_path / "sgu1_inf.json"
    m.save(str(path))
    f = gu.SGU1Forest(str(path))
    total = len(f.tree_off) - 1
    assert total == want["n_trees"]
    assert np.asarray(f.value).astype(np.float32).tobytes() == want["value"].tobytes()  # inf and 0 survive the file
    assert f.predict(X[rt], n_trees=total).tobytes() == m.fit_["pred_train"].tobytes() == want["pred_train"].tobytes()
    assert f.predict(X[rv], n_trees=total).tobytes() == m.fit_["pred_val"].tobytes() == want["pred_val"].tobytes()


def test_max_bins_in_one_launch(sgmm):
    check_cases([f"max_bin:{b}" for b in sc.MAX_BINS])


@pytest.mark.parametrize("max_bin", sc.MAX_BINS)
def test_device_cuts_equal_the_models(sgmm, max_bin):
    """sgu1_cuts (torch.unique on the device) against make_cuts (np.unique): the edge table,
    +-inf and +-0 values, and columns of exactly 256 and 257 distinct values."""
    import torch
    from sgmm_amd import gate_units as gu
    Xc = sc.cuts_table()
    tables = [sc.edge()[:3:2], sc.case("inf")[:3:2], (Xc, np.arange(len(Xc))), (Xc, np.arange(len(Xc))[::-1].copy())]
    for k, (X, rows) in enumerate(tables):
        Xd = torch.from_numpy(np.ascontiguousarray(X.T)).to("cuda")
        cuts, n_cuts = gu.sgu1_cuts(Xd, torch.from_numpy(rows).to("cuda"), max_bin)
        want = tm.make_cuts(X[rows], max_bin)
        assert cuts.dtype == np.float32 and cuts.shape == (20, 256)
        assert n_cuts.tolist() == [len(c) for c in want], k
        for f in range(20):
            assert cuts[f, :n_cuts[f]].tobytes() == want[f].tobytes(), (k, f)
            assert not cuts[f, n_cuts[f]:].any()
    if max_bin == 256:
        want = tm.make_cuts(Xc, 256)
        assert want[0].tolist() == list(range(1, 256)) and want[1].tolist() == list(range(2, 257))


def test_rows_and_tables_in_one_launch(sgmm):
    """Validation rows from a second table with its own leading dimension, one validation
    row, a bootstrap sample of the training rows (repeated indices), min_child_weight 2.5
    and 0."""
    got = dict(zip(sc.ROWS_AND_TABLES, check_cases(list(sc.ROWS_AND_TABLES))))
    assert len(got["one_val_row"]["pred_val"]) == 1 and len(got["one_val_row"]["val_rmse"]) == 16
    assert len(got["second_table"]["pred_val"]) == len(sc.case("second_table")[3])
    kids = np.ones(len(got["mcw0"]["left"]), bool)
    kids[got["mcw0"]["tree_off"][:-1]] = False
    assert got["mcw0"]["sum_hessian"][kids].min() == 1.0 and got["mcw2.5"]["sum_hessian"].min() == 3.0


# ---------------------------------------------------------------- the g14 fixture, end to end

@pytest.fixture(scope="module")
def g14(golden):
    return golden("g14_sgu1.npz")


@pytest.fixture(scope="module")
def fixture_fit(sgmm, g14):
    from sgmm_amd import gate_units as gu
    from sgmm_amd.bundle import EventBarsGPU
    bars = [{c: g14[f"d{k}_ev_{c}"] for c in sm.EV_COLS} for k in range(4)]
    ev_train, ev_val = EventBarsGPU.from_bars(bars[:3]), EventBarsGPU.from_bars(bars[3:])
    m = gu.SGU1(n_estimators=16, early_stopping_rounds=3, learning_rate=0.3)
    m.train_device(ev_train, ev_val)
    return bars, ev_train, ev_val, m


def test_train_device_on_the_fixture_days(fixture_fit):
    """Days 0-2 train, day 3 validates: the fit straight from the device tables equals the
    model on the same days' tables built in numpy, and SGU1.train on the DataFrames."""
    from sgmm_amd import gate_units as gu
    bars, ev_train, ev_val, m = fixture_fit
    tabs = [sm.feature_table(b) for b in bars]
    Xt = np.concatenate([t[:, :20] for t in tabs[:3]]).astype(np.float32)
    yt = (np.concatenate([t[:, 20] for t in tabs[:3]]) * 1000).astype(np.float32)
    Xv, yv = tabs[3][:, :20].astype(np.float32), (tabs[3][:, 20] * 1000).astype(np.float32)
    assert len(Xt) > 100 and len(Xv) > 10
    want = tm.fit(Xt, yt, Xv, yv, **dict(SMALL, min_child_weight=4.0))
    assert_same(m.fit_, want)
    assert len(want["left"]) > want["n_trees"]
    frames = [ev_train.sgu1_frame(d) for d in range(3)]
    df, dv = pd.concat(frames, axis=0), ev_val.sgu1_frame(0)
    h = gu.SGU1(n_estimators=16, early_stopping_rounds=3, learning_rate=0.3)
    h.train(df.drop(columns=["label"]), df["label"] * 1000, dv.drop(columns=["label"]), dv["label"] * 1000)
    assert_same(h.fit_, want)
    for k in FOREST:
        assert np.asarray(getattr(h.forest, k)).tobytes() == np.asarray(getattr(m.forest, k)).tobytes(), k


class M2:
    def predict(self, X):
        return np.asarray(X[:, -1, 0], dtype=np.float32).reshape(-1, 1)


class Identity:
    def transform(self, X):
        return X


def test_trained_model_takes_the_forest_path_of_the_bundle(fixture_fit, golden, tmp_path, monkeypatch):
    from sgmm_amd.bundle import load_signals_bundle
    _, _, _, m = fixture_fit
    g6 = golden("g6_bundle.npz")
    dates = [str(d) for d in g6["dates"]]
    for k, d in enumerate(dates):
        for kind in ("snap", "tick"):
            p = tmp_path / "data" / "SYN" / kind
            p.mkdir(parents=True, exist_ok=True)
            pd.DataFrame({c[len(f"d{k}_{kind}_"):]: g6[c] for c in g6 if c.startswith(f"d{k}_{kind}_")}) \
                .to_parquet(p / f"{d}.parquet")
    want = load_signals_bundle("SYN", dates, m.forest, M2(), Identity(), data_root=str(tmp_path))

    def host_path(*a, **k):
        raise AssertionError("the per-day host path was taken")

    monkeypatch.setattr(m, "predict", host_path)
    calls = []
    real = m.forest.predict_device
    monkeypatch.setattr(m.forest, "predict_device", lambda *a, **k: calls.append(1) or real(*a, **k))
    got = load_signals_bundle("SYN", dates, m, M2(), Identity(), data_root=str(tmp_path))
    assert len(calls) == 1  # every day's rows in one launch
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
