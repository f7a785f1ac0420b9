"""CPU tests of the SGU1 training contract: the formulas
pinned against real xgboost output, the numpy model against its own brute-force
twin, the rules the contract states (node numbering, min_child_weight, early
stopping, cuts), the JSON writers against the shipped checkpoint's layout, and
the argument checks of the C ABI and of gate_units.SGU1, none of which needs
a GPU.

Formula pin.  tests/golden/g14_sgu1_model.json holds the first 40 trees of a
real xgboost fit (max_depth 4, eta 0.01, reg_alpha 0.01, lambda 1) with
sum_hessian, base_weights and loss_changes per node.  T(G) of a node is
recovered from its stored weight as -w (H + lambda) (a leaf's base_weight is
eta-scaled: divided by eta first) and G as T +- alpha.  Two comparisons with the
recorded loss_changes over the 459 split nodes:
  own       gain(L) + gain(R) - gain(node) with the node's own recovered G:
            worst relative error 9.12e-5 (three float32 weights); allowed 4x,
            3.65e-4.  lambda = 0 gives 70.  (alpha cancels here: T is what the
            weights store.)
  additive  the same with the node's G taken as G_L + G_R -- gradients add,
            soft-thresholded T's do not, which is what pins alpha: worst
            3.39e-5, allowed 4x, 1.36e-4.  alpha = 0 gives 0.17, lambda = 0
            gives 41.
H_L + H_R == H holds exactly at every split node."""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest

import sgu1_model as sm
import sgu1_train_cases as sc
import sgu1_train_model as tm

GOLDEN = Path(__file__).resolve().parent / "golden"
PIN_OWN_MEASURED, PIN_ADD_MEASURED = 9.12e-5, 3.39e-5
PIN_OWN_TOL, PIN_ADD_TOL = 4 * PIN_OWN_MEASURED, 4 * PIN_ADD_MEASURED


@pytest.fixture(scope="module")
def shipped():
    with open(GOLDEN / "g14_sgu1_model.json") as fh:
        return json.load(fh)


def pin_errors(doc, lam, alpha, eta=0.01):
    """(worst own, worst additive, split nodes, nodes whose hessians do not add)."""
    def gain(G, H):
        T = G - alpha if G > alpha else (G + alpha if G < -alpha else 0.0)
        return T * T / (H + lam)

    own = add = 0.0
    splits = bad_h = 0
    for t in doc["learner"]["gradient_booster"]["model"]["trees"]:
        bw = np.array(t["base_weights"], np.float32).astype(np.float64)
        H = np.array(t["sum_hessian"], np.float64)
        L, R = np.array(t["left_children"]), np.array(t["right_children"])
        lc = np.array(t["loss_changes"], np.float32).astype(np.float64)
        T = -np.where(L == -1, bw / eta, bw) * (H + lam)
        G = np.where(T > 0, T + alpha, np.where(T < 0, T - alpha, 0.0))
        for k in np.nonzero(L != -1)[0]:
            l, r = L[k], R[k]
            splits += 1
            bad_h += H[l] + H[r] != H[k]
            children = gain(G[l], H[l]) + gain(G[r], H[r])
            own = max(own, abs(children - gain(G[k], H[k]) - lc[k]) / lc[k])
            if T[l] != 0 and T[r] != 0:  # a child inside the alpha band has no recoverable G
                add = max(add, abs(children - gain(G[l] + G[r], H[k]) - lc[k]) / lc[k])
    return own, add, splits, bad_h


def test_formula_pin_against_xgboost_output(shipped):
    own, add, splits, bad_h = pin_errors(shipped, 1.0, 0.01)
    print(f"worst relative error over {splits} split nodes: own {own:.3e} (allowed {PIN_OWN_TOL:.3e}), "
          f"additive {add:.3e} (allowed {PIN_ADD_TOL:.3e})")
    assert splits == 459 and bad_h == 0
    assert PIN_OWN_TOL < 4e-4  # node 1 of tree 0: lambda = 0 is 4.6e-4 away
    assert own <= PIN_OWN_TOL and add <= PIN_ADD_TOL


@pytest.mark.parametrize("lam,alpha", [(0.0, 0.01), (1.0, 0.0), (1.0, 0.02), (2.0, 0.01)])
def test_formula_pin_rejects_other_parameters(shipped, lam, alpha):
    own, add, _, _ = pin_errors(shipped, lam, alpha)
    assert own > PIN_OWN_TOL or add > PIN_ADD_TOL
    if lam != 1.0:
        assert own > PIN_OWN_TOL
    if alpha != 0.01:
        assert add > PIN_ADD_TOL


def test_issue_worked_example(shipped):
    """Tree 0, node 1: 629.78956 with lambda 1, 629.50 with lambda 0, recorded 629.7895."""
    t = shipped["learner"]["gradient_booster"]["model"]["trees"][0]
    assert t["left_children"][:4] == [1, 3, 5, 7] and abs(t["loss_changes"][1] - 629.7895) < 1e-4

    def score(lam, alpha=0.01):
        g = []
        for k in (3, 4, 1):
            w = np.float64(np.float32(t["base_weights"][k]))
            T = -w * (t["sum_hessian"][k] + lam)
            g.append(T * T / (t["sum_hessian"][k] + lam))
        return g[0] + g[1] - g[2]

    assert abs(score(1.0) - 629.78956) < 1e-3 and abs(score(0.0) - 629.50) < 1e-2


def small_problem(rng, n, nan=0.05):
    """Few distinct values per feature (so the cuts are the data values), NaNs everywhere,
    one continuous column, two identical columns."""
    X = (rng.integers(-4, 5, (n, 20)) / 2).astype(np.float32)
    X[:, 5] = rng.normal(size=n).astype(np.float32)
    X[rng.random((n, 20)) < nan] = np.nan
    X[:, 7] = X[:, 3]
    y = (np.where(X[:, 0] < 0.5, 1.0, -1.0) + np.where(np.isnan(X[:, 2]), 2.0, 0.0) + np.where(X[:, 3] < -1, 1.5, 0.0)
         + 0.3 * rng.normal(size=n)).astype(np.float32)
    return X, y


@pytest.mark.parametrize("seed", range(12))
def test_fit_equals_bruteforce(seed):
    rng = np.random.default_rng(seed)
    n, depth = int(rng.integers(40, 301)), seed % 6 + 1
    X, y = small_problem(rng, n)
    nv = n // 3
    kw = dict(max_depth=depth, n_estimators=4, early_stopping_rounds=0, min_child_weight=float(rng.integers(1, 5)),
              eta=0.3, reg_alpha=float(rng.choice([0.0, 0.01, 0.5])), gamma=float(rng.choice([0.0, 0.5])))
    a = tm.fit(X[nv:], y[nv:], X[:nv], y[:nv], **kw)
    b = tm.fit_bruteforce(X[nv:], y[nv:], X[:nv], y[:nv], **kw)
    assert all(len(np.unique(X[nv:, f][~np.isnan(X[nv:, f])])) <= 256 for f in range(20))
    assert tm.same_fit(a, b)
    assert a["pred_train"].tobytes() == b["pred_train"].tobytes() and a["pred_val"].tobytes() == b["pred_val"].tobytes()
    assert a["n_trees"] == 4 and len(a["left"]) > 4  # something split
    # the running predictions are the tree-order float32 sum an independent evaluator gives
    arrays = [a[k] for k in ("left", "right", "feat", "value", "default_left", "tree_off")]
    pred, _ = sm.forest_predict(*arrays, a["base_score"], X[nv:])
    assert pred.tobytes() == a["pred_train"].tobytes()


def test_node_numbering_is_xgboosts(shipped):
    """Children of the split nodes in increasing parent id, left then right -- as the shipped trees."""
    rng = np.random.default_rng(5)
    X, y = small_problem(rng, 300)
    r = tm.fit(X, y, max_depth=5, n_estimators=3, early_stopping_rounds=0, min_child_weight=2.0, eta=0.3)

    def check(left, right):
        nxt = 1
        for k in range(len(left)):
            if left[k] != -1:
                assert (left[k], right[k]) == (nxt, nxt + 1)
                nxt += 2
        assert nxt == len(left)

    for t in range(r["n_trees"]):
        a, b = r["tree_off"][t], r["tree_off"][t + 1]
        assert b - a > 7
        check(r["left"][a:b], r["right"][a:b])
    for t in shipped["learner"]["gradient_booster"]["model"]["trees"]:
        check(t["left_children"], t["right_children"])


def test_min_child_weight_boundary():
    """4 rows on each side split at min_child_weight 4; 4 and 3 do not."""
    X = np.zeros((8, 20), np.float32)
    X[4:, 2] = 1.0
    y = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.float32)
    kw = dict(n_estimators=1, early_stopping_rounds=0, min_child_weight=4.0, reg_alpha=0.0, eta=1.0)
    r = tm.fit(X, y, **kw)
    assert r["left"].tolist() == [1, -1, -1] and r["feat"][0] == 2 and r["value"][0] == 1.0
    assert r["sum_hessian"].tolist() == [8.0, 4.0, 4.0]
    # w = -G / (H + 1): the left rows have g = 0.5 - 0 each
    assert r["value"][1:].tolist() == [np.float32(-2.0 / 5.0), np.float32(2.0 / 5.0)]
    assert r["base_weight"][0] == 0.0 and np.signbit(r["base_weight"][0])  # -T(0) / 9, as the shipped root
    r = tm.fit(X[:7], y[:7], **kw)
    assert r["left"].tolist() == [-1] and r["sum_hessian"].tolist() == [7.0]
    r = tm.fit(X[:7], y[:7], **dict(kw, min_child_weight=3.0))
    assert r["left"].tolist() == [1, -1, -1] and r["sum_hessian"].tolist() == [7.0, 4.0, 3.0]


def test_trees_are_best_plus_rounds_plus_one():
    rng = np.random.default_rng(2)
    X, y = small_problem(rng, 120)
    yv = rng.normal(size=60).astype(np.float32)  # nothing to learn: validation soon stops improving
    r = tm.fit(X[60:], y[60:], X[:60], yv, n_estimators=40, early_stopping_rounds=3, eta=0.5, min_child_weight=1.0)
    assert 0 <= r["best_iteration"] and r["n_trees"] == r["best_iteration"] + 3 + 1 < 40
    h = r["val_rmse"]
    assert len(h) == r["n_trees"] and r["best_score"] == h[r["best_iteration"]] == h.min()
    assert (h[r["best_iteration"] + 1:] >= r["best_score"]).all() and (h[:r["best_iteration"]] > r["best_score"]).all()
    # off: every round runs, the best round is still tracked
    r0 = tm.fit(X[60:], y[60:], X[:60], yv, n_estimators=12, early_stopping_rounds=0, eta=0.5, min_child_weight=1.0)
    assert r0["n_trees"] == 12 and r0["best_iteration"] == r["best_iteration"]
    with pytest.raises(ValueError):
        tm.fit(X, y, n_estimators=2, early_stopping_rounds=3)


def test_cuts_rule_at_256_and_257():
    X = np.zeros((300, 20), np.float32)
    X[:, 0] = np.minimum(np.arange(300), 255)       # 256 distinct values
    X[:, 1] = np.minimum(np.arange(300), 256)       # 257
    X[:, 2] = np.where(np.arange(300) % 2, -0.0, 0.0)  # one value
    X[:, 3] = np.nan
    X[:7, 4] = [3, np.nan, 1, 2, 2, np.inf, -np.inf]
    cuts = tm.make_cuts(X, 256)
    assert cuts[0].tolist() == list(range(1, 256))
    assert cuts[1].tolist() == list(range(2, 257))  # v[ceil(257 k / 256)] = v[k + 1]
    assert len(cuts[2]) == 0 and len(cuts[3]) == 0
    assert cuts[4].tolist() == [0.0, 1.0, 2.0, 3.0, np.inf]
    assert tm.make_cuts(X, 4)[0].tolist() == [64.0, 128.0, 192.0] and tm.make_cuts(X, 4)[4].dtype == np.float32


def keys_of(d, path=""):
    out = set()
    if isinstance(d, dict):
        for k, v in d.items():
            out.add(f"{path}/{k}")
            out |= keys_of(v, f"{path}/{k}")
    elif isinstance(d, list) and d and isinstance(d[0], dict):
        for v in d:
            out |= keys_of(v, f"{path}[]")
    return out


@pytest.fixture(scope="module")
def fitted():
    rng = np.random.default_rng(9)
    X, y = small_problem(rng, 200)
    r = tm.fit(X[50:], y[50:], X[:50], y[:50], n_estimators=8, early_stopping_rounds=3, eta=0.3)
    return X, y, r


def test_writers_match_the_shipped_layout(sgmm, shipped, fitted, tmp_path):
    from sgmm_amd import gate_units as gu
    X, y, r = fitted
    p = tmp_path / "model.json"
    tm.write_json(r, p, sm.FEATURES)
    with open(p) as fh:
        doc = json.load(fh)
    assert keys_of(doc) == keys_of(shipped)
    assert doc["version"] == shipped["version"]
    assert doc["learner"]["feature_names"] == shipped["learner"]["feature_names"]
    assert doc["learner"]["feature_types"] == shipped["learner"]["feature_types"]
    tree = doc["learner"]["gradient_booster"]["model"]["trees"][0]
    assert tree["tree_param"]["num_nodes"] == str(len(tree["left_children"])) and tree["parents"][0] == 2147483647
    for k, v in shipped["learner"]["gradient_booster"]["model"]["trees"][0].items():
        assert type(tree[k]) is type(v), k
    assert doc["learner"]["learner_model_param"]["base_score"].startswith("[") and \
        "E" in doc["learner"]["learner_model_param"]["base_score"]
    # the package's writer gives the same document
    assert gu.sgu1_json(r) == doc
    # the strict loader reads it back to the same arrays
    f = gu.SGU1Forest(str(p))
    for name, key in (("left", "left"), ("right", "right"), ("feat", "feat"), ("value", "value"),
                      ("default_left", "default_left"), ("tree_off", "tree_off")):
        assert np.asarray(getattr(f, name)).tobytes() == np.asarray(r[key]).astype(getattr(f, name).dtype).tobytes(), name
    assert f.base_score.tobytes() == r["base_score"].tobytes()
    assert f.best_iteration == r["best_iteration"] and f.n_trees == r["best_iteration"] + 1
    g = gu.SGU1()
    g.load(str(p))
    assert g.best_iteration == r["best_iteration"] and g.best_score == r["best_score"]
    g.save(str(tmp_path / "again.json"))
    with open(tmp_path / "again.json") as fh:
        assert json.load(fh) == doc


def test_xgboost_reads_the_file(fitted, tmp_path):
    xgb = pytest.importorskip("xgboost")
    X, y, r = fitted
    p = tmp_path / "model.json"
    tm.write_json(r, p, sm.FEATURES)
    booster = xgb.Booster()
    booster.load_model(str(p))
    got = booster.predict(xgb.DMatrix(X[50:], feature_names=list(sm.FEATURES)),
                          iteration_range=(0, r["n_trees"]))
    assert np.array_equal(got, r["pred_train"])


def test_sanity_on_a_planted_tree():
    """Labels from a planted depth-3 tree plus noise: the validation rmse falls below the
    base score's and some round improves on the first."""
    rng = np.random.default_rng(11)
    X = rng.normal(size=(900, 20)).astype(np.float32)
    leaf = (X[:, 3] < 0) * 4 + np.where(X[:, 3] < 0, X[:, 8] < 0.5, X[:, 1] < -0.2) * 2 + (X[:, 15] < 0.1)
    y = (np.array([-3, -1, 0, 2, 1, 4, -2, 3], np.float64)[leaf] + 0.3 * rng.normal(size=900)).astype(np.float32)
    r = tm.fit(X[300:], y[300:], X[:300], y[:300], max_depth=3, n_estimators=30, early_stopping_rounds=5, eta=0.3)
    base_rmse = tm.rmse_metric(np.full(300, r["base_score"], np.float32), y[:300])
    assert r["best_iteration"] > 0 and r["best_score"] < 0.5 * base_rmse
    # the order-free metric is the plain RMSE to about 2^-20 relative
    plain = float(np.sqrt(np.mean((r["pred_val"].astype(np.float64) - y[:300]) ** 2)))
    assert abs(r["val_rmse"][-1] - plain) <= 2.0 ** -18 * plain


# ---------------------------------------------------------------- the cases of the GPU tests reach their edges
#
# tests/test_gpu_sgu1_train.py compares the device with the model on the inputs of
# tests/sgu1_train_cases.py.  That says something only where the model, on that input,
# really takes the path the case is built for: asserted here, from the model alone.

def splits(r):
    return r["left"] != -1


def children(r):
    """Every node but the roots."""
    c = np.ones(len(r["left"]), bool)
    c[r["tree_off"][:-1]] = False
    return c


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5, 6])
def test_case_depths_reach_their_last_level(depth):
    """A: at every max_depth some tree has a node at that depth, so a launch of that depth
    alone needs the node tables of its own k_sgu1_train<D>."""
    r = sc.model(f"depth:{depth}")
    sizes = np.diff(r["tree_off"])
    deepest = max(len(sc.level_widths(r, t)[0]) - 1 for t in range(r["n_trees"]))
    print(f"depth {depth}: largest tree {sizes.max()} nodes, deepest level {deepest}")
    assert deepest == depth and 2 ** depth - 1 < sizes.max() <= 2 ** (depth + 1) - 1
    if depth > 1:
        assert not tm.same_fit(r, sc.model(f"depth:{depth - 1}"))


@pytest.mark.parametrize("variant", [1, 2])
def test_case_planted_levels_are_full(variant):
    """B: every tree has 32 nodes at depth 5 (the level searched one feature per pass, 20
    passes) and splits there on feature 19, the feature of the last pass; at max_depth 5 the
    last searched level has 16 nodes (two features per pass)."""
    r = sc.model(f"planted:{variant}:6")
    assert r["n_trees"] == 4
    for t in range(4):
        w, depth = sc.level_widths(r, t)
        a, b = r["tree_off"][t], r["tree_off"][t + 1]
        at5 = splits(r)[a:b] & (depth == 5)
        print(f"variant {variant} tree {t}: widths {w.tolist()}, features split at depth 5 "
              f"{sorted(set(r['feat'][a:b][at5].tolist()))}")
        assert w[:6].tolist() == [1, 2, 4, 8, 16, 32] and len(w) == 7
        assert 19 in r["feat"][a:b][at5]
        if variant == 1:
            assert w[6] == 64  # 127 nodes: every node of every level splits
    X, y, rt, _, _ = sc.case(f"planted:{variant}:6")
    assert set(np.unique(X[rt][:, sc.PLANTED_COLS]).tolist()) == {-1.0, 1.0}
    r5 = sc.model(f"planted:{variant}:5")
    for t in range(4):
        assert sc.level_widths(r5, t)[0].tolist() == [1, 2, 4, 8, 16, 32]


def test_case_planted_equals_bruteforce():
    X, y, rt, rv, p = sc.case("planted:1:6")
    assert all(len(np.unique(X[rt, f][~np.isnan(X[rt, f])])) <= 256 for f in range(20))
    b = sc.model_fit(X, y, rt, rv, p, fit=tm.fit_bruteforce)
    a = sc.model("planted:1:6")
    assert tm.same_fit(a, b) and a["pred_train"].tobytes() == b["pred_train"].tobytes()


@pytest.mark.parametrize("k", [30, 100, 124])
def test_case_scales_up_are_exact(k):
    """C: a power of two on the labels moves nothing but the scale -- the same trees, every
    leaf, prediction and rmse times 2^k exactly.  That pins the model without itself."""
    r0, r = sc.model("scale:0"), sc.model(f"scale:{k}")
    y0, y = sc.case("scale:0")[1], sc.case(f"scale:{k}")[1]
    assert y.dtype == np.float32 and np.isfinite(y).all()
    assert (y.astype(np.float64) == np.ldexp(y0.astype(np.float64), k)).all()
    for name in ("left", "right", "feat", "default_left", "tree_off"):
        assert r[name].tobytes() == r0[name].tobytes(), name
    leaf = ~splits(r0)
    assert r["value"][~leaf].tobytes() == r0["value"][~leaf].tobytes()  # thresholds: the features did not move
    assert r["value"][leaf].tobytes() == np.ldexp(r0["value"][leaf], k).tobytes()
    assert r["pred_train"].tobytes() == np.ldexp(r0["pred_train"], k).tobytes()
    assert r["pred_val"].tobytes() == np.ldexp(r0["pred_val"], k).tobytes()
    assert r["val_rmse"].tobytes() == np.ldexp(r0["val_rmse"], k).tobytes()
    assert (r["n_trees"], r["best_iteration"]) == (r0["n_trees"], r0["best_iteration"])
    n_inf = int(np.isinf(r["loss_change"]).sum())
    print(f"k {k}: {len(r['left'])} nodes, {r['n_trees']} trees, {n_inf} infinite loss_change")
    assert len(r["left"]) > 400 and r["n_trees"] == 16
    if k >= 100:
        assert n_inf > 0 and (r["loss_change"][np.isinf(r["loss_change"])] > 0).all()
    else:
        assert n_inf == 0


def test_case_scales_down_meet_the_absolute_rule():
    """C: the split rule score > 1e-6 is absolute.  Scores go with 2^2k: at 2^-6 every split
    of k = 0 still clears it on this table, 2^-7 is the nearest scale that loses some; at
    2^-100 and below nothing splits and the fit ends by early stopping; at 2^-140 the
    labels are subnormal."""
    n0 = int(splits(sc.model("scale:0")).sum())
    X, y, rt, rv, p = sc.case("scale:0")
    n6 = int(splits(sc.model_fit(X, np.ldexp(y, -6), rt, rv, p)).sum())
    n7 = int(splits(sc.model(f"scale:{sc.SMALL_SCALE}")).sum())
    print(f"split nodes: k 0 {n0}, k -6 {n6}, k {sc.SMALL_SCALE} {n7}")
    assert sc.SMALL_SCALE == -7 and n6 == n0 and 1 <= n7 < n0
    for k in (-100, -140):
        r = sc.model(f"scale:{k}")
        assert r["n_trees"] == r["best_iteration"] + 3 + 1 < 16 and len(r["left"]) == r["n_trees"]
        print(f"k {k}: {r['n_trees']} single-leaf trees")
    y = sc.case("scale:-140")[1][rt]
    assert ((y != 0) & (np.abs(y) < np.finfo(np.float32).tiny)).any()
    assert sc.SCALES == (-140, -100, -7, 0, 30, 100, 124)


def test_case_subnormal_scale_shows_the_exponent(monkeypatch):
    """C: at 2^-130 every label is subnormal and the metric has to round (a residual times
    2^s2 is no integer), so the exponent of a subnormal matters: the model with that exponent
    off by one, either way, gives another rmse.  At 2^-140 it gives the same bytes -- all
    quantisations are exact there -- which is why that scale alone would not pin it."""
    k = sc.SUBNORMAL_SCALE
    X, y, rt, rv, p = sc.case(f"scale:{k}")
    tiny = np.finfo(np.float32).tiny
    assert ((y[rt] != 0) & (np.abs(y[rt]) < tiny)).all() and ((y[rv] != 0) & (np.abs(y[rv]) < tiny)).all()
    want = sc.model(f"scale:{k}")
    r = (want["pred_val"] - y[rv]).astype(np.float64)
    e2 = tm._exponent(np.abs(r).max())
    scaled = np.ldexp(r, 20 - e2)
    print(f"k {k}: exponent of the largest residual {e2}, {int((scaled != np.rint(scaled)).sum())} of {len(r)} round")
    assert e2 <= -126 and (scaled != np.rint(scaled)).any()
    real, want140 = tm._exponent, sc.model("scale:-140")  # the shared fits are computed before the patch
    for delta in (1, -1):
        monkeypatch.setattr(tm, "_exponent", lambda m, d=delta: real(m) + (d if np.float32(m) < tiny else 0))
        assert sc.model_fit(X, y, rt, rv, p)["val_rmse"].tobytes() != want["val_rmse"].tobytes()
        assert tm.same_fit(sc.model_fit(*sc.case("scale:-140")), want140)


def away(x):
    """Round half away from zero: what round() does where rint goes to even."""
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def test_case_rounding_rounds_ties_and_passes_2_53():
    """D: base_score exactly 0; round-0 gradients that are exact ties; the left child of the
    root sums to more than 2^53 and float64 cannot hold the sum (here it lies halfway
    between two float64, a tie of its own).  And the properties that let a wrong rounding
    show: the tiny rows under that child end in a leaf of their own, whose sum differs
    between rint and round, is no multiple of 4, and stands in the leaf's value."""
    X, y, rt, rv, p = sc.case("rounding")
    r = sc.model("rounding")
    assert len(y) == 65538 and len(rt) == 65538 and len(rv) == 64
    assert tm.base_score(y) == 0.0 and not np.signbit(tm.base_score(y))
    g = np.float32(0.0) - y
    s = 40 - tm._exponent(np.abs(g).max())
    x = np.ldexp(g.astype(np.float64), s)
    q = np.rint(x).astype(np.int64)
    ties = np.abs(x) % 1 == 0.5
    assert s == 39 and ties.sum() == 2 * sc.N_TIE and (q[ties] != away(x[ties])).any()
    assert r["feat"][0] == 0 and r["value"][0] == 1.0 and r["left"][0] == 1
    L = X[:, 0] < r["value"][0]
    Q = int(q[L].sum())
    print(f"{int(ties.sum())} ties; |Q_L| = 2^{np.log2(abs(Q)):.2f}, Q_L mod 4 = {Q % 4}")
    assert abs(Q) >= 2 ** 53 and int(float(Q)) != Q
    assert 2 ** 54 <= abs(Q) < 2 ** 55 and Q % 4 == 2  # float64 steps by 4 here: halfway
    # node 1 (the left child) splits the tiny rows off: node 4 is their leaf
    tiny = L & (X[:, 1] == 3.0)
    assert (r["feat"][1], r["value"][1], r["left"][1], r["right"][1]) == (1, 3.0, 3, 4) and r["left"][4] == -1
    assert r["sum_hessian"][4] == tiny.sum() and (np.abs(y[tiny]) < 2.0 ** -33).all()
    Qt, Qt_away = int(q[tiny].sum()), int(away(x[tiny]).sum())
    print(f"tiny leaf: {int(tiny.sum())} rows, Q = {Qt} (rint), {Qt_away} (half away from zero)")
    assert Qt != Qt_away and Qt % 4 != 0
    want = np.float32(p["eta"] * -(np.ldexp(float(Qt), -s) / (float(tiny.sum()) + p["reg_lambda"])))
    assert r["value"][4].tobytes() == want.tobytes()
    assert want != np.float32(p["eta"] * -(np.ldexp(float(Qt_away), -s) / (float(tiny.sum()) + p["reg_lambda"])))
    assert want != np.float32(p["eta"] * -(np.ldexp(float(Qt & ~3), -s) / (float(tiny.sum()) + p["reg_lambda"])))
    assert r["n_trees"] == 2 and np.diff(r["tree_off"]).tolist() == [7, 7]


def test_case_inf_and_signed_zero_thresholds():
    """E: trained thresholds at +inf and at 0, the 0 never negative, and the brute-force
    model agrees (every column has at most 256 distinct values on the training rows)."""
    X, y, rt, rv, p = sc.case("inf")
    r = sc.model("inf")
    x4, x5 = X[rt, 4], X[rt, 5]
    assert (x4 == np.inf).sum() > 10 and (x4 == -np.inf).sum() > 10
    assert ((x5 == 0) & np.signbit(x5)).any() and ((x5 == 0) & ~np.signbit(x5)).any()
    inner = splits(r)
    zero = inner & (r["value"] == 0)
    n_inf, n_zero5 = int(np.isinf(r["value"][inner]).sum()), int((zero & (r["feat"] == 5)).sum())
    print(f"{n_inf} infinite thresholds, {n_zero5} zero thresholds on feature 5")
    assert n_inf > 0 and (r["feat"][inner & np.isinf(r["value"])] == 4).all()
    assert n_zero5 > 0 and not np.signbit(r["value"][zero]).any()
    assert all(len(np.unique(X[rt, f][~np.isnan(X[rt, f])])) <= 256 for f in range(20))
    b = sc.model_fit(X, y, rt, rv, p, fit=tm.fit_bruteforce)
    assert tm.same_fit(r, b) and r["pred_val"].tobytes() == b["pred_val"].tobytes()


def test_case_max_bin_cut_counts():
    X, _, rt, _ = sc.edge()
    assert len(np.unique(X[rt, 4])) > 256
    counts = [len(sc.model(f"max_bin:{b}")["cuts"][4]) for b in sc.MAX_BINS]
    print(f"cuts of column 4 at max_bin {sc.MAX_BINS}: {counts}")
    assert counts == [1, 2, 254, 255]
    for b in sc.MAX_BINS:
        r = sc.model(f"max_bin:{b}")
        assert (splits(r) & (r["feat"] == 4)).any()
        assert all(len(c) <= b - 1 for c in r["cuts"])
    assert len({sc.model(f"max_bin:{b}")["value"].tobytes() for b in sc.MAX_BINS}) == 4
    cuts = tm.make_cuts(sc.cuts_table(), 256)
    assert len(cuts[0]) == 255 and len(cuts[1]) == 255 and cuts[0][0] == 1 and cuts[1][0] == 2


def test_case_rows_and_tables():
    """F: what each case of the rows-and-tables launch is there for."""
    X, y, rt, rv = sc.edge()
    c = sc.case("second_table")
    assert len(c) == 7 and len(c[5]) != len(X) and c[3].max() < len(c[5]) and len(set(c[3].tolist())) < len(c[3])
    assert len(sc.model("second_table")["val_rmse"]) == 16
    assert len(sc.case("one_val_row")[3]) == 1 and len(sc.model("one_val_row")["pred_val"]) == 1
    rb = sc.case("bootstrap")[2]
    assert len(rb) == 300 and len(set(rb.tolist())) < 250 and set(rb.tolist()) <= set(rt.tolist())
    assert not tm.same_fit(sc.model("bootstrap"), sc.model("depth:4"))
    # 2.5 admits what 3 admits and not what 2 admits: the comparison is in float64, not truncated
    r = sc.model("mcw2.5")
    assert r["sum_hessian"][children(r)].min() == 3.0
    assert tm.same_fit(r, sc.model_fit(X, y, rt, rv, dict(sc.SMALL, min_child_weight=3.0)))
    assert not tm.same_fit(r, sc.model("depth:4")) and sc.case("depth:4")[4]["min_child_weight"] == 2.0
    # min_child_weight 0 admits empty children; they score 0 and never win
    r = sc.model("mcw0")
    print(f"min_child_weight 0: {len(r['left'])} nodes, smallest child {r['sum_hessian'][children(r)].min()}")
    assert r["sum_hessian"][children(r)].min() == 1.0 and len(r["left"]) > 1000


# ---------------------------------------------------------------- argument checks, no GPU

def host_task(_lib, **over):
    v = 256  # a non-null, 256-aligned stand-in: the checks never follow a pointer
    t = _lib.Sgu1Task(*([v] * 22), 10, 10, 8, 2, 4, 5, 3, 256, 0.0, 0.0, 4.0, 0.01, 1.0, 0.01, 0.0)
    for k, val in over.items():
        setattr(t, k, val)
    return t


@pytest.mark.parametrize("over,msg", [
    (dict(max_depth=7), b"max_depth"), (dict(max_depth=0), b"max_depth"), (dict(max_bin=257), b"max_bin"),
    (dict(max_bin=1), b"max_bin"), (dict(n_train=0), b"n_train"), (dict(n_train=(1 << 20) + 1), b"n_train"),
    (dict(n_val=-1), b"n_val"), (dict(n_val=0), b"validation rows"), (dict(early_stopping_rounds=-1), b"negative"),
    (dict(eta=float("nan")), b"not finite"), (dict(alpha=-1.0), b"negative"), (dict(lambda_=float("inf")), b"not finite"),
    (dict(lambda_=0.0, min_child_weight=0.0), b"both 0"), (dict(X_train=None), b"null training"),
    (dict(rows_val=None), b"null validation"), (dict(cuts=None), b"null cuts"), (dict(workspace=None), b"workspace"),
    (dict(workspace=260), b"workspace"), (dict(val_rmse=None), b"null output"), (dict(n_estimators=-1), b"n_estimators"),
    # the metric's int64 sum is safe up to 2^23 - 1 validation rows: 2^23 is refused, 2^23 - 1 gets past that check
    (dict(n_val=1 << 23), b"n_val"), (dict(n_val=(1 << 23) - 1, workspace=None), b"workspace"),
])
def test_c_abi_rejects_before_any_launch(sgmm, over, msg):
    from sgmm_amd import _lib
    L = _lib.load()
    tasks = (_lib.Sgu1Task * 2)(host_task(_lib), host_task(_lib, **over))
    rc = L.sgmm_sgu1_train(ctypes.c_void_p(256), tasks, 2, None)
    assert rc == -1 and msg in L.sgmm_last_error(), L.sgmm_last_error()


def test_c_abi_workspace_and_nulls(sgmm):
    from sgmm_amd import _lib
    L = _lib.load()
    assert ctypes.sizeof(_lib.Sgu1Task) == 264 and _lib.Sgu1Task.ld_train.offset == 176
    assert _lib.Sgu1Task.min_child_weight.offset == 224
    # pred, labels, missing mask (4 bytes each), node map (1, padded to 4), 20 bin bytes; 256-aligned
    assert L.sgmm_sgu1_train_workspace_bytes(8812, 2200) == (11012 * 12 + 11012 + 11012 * 20 + 255) // 256 * 256
    assert L.sgmm_sgu1_train_workspace_bytes(1, 0) == 256
    assert L.sgmm_sgu1_train_workspace_bytes(0, 5) == 0 and L.sgmm_sgu1_train_workspace_bytes(5, -1) == 0
    tasks = (_lib.Sgu1Task * 1)(host_task(_lib))
    assert L.sgmm_sgu1_train(None, tasks, 1, None) == -1 and b"null tasks" in L.sgmm_last_error()
    assert L.sgmm_sgu1_train(ctypes.c_void_p(256), tasks, 0, None) == -1 and b"n_tasks" in L.sgmm_last_error()


@pytest.mark.parametrize("params", [dict(subsample=0.5), dict(colsample_bytree=0.9), dict(objective="reg:absoluteerror"),
                                    dict(max_depth=7), dict(max_bin=257), dict(sample_weight=[1.0]),
                                    dict(learning_rate=float("nan")), dict(reg_alpha=-0.1), dict(n_estimators=0)])
def test_sgu1_rejects_what_the_trainer_does_not_do(sgmm, params):
    from sgmm_amd import gate_units as gu
    X = np.zeros((10, 20), np.float32)
    y = np.arange(10, dtype=np.float64)
    with pytest.raises(ValueError):
        gu.SGU1(**params).train(X, y, X, y)


def test_sgu1_rejects_bad_data(sgmm):
    from sgmm_amd import gate_units as gu
    X = np.zeros((10, 20), np.float32)
    y = np.arange(10, dtype=np.float64)
    m = gu.SGU1()
    assert m.params == {"max_depth": 4, "min_child_weight": 4, "subsample": 1.0, "colsample_bytree": 1.0,
                        "learning_rate": 0.01, "reg_alpha": 0.01, "objective": "reg:squarederror",
                        "n_estimators": 1000, "early_stopping_rounds": 20}
    bad = y.copy()
    bad[3] = np.inf
    for args in ((X, bad, X, y), (X, y, X, bad), (X, y, None, None), (X[:0], y[:0], X, y), (X[:, :19], y, X, y),
                 (X, y[:9], X, y)):
        with pytest.raises(ValueError):
            m.train(*args)
    with pytest.raises(ValueError):
        gu.run_sgu1_fits([dict(X_train=np.zeros((20, 10), np.float32), y_train=np.zeros(10, np.float32),
                               rows_train=np.array([0, 10]), params=gu.sgu1_fit_params(dict(gu.SGU1_PARAMS,
                                                                                             early_stopping_rounds=0)))])
    # 2^23 validation rows: the metric's int64 sum of squares could pass 2^63 (include/sgmm.h, n_val)
    many = 1 << 23
    assert gu.MAX_VAL_ROWS == many - 1 and (many - 1) << 40 < 1 << 63 <= many << 40
    with pytest.raises(ValueError, match=r"2\^23"):
        m.train(X, y, np.broadcast_to(np.float32(0), (many, 20)), np.broadcast_to(np.float64(0), (many,)))
    with pytest.raises(ValueError, match=r"2\^23"):
        gu.run_sgu1_fits([dict(X_train=np.zeros((20, 10), np.float32), y_train=np.zeros(10, np.float32),
                               rows_train=np.arange(10), X_val=np.zeros((20, 10), np.float32),
                               y_val=np.zeros(10, np.float32), rows_val=np.broadcast_to(np.int64(0), (many,)),
                               params=gu.sgu1_fit_params(gu.SGU1_PARAMS))])
    with pytest.raises(ValueError):
        m.predict(X)


def test_dropin_exports_the_device_model(sgmm):
    """models.GateUnits.SGU1GPU is gate_units.SGU1; the xgboost-backed SGU1 beside it is untouched."""
    import subprocess
    import sys
    root = Path(__file__).resolve().parent.parent
    code = (f"import sys; sys.path.insert(0, {str(root / 'dropin')!r}); from models.GateUnits import SGU1, SGU1GPU; "
            "import sgmm_amd.gate_units as gu; assert SGU1GPU is gu.SGU1 and SGU1 is not gu.SGU1; "
            "assert SGU1GPU().params == SGU1.PARAMS; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr
