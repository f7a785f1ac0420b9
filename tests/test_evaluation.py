"""Strategy evaluation without a GPU (tests/golden/g9_evaluation.npz,
gen_golden_eval.py): the benchmark policies' quote tables, the rule arithmetic
against the reference's own backtest files, the host mirror of the device
summary against the reference's analytics, and the C ABI's argument checks."""
import ctypes

import numpy as np
import pytest

SHARPE_RTOL = 1e-9  # one-pass vs two-pass mean / variance over n <= 5472 doubles: ~n * 2^-53 * kappa


@pytest.fixture(scope="module")
def g9(golden):
    return golden("g9_evaluation.npz")


@pytest.fixture(scope="module")
def g7(golden):
    return golden("g7_recorder.npz")


def fixture_policies(B):
    return {"glft": B.GLFTPolicy(gamma=1e-4, kappa=3000, A=0.1, sigma=5e-4),
            "glft_wide": B.GLFTPolicy(gamma=1e-4, kappa=3000, A=0.1, sigma=5e-3),
            "glft_skew": B.GLFTPolicy(gamma=1e-4, kappa=3000, A=0.1, sigma=2.0),
            "foic_0_0": B.FOICPolicy(0, 0), "foic_1_m1": B.FOICPolicy(1, -1), "foic_50_50": B.FOICPolicy(50, 50)}


def fixture_rule(g9, i, inv_min=-2, inv_max=2):
    """Rule record of fixture rule i from the STORED reference get_action values."""
    from sgmm_amd.benchmarks import QUOTE_RULE_DTYPE
    q = list(g9["rule_inventory"])
    a, b = q.index(inv_min), q.index(inv_max) + 1
    r = np.zeros((), QUOTE_RULE_DTYPE)
    r["mode"], r["n_inventory"], r["quote_tick"] = int(g9["rule_glft"][i]), b - a, 0.001
    r["ask"][:b - a], r["bid"][:b - a] = g9["rule_ask"][i, a:b], g9["rule_bid"][i, a:b]
    return r


def frame_columns(g9, g7, tag):
    """cash / inventory / mid / reward / fills of a stored frame (g7's main_* or a g9 rule frame)."""
    src = g7 if tag.startswith("main_") else g9
    cols = {k: src[f"{tag}__{k}"] for k in ("cash", "inventory", "reward", "fill_buy", "fill_sell")}
    cols["mid"] = g7["bundle_mid"]
    return cols


def ulp_diff(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_quote_rule_tables_match_reference_get_action(sgmm, g9):
    from sgmm_amd import benchmarks as B
    pols = fixture_policies(B)
    assert set(pols) == {str(n) for n in g9["rule_names"]}
    for i, name in enumerate(g9["rule_names"]):
        pol = pols[str(name)]
        got = np.array([pol.get_action(int(q)) for q in g9["rule_inventory"]], np.float64)
        assert ulp_diff(got[:, 0], g9["rule_ask"][i]).max() <= 2, name
        assert ulp_diff(got[:, 1], g9["rule_bid"][i]).max() <= 2, name
        for lo, hi in ((-2, 2), (-3, 3), (-1, 1)):
            r = B.quote_rule(pol, lo, hi)
            want = fixture_rule(g9, i, lo, hi)
            n = hi - lo + 1
            assert int(r["n_inventory"]) == n and int(r["mode"]) == int(g9["rule_glft"][i])
            assert ulp_diff(r["ask"][:n], want["ask"][:n]).max() <= 2
            assert ulp_diff(r["bid"][:n], want["bid"][:n]).max() <= 2
            assert not r["ask"][n:].any() and not r["bid"][n:].any()
    assert B.quote_rule(pols["glft"], mode=0)["mode"] == 0
    for bad in (dict(inv_min=1), dict(inv_max=6), dict(quote_tick=0.0), dict(mode=2)):
        with pytest.raises(ValueError):
            B.quote_rule(pols["glft"], **bad)


@pytest.mark.parametrize("method,rule_name", [("glft", "glft"), ("foic", "foic_0_0")])
def test_rule_arithmetic_reproduces_reference_backtest_files(sgmm, g9, method, rule_name):
    """The reference's own output/510300/{glft,foic} files: from the previous
    step's inventory and the tick's ask / bid, modes 1 and 0 give the recorded
    offsets on every row."""
    from sgmm_amd.benchmarks import rule_offsets
    i = [str(n) for n in g9["rule_names"]].index(rule_name)
    pq = {c: g9[f"pq_{method}__{c}"] for c in ("ask", "bid", "inventory", "off_a", "off_b")}
    inv_prev = np.concatenate([[0], pq["inventory"][:-1]])
    oa, ob = rule_offsets(fixture_rule(g9, i), inv_prev, pq["ask"], pq["bid"])
    assert len(oa) == 960
    assert int((oa == pq["off_a"]).sum()) == 960 and int((ob == pq["off_b"]).sum()) == 960


def assert_summary(got, g9, k, what):
    """A SUMMARY_DTYPE record against analytics case k of the fixture."""
    for field, ref in (("total_pnl", "total_pnl"), ("map", "map"), ("pnl_to_map", "pnl_to_map"),
                       ("max_dd", "max_dd"), ("pnl_to_map_floor", "clean_pnl_to_map")):
        assert float(got[field]) == float(g9[f"an_{ref}"][k]), (what, field, float(got[field]), g9[f"an_{ref}"][k])
    assert int(got["trade_rows"]) == int(g9["an_trades"][k]), what
    assert int(got["fills_buy"]) == int(g9["an_fills_buy"][k]) and int(got["fills_sell"]) == int(g9["an_fills_sell"][k])
    assert int(got["fills_buy"]) + int(got["fills_sell"]) == int(g9["an_clean_fills"][k]), what
    assert int(got["steps"]) == int(g9["an_T"][k])
    for field, ref in (("sharpe_trades", "sharpe"), ("sharpe_steps", "clean_sharpe")):
        a, b = float(got[field]), float(g9[f"an_{ref}"][k])
        print(f"{what} {field}: {a!r} vs {b!r}")
        assert np.allclose(a, b, rtol=SHARPE_RTOL, atol=0.0, equal_nan=True), (what, field, a, b)


def test_summary_from_frame_matches_reference_analytics(sgmm, g9, g7):
    from sgmm_amd.analytics import summary_from_frame
    tags = [str(t) for t in g9["frame_tags"]]
    seen = set()
    for k in range(len(g9["an_T"])):
        tag, T = tags[int(g9["an_frame"][k])], int(g9["an_T"][k])
        cols = {c: v[:T] for c, v in frame_columns(g9, g7, tag).items()}
        got = summary_from_frame(cols)
        assert_summary(got, g9, k, f"{tag}[:{T}]")
        assert float(got["final_cash"]) == float(cols["cash"][-1]) and int(got["final_inventory"]) == int(cols["inventory"][-1])
        rows = int(got["trade_rows"])
        total = 0.0
        for r in cols["reward"]:
            total += float(r)
        assert float(got["fitness"]) == (total - 50.0 if rows == 0 else total)
        seen |= {f"rows{min(rows, 3)}", f"T{min(T, 3)}", f"map0={float(got['map']) == 0}"}
    assert {"rows0", "rows1", "rows2", "rows3", "T1", "T2", "T3", "map0=True", "map0=False"} <= seen
    # the blind schema has is_trade only: same numbers, fills unknown
    cols = frame_columns(g9, g7, "main_1")
    blind = {k: v for k, v in cols.items() if not k.startswith("fill_")}
    blind["is_trade"] = cols["fill_buy"] | cols["fill_sell"]
    a, b = summary_from_frame(cols), summary_from_frame(blind)
    assert int(b["fills_buy"]) == -1 and float(a["sharpe_trades"]) == float(b["sharpe_trades"])


def test_summary_rows_carry_the_reference_keys(sgmm):
    from sgmm_amd.analytics import summary_rows
    from sgmm_amd.rollout import SUMMARY_DTYPE
    s = np.zeros(2, SUMMARY_DTYPE)
    s["fills_buy"], s["fills_sell"], s["trade_rows"] = [3, 1], [2, 0], [4, 1]
    df = summary_rows(s)
    assert list(df.columns) == ["Total PnL", "MAP (Risk)", "PnLMAP (Eff)", "Max DD", "Sharpe", "Trades",
                                "Sharpe (steps)", "PnL-to-MAP (floor)", "Fills", "fitness"]
    assert list(df["Fills"]) == [5, 1] and list(df["Trades"]) == [4, 1]


def test_struct_sizes_and_argument_errors_need_no_gpu(sgmm):
    from sgmm_amd import _lib
    from sgmm_amd.benchmarks import QUOTE_RULE_DTYPE, FOICPolicy, GLFTPolicy, quote_rule
    from sgmm_amd.rollout import SUMMARY_DTYPE
    assert ctypes.sizeof(_lib.QuoteRule) == 144 == QUOTE_RULE_DTYPE.itemsize and _lib.QuoteRule.ask.offset == 16
    assert ctypes.sizeof(_lib.EpisodeSummary) == 96 == SUMMARY_DTYPE.itemsize
    assert _lib.EpisodeSummary.trade_rows.offset == 72 == SUMMARY_DTYPE.fields["trade_rows"][1]
    L = _lib.load()
    assert L.sgmm_abi_version() == 5
    v = ctypes.c_void_p(8)  # never dereferenced: every call below fails its argument check
    tk = _lib.Ticks(*[8] * 7)
    ep = _lib.Episodes(1, 10, 10, -2, 2, 8, None, 8, 8, 8, 8, None)
    summary = lambda mm, hidden, rules, host=None, n=0: L.sgmm_rollout_summary(  # noqa: E731
        ctypes.byref(tk), ctypes.byref(ep), v, mm, 4096, hidden, rules, host, n, v, None)
    err = lambda: L.sgmm_last_error()  # noqa: E731
    assert summary(v, 32, v) == -1 and b"exactly one" in err()       # both
    assert summary(None, 32, None) == -1 and b"exactly one" in err()  # neither
    assert summary(v, 12, None) == -1 and b"hidden" in err()
    assert summary(v, 64, None) == -1 and b"stride" in err()          # 4096 < 64*64 + 7*64 + 2

    def host(*rules):
        a = np.stack(rules)
        return a, a.ctypes.data

    keep, p = host(quote_rule(FOICPolicy(), -1, 1))                   # 3 inventory values, the batch has 5
    assert summary(None, 0, v, p, 1) == -1 and b"n_inventory" in err()
    bad = quote_rule(GLFTPolicy())
    bad["quote_tick"] = 0.0
    keep, p = host(quote_rule(FOICPolicy()), bad)
    assert summary(None, 0, v, p, 2) == -1 and b"quote_tick" in err() and b"rule 1" in err()
    bad["quote_tick"], bad["mode"] = 0.001, 3
    keep, p = host(bad)
    assert summary(None, 0, v, p, 1) == -1 and b"mode" in err()
    assert summary(None, 0, v, p, 0) == -1 and b"n_rules" in err()
    trace = lambda rules, hp, n: L.sgmm_rule_trace(ctypes.byref(tk), ctypes.byref(ep), v, rules, hp, n,  # noqa: E731
                                                   *[None] * 11, None)
    assert trace(None, None, 0) == -1 and b"null rules" in err()
    assert trace(v, p, 1) == -1 and b"mode" in err()
    keep, p = host(quote_rule(FOICPolicy(), -3, 3))
    assert trace(v, p, 1) == -1 and b"n_inventory" in err()
    wide = _lib.Episodes(1, 10, 10, -5, 5, 8, None, 8, 8, 8, 8, None)
    assert L.sgmm_rule_trace(ctypes.byref(tk), ctypes.byref(wide), v, v, None, 0, *[None] * 11, None) == -1
    assert b"inventory range" in err()


def test_dropin_reexports_the_benchmark_policies(sgmm):
    import importlib.util
    from pathlib import Path
    path = Path(__file__).resolve().parent.parent / "dropin" / "Env" / "benchmarks.py"
    spec = importlib.util.spec_from_file_location("_dropin_benchmarks", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.GLFTPolicy is sgmm.GLFTPolicy and mod.FOICPolicy is sgmm.FOICPolicy
    assert np.array_equal(mod.FOICPolicy(1, -1).get_action(2), [1, -1])
