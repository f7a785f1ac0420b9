"""Device strategy evaluation on the GPU: sgmm_rule_trace against the
reference's benchmark frames, sgmm_rollout_summary against the reference's
analytics (tests/golden/g9_evaluation.npz) and against the trace path."""
import numpy as np
import pytest
import torch

from conftest import has_gpu
from test_evaluation import SHARPE_RTOL, assert_summary, fixture_policies, fixture_rule

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

BUNDLE_COPIES = {"mid": "mid", "ask": "ask", "bid": "bid", "s1_pred": "s1", "s2_pred": "s2"}


@pytest.fixture(scope="module")
def g9(golden):
    return golden("g9_evaluation.npz")


@pytest.fixture(scope="module")
def g7(golden):
    return golden("g7_recorder.npz")


def bundle(g7):
    return tuple(g7[f"bundle_{k}"] for k in ("s1", "s2", "mid", "ask", "bid", "buy_max", "sell_min"))


def stats(g7):
    s = g7["stats"]
    return {"s1_m": np.float32(s[0]), "s1_s": np.float64(s[1]), "s2_m": np.float32(s[2]), "s2_s": np.float64(s[3])}


def stored_column(g9, g7, tag, c):
    """A rule frame's column: stored, or one of the copies the generator checked and left out."""
    if c in BUNDLE_COPIES:
        return g7[f"bundle_{BUNDLE_COPIES[c]}"]
    if c == "step":
        return np.arange(len(g7["bundle_mid"]))
    if c == "realized_pnl":
        return g9[f"{tag}__cash"]
    if c == "action":
        return np.stack([g9[f"{tag}__off_a"], g9[f"{tag}__off_b"]], 1)
    return g9[f"{tag}__{c}"]


def assert_rule_frame(df, g9, g7, tag):
    cols = [str(c) for c in g9[f"{tag}__columns"]]
    assert list(df.columns) == cols
    for c, dt in zip(cols, g9[f"{tag}__dtypes"]):
        v = df[c].to_numpy()
        if v.dtype == object:
            v = np.stack([np.asarray(x) for x in v])
        want = stored_column(g9, g7, tag, c)
        assert v.shape == want.shape and np.array_equal(v.astype(np.float64), want.astype(np.float64)), (tag, c)
        assert str(df[c].dtype) == str(dt), (tag, c, df[c].dtype, dt)


def rule_frames(g9):
    """(tag, rule index, phi, fee) of the fixture's rule frames."""
    return [(str(t), int(r), float(pf[0]), float(pf[1]))
            for t, r, pf in zip(g9["frame_tags"], g9["frame_rule"], g9["frame_phi_fee"]) if r >= 0]


def test_rule_trace_frames_match_reference(sgmm, g9, g7):
    """Every benchmark backtest of the fixture in ONE sgmm_rule_trace launch,
    rule tables as the reference computed them."""
    from sgmm_amd.recorder import run_rule_backtests
    fr = rule_frames(g9)
    assert len(fr) == 11
    dfs = run_rule_backtests([fixture_rule(g9, r) for _, r, _, _ in fr], bundle(g7), [f[2] for f in fr],
                             [f[3] for f in fr], 0.001, stats(g7))
    for df, (tag, _, _, _) in zip(dfs, fr):
        assert_rule_frame(df, g9, g7, tag)


@pytest.mark.parametrize("name,tag", [("glft", "glft_p0"), ("foic", "foic_1_m1_p1")])
def test_run_benchmark_and_save_round_trips(sgmm, g9, g7, tmp_path, name, tag):
    import pandas as pd
    from sgmm_amd import benchmarks as B
    from sgmm_amd.recorder import run_benchmark_and_save
    pol = fixture_policies(B)[tag[:-3]]
    phi, fee = [(f[2], f[3]) for f in rule_frames(g9) if f[0] == tag][0]
    df = run_benchmark_and_save(name, pol, bundle(g7), phi, fee, str(tmp_path / name), stats(g7))
    back = pd.read_parquet(tmp_path / name / f"backtest_{phi}.parquet")
    assert_rule_frame(df, g9, g7, tag)
    assert_rule_frame(back, g9, g7, tag)


def test_summary_matches_reference_analytics(sgmm, g9, g7):
    """Every analytics case of the fixture -- full length and every prefix --
    in one launch per policy kind, lengths mixed."""
    dev = torch.device("cuda:0")
    tags = [str(t) for t in g9["frame_tags"]]
    ts = sgmm.TickStore()
    ts.add(bundle(g7), stats(g7))
    ts.to(dev)
    pf = g9["frame_phi_fee"]
    params = sgmm.params_tensor([sgmm.EnvConfig(phi=float(p), tick_size=0.001, fee_rate=float(f)) for p, f in pf], dev)
    eng = sgmm.RolloutEngine(dev)
    frame, T = g9["an_frame"], g9["an_T"]
    is_rule = g9["frame_rule"][frame] >= 0
    n_rules = len(g9["rule_names"])
    for kind in (False, True):
        idx = np.nonzero(is_rule == kind)[0]
        genome = g9["frame_rule"][frame[idx]] if kind else np.zeros(len(idx))
        eps = sgmm.EpisodeBatch(genome, np.zeros(len(idx)), T[idx], frame[idx]).to(dev)
        assert len(set(T[idx].tolist())) >= 8
        if kind:
            rules = np.stack([fixture_rule(g9, i) for i in range(n_rules)])
            raw, got = eng.summary(ts, eps, params, rules=rules)
        else:
            mm = torch.from_numpy(g7["genome"][None]).to(dev)
            raw, got = eng.summary(ts, eps, params, mm=mm, hidden=32)
        assert raw.shape == (len(idx), 96) and raw.is_cuda
        for j, k in enumerate(idx):
            assert_summary(got[j], g9, int(k), f"{tags[int(frame[k])]}[:{int(T[k])}]")


def assert_equals_mirror(got, want, what):
    from sgmm_amd.analytics import EXACT_FIELDS, SHARPE_FIELDS
    for f in EXACT_FIELDS:
        assert got[f] == want[f] or (np.isnan(got[f]) and np.isnan(want[f])), (what, f, got[f], want[f])
    for f in SHARPE_FIELDS:
        assert np.allclose(got[f], want[f], rtol=SHARPE_RTOL, atol=0.0, equal_nan=True), (what, f, got[f], want[f])


LENGTHS = (1, 2, 63, 64, 65, 200)
PARAM_SETS = ((0.0001, 0.0), (0.001, 0.0003), (0.01, 0.0))


@pytest.fixture(scope="module")
def synth(sgmm):
    from sgmm_amd import synthetic
    b = synthetic.bundle_510300(200, seed=11, nan_frac=0.005)
    assert np.isnan(b[5]).any() or np.isnan(b[6]).any()
    return b, synthetic.train_stats(b)


@pytest.mark.parametrize("H", [8, 16, 32, 64])
def test_summary_equals_trace(sgmm, synth, H):
    """Internal consistency: the summary equals the host mirror over the trace
    columns, for every hidden size, length, parameter set and inventory cap; one
    genome saturates its outputs far beyond any 16-bit action."""
    from sgmm_amd import synthetic
    from sgmm_amd.analytics import summary_from_frame
    dev = torch.device("cuda:0")
    b, st = synth
    pop = synthetic.population(4, H, sigma=0.3, seed=H)
    pop[3] *= 200.0
    mm = pop.to(dev).contiguous()
    ts = sgmm.TickStore()
    ts.add(b, st)
    ts.to(dev)
    eng = sgmm.RolloutEngine(dev)
    g, ln, pr = (a.reshape(-1) for a in np.meshgrid(np.arange(4), LENGTHS, np.arange(len(PARAM_SETS)), indexing="ij"))
    big = 0
    for cap in (1, 2, 3):
        params = sgmm.params_tensor([sgmm.EnvConfig(phi=p, tick_size=0.001, fee_rate=f, i_max=cap, i_min=-cap)
                                     for p, f in PARAM_SETS], dev)
        eps = sgmm.EpisodeBatch(g, np.zeros(len(g)), ln, pr, inv_min=-cap, inv_max=cap).to(dev)
        _, got = eng.summary(ts, eps, params, mm=mm, hidden=H)
        fit, trd, tr = eng.trace(ts, eps, params, mm, H)
        ffit, ftrd = eng.fitness(ts, eps, params, mm, H)
        host = {k: v.cpu().numpy() for k, v in tr.items()}
        assert np.array_equal(got["fitness"], ffit.cpu().numpy()) and np.array_equal(got["trade_rows"], ftrd.cpu().numpy())
        assert np.array_equal(got["fitness"], fit.cpu().numpy()) and np.array_equal(got["trade_rows"], trd.cpu().numpy())
        for e in range(eps.n):
            a, T = int(eps.step_off[e]), int(eps.length[e])
            cols = {k: host[k][a:a + T] for k in ("cash", "inventory", "reward", "fill_buy", "fill_sell")}
            cols["mid"] = b[2][:T]
            assert np.abs(cols["inventory"]).max() <= cap
            assert_equals_mirror(got[e], summary_from_frame(cols), (H, cap, e))
            big = max(big, int(np.abs(host["off_a"][a:a + T]).max()))
    assert big > 40000


def test_rule_summary_equals_rule_trace(sgmm, synth):
    """130 rules in one launch: more than two waves at one lane per episode,
    the last one ragged; lengths mixed."""
    from sgmm_amd import benchmarks as B
    from sgmm_amd.analytics import summary_from_frame
    dev = torch.device("cuda:0")
    b, st = synth
    rng = np.random.default_rng(5)
    rules = []
    for i in range(130):
        if i % 2:
            rules.append(B.quote_rule(B.FOICPolicy(int(rng.integers(-2, 3)), int(rng.integers(-2, 3)))))
        else:
            rules.append(B.quote_rule(B.GLFTPolicy(gamma=1e-4, kappa=3000, A=0.1, sigma=float(rng.uniform(5e-4, 3.0)))))
    rules = np.stack(rules)
    ts = sgmm.TickStore()
    ts.add(b, st)
    ts.to(dev)
    params = sgmm.params_tensor([sgmm.EnvConfig(phi=p, tick_size=0.001, fee_rate=f) for p, f in PARAM_SETS], dev)
    ln = np.array(LENGTHS)[np.arange(130) % len(LENGTHS)]
    eps = sgmm.EpisodeBatch(np.arange(130), np.zeros(130), ln, np.arange(130) % 3).to(dev)
    eng = sgmm.RolloutEngine(dev)
    _, got = eng.summary(ts, eps, params, rules=rules)
    fit, trd, tr = eng.trace_rules(ts, eps, params, rules)
    host = {k: v.cpu().numpy() for k, v in tr.items()}
    assert np.array_equal(got["fitness"], fit.cpu().numpy()) and np.array_equal(got["trade_rows"], trd.cpu().numpy())
    offs = set()
    for e in range(130):
        a, T = int(eps.step_off[e]), int(eps.length[e])
        cols = {k: host[k][a:a + T] for k in ("cash", "inventory", "reward", "fill_buy", "fill_sell")}
        cols["mid"] = b[2][:T]
        assert_equals_mirror(got[e], summary_from_frame(cols), e)
        inv_prev = np.concatenate([[0], cols["inventory"][:-1]])
        oa, ob = B.rule_offsets(rules[e], inv_prev, b[3][:T], b[4][:T])
        assert np.array_equal(oa, host["off_a"][a:a + T]) and np.array_equal(ob, host["off_b"][a:a + T]), e
        offs |= set(oa.tolist())
    assert len(offs) > 4 and got["trade_rows"].max() > 50
    # rule indices outside the table: refused on the host, and never read by the kernel
    bad = sgmm.EpisodeBatch([0, 130, 5, -1], np.zeros(4), np.full(4, 64), np.zeros(4)).to(dev)
    with pytest.raises(ValueError, match="rule indices"):
        eng.summary(ts, bad, params, rules=rules)
    import ctypes
    from sgmm_amd._lib import check, ptr, stream_ptr
    from sgmm_amd.rollout import SUMMARY_DTYPE
    out = torch.zeros((4, 96), dtype=torch.uint8, device=dev)
    drules = torch.from_numpy(rules.view(np.uint8).copy()).to(dev)
    tk, ep = ts.struct(), bad.struct()
    check(eng.L.sgmm_rollout_summary(ctypes.byref(tk), ctypes.byref(ep), ptr(params), None, 0, 0, ptr(drules),
                                     rules.ctypes.data, 130, ptr(out), stream_ptr()), "sgmm_rollout_summary")
    s = out.cpu().numpy().reshape(-1).view(SUMMARY_DTYPE)
    assert list(s["steps"]) == [64, 0, 64, 0] and list(s["fitness"][[1, 3]]) == [-50.0, -50.0]
    assert s["trade_rows"][1] == 0 and s["total_pnl"][3] == 0.0


def test_summarize_mixes_policies_and_rules_in_order(sgmm, g9, g7):
    from sgmm_amd import benchmarks as B
    from sgmm_amd.analytics import summarize, summary_rows
    pols = fixture_policies(B)
    tags = [str(t) for t in g9["frame_tags"]]
    order = ["glft_p1", "main_1", "foic_1_m1_p1", "main_1", "foic_50_50_p1", "glft_skew_p1"]
    items = [g7["genome"] if t.startswith("main") else
             (pols[t[:-3]] if "foic" in t else fixture_rule(g9, list(g9["rule_names"]).index(t[:-3]))) for t in order]
    df = summarize(items, bundle(g7), stats(g7), 0.001, 0.0003)
    assert len(df) == len(order)
    full = {tags[int(f)]: k for k, (f, T) in enumerate(zip(g9["an_frame"], g9["an_T"])) if T == len(g7["bundle_mid"])}
    for row, t in zip(df.to_dict("records"), order):
        k = full[t]
        assert row["Total PnL"] == g9["an_total_pnl"][k] and row["MAP (Risk)"] == g9["an_map"][k], t
        assert row["PnLMAP (Eff)"] == g9["an_pnl_to_map"][k] and row["Max DD"] == g9["an_max_dd"][k], t
        assert row["Trades"] == g9["an_trades"][k] and row["Fills"] == g9["an_clean_fills"][k], t
        assert row["PnL-to-MAP (floor)"] == g9["an_clean_pnl_to_map"][k], t
        assert np.allclose(row["Sharpe"], g9["an_sharpe"][k], rtol=SHARPE_RTOL, atol=0.0, equal_nan=True), t
        assert np.allclose(row["Sharpe (steps)"], g9["an_clean_sharpe"][k], rtol=SHARPE_RTOL, atol=0.0, equal_nan=True), t
    assert list(df.columns) == list(summary_rows(np.zeros(0, sgmm.rollout.SUMMARY_DTYPE)).columns)
