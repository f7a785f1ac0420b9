"""Measurement of the strategy-evaluation kernels on one MI355X.

    python tools/bench_evaluation.py [--reps 20] [--out profiles/evaluation_bench.json]

Batch: 2560 episodes x 912 ticks, H = 32 (config 3's validation shape), on a
synthetic 510300-shaped bundle.  Timed, alternating within each repetition so
that drift hits both alike:
  summary_mlp     sgmm_rollout_summary   (k_summary_mlp<32>)
  rollout_direct  sgmm_rollout_trace     (k_rollout_direct<32>, 13 columns)
and, on their own:
  summary_rule    sgmm_rollout_summary over 4096 GLFT rules x 912 ticks
  host route      64 episodes: trace + device-to-host copy + frame assembly
                  (recorder.run_backtests), then per frame the pandas
                  operations of the reference's StrategyAnalytics.summary_dict
                  and get_clean_stats -- wall clock, ends in a synchronise
Kernel times are the library's own HIP events around each launch
(sgmm_profile_*): --warmup untimed launches, then --reps timed ones; median,
min and max over the repetitions are reported.  The summaries of the timed
batch are also compared with the trace path's fitness (bit-equal or the run
fails).

The hypothesis tests (--only hypothesis runs these alone; written to
profiles/hypothesis_bench.json):
  mbb_main        sgmm_mbb_sharpe at main.py's shape: 4 series x 960 rows,
                  block 100, 500 resamples (k_mbb_returns, k_mbb_replicates,
                  k_mbb_reduce: the three launches timed by their own events)
  mbb_sweep       the same at 2560 series x 912 rows
  numpy loop      get_mbb_sharpe's loop in numpy on the host (one np.concatenate,
                  np.std and np.mean per resample) for the 4 series, and for 64
                  of the sweep's -- wall clock
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def pandas_summary(df):
    """What the reference reports of one frame, with its pandas operations."""
    w = df["wealth"]
    tr = df[(df["fill_buy"] | df["fill_sell"]) == 1]
    m = df["inventory"].abs().mean()
    pnl = w.iloc[-1] - w.iloc[0]
    d = tr["wealth"].diff().dropna()
    sd = d.std() if len(tr) >= 2 else 0.0
    ret = w.diff().dropna()
    return {"Total PnL": pnl, "MAP (Risk)": m, "PnLMAP (Eff)": 0.0 if m == 0 else pnl / m,
            "Max DD": (w - w.cummax()).min(), "Sharpe": 0.0 if (len(tr) < 2 or sd == 0) else d.mean() / sd,
            "Trades": len(tr), "Sharpe (steps)": ret.mean() / (ret.std() + 1e-9),
            "PnL-to-MAP (floor)": (pnl / np.maximum(df["inventory"].abs().expanding().mean(), 1e-2)).iloc[-1],
            "Fills": int(df["fill_buy"].sum() + df["fill_sell"].sum())}


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "reps": len(a)}


def numpy_mbb(w, block_size=100, n_boot=500):
    """main.py:251-285 in numpy: the loop a user runs on the host today."""
    r = w[1:] / w[:-1] - 1.0
    r = r[~np.isnan(r)]
    n = len(r)
    if n <= block_size:
        sd = np.std(r)
        sr = np.mean(r) / sd if sd > 1e-9 else 0
        return sr, (sr, sr)
    srs = []
    for _ in range(n_boot):
        idx = np.random.randint(0, n - block_size + 1, size=max(1, n // block_size))
        x = np.concatenate([r[i:i + block_size] for i in idx])
        sd = np.std(x)
        srs.append(np.mean(x) / sd if sd > 1e-9 else 0)
    return np.mean(srs), np.percentile(srs, [2.5, 97.5])


def bench_hypothesis(a, sgmm, _lib, dev):
    """The bootstrap at main.py's shape and at a sweep's; HIP events per launch."""
    eng = sgmm.RolloutEngine(dev)
    rng = np.random.default_rng(9)
    kinds = ("mbb_returns", "mbb_replicates", "mbb_reduce")
    res = {"device": torch.cuda.get_device_name(0), "block_size": 100, "n_boot": 500}
    for name, n_series, rows, n_host in (("mbb_main", 4, 960, 4), ("mbb_sweep", a.episodes, a.ticks, 64)):
        wealth = 100.0 + np.cumsum(rng.normal(0.01, 0.3, (n_series, rows)), axis=1)
        w = torch.from_numpy(wealth.reshape(-1)).to(dev)
        off = np.arange(n_series + 1, dtype=np.int64) * rows
        for _ in range(a.warmup):
            out = eng.mbb_sharpe(w, off, 100, 500, seed=1)
        torch.cuda.synchronize()
        _lib.profile_read()
        ms = {k: [] for k in kinds + ("total",)}
        _lib.profile_enable(True)
        for _ in range(a.reps):
            out = eng.mbb_sharpe(w, off, 100, 500, seed=1)
            torch.cuda.synchronize()
            got = {k: v[0] / v[1] for k, v in _lib.profile_read().items()}
            for k in kinds:
                ms[k].append(got[k])
            ms["total"].append(sum(got[k] for k in kinds))
        _lib.profile_enable(False)
        rec = out.records()
        nb = (rows - 1) // 100
        reads = n_series * 500 * nb * 100 * 2 * 8
        t0 = time.perf_counter()
        host = [numpy_mbb(wealth[i]) for i in range(n_host)]
        host_s = time.perf_counter() - t0
        # same estimator, different random starts: the two means agree within the bootstrap's spread
        gap = float(np.max(np.abs(rec["mean_sr"][:n_host] - np.array([h[0] for h in host]))))
        med = float(np.median(ms["total"]))
        res[name] = {"series": n_series, "rows": rows, **{k: stats(v) for k, v in ms.items()},
                     "replicate_reads_bytes": reads,
                     "replicate_read_TBps": reads / (float(np.median(ms["mbb_replicates"])) * 1e-3) / 1e12,
                     "series_per_s": n_series / (med * 1e-3),
                     "numpy_loop": {"series": n_host, "wall_s": host_s, "per_series_ms": 1e3 * host_s / n_host,
                                    "max_abs_mean_gap_to_device": gap}}
    print(json.dumps(res))
    out_path = Path(a.hypothesis_out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--episodes", type=int, default=2560)
    ap.add_argument("--ticks", type=int, default=912)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--rules", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "evaluation_bench.json"))
    ap.add_argument("--hypothesis-out", default=str(ROOT / "profiles" / "hypothesis_bench.json"))
    ap.add_argument("--only", choices=("all", "evaluation", "hypothesis"), default="all")
    a = ap.parse_args()
    import sgmm_pkg
    sgmm = sgmm_pkg.load()
    from sgmm_amd import _lib, benchmarks, recorder, synthetic
    dev = torch.device("cuda:0")
    if a.only != "evaluation":
        bench_hypothesis(a, sgmm, _lib, dev)
    if a.only == "hypothesis":
        return
    E, T, H = a.episodes, a.ticks, a.hidden
    b = synthetic.bundle_510300(T, seed=4)
    st = synthetic.train_stats(b)
    ts = sgmm.TickStore()
    ts.add(b, st)
    ts.to(dev)
    phis = np.geomspace(1e-4, 1e-2, 8)
    params = sgmm.params_tensor([sgmm.EnvConfig(phi=p, tick_size=0.001) for p in phis], dev)
    eps = sgmm.EpisodeBatch(np.arange(E), np.zeros(E), np.full(E, T), np.arange(E) % 8).to(dev)
    mm = synthetic.population(E, H, sigma=0.2, seed=5).to(dev).contiguous()
    eng = sgmm.RolloutEngine(dev)

    def read():
        torch.cuda.synchronize()
        return {k: v[0] / v[1] for k, v in _lib.profile_read().items()}

    runs = {"summary_mlp": lambda: eng.summary(ts, eps, params, mm=mm, hidden=H),
            "rollout_direct": lambda: eng.trace(ts, eps, params, mm, H)}
    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
    _, summ = runs["summary_mlp"]()
    fit, trd, _ = runs["rollout_direct"]()
    same = bool(np.array_equal(summ["fitness"], fit.cpu().numpy()) and np.array_equal(summ["trade_rows"], trd.cpu().numpy()))
    read()
    ms = {k: [] for k in runs}
    _lib.profile_enable(True)
    for rep in range(a.reps):
        for k in (list(runs) if rep % 2 == 0 else list(runs)[::-1]):
            runs[k]()
            ms[k].append(read()[k])
    _lib.profile_enable(False)

    R = a.rules
    rng = np.random.default_rng(1)
    rules = np.stack([benchmarks.quote_rule(benchmarks.GLFTPolicy(gamma=1e-4, kappa=3000, A=0.1, sigma=float(s)))
                      for s in rng.uniform(5e-4, 2.0, R)])
    reps_ = sgmm.EpisodeBatch(np.arange(R), np.zeros(R), np.full(R, T), np.arange(R) % 8).to(dev)
    for _ in range(a.warmup):
        eng.summary(ts, reps_, params, rules=rules)
    read()
    rule_ms = []
    _lib.profile_enable(True)
    for _ in range(a.reps):
        eng.summary(ts, reps_, params, rules=rules)
        rule_ms.append(read()["summary_rule"])
    _lib.profile_enable(False)

    # the host route: what a user did before, on 64 episodes
    n_host = 64
    genomes = [g for g in mm[:n_host].cpu().numpy()]
    host_s, dev_s = [], []
    heps = sgmm.EpisodeBatch(np.arange(n_host), np.zeros(n_host), np.full(n_host, T), np.arange(n_host) % 8).to(dev)
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames = recorder.run_backtests(genomes, b, st, [float(phis[i % 8]) for i in range(n_host)], 0.0, 0.001)
        rows = [pandas_summary(df) for df in frames]
        host_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        _, hs = eng.summary(ts, heps, params, mm=mm[:n_host], hidden=H)
        dev_s.append(time.perf_counter() - t0)
    host_same = bool(all(r["Total PnL"] == s["total_pnl"] and r["Trades"] == s["trade_rows"] for r, s in zip(rows, hs)))

    s_, t_ = stats(ms["summary_mlp"]), stats(ms["rollout_direct"])
    res = {
        "device": torch.cuda.get_device_name(0), "batch": {"episodes": E, "ticks": T, "hidden": H},
        "summary_mlp": {**s_, "env_steps_per_s": E * T / (s_["median_ms"] * 1e-3)},
        "rollout_direct": {**t_, "env_steps_per_s": E * T / (t_["median_ms"] * 1e-3)},
        "summary_over_trace": s_["median_ms"] / t_["median_ms"],
        "summary_equals_trace_fitness": same,
        "summary_rule": {**stats(rule_ms), "rules": R, "ticks": T,
                         "env_steps_per_s": R * T / (float(np.median(rule_ms)) * 1e-3)},
        "host_route_64": {"episodes": n_host, "trace_d2h_frames_pandas_s": float(np.min(host_s)),
                          "summary_call_and_copy_s": float(np.min(dev_s)), "runs": 3,
                          "total_pnl_and_trades_equal": host_same},
    }
    print(json.dumps(res))
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    if not (same and host_same):
        raise SystemExit("summary and trace disagree")


if __name__ == "__main__":
    main()
