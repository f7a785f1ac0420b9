"""Strategy evaluation (analytics/mm_analyzer.py:5-56, main.py:300-324).

The reference evaluates a backtest from its recorder frame with pandas.  Here
``summarize`` gets the same numbers for a whole request -- MLP policies and
quote rules (benchmarks.quote_rule), a phi / fee sweep, several bundles --
from sgmm_rollout_summary: one launch per policy kind, nothing traced, 96
bytes per backtest copied back.  ``summary_from_frame`` is the host mirror of
the device summary over a recorder frame: plain numpy, the same sequential
sums and the same one-pass Sharpe algorithm (include/sgmm.h,
sgmm_episode_summary).
"""
from __future__ import annotations

import numpy as np

from .rollout import SUMMARY_DTYPE

# every field but these two is bit-exact against the reference's analytics
SHARPE_FIELDS = ("sharpe_trades", "sharpe_steps")
EXACT_FIELDS = tuple(k for k in SUMMARY_DTYPE.names if k not in SHARPE_FIELDS + ("reserved",))

# summary field -> the reference's names: StrategyAnalytics.summary_dict, then
# get_clean_stats' unrounded values, the fill count of main.py:303 and the
# training fitness
COLUMNS = (("Total PnL", "total_pnl"), ("MAP (Risk)", "map"), ("PnLMAP (Eff)", "pnl_to_map"),
           ("Max DD", "max_dd"), ("Sharpe", "sharpe_trades"), ("Trades", "trade_rows"),
           ("Sharpe (steps)", "sharpe_steps"), ("PnL-to-MAP (floor)", "pnl_to_map_floor"),
           ("Fills", None), ("fitness", "fitness"))


def _seq_sum(x) -> float:
    """x[0] + x[1] + ... in that order (np.sum adds pairwise)."""
    return float(np.cumsum(np.asarray(x, np.float64))[-1]) if len(x) else 0.0


def _moments(x):
    """(mean, std with ddof=1) by one pass of shifted sums, shift = x[0] --
    the device's Moments (csrc/sgmm_evaluate.hip).  std is NaN below two values."""
    n = len(x)
    d = x - x[0]
    s, ss = _seq_sum(d), _seq_sum(d * d)
    mean = float(x[0]) + s / n
    if n < 2:
        return mean, float("nan")
    var = (ss - s * s / n) / (n - 1)
    return mean, float(np.sqrt(var if var > 0.0 else 0.0))


def summary_from_frame(df, idle_penalty: float = 50.0):
    """sgmm_episode_summary of a recorder frame (columns cash, inventory, mid,
    reward and fill_buy / fill_sell, or is_trade where the schema has no fill
    columns: fills_buy / fills_sell are then -1).  Returns a SUMMARY_DTYPE
    record."""
    cash = np.asarray(df["cash"], np.float64)
    inv = np.asarray(df["inventory"], np.int64)
    mid = np.asarray(df["mid"], np.float64)
    T = len(cash)
    o = np.zeros((), SUMMARY_DTYPE)
    o["steps"] = T
    if "fill_buy" in df and "fill_sell" in df:
        fb, fs = np.asarray(df["fill_buy"], np.int64), np.asarray(df["fill_sell"], np.int64)
        is_trade = (fb | fs) != 0
        o["fills_buy"], o["fills_sell"] = fb.sum(), fs.sum()
    else:
        is_trade = np.asarray(df["is_trade"]).astype(bool)
        o["fills_buy"] = o["fills_sell"] = -1
    rows = int(is_trade.sum())
    o["trade_rows"] = rows
    total = _seq_sum(np.asarray(df["reward"], np.float64))
    o["fitness"] = total - idle_penalty if rows == 0 else total
    o["sharpe_steps"] = np.nan
    if T == 0:
        return o
    w = cash + inv * mid                                   # Env/recorder.py:46
    pnl = w[-1] - w[0]                                     # mm_analyzer.py:15
    m = float(np.abs(inv).sum()) / T                       # :27
    o["total_pnl"], o["map"] = pnl, m
    o["pnl_to_map"] = 0.0 if m == 0 else pnl / m           # :30-33
    o["max_dd"] = (w - np.maximum.accumulate(w)).min()     # :20-22
    o["pnl_to_map_floor"] = pnl / max(m, 1e-2)             # main.py:310-312, last element
    if rows >= 2:                                          # mm_analyzer.py:36-45
        mean, sd = _moments(np.diff(w[is_trade]))
        o["sharpe_trades"] = 0.0 if sd == 0 else mean / sd
    if T >= 2:                                             # main.py:314-315
        mean, sd = _moments(np.diff(w))
        o["sharpe_steps"] = mean / (sd + 1e-9)
    o["final_cash"], o["final_inventory"] = cash[-1], inv[-1]
    return o


def summary_rows(summaries):
    """SUMMARY_DTYPE records -> DataFrame in the reference's column names."""
    import pandas as pd
    s = np.atleast_1d(summaries)
    cols = {name: (s[f] if f else s["fills_buy"] + s["fills_sell"]) for name, f in COLUMNS}
    return pd.DataFrame(cols)


def _is_rule(p) -> bool:
    from .benchmarks import QUOTE_RULE_DTYPE, FOICPolicy, GLFTPolicy
    return isinstance(p, (FOICPolicy, GLFTPolicy)) or getattr(p, "dtype", None) == QUOTE_RULE_DTYPE


def summarize(policies_or_rules, bundles, train_stats, phis, fee_rates=0.0, tick_size=0.001, device="cuda"):
    """One row per backtest, in the caller's order, without tracing a step.

    policies_or_rules: TradingPolicy modules / state_dicts / flat genomes (one
    hidden size) and quote rules (benchmarks.quote_rule records, or FOICPolicy /
    GLFTPolicy objects, tabulated with quote_rule's defaults), mixed freely;
    the other arguments broadcast as in recorder.run_backtests.  At most two
    launches: one for the MLP policies, one for the rules.  Columns:
    StrategyAnalytics.summary_dict's keys, then 'Sharpe (steps)',
    'PnL-to-MAP (floor)', 'Fills' and 'fitness'."""
    import torch

    from .benchmarks import quote_rule
    from .model import genome_size, hidden_from_genome
    from .recorder import _broadcast, _device_batch, _genome
    from .rollout import EpisodeBatch, RolloutEngine
    items = list(policies_or_rules)
    n = len(items)
    if n == 0:
        return summary_rows(np.zeros(0, SUMMARY_DTYPE))
    bundles = _broadcast(bundles, n, "bundle")
    phis, fees, ticks_ = (_broadcast(v, n, k) for v, k in ((phis, "phis"), (fee_rates, "fee_rates"),
                                                          (tick_size, "tick_size")))
    dev = torch.device(device)
    ts, params, seg = _device_batch(bundles, train_stats, phis, ticks_, fees, dev)
    is_rule = np.array([_is_rule(p) for p in items])
    out = np.zeros(n, SUMMARY_DTYPE)
    eng = RolloutEngine(dev)
    for kind in (False, True):
        idx = np.nonzero(is_rule == kind)[0]
        if len(idx) == 0:
            continue
        eps = EpisodeBatch(np.arange(len(idx)), [seg[i][0] for i in idx], [seg[i][1] for i in idx], idx).to(dev)
        if kind:
            rules = np.stack([np.asarray(items[i] if hasattr(items[i], "dtype") else quote_rule(items[i]))
                              for i in idx])
            out[idx] = eng.summary(ts, eps, params, rules=rules)[1]
        else:
            genomes = [_genome(items[i]) for i in idx]
            H = hidden_from_genome(genomes[0].size)
            if any(g.size != genome_size(H) for g in genomes):
                raise ValueError("all policies of one batch must share hidden_dim")
            mm = torch.from_numpy(np.stack(genomes)).to(dev)
            out[idx] = eng.summary(ts, eps, params, mm=mm, hidden=H)[1]
    return summary_rows(out)
