"""Strategy evaluation (analytics/mm_analyzer.py:5-56, main.py:300-324).

The reference evaluates a backtest from its recorder frame with pandas.  Here
``summarize`` gets the same numbers for a whole request -- MLP policies and
quote rules (benchmarks.quote_rule), a phi / fee sweep, several bundles --
from sgmm_rollout_summary: one launch per policy kind, nothing traced, 96
bytes per backtest copied back.  ``summary_from_frame`` is the host mirror of
the device summary over a recorder frame: plain numpy, the same sequential
sums and the same one-pass Sharpe algorithm (include/sgmm.h,
sgmm_episode_summary).

The hypothesis tests printed between the backtests and that table
(main.py:227-297) are in the second half of this module: dm_test,
durbin_watson and get_mbb_sharpe on the device, with their host mirrors.
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


# ---------------------------------------------------------------------------
# Hypothesis tests (main.py:227-297): Diebold-Mariano, Durbin-Watson and the
# moving-block bootstrap of the per-step Sharpe ratio.  dm_test /
# durbin_watson / get_mbb_sharpe carry the reference's names and signatures and
# run on the device; mbb_sharpe is the batched form; *_from_series /
# mbb_from_wealth are the host mirrors of the device arithmetic (numpy, no GPU).
# ---------------------------------------------------------------------------
_LANES = 64
_BUTTERFLY = tuple(np.arange(_LANES) ^ d for d in (32, 16, 8, 4, 2, 1))


def lane_sum(x):
    """The device's sum over the last axis (include/sgmm.h, THE LANE SUM):
    element i in lane i mod 64, a lane adds in increasing i from 0.0, the lanes
    are combined by the xor butterfly 32, 16, ..., 1."""
    x = np.asarray(x, np.float64)
    L = x.shape[-1]
    rows = -(-L // _LANES)
    # row 0 is the 0.0 every lane starts from; the padding adds +0.0 to a sum
    # that is never -0.0, which changes nothing (NaN and inf included)
    pad = np.zeros(x.shape[:-1] + ((rows + 1) * _LANES,))
    pad[..., _LANES:_LANES + L] = x
    with np.errstate(all="ignore"):
        v = np.cumsum(pad.reshape(x.shape[:-1] + (rows + 1, _LANES)), axis=-2)[..., -1, :]
        for idx in _BUTTERFLY:
            v = v + v[..., idx]
    return v[..., 0]


def _sharpe_of(mean, var):
    """mean / std if std > 1e-9 else 0 (main.py:259-260, 278-282); a NaN std gives 0."""
    with np.errstate(all="ignore"):
        sd = np.sqrt(var)
        return np.where(sd > 1e-9, mean / sd, 0.0)


def returns_from_wealth(w):
    """pct_change().dropna() of a NaN-free wealth: w[t+1] / w[t] - 1, NaN dropped in order, inf kept."""
    w = np.asarray(w, np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        r = w[1:] / w[:-1] - 1.0
    return r[~np.isnan(r)]


def percentile_linear(sorted_values, q):
    """numpy's linear-rule percentile q of ascending values, in the device's operations."""
    n = len(sorted_values)
    v = np.float64(n - 1) * (np.float64(q) / 100.0)
    lo = int(np.floor(v))
    hi = min(lo + 1, n - 1)
    t, a, b = v - np.floor(v), sorted_values[lo], sorted_values[hi]
    with np.errstate(all="ignore"):
        diff = b - a
        return b - diff * (1.0 - t) if t >= 0.5 else a + diff * t


def mbb_from_wealth(wealth, block_size=100, n_boot=500, starts=None):
    """Host mirror of sgmm_mbb_sharpe for one wealth series.  starts: integer
    array (n_boot, >= num_blocks) of block starts (clamped as the device clamps
    them); not needed when the series is too short to resample.  Returns
    (MBB_DTYPE record, replicates f64[n_boot], returns, starts used)."""
    from .rollout import MBB_CLAMPED, MBB_DTYPE, MBB_NOT_RESAMPLED
    r = returns_from_wealth(wealth)
    n = len(r)
    o = np.zeros((), MBB_DTYPE)
    o["n_returns"] = n
    with np.errstate(all="ignore"):
        if n <= block_size:                                    # main.py:258-261
            mean = lane_sum(r) / np.float64(n)
            d = r - mean
            sr = float(_sharpe_of(mean, lane_sum(d * d) / np.float64(n)))
            o["mean_sr"] = o["ci_lo"] = o["ci_hi"] = sr
            o["zero_replicates"], o["flags"] = (n_boot if sr == 0.0 else 0), MBB_NOT_RESAMPLED
            return o, np.full(n_boot, sr), r, np.zeros((n_boot, 0), np.int32)
        nb = n // block_size                                   # :264
        if starts is None:
            raise ValueError("mbb_from_wealth: this series resamples, pass its block starts")
        given = np.asarray(starts)[:, :nb].astype(np.int64)
        if given.shape != (n_boot, nb):
            raise ValueError(f"starts: ({n_boot}, >= {nb}) block starts")
        used = np.clip(given, 0, n - block_size)
        x = r[(used[:, :, None] + np.arange(block_size)).reshape(n_boot, nb * block_size)]  # :270-276
        cnt = np.float64(nb * block_size)
        mean = lane_sum(x) / cnt
        d = x - mean[:, None]
        boot = _sharpe_of(mean, lane_sum(d * d) / cnt)         # :278-283
        o["num_blocks"] = nb
        o["mean_sr"] = lane_sum(boot) / np.float64(n_boot)     # :285
        srt = np.sort(boot)
        nan = bool(np.isnan(boot).any())
        o["ci_lo"] = np.nan if nan else percentile_linear(srt, 2.5)
        o["ci_hi"] = np.nan if nan else percentile_linear(srt, 97.5)
        o["zero_replicates"] = int((boot == 0.0).sum())
        o["flags"] = MBB_CLAMPED if (used != given).any() else 0
    return o, boot, r, used.astype(np.int32)


def dm_from_series(actual, pred1, pred2=None, crit="MSE"):
    """Host mirror of sgmm_dm_test for one series (main.py:228-236): a DM_DTYPE record."""
    import math

    from .rollout import DM_DTYPE
    a, p1 = (np.asarray(v, np.float64).reshape(-1) for v in (actual, pred1))
    p2 = np.zeros_like(a) if pred2 is None else np.asarray(pred2, np.float64).reshape(-1)
    n = len(a)
    o = np.zeros((), DM_DTYPE)
    with np.errstate(all="ignore"):
        u, v = a - p1, a - p2
        d = (u * u - v * v) if crit == "MSE" else (np.abs(u) - np.abs(v))
        mean = lane_sum(d) / np.float64(n)
        c = d - mean
        var = lane_sum(c * c) / np.float64(n - 1) if n >= 2 else np.float64(np.nan)
        stat = mean / np.sqrt(var / np.float64(n))
        p = 2.0 * (1.0 - 0.5 * math.erfc((-abs(float(stat))) / math.sqrt(2.0)))
    o["stat"], o["p_value"], o["mean_d"], o["var_d"], o["n"] = stat, p, mean, var, n
    return o


def dw_from_series(resids) -> float:
    """Host mirror of sgmm_durbin_watson: sum (e[t] - e[t-1])^2 / sum e[t]^2 in lane sums."""
    e = np.asarray(resids, np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        d = e[1:] - e[:-1]
        return float(lane_sum(d * d) / lane_sum(e * e))


def _series_batch(series_list, dev):
    import torch
    arrs = [np.ascontiguousarray(np.asarray(s, np.float64).reshape(-1)) for s in series_list]
    off = np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
    flat = np.concatenate(arrs) if arrs and off[-1] else np.zeros(1)
    return torch.from_numpy(flat).to(dev), off


def dm_test(actual, pred1, pred2, h=1, crit="MSE", device="cuda"):
    """main.py:228-236 on the device: (dm_stat, p_value).  h is accepted and
    unused, as in the reference."""
    import torch

    from .rollout import RolloutEngine
    dev = torch.device(device)
    a, off = _series_batch([actual], dev)
    p1, o1 = _series_batch([pred1], dev)
    p2, o2 = _series_batch([pred2], dev)
    if not (off[-1] == o1[-1] == o2[-1]):
        raise ValueError("dm_test: actual, pred1 and pred2 must have one length")
    rec = RolloutEngine(dev).dm_test(a, p1, p2, off, crit)[1][0]
    return float(rec["stat"]), float(rec["p_value"])


def durbin_watson(resids, device="cuda") -> float:
    """statsmodels.stats.stattools.durbin_watson (main.py:247) on the device."""
    import torch

    from .rollout import RolloutEngine
    dev = torch.device(device)
    v, off = _series_batch([resids], dev)
    return float(RolloutEngine(dev).durbin_watson(v, off).cpu()[0])


def mbb_sharpe(series_list, block_size=100, n_boot=500, seed=0, starts=None, device="cuda"):
    """get_mbb_sharpe of many wealth series in one launch set: MBB_DTYPE records
    (mean_sr, ci_lo, ci_hi, ...), one per series.  starts: one integer array
    (n_boot, >= num_blocks) per series (None for a series too short to
    resample), or None to draw every start on the device from Philox keyed by
    ``seed``."""
    import torch

    from .rollout import RolloutEngine
    dev = torch.device(device)
    w, off = _series_batch(series_list, dev)
    st = None
    if starts is not None:
        mats = [np.zeros((n_boot, 0), np.int32) if s is None else np.asarray(s).astype(np.int32) for s in starts]
        if len(mats) != len(off) - 1 or any(m.ndim != 2 or m.shape[0] != n_boot for m in mats):
            raise ValueError("starts: one (n_boot, num_blocks) array per series")
        host = np.zeros((len(mats), n_boot, max([1] + [m.shape[1] for m in mats])), np.int32)
        for i, m in enumerate(mats):
            host[i, :, :m.shape[1]] = m
        st = torch.from_numpy(host).to(dev)
    return RolloutEngine(dev).mbb_sharpe(w, off, block_size, n_boot, seed, st).records()


def _reference_starts(wealth, block_size, n_boot):
    """The block starts get_mbb_sharpe draws from numpy's global stream
    (main.py:266-268): n_boot calls of randint(0, n - block_size + 1, size=num_blocks);
    None (and nothing drawn) when the reference returns before its loop."""
    n = len(returns_from_wealth(wealth))
    if n <= block_size:
        return None
    return np.stack([np.random.randint(0, n - block_size + 1, size=max(1, n // block_size)) for _ in range(n_boot)])


def get_mbb_sharpe(wealth_series, block_size=100, n_boot=500, device="cuda"):
    """main.py:251-285 on the device.  The block starts come from numpy's global
    stream exactly as the reference draws them, so np.random.seed(k) before the
    call gives the reference's numbers.  Returns (mean, array([lo, hi])), or
    (sr, (sr, sr)) for a series too short to resample."""
    w = np.asarray(wealth_series, np.float64)
    st = _reference_starts(w, block_size, n_boot)
    rec = mbb_sharpe([w], block_size, n_boot, starts=[st], device=device)[0]
    if st is None:
        sr = float(rec["mean_sr"])
        return sr, (sr, sr)
    return float(rec["mean_sr"]), np.array([rec["ci_lo"], rec["ci_hi"]])


def hypothesis_report(frames, methods=("arl", "drl", "glft", "foic"), block_size=100, n_boot=500, device="cuda"):
    """The H1 / H2 / H3 lines of main.py:239-297 from the backtest frames
    (method -> DataFrame with mid, s2_pred, reward, wealth), printed in the
    reference's formats; H1 and H2 read frames['arl'].  H3 draws each method's
    starts from numpy's global stream in the reference's order and evaluates
    every method in one launch set.  Returns the printed values."""
    arl = frames["arl"]
    mid = np.asarray(arl["mid"], np.float64)
    pred = np.asarray(arl["s2_pred"], np.float64)
    dm_stat, p_val = dm_test(mid[1:] - mid[:-1], pred[:-1], np.zeros_like(pred)[:-1], device=device)  # :240-243
    print(f"H1 (DM Test): Statistic={dm_stat:.4f}, p-value={p_val:.4f}")
    dw_stat = durbin_watson(np.asarray(arl["reward"], np.float64), device=device)
    print(f"H2: DW-Stat = {dw_stat:.4f}")
    print("H3: 95% CI of Per-Step Sharpe:")
    have = [m for m in methods if m in frames and len(frames[m]) > 0]
    ws = [np.asarray(frames[m]["wealth"], np.float64) for m in have]
    recs = mbb_sharpe(ws, block_size, n_boot, starts=[_reference_starts(w, block_size, n_boot) for w in ws],
                      device=device) if have else []
    h3 = {}
    for m in methods:
        if m in have:
            r = recs[have.index(m)]
            h3[m] = (float(r["mean_sr"]), float(r["ci_lo"]), float(r["ci_hi"]))
            print(f"  - {m.upper():<4}: {h3[m][0]:>8.6f} | CI: [{h3[m][1]:>8.6f}, {h3[m][2]:>8.6f}]")
        else:
            print(f"  - {m.upper():<4}: No data found in DataFrame.")
    return {"dm_stat": dm_stat, "p_value": p_val, "dw_stat": dw_stat, "mbb": h3}
