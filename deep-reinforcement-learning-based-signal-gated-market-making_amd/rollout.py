"""Device-resident rollout engine: bundles in HBM, episode batches, and the
calls into libsgmm.so's hot path.

Vocabulary (reference): a *bundle* is the 7-tuple of tick columns
(s1, s2, mid_next, best_ask, best_bid, buy_max, sell_min) that
load_signals_bundle returns (pipeline/agent_trainer.py:15-77); an *episode* is
one evaluate_individual call (Env/drl_engine.py:9-67): a genome (plus an
optional adversary genome) stepped over a bundle with (phi, tick, fee).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from ._lib import (DMResult, EnvParams, EpisodeSummary, Episodes, MBBResult, QuoteRule, Ticks, check, ptr,
                   stream_ptr)

ENV_PARAMS_DTYPE = np.dtype([("phi", "<f8"), ("tick", "<f8"), ("fee", "<f8"),
                             ("idle_penalty", "<f8"), ("i_max", "<i4"), ("i_min", "<i4"),
                             ("act_scale", "<f4"), ("adv_scale", "<f4")])
assert ENV_PARAMS_DTYPE.itemsize == ctypes.sizeof(EnvParams)

SUMMARY_DTYPE = np.dtype([(k, "<f8") for k in ("total_pnl", "map", "pnl_to_map", "max_dd", "sharpe_trades",
                                               "sharpe_steps", "pnl_to_map_floor", "fitness", "final_cash")] +
                         [(k, "<i4") for k in ("trade_rows", "fills_buy", "fills_sell", "final_inventory",
                                               "steps", "reserved")])
assert SUMMARY_DTYPE.itemsize == ctypes.sizeof(EpisodeSummary) == 96
DM_DTYPE = np.dtype([(k, "<f8") for k in ("stat", "p_value", "mean_d", "var_d")] + [("n", "<i8")])
MBB_DTYPE = np.dtype([(k, "<f8") for k in ("mean_sr", "ci_lo", "ci_hi")] +
                     [(k, "<i4") for k in ("n_returns", "num_blocks", "zero_replicates", "flags")])
assert DM_DTYPE.itemsize == ctypes.sizeof(DMResult) == 40
assert MBB_DTYPE.itemsize == ctypes.sizeof(MBBResult) == 40
MBB_CLAMPED, MBB_NOT_RESAMPLED = 1, 2
RULE_TRACE_COLUMNS = ("off_a", "off_b", "inventory", "cash", "reward", "pnl", "fee_paid", "fill_buy", "fill_sell")

COLUMNS = ("s1n", "s2n", "mid_next", "best_ask", "best_bid", "buy_max", "sell_min")


def normalize_signals(s1, s2, train_stats):
    """State features of drl_engine.py:33-34 as float32 arrays.

    The reference evaluates ``(s[t] - m) / sd`` on numpy scalars and lets
    torch.tensor(..., dtype=float32) round the result; under NumPy >= 2 the
    vectorised expression has the same promotions (NEP 50), so each element
    equals the reference's per-step value."""
    a = (np.asarray(s1) - train_stats["s1_m"]) / train_stats["s1_s"]
    b = (np.asarray(s2) - train_stats["s2_m"]) / train_stats["s2_s"]
    return np.asarray(a).astype(np.float32), np.asarray(b).astype(np.float32)


@dataclass
class EnvConfig:
    """FTPEnv constructor arguments + evaluate_individual's constants."""
    phi: float = 0.01
    tick_size: float = 0.01
    fee_rate: float = 0.0
    idle_penalty: float = 50.0
    i_max: int = 2
    i_min: int = -2
    act_scale: float = 5.0
    adv_scale: float = 1.0

    def record(self):
        r = np.zeros((), ENV_PARAMS_DTYPE)
        r["phi"], r["tick"], r["fee"] = self.phi, self.tick_size, self.fee_rate
        r["idle_penalty"], r["i_max"], r["i_min"] = self.idle_penalty, self.i_max, self.i_min
        r["act_scale"], r["adv_scale"] = self.act_scale, self.adv_scale
        return r


def params_tensor(configs, device) -> torch.Tensor:
    recs = np.stack([c.record() for c in configs]).astype(ENV_PARAMS_DTYPE)
    return torch.from_numpy(recs.view(np.uint8).copy()).to(device)


class TickStore:
    """Concatenated SoA tick columns of several bundles, resident on device."""

    def __init__(self):
        self._parts = {c: [] for c in COLUMNS}
        self.segments = []  # (offset, length)
        self.n = 0
        self.cols = None

    def add(self, bundle, train_stats) -> int:
        """Append a bundle; returns its segment index."""
        s1, s2, mid, ask, bid, bmax, smin = bundle
        s1n, s2n = normalize_signals(s1, s2, train_stats)
        T = len(mid)
        for c, a, dt in zip(COLUMNS, (s1n, s2n, mid, ask, bid, bmax, smin),
                            (np.float32, np.float32) + (np.float64,) * 5):
            a = np.asarray(a)
            if len(a) != T:
                raise ValueError(f"bundle column {c} has length {len(a)} != {T}")
            self._parts[c].append(np.ascontiguousarray(a, dt))
        self.segments.append((self.n, T))
        self.n += T
        return len(self.segments) - 1

    def to(self, device):
        self.cols = {c: torch.from_numpy(np.concatenate(v) if v else np.zeros(0, np.float64)).to(device)
                     for c, v in self._parts.items()}
        self._parts = None
        return self

    def struct(self) -> Ticks:
        return Ticks(*[self.cols[c].data_ptr() for c in COLUMNS])


@dataclass
class EpisodeBatch:
    """Host description of a batch of episodes -> device arrays + C struct."""
    genome: np.ndarray
    tick_off: np.ndarray
    length: np.ndarray
    param: np.ndarray
    adv: np.ndarray | None = None
    inv_min: int = -2
    inv_max: int = 2
    dev: dict = field(default_factory=dict)

    def __post_init__(self):
        self.genome = np.ascontiguousarray(self.genome, np.int32)
        self.tick_off = np.ascontiguousarray(self.tick_off, np.int64)
        self.length = np.ascontiguousarray(self.length, np.int32)
        self.param = np.ascontiguousarray(self.param, np.int32)
        if self.adv is not None:
            self.adv = np.ascontiguousarray(self.adv, np.int32)
        self.step_off = np.concatenate([[0], np.cumsum(self.length.astype(np.int64))[:-1]]).astype(np.int64) \
            if len(self.length) else np.zeros(0, np.int64)
        self.total_steps = int(self.length.astype(np.int64).sum())
        self.max_len = int(self.length.max()) if len(self.length) else 0
        # longest first (stable): the frontier kernel's processing order
        self.order = np.argsort(-self.length.astype(np.int64), kind="stable").astype(np.int32)

    @property
    def n(self):
        return len(self.genome)

    def to(self, device):
        for k in ("genome", "tick_off", "length", "param", "step_off", "adv", "order"):
            v = getattr(self, k)
            self.dev[k] = None if v is None else torch.from_numpy(v).to(device)
        return self

    def struct(self) -> Episodes:
        d = self.dev
        return Episodes(self.n, self.max_len, self.total_steps, self.inv_min, self.inv_max,
                        d["genome"].data_ptr(), d["adv"].data_ptr() if d["adv"] is not None else None,
                        d["tick_off"].data_ptr(), d["length"].data_ptr(), d["step_off"].data_ptr(),
                        d["param"].data_ptr(), d["order"].data_ptr() if d.get("order") is not None else None)


class RolloutEngine:
    """Owns the workspace; enqueues sgmm_rollout_fitness / sgmm_rollout_trace."""

    def __init__(self, device="cuda"):
        _lib.require_gpu()
        self.L = _lib.load()
        self.device = torch.device(device)
        self._ws = None

    def workspace_bytes(self, eps: EpisodeBatch, arl: bool) -> int:
        nsi = eps.inv_max - eps.inv_min + 1
        return int(self.L.sgmm_rollout_workspace_bytes(eps.n, eps.total_steps, nsi, 1 if arl else 0))

    def reserve(self, eps: EpisodeBatch, arl: bool):
        """Grow the workspace for this batch now (never inside a graph capture:
        a captured launch must not see its workspace reallocated later)."""
        self.workspace(eps, arl)

    def workspace(self, eps: EpisodeBatch, arl: bool) -> torch.Tensor:
        need = self.workspace_bytes(eps, arl)
        if self._ws is None or self._ws.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("workspace growth during graph capture; call reserve() first")
            self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        return self._ws

    def fitness(self, ticks: TickStore, eps: EpisodeBatch, params: torch.Tensor, mm: torch.Tensor,
                hidden: int, adv: torch.Tensor | None = None, out=None, stream=None):
        """Fitness (f64[E]) and trades (i32[E]) of every episode; stream-ordered."""
        if out is None:
            out = (torch.empty(eps.n, dtype=torch.float64, device=self.device),
                   torch.empty(eps.n, dtype=torch.int32, device=self.device))
        ws = self.workspace(eps, adv is not None)
        tk, ep = ticks.struct(), eps.struct()
        rc = self.L.sgmm_rollout_fitness(
            ctypes.byref(tk), ctypes.byref(ep), ptr(params), ptr(mm), mm.stride(0), hidden,
            ptr(adv), adv.stride(0) if adv is not None else 0, ptr(out[0]), ptr(out[1]),
            ptr(ws), ws.numel(), stream_ptr(stream))
        check(rc, "sgmm_rollout_fitness")
        return out

    def trace(self, ticks: TickStore, eps: EpisodeBatch, params: torch.Tensor, mm: torch.Tensor,
              hidden: int, adv: torch.Tensor | None = None, stream=None):
        """Per-step trace of every episode (dict of device tensors, rows step_off[e]+t)."""
        n = eps.total_steps
        dv = self.device
        tr = {k: torch.empty(n, dtype=dt, device=dv) for k, dt in (
            ("off_a", torch.int32), ("off_b", torch.int32), ("adv_a", torch.int32),
            ("adv_b", torch.int32), ("inventory", torch.int32), ("cash", torch.float64),
            ("reward", torch.float64), ("pnl", torch.float64), ("fee_paid", torch.float64),
            ("fill_buy", torch.uint8), ("fill_sell", torch.uint8), ("raw_a", torch.float32),
            ("raw_b", torch.float32))}
        fit = torch.empty(eps.n, dtype=torch.float64, device=dv)
        trd = torch.empty(eps.n, dtype=torch.int32, device=dv)
        tk, ep = ticks.struct(), eps.struct()
        rc = self.L.sgmm_rollout_trace(
            ctypes.byref(tk), ctypes.byref(ep), ptr(params), ptr(mm), mm.stride(0), hidden,
            ptr(adv), adv.stride(0) if adv is not None else 0,
            *[ptr(tr[k]) for k in ("off_a", "off_b", "adv_a", "adv_b", "inventory", "cash",
                                   "reward", "pnl", "fee_paid", "fill_buy", "fill_sell",
                                   "raw_a", "raw_b")],
            ptr(fit), ptr(trd), stream_ptr(stream))
        check(rc, "sgmm_rollout_trace")
        return fit, trd, tr


    def _rules(self, rules, eps):
        """Host rule records (QUOTE_RULE_DTYPE) -> (host copy kept alive, device bytes, count)."""
        host = np.ascontiguousarray(np.atleast_1d(rules))
        if host.dtype.itemsize != ctypes.sizeof(QuoteRule) or host.ndim != 1 or len(host) == 0:
            raise ValueError("rules: a non-empty 1-d array of sgmm_quote_rule records (benchmarks.quote_rule)")
        if eps.n and not (0 <= eps.genome.min() and eps.genome.max() < len(host)):
            raise ValueError(f"episode rule indices must lie in [0, {len(host)})")
        # the device copy stays referenced until the next call: the launch reads it
        self._rules_dev = torch.from_numpy(host.view(np.uint8).copy()).to(self.device)
        return host, self._rules_dev, len(host)

    def summary(self, ticks: TickStore, eps: EpisodeBatch, params: torch.Tensor, mm: torch.Tensor | None = None,
                hidden: int | None = None, rules=None, stream=None):
        """Per-episode summary (sgmm_rollout_summary), nothing traced: exactly one
        of ``mm`` (TradingPolicy genome rows, with ``hidden``) and ``rules`` (host
        records from benchmarks.quote_rule; eps.genome indexes them).  Returns the
        device tensor (E x 96 bytes) and its host copy as a SUMMARY_DTYPE array
        (the copy waits for the launch)."""
        if (mm is None) == (rules is None):
            raise ValueError("exactly one of mm / rules must be given")
        out = torch.empty((eps.n, SUMMARY_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        tk, ep = ticks.struct(), eps.struct()
        if rules is not None:
            host, dev, n = self._rules(rules, eps)
            rc = self.L.sgmm_rollout_summary(ctypes.byref(tk), ctypes.byref(ep), ptr(params), None, 0, 0,
                                             ptr(dev), host.ctypes.data, n, ptr(out), stream_ptr(stream))
        else:
            # a one-row tensor may report any row stride: its row length is the safe one
            stride = mm.stride(0) if mm.shape[0] > 1 else mm.shape[1]
            rc = self.L.sgmm_rollout_summary(ctypes.byref(tk), ctypes.byref(ep), ptr(params), ptr(mm),
                                             stride, int(hidden or 0), None, None, 0, ptr(out),
                                             stream_ptr(stream))
        check(rc, "sgmm_rollout_summary")
        if stream is not None:  # the copy below runs on the current stream
            stream.synchronize()
        return out, out.cpu().numpy().reshape(-1).view(SUMMARY_DTYPE)

    def trace_rules(self, ticks: TickStore, eps: EpisodeBatch, params: torch.Tensor, rules, stream=None):
        """Per-step trace of rule episodes (sgmm_rule_trace): (fitness, trades,
        dict of device columns RULE_TRACE_COLUMNS, rows step_off[e]+t)."""
        n, dv = eps.total_steps, self.device
        tr = {k: torch.empty(n, dtype=dt, device=dv) for k, dt in zip(
            RULE_TRACE_COLUMNS, (torch.int32,) * 3 + (torch.float64,) * 4 + (torch.uint8,) * 2)}
        fit = torch.empty(eps.n, dtype=torch.float64, device=dv)
        trd = torch.empty(eps.n, dtype=torch.int32, device=dv)
        host, dev, nr = self._rules(rules, eps)
        tk, ep = ticks.struct(), eps.struct()
        rc = self.L.sgmm_rule_trace(ctypes.byref(tk), ctypes.byref(ep), ptr(params), ptr(dev), host.ctypes.data,
                                    nr, *[ptr(tr[k]) for k in RULE_TRACE_COLUMNS], ptr(fit), ptr(trd),
                                    stream_ptr(stream))
        check(rc, "sgmm_rule_trace")
        return fit, trd, tr


    # ------------------------------------------------------------ hypothesis tests (main.py:227-297)
    def wealth(self, ticks: TickStore, eps: EpisodeBatch, trace: dict, stream=None) -> torch.Tensor:
        """The wealth column (Env/recorder.py:46) of a trace / trace_rules result,
        f64[total_steps] on the device, rows step_off[e] + t."""
        w = torch.empty(eps.total_steps, dtype=torch.float64, device=self.device)
        tk, ep = ticks.struct(), eps.struct()
        rc = self.L.sgmm_trace_wealth(ctypes.byref(tk), ctypes.byref(ep), ptr(trace["inventory"]),
                                      ptr(trace["cash"]), ptr(w), stream_ptr(stream))
        check(rc, "sgmm_trace_wealth")
        return w

    def _series(self, off, *values):
        """Host and device copies of a series batch's offsets; the values are
        checked to be contiguous float64 device tensors that cover them."""
        off_h = np.ascontiguousarray(off, np.int64).reshape(-1)
        if len(off_h) < 1:
            raise ValueError("off: n_series + 1 offsets")
        for v in values:
            if v is None:
                continue
            if v.dtype != torch.float64 or v.dim() != 1 or not v.is_contiguous() or v.device.type != "cuda":
                raise ValueError("series values: a contiguous 1-d float64 device tensor")
            if len(off_h) > 1 and v.numel() < int(off_h.max()):
                raise ValueError(f"series values hold {v.numel()} elements, off reaches {int(off_h.max())}")
        # the device copy stays referenced until the next call: the launches read it
        self._off_dev = torch.from_numpy(off_h).to(self.device)
        return off_h, self._off_dev

    def durbin_watson(self, values: torch.Tensor, off, stream=None) -> torch.Tensor:
        """Durbin-Watson statistic of every series (sgmm_durbin_watson): f64[n] on the device."""
        off_h, off_d = self._series(off, values)
        n = len(off_h) - 1
        out = torch.empty(n, dtype=torch.float64, device=self.device)
        rc = self.L.sgmm_durbin_watson(ptr(values), ptr(off_d), off_h.ctypes.data, n, ptr(out), stream_ptr(stream))
        check(rc, "sgmm_durbin_watson")
        return out

    def dm_test(self, actual: torch.Tensor, pred1: torch.Tensor, pred2: torch.Tensor | None, off,
                crit: str = "MSE", stream=None):
        """Diebold-Mariano test of every series (sgmm_dm_test); pred2 None = the
        zero forecast.  crit as the reference: "MSE", anything else is MAD.
        Returns the device tensor (n x 40 bytes) and its host copy as DM_DTYPE
        records (the copy waits for the launch)."""
        off_h, off_d = self._series(off, actual, pred1, pred2)
        n = len(off_h) - 1
        out = torch.empty((n, DM_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        rc = self.L.sgmm_dm_test(ptr(actual), ptr(pred1), ptr(pred2), ptr(off_d), off_h.ctypes.data, n,
                                 0 if crit == "MSE" else 1, ptr(out), stream_ptr(stream))
        check(rc, "sgmm_dm_test")
        if stream is not None:
            stream.synchronize()
        return out, out.cpu().numpy().reshape(-1).view(DM_DTYPE)

    def mbb_sharpe(self, wealth: torch.Tensor, off, block_size: int = 100, n_boot: int = 500, seed: int = 0,
                   starts: torch.Tensor | None = None, want_starts: bool = False, stream=None) -> "MBBOutput":
        """Moving-block bootstrap of the per-step Sharpe ratio of every wealth
        series (sgmm_mbb_sharpe).  starts: int32 device tensor [n, n_boot, stride]
        of block starts, or None for the device's Philox stream keyed by seed;
        want_starts also returns the starts used.  Everything stays on the
        device; MBBOutput.records() copies the 40-byte results back."""
        off_h, off_d = self._series(off, wealth)
        n = len(off_h) - 1
        dv = self.device
        stride = 0
        if starts is not None:
            if starts.dtype != torch.int32 or starts.dim() != 3 or not starts.is_contiguous() \
                    or tuple(starts.shape[:2]) != (n, n_boot):
                raise ValueError(f"starts: a contiguous int32 tensor [{n}, {n_boot}, stride]")
            stride = int(starts.shape[2])
        elif want_starts:
            lens = np.diff(off_h)
            stride = max(1, int(((lens.max() if n else 1) - 1) // max(block_size, 1)))
        out = torch.empty((n, MBB_DTYPE.itemsize), dtype=torch.uint8, device=dv)
        boot = torch.empty((n, max(n_boot, 0)), dtype=torch.float64, device=dv)
        rets = torch.empty(max(int(off_h.max()), 1), dtype=torch.float64, device=dv)
        used = torch.zeros((n, n_boot, stride), dtype=torch.int32, device=dv) if want_starts else None
        rc = self.L.sgmm_mbb_sharpe(ptr(wealth), ptr(off_d), off_h.ctypes.data, n, block_size, n_boot, ptr(starts),
                                    stride, ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), ptr(out), ptr(boot),
                                    ptr(used), ptr(rets), stream_ptr(stream))
        check(rc, "sgmm_mbb_sharpe")
        return MBBOutput(out, boot, rets, used, off_h, off_d, stream)


@dataclass
class MBBOutput:
    """Device results of RolloutEngine.mbb_sharpe: result (n x 40 bytes,
    sgmm_mbb_result), boot f64[n, n_boot], returns (series s's n_returns values
    from off[s]) and, when asked for, the int32 starts used."""
    result: torch.Tensor
    boot: torch.Tensor
    returns: torch.Tensor
    starts: torch.Tensor | None
    off: np.ndarray
    off_dev: torch.Tensor
    stream: object = None

    def records(self) -> np.ndarray:
        """Host copy of the results as MBB_DTYPE records (waits for the launches)."""
        if self.stream is not None:
            self.stream.synchronize()
        return self.result.cpu().numpy().reshape(-1).view(MBB_DTYPE)


def policy_forward(genomes: torch.Tensor, hidden: int, states: torch.Tensor,
                   genome_idx: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Batched TradingPolicy forward on device (models/model.py:24-26)."""
    L = _lib.load()
    out = torch.empty((states.shape[0], 2), dtype=torch.float32, device=states.device)
    rc = L.sgmm_policy_forward(ptr(genomes), genomes.stride(0), hidden, ptr(genome_idx),
                               ptr(states.contiguous()), ptr(out), states.shape[0], stream_ptr(stream))
    check(rc, "sgmm_policy_forward")
    return out


def adversary_forward(genomes: torch.Tensor, states: torch.Tensor,
                      genome_idx: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Batched AdversaryPolicy forward on device (models/model.py:49-50)."""
    L = _lib.load()
    out = torch.empty((states.shape[0], 2), dtype=torch.float32, device=states.device)
    rc = L.sgmm_adversary_forward(ptr(genomes), genomes.stride(0), ptr(genome_idx),
                                  ptr(states.contiguous()), ptr(out), states.shape[0], stream_ptr(stream))
    check(rc, "sgmm_adversary_forward")
    return out
