"""Golden fixture for FTPEnv.step at the int32 edge of the action and for the
reference's behaviour beyond it, generated from the imported reference.

Runs ONLY where the reference is present (SGMM_REFERENCE), like gen_golden.py.
What is committed is tests/golden/g12_int_edges.npz and this script.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_int_edges.py

Rows (one fresh FTPEnv each, stepped once from inv_before / cash_before):
actions in {INT32_MIN, INT32_MIN+1, -1, 0, 1, INT32_MAX-1, INT32_MAX} on either
side, adversary deltas in {-3, -1, 0, 1, 3}, every inventory from i_min to
i_max, with and without a fee; plus rows without an adversary.  The reference
adds the delta in int64 (market_env.py:26-28, actions are astype(int)), so an
action of INT32_MAX with delta +1 quotes at ask + 2147483.648 -- an int32 sum
would wrap to ask - 2147483.648 and sell.

Documentation rows (the port departs from them on purpose):
  big_raw / big_action_ref   np.round(raw * 5.0).astype(int) as drl_engine.py:39
                             forms it, for raws beyond +-2^31 / 5: the int64
                             action does not saturate where the port's int32 does
  l2_*                       the ovf_l2 genome (tests/value_regimes.py, H = 32)
                             on three states: its layer-2 activations reach inf
                             and the layer-3 chain holds inf - inf, so both raws
                             are NaN (in the port too) and astype(int) makes
                             INT64_MIN of them where the port has INT32_MIN
  l1_*                       the ovf_l1 genome on three states whose layer-2
                             chain holds inf - inf (layer 1 overflowed): torch's
                             relu propagates that NaN to both raws; the port's
                             relu gives 0 for a NaN pre-activation and its raws
                             are not NaN
"""
from __future__ import annotations

import itertools
import os
import sys
import warnings
from pathlib import Path

import numpy as np

REF = Path(os.environ.get("SGMM_REFERENCE", "/root/reference"))
OUT = Path(__file__).resolve().parent
sys.dont_write_bytecode = True
sys.path.insert(0, str(REF))
sys.path.insert(0, str(OUT.parent))        # tests/: value_regimes
sys.path.insert(0, str(OUT.parent.parent))  # the repository root: sgmm_pkg

import torch  # noqa: E402

torch.set_num_threads(1)

from Env import market_env as ref_env  # noqa: E402
from models import model as ref_model  # noqa: E402

import value_regimes as vr  # noqa: E402

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
ACTIONS = (I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX)
DELTAS = (-3, -1, 0, 1, 3)
PHI, TICK = 0.003, 0.001


def gen_steps():
    rows = []
    ask, bid, mid = 3.491, 3.490, 3.4915
    bmax, smin = 3.492, 3.489    # a quote within a tick of the touch fills
    pairs = [(a, a) for a in ACTIONS] + [(a, b) for a, b in zip(ACTIONS, reversed(ACTIONS)) if a != b]
    dpairs = sorted(set([(d, d) for d in DELTAS] + [(d, -d) for d in DELTAS])) + [None]
    for fee, (oa, ob), dd, inv0 in itertools.product((0.0, 3e-5), pairs, dpairs, range(-2, 3)):
        env = ref_env.FTPEnv(phi=PHI, tick_size=TICK, fee_rate=fee)
        env.inventory, env.cash = inv0, 10.5
        act = np.array([oa, ob]).astype(int)                  # drl_engine.py:39
        adv = None if dd is None else np.array(dd).astype(int)  # drl_engine.py:48
        r, info = env.step(act, mid, ask, bid, bmax, smin, adv_action=adv)
        rows.append((fee, oa, ob, 0 if dd is None else 1, 0 if dd is None else dd[0],
                     0 if dd is None else dd[1], inv0, 10.5, env.inventory, env.cash, r,
                     info["pnl_reward"], info["inventory_reward"], info["fee_paid"],
                     info["fill_buy"], info["fill_sell"]))
    cols = ("fee", "off_a", "off_b", "has_adv", "adv_a", "adv_b", "inv_before", "cash_before",
            "inventory", "cash", "reward", "pnl", "inv_reward", "fee_paid", "fill_buy", "fill_sell")
    ints = {"off_a", "off_b", "has_adv", "adv_a", "adv_b", "inv_before", "inventory", "fill_buy", "fill_sell"}
    o = {c: np.array([r[i] for r in rows], np.int32 if c in ints else np.float64) for i, c in enumerate(cols)}
    o.update(phi=np.float64(PHI), tick=np.float64(TICK), mid=np.float64(mid), ask=np.float64(ask),
             bid=np.float64(bid), buy_max=np.float64(bmax), sell_min=np.float64(smin))
    return o


def ref_action(raw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # invalid value in cast
        return np.round(np.asarray(raw, np.float32) * 5.0).astype(int)


def gen_beyond():
    big = np.array([4.2949672e8, 4.2949676e8, 4.294968e8, 5e8, 1e12, 1.8e18, -4.2949672e8, -4.294968e8,
                    -5e8, -1e12, -1.8e18, 1e19, -1e19, np.inf, -np.inf, np.nan, 7.0, -7.5], np.float32)
    o = {"big_raw": big, "big_action_ref": ref_action(big).astype(np.int64)}
    _, _, s1n, s2n = vr.market()
    states = np.stack([np.repeat(s1n, 5), np.repeat(s2n, 5), np.tile(np.arange(-2, 3) / 2.0, len(s1n))],
                      1).astype(np.float32)
    H = 32
    for tag, regime in (("l2", "ovf_l2"), ("l1", "ovf_l1")):
        seed = vr.seeds(regime, H)[0]
        g = vr.genome(regime, H, seed)
        pol = ref_model.TradingPolicy(hidden_dim=H)
        pol.set_weights(torch.from_numpy(g))
        port, pre2 = vr.forward32(g, H, states, hidden=True)
        with torch.no_grad():
            ref = pol.forward(torch.from_numpy(states)).numpy()
        nan_ref, nan_pre = np.isnan(ref).all(1), np.isnan(pre2).any(1)
        print("%s: %d of %d states give NaN raws in the reference, %d have a NaN layer-2 pre-activation, "
              "%d of those leave the port a non-NaN raw" %
              (regime, nan_ref.sum(), len(states), nan_pre.sum(), (nan_pre & ~np.isnan(port).any(1)).sum()))
        # ovf_l2: NaN raws (born in the layer-3 chain, in the port as well); ovf_l1: states where
        # only the relu rule separates the port from torch
        cand = np.nonzero(nan_ref & (nan_pre & ~np.isnan(port).any(1) if tag == "l1" else ~nan_pre))[0]
        _, first = np.unique(states[cand, 2], return_index=True)
        pick = np.unique(np.concatenate([cand[first], cand[:3]]))[:3]
        assert len(pick) == 3
        o.update({f"{tag}_hidden": np.int32(H), f"{tag}_seed": np.int32(seed), f"{tag}_states": states[pick],
                  f"{tag}_raw_ref": ref[pick], f"{tag}_action_ref": ref_action(ref[pick]).astype(np.int64)})
    return o


if __name__ == "__main__":
    o = gen_steps()
    sums = np.stack([o["off_a"].astype(np.int64) + o["adv_a"], o["off_b"].astype(np.int64) + o["adv_b"]])
    wrap = ((sums > I32_MAX) | (sums < I32_MIN)).any(0)
    o.update(gen_beyond())
    np.savez_compressed(OUT / "g12_int_edges.npz", **o)
    print("g12: %d steps (%d with a sum outside int32), fills buy=%d sell=%d" %
          (len(o["off_a"]), wrap.sum(), o["fill_buy"].sum(), o["fill_sell"].sum()))
    print("big", o["big_raw"], o["big_action_ref"])
    for t in ("l2", "l1"):
        print(t, o[t + "_states"], o[t + "_raw_ref"], o[t + "_action_ref"])
