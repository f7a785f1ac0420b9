"""The benchmark strategies (Env/benchmarks.py) and their device form.

FOICPolicy / GLFTPolicy keep the reference's constructors and
``get_action(inventory)``.  ``quote_rule`` tabulates a policy over the
inventory range into an ``sgmm_quote_rule`` record: pow / log / sqrt stay on
the host, in the reference's own expressions, and the device kernels
(csrc/sgmm_evaluate.hip) do only the per-tick arithmetic of main.py:104-113.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import QuoteRule

QUOTE_RULE_DTYPE = np.dtype([("mode", "<i4"), ("n_inventory", "<i4"), ("quote_tick", "<f8"),
                             ("ask", "<f8", (8,)), ("bid", "<f8", (8,))])
assert QUOTE_RULE_DTYPE.itemsize == ctypes.sizeof(QuoteRule) == 144

MODE_TICKS, MODE_MID_RELATIVE = 0, 1


class FOICPolicy:
    """FOIC: the same tick offsets at every inventory; the environment's
    inventory limits do the rest."""

    def __init__(self, offset_a=0, offset_b=0):
        self.offset_a = offset_a
        self.offset_b = offset_b

    def get_action(self, inventory):
        return np.array([self.offset_a, self.offset_b])


class GLFTPolicy:
    """GLFT closed-form quotes: ask / bid distances from the mid price, skewed
    linearly in the inventory."""

    def __init__(self, gamma=0.001, kappa=100, A=0.1, sigma=0.01):
        self.gamma = gamma  # risk aversion
        self.kappa = kappa  # order-book depth decay
        self.A = A          # order arrival intensity
        self.sigma = sigma  # price volatility

    def get_action(self, inventory):
        # Env/benchmarks.py:28-41, the same expressions in the same order
        phi = np.sqrt(
            (self.sigma**2 * self.gamma) / (2 * self.kappa * self.A) * (1 + self.gamma / self.kappa)**(1 + self.kappa / self.gamma)
        )
        spread_term = (1 / self.gamma) * np.log(1 + self.gamma / self.kappa)
        q = inventory
        ask_offset_mid = spread_term + ((2 * q - 1) / 2) * phi
        bid_offset_mid = spread_term - ((2 * q + 1) / 2) * phi
        return np.array([ask_offset_mid, bid_offset_mid])


def rule_mode(strategy_name) -> int:
    """main.py:108: 'glft' quotes mid-relative prices, everything else tick offsets."""
    return MODE_MID_RELATIVE if strategy_name == "glft" else MODE_TICKS


def quote_rule(policy, inv_min=-2, inv_max=2, quote_tick=0.001, mode=None):
    """One sgmm_quote_rule record (numpy scalar of QUOTE_RULE_DTYPE):
    ``policy.get_action(q)`` for q = inv_min..inv_max.  mode: 0 tick offsets
    (main.py:113), 1 mid-relative price offsets divided by quote_tick
    (main.py:106-111); default 1 for a GLFTPolicy, else 0."""
    n = inv_max - inv_min + 1
    if not (inv_min <= 0 <= inv_max and n <= 8):
        raise ValueError(f"inventory range [{inv_min},{inv_max}] must contain 0 and span <= 8 values")
    if mode is None:
        mode = MODE_MID_RELATIVE if isinstance(policy, GLFTPolicy) else MODE_TICKS
    if mode not in (MODE_TICKS, MODE_MID_RELATIVE):
        raise ValueError("mode must be 0 (tick offsets) or 1 (mid-relative prices)")
    if mode == MODE_MID_RELATIVE and not quote_tick > 0:
        raise ValueError("quote_tick must be > 0 in mode 1")
    r = np.zeros((), QUOTE_RULE_DTYPE)
    r["mode"], r["n_inventory"], r["quote_tick"] = mode, n, quote_tick
    for i, q in enumerate(range(inv_min, inv_max + 1)):
        a = np.asarray(policy.get_action(q), np.float64)
        r["ask"][i], r["bid"][i] = a[0], a[1]
    return r


def rule_offsets(rule, inventory_prev, ask, bid, inv_min=-2):
    """Host mirror of the device rule arithmetic (include/sgmm.h,
    sgmm_quote_rule): the offsets quoted from inventory ``inventory_prev`` at
    ticks (ask, bid), as int64 arrays (off_a, off_b)."""
    q = np.asarray(inventory_prev, np.int64) - inv_min
    ra, rb = np.asarray(rule["ask"])[q], np.asarray(rule["bid"])[q]
    if int(rule["mode"]) == MODE_MID_RELATIVE:
        ask, bid = np.asarray(ask, np.float64), np.asarray(bid, np.float64)
        mid_p = (ask + bid) / 2.0
        ra = ((mid_p + ra) - ask) / float(rule["quote_tick"])
        rb = (bid - (mid_p - rb)) / float(rule["quote_tick"])
    return np.rint(ra).astype(np.int64), np.rint(rb).astype(np.int64)
