"""The CPU oracle at the float32 and int32 value edges (CPU-only).

The GPU parity tests compare every policy kernel with the oracle bit for bit;
in the value regimes of tests/value_regimes.py (subnormal activations,
overflowing chains, NaN inside the network, saturated actions) no reference
fixture pins the oracle, so here it is pinned against exact arithmetic, the
regimes are checked to stay non-trivial, and the env step is pinned against the
reference at the int32 edge (tests/golden/g12_int_edges.npz).
"""
import numpy as np
import pytest

import value_regimes as vr

I32_MIN, I32_MAX = vr.INT32_MIN, vr.INT32_MAX


@pytest.fixture(scope="module")
def mkt(sgmm):
    return vr.market()


def _episode(oracle, mkt, g, H, adv=None, adv_scale=1.0):
    b, _, s1n, s2n = mkt
    p = oracle.params(phi=vr.PHI, tick=vr.TICK, adv_scale=adv_scale)
    _, _, tr = oracle.evaluate(g, H, adv, s1n, s2n, *b[2:], p, trace=True)
    inv_before = np.concatenate([[0], tr["inventory"][:-1]])
    states = np.stack([s1n, s2n, inv_before / 2.0], 1).astype(np.float32)
    return tr, states


# ------------------------------------------------------------------ oracle against exact arithmetic
@pytest.mark.parametrize("H", vr.HIDDEN)
@pytest.mark.parametrize("regime", list(vr.REGIMES))
def test_oracle_policy_forward_equals_exact_arithmetic(oracle, mkt, regime, H):
    """orc_policy_forward equals, bit for bit (any NaN equal to any NaN), the
    chains evaluated with fmaf = exact Fraction product-and-sum rounded once to
    float32, on 64 states of the bundle with inventories -2..2; and the
    oracle's actions equal rint(raw * 5), saturated, formed exactly from its
    own raws along a 64-tick episode."""
    _, _, s1n, s2n = mkt
    g = vr.genome(regime, H, vr.seeds(regime, H)[0])
    for t in range(64):
        x = np.array([s1n[t], s2n[t], ((t % 5) - 2) / 2.0], np.float32)
        want, got = vr.forward_exact(g, H, x), oracle.policy_forward(g, H, x)
        assert vr.same_raw(want, got), (regime, H, t, want, got)
    b, _, _, _ = mkt
    _, _, tr = oracle.evaluate(g, H, None, s1n[:64], s2n[:64], *[c[:64] for c in b[2:]],
                               oracle.params(phi=vr.PHI, tick=vr.TICK), trace=True)
    for side in "ab":
        want = [vr.action_exact(r) for r in tr["raw_" + side]]
        assert np.array_equal(tr["off_" + side], want), (regime, H, side)


def test_exact_rounding_edges():
    """round_f32 / fma_exact at the places a wrong rounding model would slip:
    ties in the subnormal range, the subnormal / normal border, the overflow
    threshold, double rounding, signed zeros."""
    from fractions import Fraction as F
    tiny, sub = 2.0 ** -126, 2.0 ** -149
    assert vr.round_f32(F(3, 2) * F(sub)) == 2 * sub and vr.round_f32(F(5, 2) * F(sub)) == 2 * sub  # to even
    assert vr.round_f32(F(1, 2) * F(sub)) == 0.0 and vr.round_f32(F(sub) * F(501, 1000)) == sub
    assert vr.round_f32(F(tiny) - F(sub) / 2) == tiny   # a tie, up into the normals
    fmax = F(vr.F32_MAX)
    assert vr.round_f32(fmax + F(2) ** 103) == float("inf") and vr.round_f32(fmax + F(2) ** 103 - 1) == vr.F32_MAX
    # (1 + 2^-12)^2 + 2^-60 = 1 + 2^-11 + 2^-24 + 2^-60 rounds up; rounded to float64 first it
    # would lose the 2^-60, become a tie and round down to even
    x = 1 + 2.0 ** -12
    assert vr.fma_exact(x, x, 2.0 ** -60) == 1 + 2.0 ** -11 + 2.0 ** -23
    assert vr.fma32(x, x, 2.0 ** -60) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert np.float32(np.float64(x) * x + 2.0 ** -60) == np.float32(1 + 2.0 ** -11)
    assert np.signbit(vr.fma_exact(-0.0, 1.0, -0.0)) and not np.signbit(vr.fma_exact(-0.0, 1.0, 0.0))
    assert not np.signbit(vr.fma_exact(1.0, 1.0, -1.0))
    # the vectorised model is the same function
    rng = np.random.default_rng(0)
    e = rng.integers(-75, 64, (3, 4000))
    a, b, c = (np.ldexp(rng.standard_normal(4000), ee).astype(np.float32) for ee in e)
    c[::7] = -(a[::7].astype(np.float64) * b[::7]).astype(np.float32)   # cancellation
    n5 = len(a[1::5])                                                   # results in the subnormal range
    a[1::5] = np.ldexp(rng.standard_normal(n5), -100).astype(np.float32)
    b[1::5] = np.ldexp(rng.standard_normal(n5), rng.integers(-45, -30, n5)).astype(np.float32)
    c[1::5] = np.ldexp(rng.standard_normal(n5), rng.integers(-149, -130, n5)).astype(np.float32)
    a[2::5] = np.ldexp(rng.standard_normal(n5), 70).astype(np.float32)   # ... and around the overflow threshold
    b[2::5] = np.ldexp(rng.standard_normal(n5), rng.integers(50, 60, n5)).astype(np.float32)
    got = vr.fma32(a, b, c)
    want = np.array([vr.fma_exact(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    assert vr.same_raw(got, want)
    assert (np.abs(want[want != 0]) < vr.F32_TINY).sum() > 100 and np.isinf(want).sum() > 10


# ------------------------------------------------------------------ regime sanity
@pytest.mark.parametrize("H", vr.HIDDEN)
@pytest.mark.parametrize("regime", vr.SUB_REGIMES)
def test_subnormal_regimes_decide_actions(oracle, mkt, regime, H):
    """Conditions on the oracle alone, so that a regime cannot quietly become
    trivial: on the 700 ticks every seed of a sub_h* regime gives >= 16 distinct
    action values and >= 50 trading steps, and a model that flushes subnormals
    to zero changes the action on >= 600 steps.  The unflushed model is the
    oracle bit for bit, so the flush alone makes the difference.  Measured
    minima over the seeds (distinct / trading / flush differences): H = 8
    19 / 216 / 690, H = 16 and 32 29 / 73 / 696, H = 64 101 / 97 / 700."""
    for seed in vr.seeds(regime, H):
        g = vr.genome(regime, H, seed)
        tr, states = _episode(oracle, mkt, g, H)
        raw = vr.forward32(g, H, states)
        assert vr.same_raw(raw[:, 0], tr["raw_a"]) and vr.same_raw(raw[:, 1], tr["raw_b"])
        act = np.stack([tr["off_a"], tr["off_b"]], 1)
        assert np.array_equal(vr.actions32(raw), act)
        flushed = vr.actions32(vr.forward32(g, H, states, flush=True), flush=True)
        distinct = len(np.unique(act))
        trading = int((tr["fill_buy"] | tr["fill_sell"]).sum())
        differ = int(np.any(flushed != act, axis=1).sum())
        print(f"{regime} H={H} seed={seed}: distinct {distinct} trading {trading} flush differs {differ}")
        assert distinct >= 16 and trading >= 50 and differ >= 600, (regime, H, seed, distinct, trading, differ)


@pytest.mark.parametrize("H", vr.HIDDEN)
def test_overflow_regimes_reach_their_edges(oracle, mkt, H):
    """ovf_* episodes change inventory; ovf_l3 has inf raws only and both
    saturated actions; ovf_l2 has NaN raws at every H and inf raws at H <= 32
    (at H = 64 every raw of every seed tried is NaN); ovf_l1 has a NaN layer-2
    pre-activation (inf - inf: layer 1 overflowed) that the relu turns into 0.
    An fma's product is exact, so a chain over FINITE activations reaches
    +-inf but never NaN: ovf_l2's NaNs are born in the layer-3 chain."""
    seen = {}
    for regime in ("ovf_l1", "ovf_l2", "ovf_l3"):
        for seed in vr.seeds(regime, H):
            g = vr.genome(regime, H, seed)
            tr, states = _episode(oracle, mkt, g, H)
            raw, pre2 = vr.forward32(g, H, states, hidden=True)
            assert vr.same_raw(raw[:, 0], tr["raw_a"]) and vr.same_raw(raw[:, 1], tr["raw_b"])
            assert len(np.unique(tr["inventory"])) >= 2, (regime, H, seed)
            s = seen.setdefault(regime, dict(nan=0, inf=0, pre=0, acts=set()))
            s["nan"] += int(np.isnan(raw).sum())
            s["inf"] += int(np.isinf(raw).sum())
            s["pre"] += int(np.isnan(pre2).any(1).sum())
            s["acts"] |= set(np.unique([tr["off_a"], tr["off_b"]]).tolist())
    assert seen["ovf_l1"]["pre"] > 0 and seen["ovf_l2"]["pre"] == 0 and seen["ovf_l3"]["pre"] == 0
    assert seen["ovf_l2"]["nan"] > 0 and (seen["ovf_l2"]["inf"] > 0 or H == 64)
    assert seen["ovf_l3"]["nan"] == 0 and seen["ovf_l3"]["inf"] == 2 * 2 * vr.T_LONG
    assert seen["ovf_l3"]["acts"] == {I32_MIN, I32_MAX}
    assert I32_MIN in seen["ovf_l2"]["acts"]    # NaN -> INT32_MIN


def test_sub_out_raws_are_subnormal(oracle, mkt):
    """sub_out: the raw outputs are nonzero, at least 50 of the 1400 subnormal
    (measured: 20 % to 69 % of them) and none above 1e-36 (all
    actions 0), so only the raws themselves show a flush."""
    for H in vr.HIDDEN:
        g = vr.genome("sub_out", H, vr.seeds("sub_out", H)[0])
        tr, _ = _episode(oracle, mkt, g, H)
        raw = np.stack([tr["raw_a"], tr["raw_b"]])
        sub = np.abs(raw) < vr.F32_TINY
        print(f"sub_out H={H}: {sub.mean():.2f} of the raws subnormal, max |raw| {np.abs(raw).max():.3g}")
        assert np.all(raw != 0) and sub.sum() >= 50 and np.abs(raw).max() < 1e-36
        assert not tr["off_a"].any() and not tr["off_b"].any()


def test_relu_rule_is_independent_of_the_nan_sign(oracle):
    """A NaN pre-activation contributes 0 whatever its sign: NaN states of
    either sign give the bias-only network's output, bit for bit."""
    H = 16
    g = vr.genome("normal", H, 0)
    pos = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
    neg = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
    dead = g.copy()
    dead[:4 * H] = 0        # W1 = 0, b1 = 0: h1 = 0
    want = oracle.policy_forward(dead, H, np.zeros(3, np.float32))
    for nan in (pos, neg):
        for k in range(3):
            x = np.array([0.3, -0.2, 0.5], np.float32)
            x[k] = nan
            got = oracle.policy_forward(g, H, x)
            assert vr.same_raw(got, vr.forward_exact(g, H, x))
            assert not np.isnan(got).any()
            if k == 0:      # every layer-1 chain holds the NaN only if every W1[:, k] != 0
                assert np.all(g[:3 * H] != 0)
                assert vr.same_raw(got, want)


# ------------------------------------------------------------------ env step at the int32 edge
def test_g12_env_step_at_the_int32_edge(golden, oracle):
    """orc_env_step equals the reference at saturated actions with an adversary
    delta (the reference adds in int64), bit for bit."""
    d = golden("g12_int_edges.npz")
    n = len(d["off_a"])
    sums = np.stack([d["off_a"].astype(np.int64) + d["adv_a"], d["off_b"].astype(np.int64) + d["adv_b"]])
    assert ((sums > I32_MAX) | (sums < I32_MIN)).any(0).sum() >= 100   # rows an int32 sum would wrap
    for t in range(n):
        p = oracle.params(phi=float(d["phi"]), tick=float(d["tick"]), fee=float(d["fee"][t]))
        adv = (int(d["adv_a"][t]), int(d["adv_b"][t])) if d["has_adv"][t] else None
        inv, cash, r, pnl, ir, fee, fb, fs = oracle.env_step(
            p, int(d["inv_before"][t]), float(d["cash_before"][t]), int(d["off_a"][t]), int(d["off_b"][t]), adv,
            float(d["mid"]), float(d["ask"]), float(d["bid"]), float(d["buy_max"]), float(d["sell_min"]))
        assert (inv, fb, fs) == (d["inventory"][t], d["fill_buy"][t], d["fill_sell"][t]), t
        assert cash == d["cash"][t] and r == d["reward"][t] and pnl == d["pnl"][t], t
        assert ir == d["inv_reward"][t] and fee == d["fee_paid"][t], t


def test_g12_departures_from_the_reference(golden, oracle):
    """The documented departures, as relationships: the port's action is the
    reference's int64 action saturated at int32 (NaN and beyond-int64 raws:
    INT32_MIN where the reference has INT64_MIN, except +inf and > 2^63, which
    x86 also turns into INT64_MIN and the port saturates upwards); a NaN
    pre-activation contributes 0 where torch propagates it."""
    d = golden("g12_int_edges.npz")
    raw, ref = d["big_raw"], d["big_action_ref"]
    port = np.array([vr.action_exact(r) for r in raw], np.int64)
    inside = np.abs(raw.astype(np.float64) * 5) < 2.0 ** 63
    assert inside.sum() >= 12 and (np.abs(ref[inside]) > I32_MAX).sum() >= 8
    assert np.array_equal(port[inside], np.clip(ref[inside], I32_MIN, I32_MAX))
    assert np.all(ref[~inside] == -2 ** 63)
    assert np.array_equal(port[~inside], np.where(raw[~inside] > 0, I32_MAX, I32_MIN))
    # and the oracle's own conversion is that one (a one-tick episode whose raw is b3)
    for r, want in zip(raw, port):
        g = np.zeros(vr.n_params(8), np.float32)
        g[-2:] = r
        one = [np.zeros(1, np.float32)] * 2 + [np.full(1, 3.49)] * 5
        _, _, tr = oracle.evaluate(g, 8, None, *one, oracle.params(), trace=True)
        assert tr["off_a"][0] == want and tr["off_b"][0] == want, (r, tr["off_a"][0], want)
    H = int(d["l2_hidden"])
    for tag, regime in (("l2", "ovf_l2"), ("l1", "ovf_l1")):
        g = vr.genome(regime, H, int(d[tag + "_seed"]))
        assert np.isnan(d[tag + "_raw_ref"]).all() and np.all(d[tag + "_action_ref"] == -2 ** 63)
        for x in d[tag + "_states"]:
            got = oracle.policy_forward(g, H, x)
            assert vr.same_raw(got, vr.forward_exact(g, H, x))
            _, pre2 = vr.forward32(g, H, x[None], hidden=True)
            if tag == "l2":   # NaN born in the layer-3 chain: NaN raws in the port too, INT32_MIN
                assert not np.isnan(pre2).any() and np.isnan(got).all()
                assert vr.action_exact(got[0]) == I32_MIN
            else:             # NaN pre-activations in layer 2 contribute 0: the port's raws are not NaN
                assert np.isnan(pre2).any() and not np.isnan(got).any()


# ------------------------------------------------------------------ adversary on a saturated action
def test_saturated_action_meets_a_nonzero_adversary_delta(oracle, mkt):
    """The case tests/test_gpu_value_domain.py needs exists: an episode where the
    MM action is INT32_MAX or INT32_MIN on a step whose adversary delta is not
    zero, in the direction an int32 sum would wrap."""
    hit = 0
    for regime in ("ovf_l1", "ovf_l2", "ovf_l3"):
        for H in (16, 32, 64):
            g = vr.genome(regime, H, vr.seeds(regime, H)[0])
            for kind in ("sigma1", "x50"):
                for scale in (1.0, 3.0):
                    tr, _ = _episode(oracle, mkt, g, H, vr.adversary(kind, 0), scale)
                    for o, a in (("off_a", "adv_a"), ("off_b", "adv_b")):
                        hit += int(((tr[o] == I32_MAX) & (tr[a] > 0)).sum())
                        hit += int(((tr[o] == I32_MIN) & (tr[a] < 0)).sum())
    assert hit > 0
