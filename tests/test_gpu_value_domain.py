"""GPU parity at the float32 and int32 value edges: every policy kernel, the
trace, the summary and sgmm_policy_forward against the CPU oracle, bit for bit,
in the value regimes of tests/value_regimes.py -- subnormal activations in the
MFMA operands and accumulators, chains that overflow, NaN born inside the
network, NaN state inputs of both signs, saturated actions with an adversary
delta on top.  tests/test_value_domain.py pins the oracle itself in these
regimes (against exact arithmetic and the reference) and keeps them non-trivial:
a library that flushes subnormals fails every sub_* case here.
"""
import numpy as np
import pytest
import torch

import value_regimes as vr
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

DEV = torch.device("cuda:0")
LENGTHS = (vr.T_LONG, vr.T_SHORT)
CAPS = ((2, -2), (3, -4))
POS_NAN, NEG_NAN = (np.array([b], np.uint32).view(np.float32)[0] for b in (0x7FC00000, 0xFFC00000))
# (policy_path knobs, hidden sizes): the VALU table, the two MFMA tables of H = 16 / 32,
# k_policy_table_mfma (H = 64), the frontier walk with one and two chunk groups and its spill kernel
PATHS = {
    "valu": (dict(policy_path="valu"), (8, 16, 32)),
    "table_sp": (dict(policy_path="table", table_sp=1), (16, 32)),
    "table_v3": (dict(policy_path="table", table_sp=0), (16, 32)),
    "table_mfma": (dict(policy_path="table"), (64,)),
    "frontier1_spill": (dict(policy_path="frontier", groups=1, spill=1), (16, 32)),
    "frontier2_spill": (dict(policy_path="frontier", groups=2, spill=1), (16, 32)),
}
PATH_CASES = [(name, H) for name, (_, hs) in PATHS.items() for H in hs]


class World:
    """The 700-tick bundle on the device, clean and with NaN states (NaNs of
    both signs in s1n / s2n at ticks 0, 63, 64 and 699), and the oracle's
    results, computed once per shape."""

    def __init__(self, sgmm, oracle):
        self.sgmm, self.oracle = sgmm, oracle
        self.b, self.st, s1n, s2n = vr.market()
        a, c = s1n.copy(), s2n.copy()
        a[0], a[64], c[63], c[699] = POS_NAN, NEG_NAN, NEG_NAN, POS_NAN
        unit = {"s1_m": np.float32(0), "s1_s": np.float32(1), "s2_m": np.float32(0), "s2_s": np.float32(1)}
        self.stores, self.signals = {}, {}
        for name, bundle, st in (("clean", self.b, self.st), ("nan_states", (a, c) + tuple(self.b[2:]), unit)):
            ts = sgmm.TickStore()
            ts.add(bundle, st)
            ts.to(DEV)
            self.stores[name] = ts
            # the oracle reads the signals as they arrived on the device
            self.signals[name] = (ts.cols["s1n"].cpu().numpy(), ts.cols["s2n"].cpu().numpy())
        assert np.array_equal(self.signals["clean"][0], s1n) and np.array_equal(self.signals["clean"][1], s2n)
        x = np.concatenate(self.signals["nan_states"])
        assert np.isnan(x).sum() == 4 and np.signbit(x[np.isnan(x)]).sum() == 2
        self.eng = sgmm.RolloutEngine(DEV)
        self._ref = {}

    def batch(self, H):
        """36 episodes: every regime, two seeds, 700 and 65 ticks.  Returns the
        genome rows, (row, length, regime) per episode."""
        rows, eps = [], []
        for regime in vr.REGIMES:
            for seed in vr.seeds(regime, H):
                rows.append(vr.genome(regime, H, seed))
                eps += [(len(rows) - 1, L, regime) for L in LENGTHS]
        return np.stack(rows), eps

    def params(self, caps, adv_scales=(1.0,)):
        cfg = [self.sgmm.EnvConfig(phi=vr.PHI, tick_size=vr.TICK, i_max=caps[0], i_min=caps[1], adv_scale=s)
               for s in adv_scales]
        orc = [self.oracle.params(phi=vr.PHI, tick=vr.TICK, i_max=caps[0], i_min=caps[1], adv_scale=s)
               for s in adv_scales]
        return self.sgmm.params_tensor(cfg, DEV), orc

    def episodes(self, eps, caps, adv=None, param=None):
        n = len(eps)
        return self.sgmm.EpisodeBatch([e[0] for e in eps], np.zeros(n), [e[1] for e in eps],
                                      np.zeros(n) if param is None else param, adv=adv,
                                      inv_min=caps[1], inv_max=caps[0]).to(DEV)

    def want(self, H, caps, signals):
        """The oracle's (fitness, trades) of batch(H)."""
        key = (H, caps, signals)
        if key not in self._ref:
            mm, eps = self.batch(H)
            n = len(eps)
            _, orc = self.params(caps)
            self._ref[key] = self.oracle.evaluate_batch(
                mm, H, None, self.signals[signals] + tuple(self.b[2:]), [e[0] for e in eps], None, np.zeros(n),
                [e[1] for e in eps], np.zeros(n), orc, n_threads=8)
        return self._ref[key]

    def trace(self, mm_row, H, L, caps, signals, adv=None, adv_scale=1.0):
        s1n, s2n = self.signals[signals]
        p = self.oracle.params(phi=vr.PHI, tick=vr.TICK, i_max=caps[0], i_min=caps[1], adv_scale=adv_scale)
        return self.oracle.evaluate(mm_row, H, adv, s1n[:L], s2n[:L], *[c[:L] for c in self.b[2:]], p, trace=True)


@pytest.fixture(scope="module")
def world(sgmm, oracle):
    return World(sgmm, oracle)


def assert_trace_equal(got, want, sl, what):
    for k, v in want.items():
        g = got[k][sl]
        if k.startswith("raw_"):
            assert vr.same_raw(g, v), (what, k)
        else:
            assert np.array_equal(g, v), (what, k, np.nonzero(g != v)[0][:5])


# ------------------------------------------------------------------ every regime x every path
@pytest.mark.parametrize("signals", ["clean", "nan_states"])
@pytest.mark.parametrize("caps", CAPS, ids=["nsi5", "nsi8"])
@pytest.mark.parametrize("path,H", PATH_CASES, ids=[f"{p}-h{h}" for p, h in PATH_CASES])
def test_regimes_on_every_policy_kernel(world, plan, path, H, caps, signals):
    """Fitness (float64) and trades of every regime equal the oracle's bits on
    every policy kernel, with 5 and 8 inventory values, on clean signals and
    with NaN states of both signs at ticks 0, 63, 64 and 699."""
    plan(**PATHS[path][0])
    mm, eps = world.batch(H)
    prm, _ = world.params(caps)
    eb = world.episodes(eps, caps)
    fit, trd = world.eng.fitness(world.stores[signals], eb, prm, torch.from_numpy(mm).to(DEV), H)
    fit, trd = fit.cpu().numpy(), trd.cpu().numpy()
    want_f, want_t = world.want(H, caps, signals)
    bad = [(e[2], e[1], fit[i], want_f[i], trd[i], want_t[i]) for i, e in enumerate(eps)
           if not (fit[i] == want_f[i] or (np.isnan(fit[i]) and np.isnan(want_f[i]))) or trd[i] != want_t[i]]
    assert not bad, (path, H, caps, signals, bad)
    assert np.array_equal(trd, want_t) and np.array_equal(fit, want_f, equal_nan=True)


# ------------------------------------------------------------------ trace columns and the summary
@pytest.mark.parametrize("signals", ["clean", "nan_states"])
@pytest.mark.parametrize("H", vr.HIDDEN)
def test_trace_columns_and_summary(world, H, signals):
    """Per step: both offsets, the raws (bits, any NaN = any NaN), inventory,
    fills, cash, reward, pnl and fees of every regime equal the oracle's trace;
    the episode summary equals the host mirror over the oracle's columns."""
    from sgmm_amd.analytics import summary_from_frame
    from test_gpu_evaluation import assert_equals_mirror
    caps = CAPS[H == 32]   # 8 inventory values at H = 32, 5 elsewhere
    mm, eps = world.batch(H)
    prm, _ = world.params(caps)
    eb = world.episodes(eps, caps)
    mmd = torch.from_numpy(mm).to(DEV)
    fit, trd, tr = world.eng.trace(world.stores[signals], eb, prm, mmd, H)
    _, summ = world.eng.summary(world.stores[signals], eb, prm, mm=mmd, hidden=H)
    tr = {k: v.cpu().numpy() for k, v in tr.items()}
    want_f, want_t = world.want(H, caps, signals)
    assert np.array_equal(trd.cpu().numpy(), want_t) and np.array_equal(fit.cpu().numpy(), want_f, equal_nan=True)
    for i, (row, L, regime) in enumerate(eps):
        f, t, want = world.trace(mm[row], H, L, caps, signals)
        assert (f == want_f[i] or np.isnan(f)) and t == want_t[i]
        a = int(eb.step_off[i])
        assert_trace_equal(tr, want, slice(a, a + L), (regime, H, L))
        cols = {k: want[k] for k in ("cash", "inventory", "reward", "fill_buy", "fill_sell")}
        cols["mid"] = world.b[2][:L]
        assert_equals_mirror(summ[i], summary_from_frame(cols), (regime, H, L))


# ------------------------------------------------------------------ sgmm_policy_forward raws
@pytest.mark.parametrize("H", vr.HIDDEN)
def test_policy_forward_raws(world, H):
    """sgmm_policy_forward's raws equal the oracle's bit for bit in every regime
    (sub_out: subnormal raws), NaN states of both signs included; and the relu
    rule as measured: a NaN state contributes 0 in every layer-1 chain, so the
    output is that of the network with a dead first layer -- not NaN."""
    sgmm, oracle = world.sgmm, world.oracle
    mm, _ = world.batch(H)
    s1n, s2n = world.signals["clean"]
    n = 320
    rng = np.random.default_rng(H)
    states = np.stack([s1n[:n], s2n[:n], rng.integers(-4, 4, n) / 2.0], 1).astype(np.float32)
    for k, (col, nan) in enumerate([(0, POS_NAN), (1, NEG_NAN), (2, POS_NAN), (0, NEG_NAN), (2, NEG_NAN)]):
        states[k::16, col] = nan
    idx = (np.arange(n) % len(mm)).astype(np.int32)
    # genome rows whose first layer is dead (W1 = 0, b1 = 0), evaluated at a zero state
    dead = mm.copy()
    dead[:, :4 * H] = 0
    out = sgmm.policy_forward(torch.from_numpy(mm).to(DEV), H, torch.from_numpy(states).to(DEV),
                              torch.from_numpy(idx).to(DEV)).cpu().numpy()
    out_dead = sgmm.policy_forward(torch.from_numpy(dead).to(DEV), H, torch.zeros((n, 3), device=DEV),
                                   torch.from_numpy(idx).to(DEV)).cpu().numpy()
    want = np.stack([oracle.policy_forward(mm[idx[i]], H, states[i]) for i in range(n)])
    bad = [(i, out[i], want[i]) for i in range(n) if not vr.same_raw(out[i], want[i])]
    assert not bad, (H, bad[:4])
    nan_rows = np.isnan(states).any(1)
    assert nan_rows.sum() >= 90
    assert vr.same_raw(out[nan_rows], out_dead[nan_rows])
    sub = [r for r in range(len(mm)) if list(vr.REGIMES)[r // 2] == "sub_out"]   # two rows per regime
    o = out[np.isin(idx, sub) & ~nan_rows]
    assert (np.abs(o[o != 0]) < vr.F32_TINY).sum() >= 10   # subnormal raws came back


# ------------------------------------------------------------------ the adversary on every regime
ADV_CASES = [("table", 16), ("table", 32), ("table", 64), ("valu", 8), ("valu", 16), ("trace", 16), ("trace", 64)]


@pytest.mark.parametrize("path,H", ADV_CASES, ids=[f"{p}-h{h}" for p, h in ADV_CASES])
def test_adversary_on_every_regime(world, plan, path, H):
    """Every MM regime against every adversary kind (tanh in its linear range,
    saturated, on subnormals) at adv_scale 1 and 3: k_policy_table_mfma with the
    adversary (H = 16 / 32 / 64), the VALU table with the adversary and the
    direct (trace) path equal the oracle bit for bit.  The oracle's trace must
    hold the case the int32 offset sum got wrong: an action of INT32_MAX
    (INT32_MIN) on a step whose adversary delta is positive (negative)."""
    sgmm, oracle = world.sgmm, world.oracle
    caps = CAPS[H == 32]   # 8 inventory values at H = 32, 5 elsewhere
    advs = np.stack([vr.adversary(kind, s) for kind in vr.ADV_KINDS for s in (0, 1)])
    scales = (1.0, 3.0)
    rows, eps, adv_idx, par = [], [], [], []
    for ri, regime in enumerate(vr.REGIMES):
        rows.append(vr.genome(regime, H, vr.seeds(regime, H)[0]))
        for ai in range(len(advs)):
            k = ri * len(advs) + ai
            eps.append((ri, LENGTHS[k % 5 == 4], regime))
            adv_idx.append(ai)
            par.append(k % 2)
    mm = np.stack(rows)
    prm, orc = world.params(caps, scales)
    eb = world.episodes(eps, caps, adv=adv_idx, param=par)
    mmd, advd = torch.from_numpy(mm).to(DEV), torch.from_numpy(advs).to(DEV)
    if path == "trace":
        fit, trd, tr = world.eng.trace(world.stores["clean"], eb, prm, mmd, H, advd)
        tr = {k: v.cpu().numpy() for k, v in tr.items()}
    else:
        plan(policy_path=path)
        fit, trd = world.eng.fitness(world.stores["clean"], eb, prm, mmd, H, advd)
    fit, trd = fit.cpu().numpy(), trd.cpu().numpy()
    wrapped = moved = 0
    for i, (row, L, regime) in enumerate(eps):
        f, t, want = world.trace(mm[row], H, L, caps, "clean", advs[adv_idx[i]], scales[par[i]])
        assert trd[i] == t and (fit[i] == f or (np.isnan(f) and np.isnan(fit[i]))), \
            (path, H, regime, vr.ADV_KINDS[adv_idx[i] // 2], scales[par[i]], L, fit[i], f, trd[i], t)
        if path == "trace":
            a = int(eb.step_off[i])
            assert_trace_equal(tr, want, slice(a, a + L), (regime, H, L, adv_idx[i]))
        for o, d in (("off_a", "adv_a"), ("off_b", "adv_b")):
            wrapped += int(((want[o] == vr.INT32_MAX) & (want[d] > 0)).sum() +
                           ((want[o] == vr.INT32_MIN) & (want[d] < 0)).sum())
            moved += int((want[d] != 0).sum())
    assert wrapped > 0 and moved > 100, (wrapped, moved)


# ------------------------------------------------------------------ raw -> action at the int32 edge
@pytest.mark.parametrize("path", ["trace", "valu", "table_sp", "table_v3", "frontier1_spill"])
def test_action_conversion_edges(golden, world, plan, path):
    """rint(raw * 5) -> int32 at the edge of the range: one-tick episodes whose
    raws are b3 (every other parameter 0), for raws around +-2^31 / 5, beyond
    int64, inf and NaN.  The trace's offsets equal the reference's int64 action
    saturated at int32 (2147483520 = 2^31 - 128, the largest float below 2^31,
    is an int32 value and stays itself); every kernel's fitness equals the oracle's."""
    H = 16
    raws = golden("g12_int_edges.npz")["big_raw"]
    mm = np.zeros((len(raws), vr.n_params(H)), np.float32)
    mm[:, -2], mm[:, -1] = raws, raws[::-1]
    eps = [(i, 1, "b3") for i in range(len(raws))]
    prm, _ = world.params(CAPS[0])
    eb = world.episodes(eps, CAPS[0])
    mmd = torch.from_numpy(mm).to(DEV)
    want = [world.trace(mm[i], H, 1, CAPS[0], "clean") for i in range(len(raws))]
    acts = np.array([vr.action_exact(r) for r in raws])
    assert 2147483520 in acts and -2147483520 in acts and vr.INT32_MAX in acts and vr.INT32_MIN in acts
    assert np.array_equal([w[2]["off_a"][0] for w in want], acts)
    if path == "trace":
        fit, trd, tr = world.eng.trace(world.stores["clean"], eb, prm, mmd, H)
        assert np.array_equal(tr["off_a"].cpu().numpy(), acts)
        assert np.array_equal(tr["off_b"].cpu().numpy(), acts[::-1])
    else:
        plan(**PATHS[path][0])
        fit, trd = world.eng.fitness(world.stores["clean"], eb, prm, mmd, H)
    assert np.array_equal(fit.cpu().numpy(), [w[0] for w in want])
    assert np.array_equal(trd.cpu().numpy(), [w[1] for w in want])


# ------------------------------------------------------------------ env step at the int32 edge
def test_env_step_batch_at_the_int32_edge(golden, sgmm):
    """sgmm_env_step_batch equals the reference where the action has saturated
    and the adversary's delta is added on top (tests/golden/g12_int_edges.npz)."""
    d = golden("g12_int_edges.npz")
    n = len(d["off_a"])
    env = sgmm.FTPEnvBatch(n, phi=float(d["phi"]), tick_size=float(d["tick"]), fee_rate=d["fee"], device=DEV)
    env.inventory.copy_(torch.from_numpy(d["inv_before"].astype(np.int32)))
    env.cash.copy_(torch.from_numpy(d["cash_before"]))
    act = np.stack([d["off_a"], d["off_b"]], 1)
    adv = np.stack([d["adv_a"], d["adv_b"]], 1)   # rows without an adversary carry zero deltas
    r, info = env.step(act, float(d["mid"]), float(d["ask"]), float(d["bid"]), float(d["buy_max"]),
                       float(d["sell_min"]), adv_action=adv)
    assert np.array_equal(env.inventory.cpu().numpy(), d["inventory"])
    assert np.array_equal(env.cash.cpu().numpy(), d["cash"])
    assert np.array_equal(r.cpu().numpy(), d["reward"])
    assert np.array_equal(info["pnl_reward"].cpu().numpy(), d["pnl"])
    assert np.array_equal(info["inventory_reward"].cpu().numpy(), d["inv_reward"])
    assert np.array_equal(info["fee_paid"].cpu().numpy(), d["fee_paid"])
    assert np.array_equal(info["fill_buy"].cpu().numpy(), d["fill_buy"])
    assert np.array_equal(info["fill_sell"].cpu().numpy(), d["fill_sell"])
