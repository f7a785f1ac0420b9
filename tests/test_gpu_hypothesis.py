"""The device hypothesis tests on the GPU: sgmm_mbb_sharpe / sgmm_dm_test /
sgmm_durbin_watson / sgmm_trace_wealth bit for bit against the host mirrors of
analytics.py (float64 division and square root are correctly rounded on the
device; only the DM p-value, which goes through erfc, is compared at
16 * 2^-53 absolute), and against the reference's own values
(tests/golden/g10_hypothesis.npz) at the tolerances of test_hypothesis.py."""
import numpy as np
import pytest
import torch

from conftest import has_gpu
from ga_model import philox4x32_10
from test_hypothesis import dm_inputs, dm_tols, mbb_cases, tol, zero_wealth

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

P_TOL = 16 * 2.0 ** -53
DEV = "cuda:0"


@pytest.fixture(scope="module")
def g10(golden):
    return golden("g10_hypothesis.npz")


@pytest.fixture(scope="module")
def eng(sgmm):
    return sgmm.RolloutEngine(torch.device(DEV))


def batch(series):
    """(device values, host offsets) of a list of host series."""
    arrs = [np.ascontiguousarray(s, np.float64).reshape(-1) for s in series]
    off = np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
    flat = np.concatenate(arrs + [np.zeros(1)])
    return torch.from_numpy(flat).to(DEV), off


def starts_tensor(mats, n_boot):
    """Per-series (n_boot, num_blocks) start matrices (None: not resampled) -> [n, n_boot, stride]."""
    stride = max([1] + [m.shape[1] for m in mats if m is not None])
    host = np.zeros((len(mats), n_boot, stride), np.int32)
    for i, m in enumerate(mats):
        if m is not None:
            host[i, :, :m.shape[1]] = m
    return torch.from_numpy(host).to(DEV)


def same(a, b):
    """Bit equality of float64 values (zero signs count); a NaN equals a NaN:
    the sign and payload of a generated NaN (0 / 0) are not part of the contract."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    keep = ~np.isnan(a)
    return a[keep].tobytes() == b[keep].tobytes()


def assert_equals_mirror(out, series, bs, n_boot, what=""):
    """Every output of one mbb_sharpe call (made with want_starts) against
    analytics.mbb_from_wealth run on the starts the device used."""
    from sgmm_amd.analytics import mbb_from_wealth
    rec = out.records()
    boot, rets, used = out.boot.cpu().numpy(), out.returns.cpu().numpy(), out.starts.cpu().numpy()
    for s, w in enumerate(series):
        nb = int(rec["num_blocks"][s])
        o, mboot, r, mused = mbb_from_wealth(w, bs, n_boot, used[s, :, :nb] if nb else None)
        tag = (what, s, len(w), bs, n_boot)
        a = int(out.off[s])
        assert rec["n_returns"][s] == len(r) and same(rets[a:a + len(r)], r), tag
        assert nb == o["num_blocks"] and np.array_equal(used[s, :, :nb], mused), tag
        assert same(boot[s], mboot), tag
        for f in ("mean_sr", "ci_lo", "ci_hi"):
            assert same(rec[f][s], o[f]), (tag, f, rec[f][s], o[f])
        assert rec["zero_replicates"][s] == o["zero_replicates"] and rec["flags"][s] == o["flags"], tag
    return rec


def walk(T, seed, level=100.0):
    return level + np.cumsum(np.random.default_rng(seed).normal(0, 0.5, T))


# ------------------------------------------------------------------ the fixture
def test_fixture_cases_equal_mirror_and_reference(sgmm, eng, g10):
    """The 32 bootstrap cases with the starts the reference drew, one launch set
    per (block_size, n_boot): the device equals the mirror bit for bit and the
    reference's return values within tolerance."""
    cases = list(mbb_cases(g10))
    shapes = sorted({(c[2], c[3]) for c in cases})
    assert len(shapes) == 3
    for bs, n_boot in shapes:
        grp = [c for c in cases if (c[2], c[3]) == (bs, n_boot)]
        series = [c[1] for c in grp]
        w, off = batch(series)
        out = eng.mbb_sharpe(w, off, bs, n_boot, starts=starts_tensor([c[4] for c in grp], n_boot), want_starts=True)
        rec = assert_equals_mirror(out, series, bs, n_boot, "fixture")
        used = out.starts.cpu().numpy()
        for s, c in enumerate(grp):
            if c[4] is not None:
                assert np.array_equal(used[s, :, :c[4].shape[1]], c[4])   # in range: used as given
            for f, want in zip(("mean_sr", "ci_lo", "ci_hi"), c[5]):
                assert abs(rec[f][s] - want) <= tol(want), (c[0], f, rec[f][s], want)
            assert rec["zero_replicates"][s] == c[6] and (rec["flags"][s] == 2) == (c[4] is None)


def test_get_mbb_sharpe_under_numpy_seed(sgmm, g10):
    """analytics.get_mbb_sharpe draws from numpy's global stream as the
    reference does: np.random.seed(7) gives the reference's numbers."""
    from sgmm_amd.analytics import get_mbb_sharpe
    import pandas as pd
    for k, w, bs, n_boot, st, ref, zero in mbb_cases(g10):
        if (bs, n_boot) != (100, 500) or len(w) not in (960, 101, 102):
            continue
        np.random.seed(int(g10["mbb_seed"][k]))
        mean, ci = get_mbb_sharpe(pd.Series(w), block_size=bs, n_boot=n_boot)
        assert abs(mean - ref[0]) <= tol(ref[0]) and abs(ci[0] - ref[1]) <= tol(ref[1]) and abs(ci[1] - ref[2]) <= tol(ref[2])
        assert isinstance(ci, tuple if st is None else np.ndarray)
    np.random.seed(7)
    mean, ci = get_mbb_sharpe(pd.Series(g10["wealth"][0]))
    assert abs(mean - 0.3192090092130385) <= 1e-12 and np.allclose(ci, [0.01888955, 0.49677898], atol=1e-8)


# ------------------------------------------------------------------ shapes
def lengths(bs):
    return [0, 1, 2, bs, bs + 1, bs + 2, 2 * bs, 2 * bs + 1, 960]


@pytest.mark.parametrize("bs", [1, 7, 63, 64, 65, 100])
def test_shapes_equal_mirror(sgmm, eng, bs):
    """A ragged batch of every length around the branches, at every n_boot
    around the sort's padding and the wave tiles; Philox starts."""
    series = [walk(T, 10 * bs + i) for i, T in enumerate(lengths(bs))]
    w, off = batch(series)
    seen = set()
    for n_boot in (1, 2, 3, 41, 64, 65, 500, 512, 513):
        out = eng.mbb_sharpe(w, off, bs, n_boot, seed=bs * 1000 + n_boot, want_starts=True)
        rec = assert_equals_mirror(out, series, bs, n_boot, "shapes")
        seen |= set(rec["num_blocks"].tolist())
        assert (rec["flags"] & 1).sum() == 0
    # one block needs bs < n < 2 bs: no such n at block size 1
    assert ({0, 2, 959 // bs} | ({1} if bs > 1 else set())) <= seen


def test_300_ragged_series_in_one_launch(sgmm, eng):
    rng = np.random.default_rng(8)
    pool = sorted({T for bs in (7, 63, 64, 65, 100) for T in lengths(bs)})
    series = [walk(int(rng.choice(pool)), 500 + i, level=20.0 + i) for i in range(300)]
    w, off = batch(series)
    out = eng.mbb_sharpe(w, off, 7, 65, seed=99, want_starts=True)
    rec = assert_equals_mirror(out, series, 7, 65, "300")
    assert len(set(rec["num_blocks"].tolist())) >= 8 and (rec["flags"] == 2).any() and (rec["flags"] == 0).any()


def test_long_series(sgmm, eng):
    """Series of more than 8192 returns (64 KB) beside a short one: 82 blocks
    (two rounds of 64 block starts) at block 100, two blocks of 4000."""
    series = [walk(T, 70 + i, level=500.0) for i, T in enumerate((8193, 8194, 960, 8300, 8192))]
    w, off = batch(series)
    for bs, n_boot in ((100, 17), (4000, 3)):
        out = eng.mbb_sharpe(w, off, bs, n_boot, seed=bs, want_starts=True)
        rec = assert_equals_mirror(out, series, bs, n_boot, "long")
        assert rec["n_returns"].tolist() == [8192, 8193, 959, 8299, 8191]
        assert rec["num_blocks"].tolist() == ([81, 81, 9, 82, 81] if bs == 100 else [2, 2, 0, 2, 2])


def test_constant_zero_and_inf_wealth(sgmm, eng):
    """std 0 gives 0 everywhere; 0 / 0 returns are dropped in order and x / 0
    kept, as pandas does; a replicate that holds an inf comes out 0."""
    import pandas as pd
    wz = zero_wealth()
    series = [np.full(50, 3.0), wz, np.zeros(40), np.concatenate([[0.0], walk(80, 4)])]
    w, off = batch(series)
    out = eng.mbb_sharpe(w, off, 7, 64, seed=5, want_starts=True)
    rec = assert_equals_mirror(out, series, 7, 64, "special")
    boot, rets = out.boot.cpu().numpy(), out.returns.cpu().numpy()
    assert (boot[0] == 0.0).all() and rec["zero_replicates"][0] == 64 and rec["mean_sr"][0] == rec["ci_lo"][0] == 0.0
    want = pd.Series(wz).pct_change().dropna().values
    assert rec["n_returns"][1] == len(want) and same(rets[off[1]:off[1] + len(want)], want) and np.isinf(want).sum() == 3
    assert rec["n_returns"][2] == 0 and rec["flags"][2] == 2 and rec["mean_sr"][2] == 0.0
    assert 0 < rec["zero_replicates"][3] < 64 and np.isinf(rets[off[3]])
    assert not np.isnan(boot).any()


# ------------------------------------------------------------------ Philox starts
def philox_starts(seed, s, n_boot, nb, span):
    """The header's stream: block j of replicate b of series s takes output
    j % 4 of Philox4x32-10 with counter (j / 4, b, s, 2) and the seed's two
    words as key; start = (word * (span + 1)) >> 32."""
    j, b = np.meshgrid(np.arange(nb, dtype=np.uint64), np.arange(n_boot, dtype=np.uint64))
    words = philox4x32_10((j // np.uint64(4), b, np.full_like(j, s), np.full_like(j, 2)),
                          (seed & 0xFFFFFFFF, seed >> 32))
    word = np.choose((j % np.uint64(4)).astype(np.int64), [np.asarray(x, np.uint64) for x in words])
    return ((word * np.uint64(span + 1)) >> np.uint64(32)).astype(np.int32)


def test_philox_starts(sgmm, eng):
    seed = 0x9E3779B97F4A7C15
    bs = 5
    series = [walk(T, 40 + i) for i, T in enumerate((960, 8, 333, 4, 71))]   # 8 rows: n - bs + 1 = 3
    w, off = batch(series)
    out = eng.mbb_sharpe(w, off, bs, 4096, seed=seed, want_starts=True)
    rec, used = out.records(), out.starts.cpu().numpy()
    assert rec["num_blocks"].tolist() == [191, 1, 66, 0, 14]
    for s in range(5):
        nb, n = int(rec["num_blocks"][s]), int(rec["n_returns"][s])
        if nb == 0:
            continue
        want = philox_starts(seed, s, 4096, nb, n - bs)
        assert np.array_equal(used[s, :, :nb], want), s
        assert used[s, :, :nb].min() >= 0 and used[s, :, :nb].max() <= n - bs
    assert sorted(set(used[1, :, 0].tolist())) == [0, 1, 2] and np.bincount(used[1, :, 0]).min() > 1200
    # the starts fed back give identical bits; so does the same seed; another seed differs
    again = eng.mbb_sharpe(w, off, bs, 4096, starts=out.starts, want_starts=True)
    twice = eng.mbb_sharpe(w, off, bs, 4096, seed=seed)
    other = eng.mbb_sharpe(w, off, bs, 4096, seed=seed + 1, want_starts=True)
    for o in (again, twice):
        assert o.records().tobytes() == rec.tobytes() and torch.equal(o.boot, out.boot)
    assert torch.equal(again.starts, out.starts)
    assert not torch.equal(other.starts, out.starts) and not torch.equal(other.boot[0], out.boot[0])
    assert other.records()["mean_sr"][0] != rec["mean_sr"][0]


def test_out_of_range_starts_are_clamped_and_flagged(sgmm, eng):
    bs, n_boot = 7, 65
    series = [walk(120, 1), walk(300, 2), walk(90, 3)]
    rng = np.random.default_rng(6)
    good = [rng.integers(0, len(s) - 1 - bs + 1, (n_boot, (len(s) - 1) // bs)) for s in series]
    bad = [g.copy() for g in good]
    bad[0][bad[0] == 0] = -1
    bad[0][3, 2] = -2 ** 31
    bad[2][bad[2] == len(series[2]) - 1 - bs] = len(series[2]) - 1      # n
    bad[2][5, 1] = 2 ** 31 - 1
    good[0][3, 2], good[2][5, 1] = 0, len(series[2]) - 1 - bs
    w, off = batch(series)
    a = eng.mbb_sharpe(w, off, bs, n_boot, starts=starts_tensor(good, n_boot), want_starts=True)
    b = eng.mbb_sharpe(w, off, bs, n_boot, starts=starts_tensor(bad, n_boot), want_starts=True)
    ra, rb = assert_equals_mirror(a, series, bs, n_boot, "good"), b.records()
    assert ra["flags"].tolist() == [0, 0, 0] and rb["flags"].tolist() == [1, 0, 1]
    assert torch.equal(a.starts, b.starts) and torch.equal(a.boot, b.boot)
    for f in ("mean_sr", "ci_lo", "ci_hi", "zero_replicates"):
        assert same(ra[f], rb[f]) if ra[f].dtype == np.float64 else np.array_equal(ra[f], rb[f])


# ------------------------------------------------------------------ DM / DW
def test_dm_and_dw_equal_mirror_and_reference(sgmm, eng, g10):
    from sgmm_amd.analytics import dm_from_series, dw_from_series
    rng = np.random.default_rng(12)
    for crit in ("MSE", "MAD"):
        ks = [k for k in range(len(g10["dm_crit"])) if (g10["dm_crit"][k] == 0) == (crit == "MSE")]
        trip = [dm_inputs(g10, k)[:3] for k in ks]
        for T in (0, 1, 2, 63, 64, 65, 300):   # ragged, around the lane count
            trip.append((rng.normal(0, 1, T), rng.normal(0, 1, T), rng.normal(0, 1, T)))
        nan = rng.normal(0, 1, 100)
        nan[17] = np.nan
        trip.append((nan, rng.normal(0, 1, 100), rng.normal(0, 1, 100)))
        (a, off), (p1, _), (p2, _) = (batch([t[i] for t in trip]) for i in range(3))
        _, got = eng.dm_test(a, p1, p2, off, crit)
        _, naive = eng.dm_test(a, p1, None, off, crit)
        for s, t in enumerate(trip):
            for rec, m in ((got[s], dm_from_series(*t, crit)), (naive[s], dm_from_series(t[0], t[1], None, crit))):
                for f in ("stat", "mean_d", "var_d"):
                    assert same(rec[f], m[f]), (crit, s, f, rec[f], m[f])
                assert rec["n"] == m["n"] == len(t[0])
                assert (np.isnan(rec["p_value"]) and np.isnan(m["p_value"])) or abs(rec["p_value"] - m["p_value"]) <= P_TOL
        for s, k in enumerate(ks):
            stat, p = g10["dm_result"][k]
            ts, tp = dm_tols(stat, len(trip[s][0]))
            assert abs(got["stat"][s] - stat) <= ts and abs(got["p_value"][s] - p) <= tp, (k, got[s])
        assert np.isnan(got["stat"][len(ks)]) and np.isnan(got["stat"][len(ks) + 1]) and np.isnan(got["stat"][-1])
    series = [g10["reward"][f, :rows] for f, rows in zip(g10["dw_frame"], g10["dw_rows"])]
    series += [np.zeros(0), rng.normal(0, 1, 64), rng.normal(0, 1, 129), np.zeros(5)]
    v, off = batch(series)
    dw = eng.durbin_watson(v, off).cpu().numpy()
    assert same(dw, [dw_from_series(e) for e in series])
    for s, want in enumerate(g10["dw_value"]):
        assert (np.isnan(dw[s]) and np.isnan(want)) or abs(dw[s] - want) <= tol(want)
    assert np.isnan(dw[len(g10["dw_value"])]) and np.isnan(dw[-1])


def test_reference_named_functions_and_report(sgmm, g10, capsys):
    """analytics.dm_test / durbin_watson with the reference's signatures, and
    hypothesis_report's lines in main.py's formats."""
    import pandas as pd
    from sgmm_amd import analytics as A
    a, p1, p2, _ = dm_inputs(g10, 0)
    stat, p = A.dm_test(pd.Series(a), pd.Series(p1), p2, h=1, crit="MSE")
    ts, tp = dm_tols(g10["dm_result"][0, 0], len(a))
    assert abs(stat - g10["dm_result"][0, 0]) <= ts and abs(p - g10["dm_result"][0, 1]) <= tp
    full = [k for k in range(16) if g10["dw_rows"][k] == 960 and g10["dw_frame"][k] == 0][0]
    dw = A.durbin_watson(pd.Series(g10["reward"][0]))
    assert abs(dw - g10["dw_value"][full]) <= tol(dw)
    methods = [str(m) for m in g10["methods"]]
    frames = {m: pd.DataFrame({"wealth": g10["wealth"][i], "reward": g10["reward"][i], "mid": g10["arl_mid"],
                               "s2_pred": g10["arl_s2_pred"]}) for i, m in enumerate(methods)}
    del frames["foic"]
    capsys.readouterr()
    np.random.seed(7)
    res = A.hypothesis_report(frames)
    lines = capsys.readouterr().out.splitlines()
    # the ARL frame is drawn first, so its starts are the fixture's seed-7 starts
    ref = next(c[5] for c in mbb_cases(g10) if g10["mbb_frame"][c[0]] == 0 and (c[2], c[3], len(c[1])) == (100, 500, 960))
    assert lines[0] == f"H1 (DM Test): Statistic={g10['dm_result'][0, 0]:.4f}, p-value={g10['dm_result'][0, 1]:.4f}"
    assert lines[1] == f"H2: DW-Stat = {g10['dw_value'][full]:.4f}" and lines[2] == "H3: 95% CI of Per-Step Sharpe:"
    assert lines[3] == f"  - {'ARL':<4}: {ref[0]:>8.6f} | CI: [{ref[1]:>8.6f}, {ref[2]:>8.6f}]"
    assert lines[4].startswith("  - DRL :") and lines[5].startswith("  - GLFT:")
    assert lines[6] == "  - FOIC: No data found in DataFrame." and len(lines) == 7
    assert abs(res["mbb"]["arl"][0] - ref[0]) <= tol(ref[0]) and set(res["mbb"]) == {"arl", "drl", "glft"}


# ------------------------------------------------------------------ traces
@pytest.fixture(scope="module")
def traced(sgmm, eng):
    """An MLP trace and a rule trace of ragged episodes, one of length 0."""
    from sgmm_amd import benchmarks as B
    from sgmm_amd import synthetic
    dev = torch.device(DEV)
    b = synthetic.bundle_510300(400, seed=21)
    st = synthetic.train_stats(b)
    ts = sgmm.TickStore()
    ts.add(b, st)
    ts.to(dev)
    ln = np.array([400, 0, 1, 65, 130, 0, 257, 2])
    to = np.array([0, 7, 399, 100, 5, 0, 143, 11])
    params = sgmm.params_tensor([sgmm.EnvConfig(phi=1e-4, tick_size=0.001), sgmm.EnvConfig(phi=1e-3, tick_size=0.001)], dev)
    eps = sgmm.EpisodeBatch(np.arange(8) % 3, to, ln, np.arange(8) % 2).to(dev)
    mm = synthetic.population(3, 16, sigma=0.3, seed=2).to(dev).contiguous()
    rules = np.stack([B.quote_rule(B.FOICPolicy(0, 0)), B.quote_rule(B.FOICPolicy(1, -1)),
                      B.quote_rule(B.GLFTPolicy(gamma=1e-4, kappa=3000, A=0.1, sigma=2.0))])
    _, _, tr = eng.trace(ts, eps, params, mm, 16)
    _, _, rtr = eng.trace_rules(ts, eps, params, rules)
    return b, ts, eps, tr, rtr


def test_trace_wealth_equals_host_columns(sgmm, eng, traced):
    b, ts, eps, tr, rtr = traced
    held = 0
    for t in (tr, rtr):
        w = eng.wealth(ts, eps, t).cpu().numpy()
        cash, inv = t["cash"].cpu().numpy(), t["inventory"].cpu().numpy()
        assert len(w) == eps.total_steps == 855
        for e in range(eps.n):
            a, T, o = int(eps.step_off[e]), int(eps.length[e]), int(eps.tick_off[e])
            assert same(w[a:a + T], cash[a:a + T] + inv[a:a + T] * b[2][o:o + T]), e
        held += int(np.abs(inv).max())
    assert held > 0


def test_trace_to_bootstrap_stays_on_device(sgmm, eng, traced):
    """trace -> wealth -> mbb_sharpe with nothing copied to the host equals the
    route through host frames (analytics.mbb_sharpe on the copied wealth)."""
    from sgmm_amd.analytics import mbb_sharpe
    b, ts, eps, tr, rtr = traced
    off = np.concatenate([eps.step_off, [eps.total_steps]])
    resampled = 0
    for t in (tr, rtr):
        w = eng.wealth(ts, eps, t)
        out = eng.mbb_sharpe(w, off, 20, 41, seed=3, want_starts=True)
        host = w.cpu().numpy()
        series = [host[off[e]:off[e + 1]] for e in range(eps.n)]
        rec = assert_equals_mirror(out, series, 20, 41, "trace")
        assert mbb_sharpe(series, 20, 41, seed=3).tobytes() == rec.tobytes()
        assert set(rec["num_blocks"].tolist()) <= {0, 3, 6, 12, 19}   # fewer where 0 / 0 returns were dropped
        resampled += int((rec["num_blocks"] > 0).sum())
    assert resampled > 0


def test_streams_give_the_same_results(sgmm, eng, g10):
    """A non-default stream and the NULL stream."""
    import ctypes
    from sgmm_amd._lib import check, ptr
    from sgmm_amd.rollout import MBB_DTYPE
    series = [g10["wealth"][i, :rows] for i, rows in ((0, 960), (1, 333), (2, 50))]
    w, off = batch(series)
    base = eng.mbb_sharpe(w, off, 64, 65, seed=11)
    dw0 = eng.durbin_watson(w, off)
    _, dm0 = eng.dm_test(w, w * 0.5, None, off)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = eng.mbb_sharpe(w, off, 64, 65, seed=11, stream=side)
        dw1 = eng.durbin_watson(w, off, stream=side)
        _, dm1 = eng.dm_test(w, w * 0.5, None, off, stream=side)
    side.synchronize()
    assert other.records().tobytes() == base.records().tobytes() and torch.equal(other.boot, base.boot)
    assert torch.equal(dw0, dw1) and dm0.tobytes() == dm1.tobytes()
    # the NULL stream, through the C ABI itself
    out = torch.zeros((3, 40), dtype=torch.uint8, device=DEV)
    boot = torch.zeros((3, 65), dtype=torch.float64, device=DEV)
    rets = torch.zeros(int(off[-1]), dtype=torch.float64, device=DEV)
    off_d = torch.from_numpy(off).to(DEV)
    torch.cuda.synchronize()
    check(eng.L.sgmm_mbb_sharpe(ptr(w), ptr(off_d), off.ctypes.data, 3, 64, 65, None, 0, ctypes.c_uint64(11), ptr(out),
                                ptr(boot), None, ptr(rets), None), "sgmm_mbb_sharpe")
    torch.cuda.synchronize()
    assert out.cpu().numpy().reshape(-1).view(MBB_DTYPE).tobytes() == base.records().tobytes()
    assert torch.equal(boot, base.boot)
