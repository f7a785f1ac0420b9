"""The hypothesis tests of main.py:227-297 without a GPU: the host mirrors of
the device arithmetic (analytics.mbb_from_wealth / dm_from_series /
dw_from_series) against the reference's own values
(tests/golden/g10_hypothesis.npz), the summation order they restate, the
returns compaction against pandas, and the C ABI's structs and argument checks.

Tolerances against the reference (whose numpy sums are pairwise, the device's
are lane sums):
  mean, CI bounds, DW   |d| <= 1e-9 |x| + 1e-12: 1e-9 is the project's Sharpe
                        tolerance; the absolute term bounds a reordered sum of
                        m <= 1000 doubles in mean / std (m 2^-53 ~ 1e-13)
  DM statistic          1e-9 |x| + n^1.5 2^-52 (the mean's reorder error times sqrt(n) / std)
  DM p-value            absolute 0.8 tol(stat) + 16 2^-53 (0.8 >= 2 phi(x); the
                        erfc form against scipy's norm.cdf form, and head-room
                        for the device's erfc)
"""
import ctypes
import math
import re

import numpy as np
import pytest

from test_capi import HEADER


@pytest.fixture(scope="module")
def g10(golden):
    return golden("g10_hypothesis.npz")


def tol(x):
    return 1e-9 * abs(x) + 1e-12


def dm_tols(stat, n):
    ts = 1e-9 * abs(stat) + n ** 1.5 * 2.0 ** -52
    return ts, 0.8 * ts + 16 * 2.0 ** -53


def close(got, want, t):
    return (np.isnan(got) and np.isnan(want)) or abs(got - want) <= t


def mbb_cases(g):
    """(k, wealth, block_size, n_boot, starts or None, reference (mean, lo, hi), zero replicates)"""
    for k in range(len(g["mbb_frame"])):
        n_boot, nb = int(g["mbb_n_boot"][k]), int(g["mbb_num_blocks"][k])
        a, b = g["mbb_starts_off"][k:k + 2]
        st = g["mbb_starts"][a:b].reshape(n_boot, nb) if nb else None
        yield (k, g["wealth"][g["mbb_frame"][k], :g["mbb_rows"][k]], int(g["mbb_block_size"][k]), n_boot, st,
               g["mbb_result"][k], int(g["mbb_zero"][k]))


def dm_inputs(g, k):
    mid, s2 = g["arl_mid"], g["arl_s2_pred"]
    actual, pred = mid[1:] - mid[:-1], s2[:-1]
    return actual, g["dm_k"][k] * pred, g["dm_c"][k] * pred, "MSE" if g["dm_crit"][k] == 0 else "MAD"


def lane_sum_spec(x):
    """include/sgmm.h's lane sum, one scalar operation at a time."""
    lanes = [0.0] * 64
    for i, v in enumerate(x):
        lanes[i % 64] = lanes[i % 64] + float(v)
    for d in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[j] + lanes[j ^ d] for j in range(64)]
    assert len(set(lanes)) == 1 or any(math.isnan(v) for v in lanes)
    return lanes[0]


def zero_wealth(T=260, seed=3):
    """A wealth path with zeros at rows 0, 1, 63, 64 and three consecutive rows:
    0 / 0 returns (NaN, dropped), x / 0 (inf, kept) and 0 / x - 1 = -1."""
    w = 100.0 + np.cumsum(np.random.default_rng(seed).normal(0, 1.0, T))
    w[[0, 1, 63, 64, 130, 131, 132]] = 0.0
    return w


def test_lane_sum_is_the_documented_order(sgmm):
    from sgmm_amd.analytics import lane_sum
    rng = np.random.default_rng(0)
    for n in (0, 1, 2, 63, 64, 65, 128, 200, 959):
        x = rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 8, n)
        assert lane_sum(x) == lane_sum_spec(x), n
    x = rng.normal(0, 1, (5, 300))
    assert lane_sum(x).tolist() == [lane_sum_spec(r) for r in x]
    x[2, 70] = np.inf
    x[3, 5] = np.nan
    got = lane_sum(x)
    assert got[2] == np.inf and np.isnan(got[3]) and got[0] == lane_sum_spec(x[0])
    assert lane_sum(np.array([-0.0])) == 0.0 and not np.signbit(lane_sum(np.array([-0.0])))


def test_percentile_rule_is_numpys(sgmm):
    from sgmm_amd.analytics import percentile_linear
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 41, 64, 65, 500, 512, 513, 4096):
        v = np.sort(rng.normal(0, 1, n))
        want = np.percentile(v, [2.5, 97.5])
        assert [percentile_linear(v, 2.5), percentile_linear(v, 97.5)] == want.tolist(), n


def test_returns_compaction_equals_pandas(sgmm):
    import pandas as pd
    from sgmm_amd.analytics import returns_from_wealth
    w = zero_wealth()
    want = pd.Series(w).pct_change().dropna().values
    got = returns_from_wealth(w)
    assert got.tobytes() == want.tobytes()
    # 0 / 0 at rows 1, 64, 131 and 132 (dropped); x / 0 at rows 2, 65, 133; 0 / x at rows 63 and 130
    assert np.isinf(got).sum() == 3 and len(got) == len(w) - 1 - 4 and (got == -1.0).sum() == 2
    assert len(returns_from_wealth([])) == 0 and len(returns_from_wealth([5.0])) == 0


def test_mbb_mirror_matches_reference(sgmm, g10):
    """Every bootstrap case of the fixture, with the starts the reference drew."""
    from sgmm_amd.analytics import mbb_from_wealth
    worst, n_cases = 0.0, 0
    for k, w, bs, n_boot, st, ref, zero in mbb_cases(g10):
        o, boot, r, used = mbb_from_wealth(w, bs, n_boot, st)
        for f, want in zip(("mean_sr", "ci_lo", "ci_hi"), ref):
            d = abs(o[f] - want)
            worst = max(worst, d)
            print(f"case {k} bs={bs} n_boot={n_boot} rows={len(w)} {f}: {o[f]!r} vs {want!r} (|d| = {d:.3g})")
            assert d <= tol(want), (k, f)
        assert o["zero_replicates"] == zero and o["num_blocks"] == g10["mbb_num_blocks"][k]
        assert (o["flags"] == 2) == (st is None) and o["n_returns"] == len(r)
        n_cases += 1
    print("worst |mirror - reference| over", n_cases, "cases:", worst)
    assert n_cases == 32


def test_mbb_mirror_keeps_inf_by_ieee(sgmm, g10):
    """The DRL frame starts at wealth 0: one inf return, and exactly the
    replicates that contain it come out 0 (NaN std compares false)."""
    from sgmm_amd.analytics import mbb_from_wealth
    k, w, bs, n_boot, st, ref, zero = next(c for c in mbb_cases(g10)
                                           if c[2] == 100 and c[3] == 500 and len(c[1]) == 960
                                           and g10["mbb_frame"][c[0]] == 1)
    o, boot, r, used = mbb_from_wealth(w, bs, n_boot, st)
    assert np.isinf(r).sum() == 1 and zero == 5
    i = int(np.nonzero(np.isinf(r))[0][0])
    hit = ((used <= i) & (i < used + bs)).any(axis=1)
    assert np.array_equal(boot == 0.0, hit) and hit.sum() == 5


def test_mbb_mirror_branches(sgmm):
    from sgmm_amd.analytics import mbb_from_wealth
    rng = np.random.default_rng(2)
    w = 50.0 + np.cumsum(rng.normal(0, 0.3, 40))
    for rows, bs in ((0, 5), (1, 5), (2, 5), (6, 5), (40, 39), (40, 100)):   # n = rows - 1 <= bs: no bootstrap
        o, boot, r, used = mbb_from_wealth(w[:rows], bs, 7)
        want = 0.0 if len(r) == 0 or not np.std(r) > 1e-9 else np.mean(r) / np.std(r)
        assert o["flags"] == 2 and o["num_blocks"] == 0 and used.shape == (7, 0)
        assert abs(o["mean_sr"] - want) <= tol(want) and o["ci_lo"] == o["ci_hi"] == o["mean_sr"]
        assert (boot == o["mean_sr"]).all()
    with pytest.raises(ValueError, match="block starts"):
        mbb_from_wealth(w, 5, 7)
    # an all-constant wealth: std 0, every replicate 0
    o, boot, _, _ = mbb_from_wealth(np.full(30, 3.0), 4, 9, np.zeros((9, 7), np.int64))
    assert (boot == 0.0).all() and o["zero_replicates"] == 9 and o["mean_sr"] == o["ci_lo"] == o["ci_hi"] == 0.0
    # starts outside [0, n - block_size] are clamped and flagged
    st = rng.integers(0, 36, (7, 7))
    a = mbb_from_wealth(w, 5, 7, np.clip(st, 0, 34))
    st2 = st.copy()
    st2[st2 == 0] = -1
    st2[st2 >= 34] = 39
    b = mbb_from_wealth(w, 5, 7, st2)
    assert (st2 != np.clip(st, 0, 34)).any()
    assert b[0]["flags"] == 1 and a[0]["flags"] == 0 and np.array_equal(a[3], b[3]) and np.array_equal(a[1], b[1])


def test_reference_starts_follow_numpys_global_stream(sgmm, g10):
    """get_mbb_sharpe's draws: n_boot calls of randint(0, n - block_size + 1, size=num_blocks)."""
    from sgmm_amd.analytics import _reference_starts
    for k, w, bs, n_boot, st, ref, zero in mbb_cases(g10):
        np.random.seed(int(g10["mbb_seed"][k]))
        before = np.random.get_state()[1].copy()
        got = _reference_starts(w, bs, n_boot)
        if st is None:
            assert got is None and np.array_equal(np.random.get_state()[1], before)   # nothing drawn
        else:
            assert np.array_equal(got, st), k


def test_dw_mirror_matches_the_ratio(sgmm, g10):
    from sgmm_amd.analytics import dw_from_series
    worst = 0.0
    for f, rows, want in zip(g10["dw_frame"], g10["dw_rows"], g10["dw_value"]):
        e = g10["reward"][f, :rows]
        with np.errstate(all="ignore"):
            again = float(((e[1:] - e[:-1]) ** 2).sum() / (e * e).sum())   # the ratio, restated here
        got = dw_from_series(e)
        assert close(again, want, tol(want)) and close(got, again, tol(again)), (f, rows, got, again)
        if not np.isnan(again):
            worst = max(worst, abs(got - again))
        print(f"DW frame {f} rows {rows}: {got!r} vs {again!r}")
    print("worst |mirror - ratio|:", worst)
    assert np.isnan(dw_from_series([])) and dw_from_series([2.0]) == 0.0 and np.isnan(dw_from_series([0.0]))
    assert dw_from_series([1.0, -1.0]) == 2.0


def test_dm_mirror_matches_reference(sgmm, g10):
    from sgmm_amd.analytics import dm_from_series
    for k in range(len(g10["dm_crit"])):
        a, p1, p2, crit = dm_inputs(g10, k)
        o = dm_from_series(a, p1, p2, crit)
        stat, p = g10["dm_result"][k]
        ts, tp = dm_tols(stat, len(a))
        print(f"DM case {k} {crit}: stat {o['stat']!r} vs {stat!r} (|d| = {abs(o['stat'] - stat):.3g}, tol {ts:.3g}); "
              f"p {o['p_value']!r} vs {p!r} (|d| = {abs(o['p_value'] - p):.3g}, tol {tp:.3g})")
        assert abs(o["stat"] - stat) <= ts and abs(o["p_value"] - p) <= tp and o["n"] == 959
    assert abs(g10["dm_result"][0, 0] - 20.88) < 0.01 and g10["dm_result"][0, 1] == 0.0
    a, p1, _, _ = dm_inputs(g10, 0)
    assert dm_from_series(a, p1, None).tobytes() == dm_from_series(a, p1, np.zeros_like(a)).tobytes()
    # n < 2: NaN variance, statistic and p-value; NaN inputs propagate
    for n in (0, 1):
        o = dm_from_series(a[:n], p1[:n], None)
        assert np.isnan(o["var_d"]) and np.isnan(o["stat"]) and np.isnan(o["p_value"]) and o["n"] == n
    assert np.isnan(dm_from_series(a[:0], p1[:0])["mean_d"]) and not np.isnan(dm_from_series(a[:1], p1[:1])["mean_d"])
    b = a.copy()
    b[100] = np.nan
    o = dm_from_series(b, p1, None)
    assert np.isnan(o["stat"]) and np.isnan(o["p_value"]) and np.isnan(o["mean_d"])


def test_erfc_form_of_the_p_value(sgmm):
    """2 (1 - Phi(|x|)) with Phi(x) = erfc(-x / sqrt 2) / 2 against scipy's norm.cdf."""
    from scipy import stats
    x = np.linspace(0.0, 9.0, 4001)
    ours = np.array([2.0 * (1.0 - 0.5 * math.erfc((-v) / math.sqrt(2.0))) for v in x])
    assert np.abs(ours - 2 * (1 - stats.norm.cdf(x))).max() <= 4 * 2.0 ** -53


def test_struct_layouts_match_header(sgmm):
    from sgmm_amd import _lib
    from sgmm_amd.rollout import DM_DTYPE, MBB_DTYPE
    text = HEADER.read_text()
    for name, ct, dt in (("sgmm_dm_result", _lib.DMResult, DM_DTYPE), ("sgmm_mbb_result", _lib.MBBResult, MBB_DTYPE)):
        body, size = re.search(r"typedef struct %s \{(.*?)\} %s;\s*/\* (\d+) bytes \*/" % (name, name), text, re.S).groups()
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*\w+\s", "", decl.strip()).split(",") if f.strip()]
        assert fields == [f[0] for f in ct._fields_] == list(dt.names), name
        assert int(size) == ctypes.sizeof(ct) == dt.itemsize == 40
        assert [getattr(ct, f).offset for f in fields] == [dt.fields[f][1] for f in fields]
    assert _lib.DMResult.n.offset == 32 and _lib.MBBResult.n_returns.offset == 24 and _lib.MBBResult.flags.offset == 36
    assert "SGMM_MBB_CLAMPED = 1" in text and "SGMM_MBB_NOT_RESAMPLED = 2" in text


def test_argument_errors_need_no_gpu(sgmm):
    """Validation happens before any HIP call: bad arguments fail cleanly on a machine without a GPU."""
    from sgmm_amd import _lib
    L = _lib.load()
    v = ctypes.c_void_p(8)
    off = np.array([0, 5, 9], np.int64)
    bad = np.array([0, 5, 3], np.int64)

    def mbb(block_size=4, n_boot=10, o=off, starts=None, stride=0, starts_out=None, off_host=True):
        return L.sgmm_mbb_sharpe(v, v, o.ctypes.data if off_host else None, 2, block_size, n_boot, starts, stride, 1, v, v,
                                 starts_out, v, None)

    for kw, msg in ((dict(n_boot=0), b"n_boot"), (dict(n_boot=4097), b"n_boot"), (dict(block_size=0), b"block_size"),
                    (dict(o=bad), b"off decreases"), (dict(starts=v, stride=0), b"starts_stride"),
                    (dict(block_size=1, starts_out=v, stride=3), b"starts_stride=3 <"),
                    (dict(starts=v, stride=4, off_host=False), b"need off_host")):
        assert mbb(**kw) == -1 and msg in L.sgmm_last_error(), (kw, L.sgmm_last_error())
    assert L.sgmm_dm_test(v, v, None, v, off.ctypes.data, 2, 2, v, None) == -1 and b"crit" in L.sgmm_last_error()
    assert L.sgmm_dm_test(v, v, None, v, bad.ctypes.data, 2, 0, v, None) == -1 and b"off decreases" in L.sgmm_last_error()
    assert L.sgmm_dm_test(v, None, None, v, off.ctypes.data, 2, 0, v, None) == -1 and b"null" in L.sgmm_last_error()
    assert L.sgmm_durbin_watson(v, v, bad.ctypes.data, 2, v, None) == -1 and b"off decreases" in L.sgmm_last_error()
    assert L.sgmm_durbin_watson(v, None, None, 2, v, None) == -1 and b"null off" in L.sgmm_last_error()
    assert L.sgmm_durbin_watson(v, v, None, -1, v, None) == -1 and b"n_series" in L.sgmm_last_error()
    assert L.sgmm_trace_wealth(None, None, v, v, v, None) == -1 and b"null" in L.sgmm_last_error()
    # nothing to do is not an error, and needs no device either
    assert L.sgmm_durbin_watson(None, None, None, 0, None, None) == 0
    assert L.sgmm_mbb_sharpe(None, None, None, 0, 100, 500, None, 0, 0, None, None, None, None, None) == 0
