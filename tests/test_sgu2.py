"""SGU2 inference against the reference's SGU2.predict on
its own checkpoints (tests/golden/g8_sgu2.npz, gen_golden_sgu2.py).

Tolerance: the reference evaluates the LSTM in float32 on the CPU (oneDNN /
BLAS summation order, libm transcendentals); the kernel in float32 on the GPU
(packed FMAs over even/odd columns, hardware exp2/rcp for sigmoid and tanh).
Both are compared with |out - want| <= ATOL + RTOL * |want| (ATOL = RTOL =
2e-6 on outputs of magnitude <= ~3; measured: reference vs float64 3.3e-7,
kernel vs reference 6.0e-7).  The scaler (float32 elementwise) is bit-exact.

Beyond the shipped H = 10 checkpoints, every instantiation of the kernel
(H = 10, 16, 32) runs against the float64 oracle with random weights of scale
gain / sqrt(H) (gain 4 saturates the gates), T in {1, 2, 10, 37} and four input
regimes up to +-FLT_MAX and +-inf; the oracle at H = 16 / 32 is itself pinned
to torch's float32 CPU LSTM.  Worst |kernel - oracle| / (1 + |oracle|) measured
on an MI355X over those cases (1 000 windows per regime, |oracle| <= 3.3):
H = 10: 2.3e-7, H = 16: 4.7e-7, H = 32: 4.1e-7 -- a quarter of the tolerance."""
import numpy as np
import pytest
import torch

import sgu2_oracle as so
from conftest import has_gpu

ATOL = RTOL = 2e-6
gpu = pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")


def close(a, want):
    a, want = np.asarray(a, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    return a.shape == want.shape and bool(np.all(np.abs(a - want) <= ATOL + RTOL * np.abs(want)))


@pytest.fixture(scope="module")
def g8(golden):
    return golden("g8_sgu2.npz")


def test_oracle_matches_reference(g8):
    xs = so.scale(g8["X"], g8["mean"], g8["std"])
    assert np.array_equal(xs, g8["X_scaled_f32"])
    for k in range(3):
        assert close(so.forward(g8[f"w{k}"], xs), g8[f"y{k}"]), k
        assert close(so.forward(g8[f"w{k}"], g8["X"]), g8[f"y{k}_raw"]), k


def test_scaler_and_checkpoint_layout(sgmm, g8):
    from sgmm_amd.gate_units import SGU2, StandardScaler3D
    sc = StandardScaler3D()
    sc.fit(g8["X"])
    assert sc.mean.dtype == np.float32 and np.array_equal(sc.mean.reshape(-1), g8["mean"])
    assert np.array_equal(sc.std.reshape(-1), g8["std"])
    assert np.array_equal(sc.transform(g8["X"]), g8["X_scaled_f32"])
    m = SGU2(input_size=1, hidden_size=10)
    w = g8["w0"]
    parts = so.unpack(w)
    sd = {k: torch.from_numpy(np.asarray(p, np.float32)) for k, p in zip(
        ("lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "fc.weight", "fc.bias"), parts)}
    m.model.load_state_dict(sd)
    assert np.array_equal(m.model.flat_weights().numpy(), w)


def test_argument_errors_need_no_gpu(sgmm):
    import ctypes
    from sgmm_amd import _lib
    L = _lib.load()
    p = ctypes.c_void_p(8)
    assert L.sgmm_sgu2_forward(p, 12, p, 4, 10, None, None, p, None) == -1
    assert b"hidden" in L.sgmm_last_error()
    assert L.sgmm_sgu2_forward(p, 10, p, 4, 10, p, None, p, None) == -1
    assert L.sgmm_sgu2_forward(None, 10, p, 4, 10, None, None, p, None) == -1


@pytest.mark.parametrize("hidden", [0, 8, 11, 64])
def test_unsupported_hidden_is_an_error(sgmm, hidden):
    import ctypes
    from sgmm_amd import _lib
    L = _lib.load()
    p = ctypes.c_void_p(8)
    assert L.sgmm_sgu2_forward(p, hidden, p, 4, 10, None, None, p, None) == -1
    assert b"hidden" in L.sgmm_last_error()


# ---- every instantiation (H = 10, 16, 32) against the float64 oracle ----

FLT_MAX = float(np.finfo(np.float32).max)
HIDDEN, STEPS, GAINS = (10, 16, 32), (1, 2, 10, 37), (1, 4)
EXTREME = np.array([3.4e5, -3.4e5, FLT_MAX, -FLT_MAX, np.inf, -np.inf, 0.0, -0.0, 1e-30, 1e-40], np.float32)


def rand_weights(hidden, gain, seed=0):
    """Flat weights of scale gain / sqrt(H); gain 4 drives the gates into saturation."""
    H = hidden
    rng = np.random.default_rng([seed, H, gain])
    return (rng.uniform(-1, 1, 4 * H + 4 * H * H + 8 * H + H + 1) / np.sqrt(H) * gain).astype(np.float32)


def regimes(rng, n, T):
    """The input regimes the bundle can produce: returns, scaled windows, heavy
    tails, and what nan_to_num / a floored bar / a constant-window scaler emit."""
    ext = rng.standard_normal((n, T, 1)).astype(np.float32)
    hit = rng.random((n, T, 1)) < 0.15
    ext[hit] = rng.choice(EXTREME, int(hit.sum()))
    return {"returns": (rng.standard_t(4, (n, T, 1)) * 3e-4).astype(np.float32),
            "normal": rng.standard_normal((n, T, 1)).astype(np.float32),
            "heavy": (rng.standard_t(3, (n, T, 1)) * 30).astype(np.float32),
            "extreme": ext}


def oracle_forward(w, X, hidden):
    with np.errstate(over="ignore"):  # exp(+large) = inf is the saturated gate
        return so.forward(w, X, hidden=hidden).reshape(-1)


def worst(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    return float(np.max(np.abs(got - want) / (1.0 + np.abs(want))))


def torch_model(w, hidden):
    from sgmm_amd.gate_units import SGU2
    m = SGU2(1, hidden)
    sd = {n: torch.from_numpy(np.asarray(p, np.float32)) for n, p in zip(
        ("lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "fc.weight", "fc.bias"),
        so.unpack(w, hidden))}
    m.model.load_state_dict(sd)
    m.model.eval()
    return m


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("hidden", [16, 32])
def test_oracle_matches_torch_lstm_beyond_h10(sgmm, hidden, T, gain):
    """The checker itself at H = 16 / 32: torch's float32 CPU nn.LSTM + Linear,
    loaded from the same flat weights, in every input regime."""
    w = rand_weights(hidden, gain)
    model = torch_model(w, hidden).model
    for name, X in regimes(np.random.default_rng([1, hidden, T, gain]), 250, T).items():
        want = oracle_forward(w, X, hidden)
        assert np.all(np.isfinite(want)), name
        with torch.no_grad():
            h, _ = model.lstm(torch.from_numpy(X))
            got = model.fc(h[:, -1, :]).numpy().reshape(-1)
        assert close(got, want), (name, worst(got, want))


def _model(g8, k):
    from sgmm_amd.gate_units import SGU2
    m = SGU2(1, 10)
    sd = {n: torch.from_numpy(np.asarray(p, np.float32)) for n, p in zip(
        ("lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "fc.weight", "fc.bias"),
        so.unpack(g8[f"w{k}"]))}
    m.model.load_state_dict(sd)
    return m


@pytest.mark.gpu
@gpu
def test_predict_matches_reference(sgmm, g8):
    from sgmm_amd.gate_units import StandardScaler3D
    sc = StandardScaler3D()
    sc.fit(g8["X"])
    for k in range(3):
        m = _model(g8, k)
        assert close(m.predict(g8["X"]), g8[f"y{k}_raw"]), k
        assert close(m.predict(g8["X_scaled_f32"]), g8[f"y{k}"]), k
        X = torch.from_numpy(g8["X"]).cuda()
        assert close(m.predict_device(X, sc).cpu().numpy(), g8[f"y{k}"]), k   # scaler in the kernel
        assert m.predict(g8["X"]).shape == (len(g8["X"]), 1)


@pytest.mark.gpu
@gpu
def test_predict_many_windows_matches_oracle(sgmm, g8):
    rng = np.random.default_rng(3)
    X = (rng.standard_t(4, size=(200_003, 10, 1)) * 3e-4).astype(np.float32)
    X[::7] = 0.0
    for k in (0, 1):
        m = _model(g8, k)
        got = m.predict_device(torch.from_numpy(X).cuda()).cpu().numpy()
        assert close(got, so.forward(g8[f"w{k}"], X)), k
    empty = _model(g8, 0).predict_device(torch.zeros((0, 10), dtype=torch.float32, device="cuda"))
    assert empty.numel() == 0


@pytest.mark.gpu
@gpu
def test_bundle_with_device_sgu2(sgmm, golden, tmp_path):
    """load_signals_bundle with this package's SGU2 + a float32 scaler runs SGU2
    on the device windows of all days in one launch; equal to the host path
    (the same kernel fed the host windows) and within tolerance of the oracle."""
    import pandas as pd
    from sgmm_amd.bundle import load_signals_bundle
    from sgmm_amd.gate_units import StandardScaler3D
    g6, g8 = golden("g6_bundle.npz"), golden("g8_sgu2.npz")
    dates = [str(d) for d in g6["dates"]]
    for k, d in enumerate(dates):
        for kind in ("snap", "tick"):
            p = tmp_path / "data" / "SYN" / kind
            p.mkdir(parents=True, exist_ok=True)
            pd.DataFrame({c[len(f"d{k}_{kind}_"):]: g6[c] for c in g6 if c.startswith(f"d{k}_{kind}_")}) \
                .to_parquet(p / f"{d}.parquet")
    sc = StandardScaler3D()
    sc.fit(np.concatenate([g6[f"d{k}_sgu2_X"] for k in range(len(dates)) if g6[f"d{k}_sgu2_X"].ndim == 3]))
    m2 = _model(g8, 0)

    class HostM2:  # any non-package model: the reference's host path
        def predict(self, X):
            return m2.predict(X)

    class M1:
        def predict(self, X):
            return np.asarray(X.iloc[:, 0].values, dtype=np.float32)

    def feats():
        it = iter([g6[f"d{k}_sgu1_f0"] for k in range(len(dates))])
        return lambda bars: (lambda v: pd.DataFrame({"f0": v, "label": np.zeros(len(v))}))(next(it))

    fused = load_signals_bundle("SYN", dates, M1(), m2, sc, sgu1_features=feats(), data_root=str(tmp_path))
    host = load_signals_bundle("SYN", dates, M1(), HostM2(), sc, sgu1_features=feats(), data_root=str(tmp_path))
    for a, b in zip(fused, host):
        assert np.array_equal(a, b, equal_nan=True)
    assert fused[1].dtype == np.float32
    # s2 against the oracle on the reference's windows (aligned tails, last step dropped)
    want = []
    for k in range(len(dates)):
        X = g6[f"d{k}_sgu2_X"]
        if X.ndim != 3:
            continue
        y = so.forward(g8["w0"], so.scale(X, sc.mean, sc.std)).reshape(-1)
        n = min(len(g6[f"d{k}_sgu1_f0"]), len(y))
        want.append(y[-n:][:-1])
    assert close(fused[1], np.concatenate(want))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


@pytest.mark.gpu
@gpu
@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("hidden", HIDDEN)
def test_every_instantiation_matches_oracle(sgmm, hidden, T, gain):
    """k_sgu2<10>, <16> and <32> over 1 000 windows of every input regime."""
    w = rand_weights(hidden, gain)
    m = torch_model(w, hidden)
    for name, X in regimes(np.random.default_rng([2, hidden, T, gain]), 1000, T).items():
        want = oracle_forward(w, X, hidden)
        assert np.all(np.isfinite(want)), name  # no row is left out of the comparison
        got = m.predict_device(torch.from_numpy(X).cuda()).cpu().numpy()
        print(f"sgu2 H={hidden} T={T} gain={gain} {name}: worst |kernel - oracle| / (1 + |oracle|) = "
              f"{worst(got, want):.3e}, max |oracle| = {np.abs(want).max():.3f}")
        assert close(got, want), (name, worst(got, want))


SENTINEL = np.float32(-1234.5678)


@pytest.mark.gpu
@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("hidden", [16, 32])
def test_launch_edges_write_n_outputs_only(sgmm, hidden, n):
    """Around the 256-thread block: the first n outputs match the oracle and
    the 64 elements behind them keep the sentinel bit for bit."""
    w = rand_weights(hidden, 1)
    X = np.random.default_rng([3, hidden, n]).standard_normal((n, 10, 1)).astype(np.float32)
    out = torch.full((n + 64,), float(SENTINEL), dtype=torch.float32, device="cuda")
    got = torch_model(w, hidden).predict_device(torch.from_numpy(X).cuda(), out=out)
    assert got.shape == (n,)
    host = out.cpu().numpy()
    assert close(host[:n], oracle_forward(w, X, hidden))
    assert np.array_equal(bits(host[n:]), bits(np.full(64, SENTINEL)))


@pytest.mark.gpu
@gpu
@pytest.mark.parametrize("hidden", [16, 32])
def test_tiled_window_gives_identical_bits(sgmm, hidden):
    """One window at all 513 positions (three blocks, the last one thread wide)."""
    w = rand_weights(hidden, 4)
    X = np.tile(np.random.default_rng([4, hidden]).standard_normal((1, 10, 1)).astype(np.float32), (513, 1, 1))
    got = torch_model(w, hidden).predict_device(torch.from_numpy(X).cuda()).cpu().numpy()
    assert got.shape == (513,) and len(np.unique(bits(got))) == 1
    assert close(got, oracle_forward(w, X, hidden))


@pytest.mark.gpu
@gpu
@pytest.mark.parametrize("hidden", HIDDEN)
def test_nan_stays_in_its_window(sgmm, hidden):
    w = rand_weights(hidden, 1)
    m = torch_model(w, hidden)
    X = np.random.default_rng([5, hidden]).standard_normal((300, 10, 1)).astype(np.float32)
    clean = m.predict_device(torch.from_numpy(X).cuda()).cpu().numpy()
    i = 257
    X[i, 4, 0] = np.nan
    got = m.predict_device(torch.from_numpy(X).cuda()).cpu().numpy()
    assert np.isnan(got[i]) and np.all(np.isfinite(clean))
    keep = np.arange(300) != i
    assert np.array_equal(bits(got[keep]), bits(clean[keep]))


def scalers():
    """(name, mean, std, windows): an ordinary fit; the fit on constant windows
    (std = 0 + 1e-9), whose quotients of nan_to_num'ed windows overflow to
    +-inf; a fit on huge symmetric windows, whose quotients are subnormal."""
    from sgmm_amd.gate_units import StandardScaler3D
    rng = np.random.default_rng(6)
    X = (rng.standard_t(4, (500, 10, 1)) * 3e-4).astype(np.float32)
    fit = StandardScaler3D()
    fit.fit(X)
    const = StandardScaler3D()
    const.fit(np.zeros((4, 10, 1), np.float32))
    assert const.mean.dtype == np.float32 and const.mean.item() == 0.0 and const.std.item() == np.float32(1e-9)
    Xc = X.copy()
    hit = rng.random(Xc.shape) < 0.15
    Xc[hit] = rng.choice(np.array([FLT_MAX, -FLT_MAX, 3.4e5, -3.4e5, 0.0, 1e30, -1e30], np.float32), int(hit.sum()))
    huge = StandardScaler3D()
    huge.fit(np.array([[[-1e10], [1e10]]], np.float32))
    assert huge.mean.item() == 0.0
    Xs = (rng.standard_normal((500, 10, 1)) * 1e-30).astype(np.float32)
    return [("fit", fit, X), ("constant", const, Xc), ("subnormal", huge, Xs)]


@pytest.mark.gpu
@gpu
@pytest.mark.parametrize("hidden", HIDDEN)
def test_fused_scaler_is_bit_exact(sgmm, hidden):
    """predict_device(X, scaler) against the same kernel on the float32
    (X - mean) / std of the host: only the division differs, so the bits agree."""
    w = rand_weights(hidden, 1)
    m = torch_model(w, hidden)
    for name, sc, X in scalers():
        with np.errstate(over="ignore"):
            xs = so.scale(X, sc.mean, sc.std)
        if name == "constant":
            assert np.isinf(xs).any()
        if name == "subnormal":
            tiny = np.abs(xs[xs != 0])
            assert tiny.size and np.all(tiny < np.finfo(np.float32).tiny)
        want = oracle_forward(w, xs, hidden)
        assert np.all(np.isfinite(want)), name
        fused = m.predict_device(torch.from_numpy(X).cuda(), sc).cpu().numpy()
        plain = m.predict_device(torch.from_numpy(xs).cuda()).cpu().numpy()
        assert np.array_equal(bits(fused), bits(plain)), name
        assert close(fused, want) and close(plain, want), name
