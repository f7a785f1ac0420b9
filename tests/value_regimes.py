"""Value regimes for the policy MLP and the env step: genomes whose float32
activations are subnormal, overflow, or turn into NaN inside the network, and
two plain models of the forward pass the oracle is checked against.  Nothing
here shares code with csrc/ or oracle/sgmm_oracle.c.

Genomes are N(0, 1) * a per-layer scale from a seeded default_rng, cast to
float32.  The cast is clipped to the largest finite float32: N(0, 1) * 3e38
passes it for |z| > 1.13, and every regime is meant to have finite weights
(the overflow has to happen inside the network).

  exact model   fmaf as an exact fractions.Fraction product-and-sum rounded once
                to float32 (round to nearest even, subnormals included); slow,
                for a few dozen states.
  fma32 model   the same chain vectorised over states: the float32 x float32
                product is exact in float64, the sum is rounded to odd in
                float64 (TwoSum gives the rounding error's sign) and then once
                to float32 -- 53 >= 2 * 24 + 2 bits make that a single
                rounding.  With flush=True every fma flushes subnormal inputs
                and results to zero: what a kernel built with denormal flushing
                would compute.

Both apply the port's relu: positive values pass, everything else -- NaN of
either sign included -- gives +0.
"""
import math
from fractions import Fraction

import numpy as np

F32_MAX = float(np.finfo(np.float32).max)
F32_TINY = float(np.finfo(np.float32).tiny)  # smallest normal
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

# name -> ((W1, b1), (W2, b2), (W3, b3)) multipliers on N(0, 1)
REGIMES = {
    "sub_h1": ((1e-39, 1e-39), (1e19, 1e-20), (2e19, 0.3)),     # subnormal layer-1 activations (the MFMA B operand)
    "sub_h2": ((1e-19, 1e-19), (1e-20, 1e-39), (1e38, 0.3)),    # subnormal layer-2 accumulator (the MFMA C operand)
    "sub_both": ((2e-39, 2e-39), (1.0, 1e-39), (1e38, 0.3)),    # both
    "sub_out": ((1e-13, 1e-13), (1e-13, 1e-26), (1e-13, 1e-39)),  # subnormal raw outputs (actions all 0)
    "large": ((30.0, 30.0), (30.0, 30.0), (30.0, 30.0)),        # finite offsets up to +-5e6
    "ovf_l1": ((3e38, 3e38), (1.0, 1.0), (1e-30, 1e-30)),       # +-inf after layer 1
    "ovf_l2": ((1e19, 1e19), (1e19, 1e19), (1.0, 1.0)),         # inf - inf inside the layer-2 chain, inf / NaN raws
    "ovf_l3": ((1e13, 1e13), (1e13, 1e13), (1e13, 1e13)),       # inf raws only: actions INT32_MIN / INT32_MAX
    "normal": ((0.4, 0.4), (0.4, 0.4), (0.4, 0.4)),             # control
}
SUB_REGIMES = ("sub_h1", "sub_h2", "sub_both")
HIDDEN = (8, 16, 32, 64)

# Two genome seeds per (regime, H).  For the sub_h* regimes each seed meets the
# sanity conditions of tests/test_value_domain.py (>= 16 distinct action values,
# >= 50 trading steps, the flushing model differs on >= 600 of 700 steps): many
# seeds give a genome that hardly trades, so these were searched for (seeds
# 0..3, sub_h1 at H = 64 up to 59).  ovf_l2 at H = 32: seeds whose raws hold
# both NaN and inf (at H = 64 every raw of every seed tried is NaN).
DEFAULT_SEEDS = (0, 1)
SEEDS = {
    ("sub_h1", 8): (2, 3), ("sub_h1", 16): (1, 3), ("sub_h1", 32): (0, 1), ("sub_h1", 64): (16, 18),
    ("sub_h2", 8): (0, 2), ("sub_h2", 64): (0, 2),
    ("sub_both", 32): (0, 2), ("sub_both", 64): (0, 2),
    ("ovf_l2", 32): (0, 2),
}

ADV_KINDS = ("sigma1", "x50", "tiny")  # tanh in its linear range / saturated / on subnormals
ADV_LEN = 1250  # adversary genome rows are TradingPolicy(32)-sized; the first 74 floats are used


def seeds(regime, H):
    return SEEDS.get((regime, H), DEFAULT_SEEDS)


def n_params(H):
    return H * H + 7 * H + 2


def _f32(v):
    return np.clip(v, -F32_MAX, F32_MAX).astype(np.float32)


def genome(regime, H, seed):
    """float32[H*H + 7H + 2] in parameters() order: W1[H,3] b1[H] W2[H,H] b2[H] W3[2,H] b3[2]."""
    (w1, b1), (w2, b2), (w3, b3) = REGIMES[regime]
    rng = np.random.default_rng([seed, H, sorted(REGIMES).index(regime)])
    parts = [(3 * H, w1), (H, b1), (H * H, w2), (H, b2), (2 * H, w3), (2, b3)]
    g = np.concatenate([rng.standard_normal(n) * s for n, s in parts])
    assert np.isfinite(_f32(g)).all()
    return _f32(g)


def adversary(kind, seed):
    """float32[1250] adversary genome row."""
    scale = {"sigma1": 1.0, "x50": 50.0, "tiny": 1e-39}[kind]
    rng = np.random.default_rng([seed, 74, ADV_KINDS.index(kind)])
    return _f32(rng.standard_normal(ADV_LEN) * scale)


def layers(g, H):
    g = np.asarray(g, np.float32)
    o = np.cumsum([0, 3 * H, H, H * H, H, 2 * H, 2])
    return (g[o[0]:o[1]].reshape(H, 3), g[o[1]:o[2]], g[o[2]:o[3]].reshape(H, H), g[o[3]:o[4]],
            g[o[4]:o[5]].reshape(2, H), g[o[5]:o[6]])


# ------------------------------------------------------------------ exact model
def round_f32(x):
    """A nonzero Fraction -> the nearest float32 (ties to even, gradual
    underflow, overflow to inf), as a Python float."""
    sign = -1.0 if x < 0 else 1.0
    n, d = abs(x.numerator), x.denominator
    e = n.bit_length() - d.bit_length()
    if (n << -e if e < 0 else n) < (d << e if e > 0 else d):
        e -= 1                      # 2^e <= |x| < 2^(e+1)
    q = max(e, -126) - 23           # exponent of the last place
    num, den = (n, d << q) if q >= 0 else (n << -q, d)
    m, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and m & 1):
        m += 1
    if m.bit_length() + q > 128:
        return sign * math.inf
    return sign * math.ldexp(m, q)


def fma_exact(a, b, c):
    """fmaf(a, b, c) on Python floats holding float32 values."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        # the product of two float32 values is exact (and finite) in float64,
        # so float64 gives the IEEE class of the result: inf, -inf or NaN
        with np.errstate(invalid="ignore", over="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    p = Fraction(a) * Fraction(b)
    s = p + Fraction(c)
    if s != 0:
        return round_f32(s)
    if p == 0 and c == 0:           # (+-0) + (+-0)
        ps = math.copysign(1.0, a) * math.copysign(1.0, b)
        return c if ps == math.copysign(1.0, c) else 0.0
    return 0.0                      # exact cancellation: +0 in round-to-nearest


def relu_port(a):
    return a if a > 0 else 0.0      # NaN > 0 is False: a NaN contributes +0


def forward_exact(g, H, x):
    """The canonical chains (bias first, k ascending) in exact arithmetic."""
    W1, b1, W2, b2, W3, b3 = (a.tolist() for a in layers(g, H))  # float32 -> Python float: exact
    x = [float(np.float32(v)) for v in x]
    h1 = []
    for j in range(H):
        a = b1[j]
        for k in range(3):
            a = fma_exact(W1[j][k], x[k], a)
        h1.append(relu_port(a))
    h2 = []
    for j in range(H):
        a = b2[j]
        for k in range(H):
            a = fma_exact(W2[j][k], h1[k], a)
        h2.append(relu_port(a))
    out = []
    for o in range(2):
        a = b3[o]
        for j in range(H):
            a = fma_exact(W3[o][j], h2[j], a)
        out.append(a)
    return np.array(out, np.float32)


def action_exact(raw, scale=5.0):
    """act = int(rint(float32(raw * scale))): saturating at int32, NaN -> INT32_MIN."""
    raw = float(np.float32(raw))
    if math.isnan(raw):
        return INT32_MIN
    if math.isinf(raw):
        return INT32_MAX if raw > 0 else INT32_MIN
    v = Fraction(raw) * Fraction(float(np.float32(scale)))
    if v == 0:
        return 0
    v = round_f32(v)
    if math.isinf(v):
        return INT32_MAX if v > 0 else INT32_MIN
    return int(min(max(round(Fraction(v)), INT32_MIN), INT32_MAX))  # round(): half to even


# ------------------------------------------------------------------ fma32 model
def _flush(v):
    return np.where(np.abs(v) < np.float32(F32_TINY), np.copysign(np.float32(0), v), v)


def fma32(a, b, c, flush=False):
    """Element-wise fmaf on float32 arrays, correctly rounded (see the module docstring)."""
    a, b, c = (np.asarray(v, np.float32) for v in (a, b, c))
    if flush:
        a, b, c = _flush(a), _flush(b), _flush(c)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)   # exact
        cd = c.astype(np.float64)
        s = p + cd
        bb = s - p
        err = (p - (s - bb)) + (cd - bb)                  # TwoSum: p + cd = s + err exactly
        fin = np.isfinite(s) & np.isfinite(err)
        even = (s.view(np.int64) & 1) == 0
        up = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        s = np.where(fin & (err != 0) & even, up, s)      # round to odd
        r = s.astype(np.float32)
    return _flush(r) if flush else r


def forward32(g, H, states, flush=False, hidden=False):
    """Raw outputs float32[n, 2] of states float32[n, 3]; hidden=True also returns the
    layer-2 pre-activations float32[n, H]."""
    W1, b1, W2, b2, W3, b3 = layers(g, H)
    x = np.asarray(states, np.float32)
    n = len(x)

    def relu(a):
        return np.where(a > 0, a, np.float32(0)).astype(np.float32)

    a = np.broadcast_to(b1, (n, H))
    for k in range(3):
        a = fma32(W1[None, :, k], x[:, k:k + 1], a, flush)
    h1 = relu(a)
    a = np.broadcast_to(b2, (n, H))
    for k in range(H):
        a = fma32(W2[None, :, k], h1[:, k:k + 1], a, flush)
    pre2, h2 = a, relu(a)
    a = np.broadcast_to(b3, (n, 2))
    for j in range(H):
        a = fma32(W3[None, :, j], h2[:, j:j + 1], a, flush)
    return (a, pre2) if hidden else a


def actions32(raw, scale=5.0, flush=False):
    """int64[...] actions of float32 raws: rint(raw * scale), saturating, NaN -> INT32_MIN."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(raw, np.float32) * np.float32(scale)
        if flush:
            v = _flush(v)
        r = np.rint(v).astype(np.float64)
    out = np.clip(np.nan_to_num(r, nan=float(INT32_MIN)), INT32_MIN, INT32_MAX)
    return out.astype(np.int64)


def same_raw(a, b):
    """Bit equality of float32 arrays, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------ the shared episode data
T_LONG, T_SHORT = 700, 65
PHI, TICK = 0.0005, 0.001


def market(nan_bounds=True):
    """The 700-tick bundle every value-domain test runs on, with its train
    stats and normalised signals."""
    import sgmm_pkg
    sgmm_pkg.load()
    from sgmm_amd import synthetic
    b =synthetic.bundle_510300(T_LONG, seed=17, nan_frac=0.02 if nan_bounds else 0.0)
    st = synthetic.train_stats(b)
    a = ((np.asarray(b[0]) - st["s1_m"]) / st["s1_s"]).astype(np.float32)
    c = ((np.asarray(b[1]) - st["s2_m"]) / st["s2_s"]).astype(np.float32)
    return b, st, a, c
