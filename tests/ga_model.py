"""An independent model of the device GA boundary: the ask's random stream
(Philox4x32-10 + Box-Muller with the counter layout of include/sgmm.h) and the
tell / validation / sigma bookkeeping of one generation.  Plain numpy, written
from the published Philox algorithm and from the reference's
Env/drl_engine.py:119-171 and models/model.py:65-76 -- nothing here shares
code with csrc/.  The only things taken from the package are the two record
dtypes (imported when first needed)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # Weyl key increments
MASK = 0xFFFFFFFF


def philox4x32_10(counter4, key2):
    """Philox4x32 with 10 rounds (Salmon et al., SC'11; Random123).  counter4:
    four 32-bit words (Python ints or equal-shaped integer arrays), key2: two
    32-bit ints.  Returns the four output words as uint64 arrays (or ints when
    every input was a Python int)."""
    scalar = all(isinstance(c, (int, np.integer)) for c in counter4)
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & np.uint64(MASK) for c in counter4)
    k0, k1 = int(key2[0]) & MASK, int(key2[1]) & MASK
    m32 = np.uint64(MASK)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0  # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32,
                          (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32)
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    if scalar:
        return tuple(int(c) for c in (c0, c1, c2, c3))
    return c0, c1, c2, c3


def _u_open_closed(r):
    """Raw word -> uniform in (0, 1], float32 arithmetic: min((f32(r) + 1) 2^-32, 1)."""
    f = np.asarray(r, np.uint64).astype(np.float32)
    u = (f + np.float32(1.0)) * np.float32(2.0 ** -32)
    return np.minimum(u, np.float32(1.0))


def _u_closed_open(r):
    """Raw word -> uniform in [0, 1] (float32): f32(r) 2^-32."""
    return np.asarray(r, np.uint64).astype(np.float32) * np.float32(2.0 ** -32)


def _cos_sin_2pi(u):
    """cos(2 pi u), sin(2 pi u) in float64 for u in [0, 1].  x = 2u is reduced
    to the nearest multiple of 1/2 exactly (x comes from a float32, so x - n/2
    has no rounding), which keeps the relative error of the result at a few
    float64 ulps next to the zeros of either function and makes the zeros
    exact -- a plain cos(2 pi u) is off by 1e-16 absolute there, which is an
    unbounded relative error."""
    x = 2.0 * np.asarray(u, np.float64)
    n = np.rint(2.0 * x)
    t = x - n / 2.0                      # |t| <= 1/4, exact
    c, s = np.cos(np.pi * t), np.sin(np.pi * t)
    q = n.astype(np.int64) & 3
    cos = np.select([q == 0, q == 1, q == 2], [c, -s, -c], s)
    sin = np.select([q == 0, q == 1, q == 2], [s, c, -s], -c)
    return cos, sin


def box_muller(r0, r1, r2, r3):
    """The four N(0, 1) values of one Philox output (float64 after the float32
    uniforms): z0 = m cos 2 pi u1, z1 = m sin 2 pi u1 with m = sqrt(-2 ln u0),
    and z2, z3 likewise from (u2, u3)."""
    out = []
    for ra, rb in ((r0, r1), (r2, r3)):
        ua = _u_open_closed(ra).astype(np.float64)
        m = np.sqrt(-2.0 * np.log(ua))
        c, s = _cos_sin_2pi(_u_closed_open(rb))
        out += [m * c, m * s]
    return tuple(out)


def normal4(seed, stream, gen, indiv, block):
    """z[4 block .. 4 block + 3] of individual `indiv` in generation `gen` of
    stream `stream` (0: market maker, 1: adversary) under the 64-bit key `seed`:
    counter (block, indiv, gen, stream), key (seed low word, seed high word)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = philox4x32_10((block, indiv, gen, stream), (seed & MASK, seed >> 32))
    return box_muller(*r)


def ask_z(n_params, seed, stream, gen, i0, n):
    """float64 z[n, n_params]: parameter k of individual i0 + i takes output
    k % 4 of block k // 4."""
    nk4 = (n_params + 3) // 4
    blk, ind = np.meshgrid(np.arange(nk4, dtype=np.uint64), np.arange(i0, i0 + n, dtype=np.uint64))
    z = normal4(seed, np.full_like(blk, stream), np.full_like(blk, int(gen) & MASK), ind, blk)
    return np.stack(z, axis=-1).reshape(n, 4 * nk4)[:, :n_params]


def ask_rows(master, sigma, seed, stream, gen, i0, n):
    """float64 reference of NeuroEvolution.ask: master + sigma z, rows
    i0 .. i0 + n - 1 (master = 0, sigma = 1: z itself)."""
    master = np.asarray(master, np.float64)
    return master[None, :] + float(sigma) * ask_z(len(master), seed, stream, gen, i0, n)


# ------------------------------------------------------------------ the boundary
def _dtypes():
    from sgmm_amd.drl_engine import HIST_DTYPE, STATE_DTYPE
    return STATE_DTYPE, HIST_DTYPE


def new_state(sigma=0.05, patience=15, decay=0.5, sigma_adv=None, gen=0, best_val=-np.inf, no_improve=0):
    """A GA state record as sgmm_ga_state_init leaves it (fields overridable)."""
    st = np.zeros((), _dtypes()[0])
    st["sigma_mm"], st["sigma_adv"] = sigma, sigma if sigma_adv is None else sigma_adv
    st["best_val"], st["patience"], st["decay"] = best_val, patience, decay
    st["best_idx"] = st["adv_best_idx"] = -1
    st["gen"], st["no_improve"] = gen, no_improve
    return st


class Boundary:
    """What one boundary leaves behind: the new state record, the history row
    of the generation it closed, the two tell indices (None for a
    validation-only boundary) and whether the checkpoint slot is overwritten."""

    def __init__(self, state, row, best, abest, checkpoint):
        self.state, self.row, self.best, self.abest, self.checkpoint = state, row, best, abest, checkpoint


def _new_row(row):
    return np.zeros((), _dtypes()[1]) if row is None else np.array(row, copy=True)


def tell(state, f, tr, row=None):
    """NeuroEvolution.tell of both evolvers (model.py:73-76, drl_engine.py:119-129):
    best = np.argmax(f), adversary best = np.argmax(-f); the best training
    record goes into the state and the history row.  gen does not advance."""
    f = np.asarray(f, np.float64)
    st, row = np.array(state, copy=True), _new_row(row)
    best, abest = int(np.argmax(f)), int(np.argmax(-f))
    st["best_idx"], st["adv_best_idx"], st["last_train_f"] = best, abest, f[best]
    row["train_f"], row["train_trades"], row["best_idx"] = f[best], int(np.asarray(tr)[best]), best
    return Boundary(st, row, best, abest, False)


def val_update(state, v, vtr, row=None):
    """drl_engine.py:143-167 for the validation record (v, vtr) of the new
    master: strictly-greater improvement (a NaN never improves), the
    no-improvement counter, sigma decay of both evolvers after `patience`
    generations, the history row's validation half, gen + 1."""
    st, row = np.array(state, copy=True), _new_row(row)
    v = np.float64(v)
    improved = bool(v > st["best_val"])
    if improved:
        st["best_val"], st["no_improve"] = v, 0
    else:
        st["no_improve"] += 1
    decayed = bool(st["no_improve"] >= st["patience"])
    if decayed:
        st["sigma_mm"] = st["sigma_mm"] * st["decay"]
        st["sigma_adv"] = st["sigma_adv"] * st["decay"]
        st["no_improve"] = 0
    st["improved"], st["decayed"], st["last_val_f"] = int(improved), int(decayed), v
    st["gen"] += 1
    row["val_f"], row["val_trades"], row["sigma_after"] = v, int(vtr), st["sigma_mm"]
    row["flags"] = int(improved) | (int(decayed) << 1)
    return Boundary(st, row, None, None, improved)


def boundary(state, f, tr, vf, vtr):
    """One whole generation boundary with the validation record of every
    individual at hand (vf, vtr arrays: the best individual's entry is used)."""
    t = tell(state, f, tr)
    v = val_update(t.state, np.asarray(vf, np.float64)[t.best], np.asarray(vtr)[t.best], t.row)
    return Boundary(v.state, v.row, t.best, t.abest, v.checkpoint)


def same_bits(a, b):
    """Record / array equality on the bytes (NaN payloads and zero signs count)."""
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()
