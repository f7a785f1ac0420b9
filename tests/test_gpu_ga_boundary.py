"""GPU tests of the generation boundary -- the ask, every tell implementation,
the validation and sigma bookkeeping -- against the independent model in
tests/ga_model.py, on inputs that real rollouts essentially never produce:
exact ties, ties whose later index sits in a lower lane, NaN next to +inf,
all-equal populations, neighbours one ulp apart.

(a) sgmm_ga_ask against the Philox / Box-Muller reference;
(b) the tell through the direct entry points (sgmm_ga_tell, sgmm_ga_step,
    contiguous and sharded, sgmm_ga_step_multi, sgmm_ga_tell_multi), and the
    validation bookkeeping alone (sgmm_ga_val_update);
(c) the same vectors through the tails that run inside the rollout launches,
    injected as idle penalties: an episode whose buy_max / sell_min are NaN never
    fills, so its fitness is exactly 0.0 - params[param[e]].idle_penalty.
tests/test_plan.py pins the launch plan of every (shape, knobs) of (c)."""
import ctypes

import numpy as np
import pytest
import torch

import ga_model as gm
from conftest import has_gpu

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

DEV = torch.device("cuda:0")
H = 16
G_MM, G_ADV = H * H + 7 * H + 2, 1250
NAN, INF = float("nan"), float("inf")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _state_dev(recs):
    """GA state records written by hand through STATE_DTYPE -> device bytes [K, 80]."""
    recs = np.atleast_1d(np.asarray(recs))
    return _dev(recs.view(np.uint8).reshape(len(recs), -1).copy())


def _state_host(t):
    from sgmm_amd.drl_engine import STATE_DTYPE
    return t.cpu().numpy().reshape(-1).view(STATE_DTYPE).copy()


def _hist_host(t):
    from sgmm_amd.drl_engine import HIST_DTYPE
    return t.cpu().numpy().reshape(-1).view(HIST_DTYPE).copy()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """float32 tensors equal bit for bit"""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _ask(L, master, st, sid, seed, i0, n):
    from sgmm_amd import _lib
    out = torch.empty((n, master.numel()), dtype=torch.float32, device=DEV)
    _lib.check(L.sgmm_ga_ask(_lib.ptr(master), master.numel(), _lib.ptr(st), sid, seed, i0, n, _lib.ptr(out),
                             master.numel(), _lib.stream_ptr()), "sgmm_ga_ask")
    return out


# ------------------------------------------------------------------ (a) the ask
ASK_SIZES = [1, 2, 3, 4, 5, 7, 74, 122, 370, 1250, 4546]
ASK_GENS = [0, 1, 7, 2 ** 31 - 1]
ASK_SEEDS = [0, 77, 0x0123456789ABCDEF, 5, 5 + 2 ** 32]
ASK_SHARDS = [(i0, n) for i0 in (0, 40, 2_000_000_000) for n in (1, 64, 65)]
# float32 ulps of the reference value.  The device evaluates m = sqrtf(-2 logf(u0))
# and sincospif(2 u1) in float32; the OpenCL full-profile limits the ROCm device
# library documents are logf <= 3 ulp, sqrtf <= 3, sincospif <= 4.  The log's error
# halves through the square root (1.5), the product adds 1/2, and a result that
# crosses a binade is measured in ulps half as large: 2 (1.5 + 3 + 4 + 0.5).
ASK_ULP_BOUND = 18.0
CANARY = 0x5EED1234


def _ask_combos():
    """Every gen x seed x stream; the (i0, n) shards go round, each used 4 times or more."""
    j = 0
    for gen in ASK_GENS:
        for seed in ASK_SEEDS:
            for sid in (0, 1):
                yield (gen, seed, sid) + ASK_SHARDS[j % len(ASK_SHARDS)]
                j += 1


def _ask_padded(L, master, st, sid, seed, i0, n, pad=3):
    """sgmm_ga_ask into rows of n_params + pad with canaries in the padding and in
    a row after the last; returns the n x n_params values after checking them."""
    from sgmm_amd import _lib
    G = master.numel()
    buf = torch.full((n + 1, G + pad), CANARY, dtype=torch.int32, device=DEV)
    _lib.check(L.sgmm_ga_ask(_lib.ptr(master), G, _lib.ptr(st), sid, seed, i0, n, _lib.ptr(buf), G + pad,
                             _lib.stream_ptr()), "sgmm_ga_ask")
    assert bool((buf[:n, G:] == CANARY).all()) and bool((buf[n] == CANARY).all()), "canary overwritten"
    return buf[:n, :G].contiguous().view(torch.float32)


def _ulp_err(dev32, ref):
    dev = dev32.astype(np.float64)
    zero = ref == 0.0
    assert np.all(dev[zero] == 0.0), "reference 0 but device != 0"
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return float((np.abs(dev - ref)[~zero] / ulp[~zero]).max(initial=0.0))


@pytest.mark.parametrize("G", ASK_SIZES)
def test_ask_matches_reference_stream(sgmm, G):
    """master = 0, sigma = 1: the output is z itself, within ASK_ULP_BOUND float32
    ulps of the float64 reference; any counter-layout, key, constant or
    sine / cosine mistake is wrong by O(1)."""
    from sgmm_amd import _lib
    L = _lib.load()
    master = torch.zeros(G, device=DEV)
    worst = 0.0
    for gen, seed, sid, i0, n in _ask_combos():
        # the stream's own sigma is 1, the other evolver's is not
        st = _state_dev(gm.new_state(sigma=1.0 if sid == 0 else 3.0, sigma_adv=1.0 if sid == 1 else 3.0, gen=gen))
        z = _ask_padded(L, master, st, sid, seed, i0, n).cpu().numpy()
        err = _ulp_err(z, gm.ask_rows(np.zeros(G), 1.0, seed, sid, gen, i0, n))
        worst = max(worst, err)
        assert err <= ASK_ULP_BOUND, (G, gen, hex(seed), sid, i0, n, err)
    print(f"sgmm_ga_ask n_params={G}: max error {worst:.2f} float32 ulps (bound {ASK_ULP_BOUND})")
    # the key's high word reaches the stream
    st = _state_dev(gm.new_state(sigma=1.0, gen=7))
    lo, hi = (_ask_padded(L, master, st, 0, s, 40, 65) for s in (5, 5 + 2 ** 32))
    assert float((lo == hi).float().mean()) < 1e-3  # two independent streams (chance equalities aside)


@pytest.mark.parametrize("G", [7, 370, 1250])
def test_ask_applies_sigma_in_float32(sgmm, G):
    """out = f32(master + f32(z f32(sigma))) bit for bit (model.py:69-70), z the
    device's own sigma = 1 output; stream 1 reads sigma_adv."""
    from sgmm_amd import _lib
    L = _lib.load()
    gen, seed, i0, n = 7, 0x0123456789ABCDEF, 40, 65
    torch.manual_seed(G)
    master = torch.randn(G, device=DEV)
    one = _state_dev(gm.new_state(sigma=1.0, gen=gen))
    st = _state_dev(gm.new_state(sigma=0.05, sigma_adv=0.07, gen=gen))
    m = master.cpu().numpy()
    for sid, sigma in ((0, 0.05), (1, 0.07)):
        z = _ask_padded(L, torch.zeros(G, device=DEV), one, sid, seed, i0, n).cpu().numpy()
        out = _ask_padded(L, master, st, sid, seed, i0, n).cpu().numpy()
        want = m[None, :] + z * np.float32(sigma)
        assert want.dtype == np.float32
        assert np.array_equal(out.view(np.int32), want.view(np.int32)), (G, sid)


# ------------------------------------------------------------------ adversarial fitness vectors
def _nextafter(x, to):
    return float(np.nextafter(np.float64(x), np.float64(to)))


CLOSE_PAIRS = [(1.0, _nextafter(1.0, 2.0)), (-1.0, _nextafter(-1.0, 0.0)), (5e-324, 1e-323), (0.0, 5e-324),
               (-5e-324, 0.0), (1.797e308, _nextafter(1.797e308, 0.0)), (-1.797e308, _nextafter(-1.797e308, 0.0)),
               (2.5e-310, _nextafter(2.5e-310, 1.0))]


def vector_families(P, injectable=False):
    """[(name, float64[P])]: the families of the module docstring for a population
    of P.  injectable: only vectors an idle penalty can produce bit for bit --
    no -0.0 (0.0 - 0.0 is +0.0) and no NaN with the sign bit set (the sign of a
    NaN that went through a subtraction is not specified)."""
    rng = np.random.default_rng(P)
    base = rng.normal(size=P)            # distinct, |x| < 7
    out = []

    def put(name, bg, **at):
        f = np.array(bg, np.float64, copy=True)
        for v, idx in at.values():
            f[list(idx)] = v
        out.append((name, f))

    spots = sorted({s for s in (0, 1, 62, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, P - 1) if s < P})
    for s in spots:
        put(f"max@{s}", base, a=(9.0, [s]))
        put(f"min@{s}", base, a=(-9.0, [s]))
    put("all -3", np.full(P, -3.0))
    put("all 0", np.zeros(P))
    pairs = {(63, 64), (10, 69), (5, 1030), (1023, 1024), (P - 2, P - 1)}
    for d in (1, 64, 256, 1024):
        pairs.add((min(7, P - 1 - d), min(7, P - 1 - d) + d))
    pairs = sorted(p for p in pairs if 0 <= p[0] < p[1] < P)
    for a, b in pairs:
        put(f"tie max {a},{b}", base, a=(9.0, [a, b]))
        put(f"tie min {a},{b}", base, a=(-9.0, [a, b]))
    j = P // 2
    put(f"nan@{j}", base, a=(NAN, [j]))
    put("nan@0", base, a=(NAN, [0]))
    if j >= 1:
        put(f"nan@{j} +inf@{j // 2}", np.full(P, -INF), a=(INF, [j // 2]), b=(NAN, [j]))
    put("several nan", base, a=(NAN, sorted({P - 1, P // 3, (2 * P) // 3})))
    put("all nan", np.full(P, NAN))
    if not injectable:
        put(f"-nan@{j}", base, a=(-NAN, [j]))
        put("-nan before nan", base, a=(np.copysign(NAN, -1.0), [P // 3]), b=(NAN, [P - 1]))
    put("all -inf", np.full(P, -INF))
    put("all +inf", np.full(P, INF))
    put("inf mixed", base, a=(INF, [P // 3]), b=(-INF, [(2 * P) // 3]))
    put("two +inf two -inf", base, a=(INF, sorted({P // 3, P - 1})), b=(-INF, sorted({0, P // 2} - {P // 3, P - 1})))
    a, b = (10, 69) if P >= 70 else (0, P - 1)
    lo = -1.79765e308 - np.abs(base) * 1e302   # below / above every pair, distinct, finite
    if P >= 2:
        if not injectable:
            z = 63 if P > 64 else P - 2      # neighbours in two waves where P allows
            for bg, side in ((-1.0 - np.abs(base), "neg"), (1.0 + np.abs(base), "pos")):
                put(f"-0,+0 among {side}", bg, a=(-0.0, [z]), b=(0.0, [z + 1]))
                put(f"+0,-0 among {side}", bg, a=(0.0, [z]), b=(-0.0, [z + 1]))
        for x, y in CLOSE_PAIRS:
            for bg, side in ((lo, "low"), (-lo, "high")):
                put(f"{x!r},{y!r} over {side}", bg, a=(x, [a]), b=(y, [b]))
                put(f"{y!r},{x!r} over {side}", bg, a=(y, [a]), b=(x, [b]))
    if injectable:
        for name, f in out:
            assert not np.any((f == 0.0) & np.signbit(f)) and not np.any(np.isnan(f) & np.signbit(f)), name
    return out


def _val_value(j, best_val):
    """The best individual's validation fitness of vector j: improvement, no
    improvement, NaN, -inf, an exact tie with best_val, no improvement."""
    k = j % 6
    if k == 0:
        return 1.0 if np.isinf(best_val) else float(best_val) + 1.0
    if k == 2:
        return NAN
    if k == 3:
        return -INF
    if k == 4:
        return float(best_val)
    return float(best_val) - 0.5


def _val_vector(P, j, best, v):
    """Validation fitness of the population: the best individual's is v, every
    other one would improve best_val if it were read instead."""
    vf = 1000.0 + np.random.default_rng(j).normal(size=P)
    vf[best] = v
    return vf


def _pre_state(j):
    """State before vector j's boundary: sigma_mm != sigma_adv, gen 0..2, and for
    every sixth vector the no-improvement counter one short of patience (a decay)."""
    return gm.new_state(sigma=0.1, sigma_adv=0.3, patience=3, decay=0.5, gen=j % 3, best_val=1.0,
                        no_improve=2 if j % 6 == 5 else j % 2)


def _check_boundary(tag, want, post, rows, gen, master, exp_mm, madv, exp_adv, best_slot, slot_before):
    """State, history row, masters and checkpoint slot after a boundary."""
    assert gm.same_bits(post, want.state), (tag, post, want.state)
    if rows is not None:
        assert gm.same_bits(rows[gen], want.row), (tag, rows[gen], want.row)
        others = np.delete(rows, gen)
        assert others.tobytes() == bytes(others.nbytes), (tag, "another history row was written")
    assert _same(master, exp_mm), (tag, "master != asked row best")
    if madv is not None:
        assert _same(madv, exp_adv), (tag, "adversary master != asked row adv_best")
    if best_slot is not None:
        assert _same(best_slot, master if want.checkpoint else slot_before), (tag, "checkpoint slot", want.checkpoint)


# ------------------------------------------------------------------ (b) the direct entry points
TELL_P = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4100]
HIST_CAP = 4


def _shard_layout(P):
    """A shard size that does not divide P, the shard count, the byte stride
    (three more doubles than a shard holds: the padding to poison)."""
    n = max(2, P // 3 + 1)
    if P % n == 0:
        n += 1
    return n, (P + n - 1) // n, 8 * (n + 3)


def _sharded(values, P, dtype, poison):
    """values[P] laid out shard by shard in rows of `stride` bytes, the rest of
    each row (and of the last shard) filled with poison."""
    n, count, stride = _shard_layout(P)
    item = np.dtype(dtype).itemsize
    buf = np.empty((count, stride // item), dtype)
    buf[:] = np.resize(np.asarray(poison, dtype), buf.shape[1])
    for s in range(count):
        part = values[s * n:(s + 1) * n]
        buf[s, :len(part)] = part
    return _dev(buf)


@pytest.mark.parametrize("entry", ["tell_regen", "tell_rows", "step", "step_sharded"])
@pytest.mark.parametrize("P", TELL_P)
def test_single_population_boundary(sgmm, P, entry):
    """sgmm_ga_tell (masters regenerated / copied from host-supplied rows) and
    sgmm_ga_step (contiguous / sharded records with NaN and +inf in the shard
    padding) on every vector family: indices, records, history row, masters bit
    for bit against rows asked beforehand, validation half, checkpoint slot and
    the next generation's ask."""
    from sgmm_amd import _lib
    L, ptr, s = _lib.load(), _lib.ptr, _lib.stream_ptr()
    torch.manual_seed(P)
    master0, madv0 = torch.randn(G_MM, device=DEV), torch.randn(G_ADV, device=DEV)
    tr_h = np.arange(P, dtype=np.int32)
    vtr_h = tr_h + 1000
    tr, vtr = _dev(tr_h), _dev(vtr_h)
    if entry == "tell_rows":  # row strides longer than the genomes
        pop_mm, pop_adv = torch.randn(P, G_MM + 3, device=DEV), torch.randn(P, G_ADV + 1, device=DEV)
    shard_n, _, shard_stride = _shard_layout(P)
    i0n, nn = 5, 3
    for j, (name, f) in enumerate(vector_families(P)):
        tag = (entry, P, name)
        pre, seed = _pre_state(j), 1000 + j + (j << 33)
        gen = int(pre["gen"])
        st = _state_dev(pre)
        step = entry.startswith("step")
        if step:
            best = int(np.argmax(f))
            vf = _val_vector(P, j, best, _val_value(j, pre["best_val"]))
            want = gm.boundary(pre, f, tr_h, vf, vtr_h)
        else:
            want = gm.tell(pre, f, tr_h)
        if entry == "tell_rows":
            exp_mm, exp_adv = pop_mm[want.best, :G_MM], pop_adv[want.abest, :G_ADV]
        else:  # the rows the ask materialises from the same state, beforehand
            exp_mm = _ask(L, master0, st, 0, seed, want.best, 1)[0]
            exp_adv = _ask(L, madv0, st, 1, seed, want.abest, 1)[0]
        master, madv = master0.clone(), madv0.clone()
        hist = torch.zeros((HIST_CAP, 40), dtype=torch.uint8, device=DEV)
        slot0 = torch.full((G_MM,), 123.0, device=DEV)
        slot = slot0.clone()
        if not step:
            rows_mm = (ptr(pop_mm), pop_mm.stride(0)) if entry == "tell_rows" else (None, 0)
            rows_adv = (ptr(pop_adv), pop_adv.stride(0)) if entry == "tell_rows" else (None, 0)
            fd = _dev(f)
            _lib.check(L.sgmm_ga_tell(ptr(st), ptr(fd), ptr(tr), P, ptr(master), *rows_mm, ptr(madv), *rows_adv,
                                      G_MM, G_ADV, seed, ptr(hist), HIST_CAP, s), "sgmm_ga_tell")
            slot = None
        else:
            if entry == "step_sharded":
                poison_f, poison_i = [NAN, INF], [2 ** 31 - 1, -1]
                cols = (_sharded(f, P, np.float64, poison_f), _sharded(tr_h, P, np.int32, poison_i),
                        _sharded(vf, P, np.float64, [INF, NAN]), _sharded(vtr_h, P, np.int32, poison_i))
                shard = (shard_n, shard_stride)
            else:
                cols, shard = (_dev(f), tr, _dev(vf), vtr), (0, 0)
            next_mm = torch.full((nn + 1, G_MM), 7.0, device=DEV)
            next_adv = torch.full((nn + 1, G_ADV), 7.0, device=DEV)
            _lib.check(L.sgmm_ga_step(ptr(st), *[ptr(c) for c in cols], P, *shard, ptr(master), ptr(madv), ptr(slot),
                                      G_MM, G_ADV, seed, ptr(hist), HIST_CAP, ptr(next_mm), ptr(next_adv), i0n, nn, s),
                       "sgmm_ga_step")
        _check_boundary(tag, want, _state_host(st)[0], _hist_host(hist), gen, master, exp_mm, madv, exp_adv,
                        slot, slot0)
        if step:  # the next generation's ask == sgmm_ga_ask from the post-boundary state
            assert _same(next_mm[:nn], _ask(L, master, st, 0, seed, i0n, nn)), (tag, "next ask")
            assert _same(next_adv[:nn], _ask(L, madv, st, 1, seed, i0n, nn)), (tag, "next adversary ask")
            assert bool((next_mm[nn] == 7.0).all()) and bool((next_adv[nn] == 7.0).all()), (tag, "next ask overran")


def _populations(_lib, K, P, cap, st, masters, madv, slots, seeds, hist):
    return _lib.Populations(K, P, H, cap, st.data_ptr(), masters.data_ptr(), None if madv is None else madv.data_ptr(),
                            None if slots is None else slots.data_ptr(), seeds.data_ptr(), hist.data_ptr(), None)


def _seeds_dev(seeds):
    return _dev(np.array(seeds, np.uint64).view(np.int64))


@pytest.mark.parametrize("entry", ["step_multi", "tell_multi"])
@pytest.mark.parametrize("P", TELL_P)
def test_multi_population_boundary(sgmm, P, entry):
    """sgmm_ga_step_multi / sgmm_ga_tell_multi: every vector family of P is one
    population of a single launch, each with its own state, generation, key and
    masters; the populations' records lie fit_pop_stride > 8 P apart with NaN
    and +inf in the gap."""
    from sgmm_amd import _lib
    L, ptr, s = _lib.load(), _lib.ptr, _lib.stream_ptr()
    vecs = vector_families(P)
    K = len(vecs)
    assert K >= 3
    torch.manual_seed(P + 1)
    masters0, madv0 = torch.randn(K, G_MM, device=DEV), torch.randn(K, G_ADV, device=DEV)
    tr_h = np.arange(P, dtype=np.int32)
    vtr_h = tr_h + 1000
    pre = np.stack([_pre_state(j) for j in range(K)])
    seeds = [1000 + j + (j << 33) for j in range(K)]
    st = _state_dev(pre)
    step = entry == "step_multi"
    fit = np.empty((K, P + 5)); fit[:, 0::2], fit[:, 1::2] = NAN, INF
    vfit = fit.copy()
    trd = np.full((K, P + 7), 2 ** 31 - 1, np.int32)
    vtrd = trd.copy()
    want, exp = [], []
    for j, (name, f) in enumerate(vecs):
        fit[j, :P], trd[j, :P], vtrd[j, :P] = f, tr_h, vtr_h
        if step:
            vfit[j, :P] = _val_vector(P, j, int(np.argmax(f)), _val_value(j, pre[j]["best_val"]))
            want.append(gm.boundary(pre[j], f, tr_h, vfit[j, :P], vtr_h))
        else:
            want.append(gm.tell(pre[j], f, tr_h))
        exp.append((_ask(L, masters0[j], st[j], 0, seeds[j], want[j].best, 1)[0],
                    _ask(L, madv0[j], st[j], 1, seeds[j], want[j].abest, 1)[0]))
    masters, madv = masters0.clone(), madv0.clone()
    slots0 = torch.full((K, G_MM), 123.0, device=DEV)
    slots = slots0.clone()
    hist = torch.zeros((K, HIST_CAP, 40), dtype=torch.uint8, device=DEV)
    seeds_d = _seeds_dev(seeds)
    pops = _populations(_lib, K, P, HIST_CAP, st, masters, madv, slots, seeds_d, hist)
    cols = [_dev(c) for c in (fit, trd, vfit, vtrd)]
    if step:
        rc = L.sgmm_ga_step_multi(ctypes.byref(pops), *[ptr(c) for c in cols], 8 * (P + 5), 4 * (P + 7), 0, 0, s)
    else:
        rc = L.sgmm_ga_tell_multi(ctypes.byref(pops), ptr(cols[0]), ptr(cols[1]), 8 * (P + 5), 4 * (P + 7), 0, 0, s)
    _lib.check(rc, entry)
    post, rows = _state_host(st), _hist_host(hist).reshape(K, HIST_CAP)
    for j, (name, _) in enumerate(vecs):
        _check_boundary((entry, P, name), want[j], post[j], rows[j], int(pre[j]["gen"]), masters[j], exp[j][0],
                        madv[j], exp[j][1], slots[j] if step else None, slots0[j])
    if not step:
        assert _same(slots, slots0)


@pytest.mark.parametrize("use_best", [0, 1])
def test_val_update_alone(sgmm, use_best):
    """sgmm_ga_val_update, the validation bookkeeping with no tell before it (the
    path sgmm_validate_multi's tail shares): _val_value's six cases in sequence on
    one state with patience 2 -- improvement, no improvement, NaN, -inf, an exact
    tie with best_val, the decay case -- reading record 0 or record best_idx;
    state, history (two generations lie past its capacity) and checkpoint slot
    bit for bit against ga_model.val_update."""
    from sgmm_amd import _lib
    L, ptr, s = _lib.load(), _lib.ptr, _lib.stream_ptr()
    n_rec, best_idx = 5, 3
    idx = best_idx if use_best else 0
    model = gm.new_state(sigma=0.1, sigma_adv=0.3, patience=2, decay=0.5)
    model["best_idx"] = best_idx
    st = _state_dev(model)
    hist = torch.zeros((HIST_CAP, 40), dtype=torch.uint8, device=DEV)
    rows_want = np.zeros(HIST_CAP, _hist_host(hist).dtype)
    slot = torch.full((G_MM,), 123.0, device=DEV)
    decays = checkpoints = 0
    for j in range(6):
        torch.manual_seed(j)
        master = torch.randn(G_MM, device=DEV)
        master0, slot_before = master.clone(), slot.clone()
        v = _val_value(j, model["best_val"])
        vf = np.full(n_rec, 1000.0)       # any other record would improve
        vtr = np.arange(n_rec, dtype=np.int32)
        vf[idx], vtr[idx] = v, 1000 + j
        vf_d, vtr_d = _dev(vf), _dev(vtr)
        _lib.check(L.sgmm_ga_val_update(ptr(st), ptr(vf_d), ptr(vtr_d), use_best, ptr(master), ptr(slot),
                                        G_MM, ptr(hist), HIST_CAP, s), "sgmm_ga_val_update")
        gen = int(model["gen"])
        want = gm.val_update(model, v, 1000 + j)
        if gen < HIST_CAP:
            rows_want[gen] = want.row
        tag = (use_best, j, v)
        assert gm.same_bits(_state_host(st)[0], want.state), (tag, _state_host(st)[0], want.state)
        assert gm.same_bits(_hist_host(hist), rows_want), (tag, _hist_host(hist), rows_want)
        assert _same(master, master0), (tag, "master written")
        assert _same(slot, master if want.checkpoint else slot_before), (tag, "checkpoint slot", want.checkpoint)
        model = want.state
        decays += int(want.state["decayed"])
        checkpoints += int(want.checkpoint)
    assert decays >= 1 and checkpoints >= 1


# ------------------------------------------------------------------ (c) the in-launch tails
T_TRAIN, T_VAL = 12, 8
GENS = 3

# mode 0, the whole boundary in the rollout's tail (sgmm_generation, K = 1, and
# sgmm_generation_multi, K = 3): name -> (P, plan knobs, adversary).  The tail
# is ga_step_fused when P <= scan workgroup (and both genomes <= 16 floats a
# thread), else ga_step_dev.
TAIL_WHOLE = {
    "default_P24": (24, {}, False),
    "w64_P64": (64, dict(scan_threads=64), False),
    "w64_P65": (65, dict(scan_threads=64), False),
    "w256_P256": (256, dict(scan_threads=256), False),
    "w256_P257": (257, dict(scan_threads=256), False),
    "w512_P512": (512, dict(scan_threads=512), False),
    "w512_P513": (513, dict(scan_threads=512), False),
    "default_P600": (600, {}, False),
    "default_P1100": (1100, {}, False),
    "arl_P24": (24, {}, True),
    "arl_P600": (600, {}, True),
}
# modes 3 + 4 (sgmm_generation_multi_best, K = 3): the tell's argmax in the
# training scan's tail, regeneration and bookkeeping in the validation launch's
BEST_KNOBS = {
    "wave_table": dict(policy_path="table", scan_threads=64),
    "wave_frontier": dict(policy_path="frontier", groups=1, scan_threads=64, lanes_scan=0, fused_scan=0),
    "lanes": dict(policy_path="frontier", groups=1, lanes_scan=1, fused_scan=0, seq_sum=1),
    "fused": dict(policy_path="frontier", groups=1, fused_scan=1),
    "arl_table": {},
}
BEST_P = [24, 64, 65, 1024, 1025, 1100]
TAIL_BEST = {f"{k}_P{P}": (P, knobs, k == "arl_table") for k, knobs in BEST_KNOBS.items() for P in BEST_P
             if (k != "lanes" or P % 4 == 0) and (k != "arl_table" or P in (24, 1025))}


class _IdleWorld:
    """K populations of P individuals over a tick bundle that never fills:
    fitness is injected through the idle penalty of each episode's own params
    entry (param[e] = e).  whole: P training + P validation episodes per
    population in one batch (mode 0); else a training batch and one validation
    episode per population (modes 3 + 4)."""

    def __init__(self, sgmm, K, P, arl, whole):
        from sgmm_amd import _lib
        from sgmm_amd.rollout import ENV_PARAMS_DTYPE
        self.L, self.lib, self.K, self.P, self.arl, self.whole = _lib.load(), _lib, K, P, arl, whole
        rng = np.random.default_rng(3)
        stats = {k: np.float32(v) for k, v in (("s1_m", 0.0), ("s1_s", 1.0), ("s2_m", 0.0), ("s2_s", 1.0))}
        self.ticks = sgmm.TickStore()
        offs = []
        for T in (T_TRAIN, T_VAL):
            mid = 3.0 + 0.01 * rng.normal(size=T)
            nan = np.full(T, NAN)
            offs.append(self.ticks.segments[self.ticks.add((rng.normal(size=T), rng.normal(size=T), mid, mid + 0.001,
                                                            mid - 0.001, nan, nan), stats)][0])
        self.ticks.to(DEV)
        idx, none = np.arange(P), np.full(P, -1)
        if whole:
            n = 2 * P * K
            batches = [sgmm.EpisodeBatch(np.tile(idx, 2 * K), np.tile(np.repeat(offs, P), K),
                                         np.tile(np.repeat([T_TRAIN, T_VAL], P), K), np.arange(n),
                                         adv=np.tile(np.concatenate([idx, none]), K) if arl else None)]
        else:
            n = K * P + K
            batches = [sgmm.EpisodeBatch(np.tile(idx, K), np.full(K * P, offs[0]), np.full(K * P, T_TRAIN),
                                         np.arange(K * P), adv=np.tile(idx, K) if arl else None),
                       sgmm.EpisodeBatch(np.arange(K), np.full(K, offs[1]), np.full(K, T_VAL), K * P + np.arange(K))]
        self.batches = [b.to(DEV) for b in batches]
        self.rec = np.stack([sgmm.EnvConfig(phi=0.0005, tick_size=0.001).record()] * n).astype(ENV_PARAMS_DTYPE)
        self.params = torch.zeros(n * ENV_PARAMS_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
        need = max(self.L.sgmm_rollout_workspace_bytes(b.n, b.total_steps, 5, int(arl and i == 0))
                   for i, b in enumerate(self.batches))
        self.ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        self.fit = torch.zeros(self.batches[0].n, dtype=torch.float64, device=DEV)
        self.trd = torch.full((self.batches[0].n,), -1, dtype=torch.int32, device=DEV)
        self.vfit = torch.zeros(K, dtype=torch.float64, device=DEV)
        self.vtrd = torch.full((K,), -1, dtype=torch.int32, device=DEV)

    def inject(self, values):
        """values[e] = the fitness episode e is to report"""
        v = np.asarray(values, np.float64)
        self.rec["idle_penalty"] = np.where(np.isnan(v), NAN, -v)
        self.params.copy_(torch.from_numpy(self.rec.view(np.uint8).reshape(-1).copy()))

    def launch(self, single, st, masters, madv, slots, seeds, hist):
        lib, L, ptr, s = self.lib, self.L, self.lib.ptr, self.lib.stream_ptr()
        tk = self.ticks.struct()
        eps = [b.struct() for b in self.batches]
        seeds_d = _seeds_dev(seeds)
        pops = _populations(lib, self.K, self.P, GENS, st, masters, madv, slots, seeds_d, hist)
        if single:
            rc = L.sgmm_generation(ctypes.byref(tk), ctypes.byref(eps[0]), ptr(self.params), ptr(st), ptr(masters),
                                   ptr(madv), ptr(slots), H, seeds[0], self.P, ptr(self.fit), ptr(self.trd),
                                   ptr(hist), GENS, ptr(self.ws), self.ws.numel(), s)
        elif self.whole:
            rc = L.sgmm_generation_multi(ctypes.byref(tk), ctypes.byref(eps[0]), ptr(self.params), ctypes.byref(pops),
                                         ptr(self.fit), ptr(self.trd), ptr(self.ws), self.ws.numel(), s)
        else:
            rc = L.sgmm_generation_multi_best(ctypes.byref(tk), ctypes.byref(eps[0]), ctypes.byref(eps[1]),
                                              ptr(self.params), ctypes.byref(pops), ptr(self.fit), ptr(self.trd),
                                              ptr(self.vfit), ptr(self.vtrd), ptr(self.ws), self.ws.numel(), s)
        lib.check(rc, "generation")


def _run_tails(sgmm, K, P, arl, whole, single=False):
    """Every injectable vector family of P through the launch's own tail, GENS
    consecutive generations per fresh state (sigma decays and best_val carries
    over, so each regeneration must pick up the new sigma and generation)."""
    from sgmm_amd import _lib
    L = _lib.load()
    w = _IdleWorld(sgmm, K, P, arl, whole)
    vecs = vector_families(P, injectable=True)
    per_case = GENS * K
    zeros = np.zeros(P, np.int32)
    decays, seen_improved = 0, False
    for c in range((len(vecs) + per_case - 1) // per_case):
        torch.manual_seed(c)
        masters = 0.1 * torch.randn(K, G_MM, device=DEV)
        madv = 0.1 * torch.randn(K, G_ADV, device=DEV) if arl else None
        slots = torch.full((K, G_MM), 123.0, device=DEV)
        hist = torch.zeros((K, GENS, 40), dtype=torch.uint8, device=DEV)
        model = [gm.new_state(sigma=0.1, sigma_adv=0.3, patience=2, decay=0.5) for _ in range(K)]
        seeds = [77 + c + (k << 32) for k in range(K)]
        st = _state_dev(np.stack(model))
        rows_want = np.zeros((K, GENS), _hist_host(hist).dtype)
        for g in range(GENS):
            js = [((c * GENS + g) * K + k) % len(vecs) for k in range(K)]
            fs = [vecs[j][1] for j in js]
            vs = [_val_value(j + g, model[k]["best_val"]) for k, j in enumerate(js)]
            exp, inj = [], []
            for k in range(K):
                best, abest = int(np.argmax(fs[k])), int(np.argmax(-fs[k]))
                # whole: every individual is validated; the best one's record counts
                inj += [fs[k], _val_vector(P, js[k], best, vs[k])] if whole else [fs[k]]
                exp.append((_ask(L, masters[k], st[k], 0, seeds[k], best, 1)[0],
                            _ask(L, madv[k], st[k], 1, seeds[k], abest, 1)[0] if arl else None))
            inj = np.concatenate(inj + ([] if whole else [np.array(vs)]))
            w.inject(inj)
            slots_before = slots.clone()
            w.launch(single, st, masters, madv, slots, seeds, hist)
            tag = (K, P, arl, c, g, [vecs[j][0] for j in js])
            # the injection itself: the launch's fitness is the injected vector bit for bit
            # (a NaN as some NaN: 0.0 - NaN keeps the operand's sign on x86 and flips it
            # here, and IEEE 754 specifies neither), and no trades.  The model is then fed
            # the launch's own records, so the bits the tail passes on are checked too.
            got = np.concatenate([w.fit.cpu().numpy()] + ([] if whole else [w.vfit.cpu().numpy()]))
            nan = np.isnan(inj)
            diff = np.flatnonzero((got.view(np.int64) != inj.view(np.int64)) & ~nan)
            assert len(diff) == 0 and np.all(np.isnan(got[nan])), (tag, "fitness != injected", diff[:8], got[diff[:8]])
            assert not bool(w.trd.any()) and (whole or not bool(w.vtrd.any())), (tag, "trades on a no-fill bundle")
            want = []
            for k in range(K):
                if whole:
                    f, vf = got[2 * P * k:2 * P * k + P], got[2 * P * k + P:2 * P * (k + 1)]
                    want.append(gm.boundary(model[k], f, zeros, vf, zeros))
                else:
                    t = gm.tell(model[k], got[P * k:P * (k + 1)], zeros)
                    v = gm.val_update(t.state, got[K * P + k], 0, t.row)
                    want.append(gm.Boundary(v.state, v.row, t.best, t.abest, v.checkpoint))
                assert (want[k].best, want[k].abest) == (int(np.argmax(fs[k])), int(np.argmax(-fs[k])))
            post, rows = _state_host(st), _hist_host(hist).reshape(K, GENS)
            for k in range(K):
                rows_want[k, g] = want[k].row
                assert gm.same_bits(post[k], want[k].state), (tag, k, post[k], want[k].state)
                assert gm.same_bits(rows[k], rows_want[k]), (tag, k, rows[k], rows_want[k])
                assert _same(masters[k], exp[k][0]), (tag, k, "master != asked row best")
                assert not arl or _same(madv[k], exp[k][1]), (tag, k, "adversary master != asked row adv_best")
                assert _same(slots[k], masters[k] if want[k].checkpoint else slots_before[k]), (tag, k, "checkpoint slot")
                model[k] = want[k].state
                seen_improved |= want[k].checkpoint
        decays += sum(int(r["flags"]) >> 1 for r in rows_want.reshape(-1))
    assert decays > 0 and bool(seen_improved)  # the regenerations picked up decayed sigmas; checkpoints were taken


@pytest.mark.parametrize("K", [1, 3], ids=["generation", "multi3"])
@pytest.mark.parametrize("name", list(TAIL_WHOLE))
def test_whole_boundary_in_the_rollout_tail(sgmm, plan, name, K):
    """Mode 0: sgmm_generation and sgmm_generation_multi (K = 3) run ga_step_fused
    (P <= scan workgroup) or ga_step_dev (P beyond it) in the scan's last
    workgroup, on the injected vectors."""
    P, knobs, arl = TAIL_WHOLE[name]
    plan(**knobs)
    _run_tails(sgmm, K, P, arl, whole=True, single=K == 1)


@pytest.mark.parametrize("name", list(TAIL_BEST))
def test_tell_in_the_training_tail_then_validation(sgmm, plan, name):
    """Modes 3 + 4 (sgmm_generation_multi_best, K = 3): tell_wave's argmax in the
    one-wave scan's tail (table / frontier), the lanes scan, the frontier's fused
    scan and the adversary scan; regen_master_block and val_update_dev in the
    validation launch.  val_fitness[k] is the injected value."""
    P, knobs, arl = TAIL_BEST[name]
    plan(**knobs)
    _run_tails(sgmm, 3, P, arl, whole=False)
