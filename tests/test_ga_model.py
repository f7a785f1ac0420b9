"""CPU checks of tests/ga_model.py, the independent reference the GPU boundary
tests (test_gpu_ga_boundary.py) compare the device against: the published
Philox4x32-10 known answers, the Box-Muller mapping at its edge words, the
counter layout, and the boundary bookkeeping on generations worked out by hand."""
import math

import numpy as np
import pytest

import ga_model as gm

# Random123's kat_vectors for philox4x32 with 10 rounds: counter, key, result
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, want):
    assert gm.philox4x32_10(ctr, key) == want
    # the vectorised form: the vector among other counters
    arr = [np.array([1, c, 2], np.uint64) for c in ctr]
    got = gm.philox4x32_10(arr, key)
    assert tuple(int(g[1]) for g in got) == want
    assert tuple(int(g[0]) for g in got) == gm.philox4x32_10((1, 1, 1, 1), key)


def test_box_muller_edge_words():
    top = math.sqrt(64 * math.log(2))  # 6.6604...: raw word 0, u0 = 2^-32
    angle = [0, 1, 0x3fffffff, 0x40000000, 0x7fffffff, 0x80000000, 0xc0000000, 0xffffff7f, 0xffffff80, 0xffffffff]
    for r1 in angle:
        z = {r0: gm.box_muller(r0, r1, r0, r1) for r0 in (0, 1, 0xffffff7f, 0xffffff80, 0xffffffff)}
        # every raw word >= 0xffffff80 rounds to 2^32 in float32: u0 = 1, ln = 0, z = 0
        for r0 in (0xffffff80, 0xffffffff):
            assert all(float(v) == 0.0 for v in z[r0]), (r0, r1)
        # the radius: word 0 gives the largest, sqrt(64 ln 2); word 1 sqrt(62 ln 2); the
        # last word below the clamp u0 = 1 - 2^-24
        for r0, m in ((0, top), (1, math.sqrt(62 * math.log(2))),
                      (0xffffff7f, math.sqrt(-2 * math.log1p(-2.0 ** -24)))):
            z0, z1, z2, z3 = (float(v) for v in z[r0])
            assert math.hypot(z0, z1) == pytest.approx(m, rel=1e-14) and (z0, z1) == (z2, z3)
            assert max(abs(z0), abs(z1)) <= top
    assert 6.6604 < top < 6.6605
    # the angle's exact points: u1 = 0, 1/4, 1/2, 3/4 and the words that round to u1 = 1
    m = math.sqrt(62 * math.log(2))
    for r1, (c, s) in ((0, (1, 0)), (0x40000000, (0, 1)), (0x80000000, (-1, 0)), (0xc0000000, (0, -1)),
                       (0xffffff80, (1, 0)), (0xffffffff, (1, 0))):
        z0, z1, _, _ = gm.box_muller(1, r1, 1, r1)
        assert (float(z0), float(z1)) == (m * c, m * s), hex(r1)
    # cosine first, sine second: a small positive angle
    z0, z1, _, _ = gm.box_muller(1, 1 << 20, 1, 1 << 20)
    assert 0 < float(z1) < 0.01 * float(z0)


def test_uniform_mapping_is_float32():
    # 2^24 + 1 is not a float32: it rounds to 2^24 before the + 1
    assert float(gm._u_open_closed((1 << 24) + 1)) == ((1 << 24) + 1) * 2.0 ** -32 - 2.0 ** -32
    assert float(gm._u_closed_open((1 << 24) + 1)) == 2.0 ** -8
    assert float(gm._u_open_closed(0)) == 2.0 ** -32 and float(gm._u_closed_open(0)) == 0.0
    assert float(gm._u_open_closed(0xffffffff)) == 1.0 and float(gm._u_closed_open(0xffffffff)) == 1.0
    assert gm._u_open_closed(5).dtype == np.float32


def test_counter_layout():
    seed, G = 0x0123456789ABCDEF, 7
    z = gm.ask_z(G, seed, 1, 9, 40, 3)
    assert z.shape == (3, G) and z.dtype == np.float64
    for i in range(3):
        for k in range(G):
            r = gm.philox4x32_10((k // 4, 40 + i, 9, 1), (0x89ABCDEF, 0x01234567))
            assert z[i, k] == float(gm.box_muller(*r)[k % 4])
    # every counter word and both key words reach the stream
    base = gm.ask_z(G, 5, 0, 3, 0, 2)
    for other in (gm.ask_z(G, 5 + (1 << 32), 0, 3, 0, 2), gm.ask_z(G, 6, 0, 3, 0, 2), gm.ask_z(G, 5, 1, 3, 0, 2),
                  gm.ask_z(G, 5, 0, 4, 0, 2), gm.ask_z(G, 5, 0, 3, 1, 2)):
        assert not np.any(other == base)
    assert np.array_equal(gm.ask_z(G, 5, 0, 3, 1, 1)[0], base[1])  # rows are individuals
    # gen is the state's int32 read as 32 bits
    assert np.array_equal(gm.ask_z(G, 5, 0, 2 ** 31 - 1, 2_000_000_000, 1), gm.ask_z(G, 5, 0, 0x7fffffff, 2_000_000_000, 1))
    rows = gm.ask_rows(np.arange(G, dtype=np.float32), 0.5, 5, 0, 3, 0, 2)
    assert np.array_equal(rows, np.arange(G)[None, :] + 0.5 * base)


def test_stream_is_standard_normal():
    z = gm.ask_z(1250, 77, 0, 0, 0, 64)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01
    assert abs(np.corrcoef(z[:, 0::4].ravel(), z[:, 1::4].ravel())[0, 1]) < 0.02
    assert np.abs(z).max() <= math.sqrt(64 * math.log(2))


# ------------------------------------------------------------------ the boundary
NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("f,best,abest", [
    ([0.5, 2.0, -1.0, 2.0], 1, 2),            # the first of two maxima
    ([1.0, NAN, 3.0, NAN], 1, 1),             # np.argmax: the first NaN, on both sides
    ([-3.0] * 5, 0, 0),
    ([INF, NAN, -INF], 1, 1),                 # NaN above +inf
    ([-1.0, -0.0, 0.0, -2.0], 1, 3),          # signed zeros tie
    ([2.0, 0.0, -0.0, 3.0], 3, 1),
    ([-INF, -INF], 0, 0),
    ([7.0], 0, 0),
])
def test_tell_model(sgmm, f, best, abest):
    st = gm.new_state(sigma=0.1, gen=4, no_improve=2, best_val=1.5)
    b = gm.tell(st, f, np.arange(10, 10 + len(f)))
    assert (b.best, b.abest, b.checkpoint) == (best, abest, False)
    assert b.state["best_idx"] == best and b.state["adv_best_idx"] == abest
    assert gm.same_bits(b.state["last_train_f"], np.float64(f[best])) and gm.same_bits(b.row["train_f"], np.float64(f[best]))
    assert b.row["train_trades"] == 10 + best and b.row["best_idx"] == best
    for k in ("gen", "no_improve", "best_val", "sigma_mm", "sigma_adv", "improved", "decayed"):
        assert b.state[k] == st[k]            # a tell advances nothing else
    assert st["best_idx"] == -1               # the input record is not modified


def test_val_update_model_on_the_schedule(sgmm):
    """The generations of test_gpu_ga.py::test_val_update_schedule, each step worked out by hand."""
    vals = [1.0, 0.5, 0.7, 0.9, 2.0, NAN, 1.0, 1.5, 1.9, 3.0]
    want = [  # flags, no_improve after, sigma after, best_val after
        (1, 0, 0.05, 1.0), (0, 1, 0.05, 1.0), (0, 2, 0.05, 1.0), (2, 0, 0.025, 1.0), (1, 0, 0.025, 2.0),
        (0, 1, 0.025, 2.0), (0, 2, 0.025, 2.0), (2, 0, 0.0125, 2.0), (0, 1, 0.0125, 2.0), (1, 0, 0.0125, 3.0)]
    st = gm.new_state(sigma=0.05, patience=3, decay=0.5, sigma_adv=0.2)
    for g, (v, (flags, noimp, sigma, bv)) in enumerate(zip(vals, want)):
        b = gm.val_update(st, v, 7)
        st = b.state
        assert (int(b.row["flags"]), int(st["no_improve"]), float(st["sigma_mm"]), float(st["best_val"])) == \
            (flags, noimp, sigma, bv), g
        assert b.checkpoint == bool(flags & 1) and st["gen"] == g + 1 and b.row["val_trades"] == 7
        assert st["sigma_adv"] == 4 * sigma and b.row["sigma_after"] == sigma
        assert gm.same_bits(b.row["val_f"], np.float64(v)) and gm.same_bits(st["last_val_f"], np.float64(v))
        assert (int(st["improved"]), int(st["decayed"])) == (flags & 1, flags >> 1)


def test_boundary_model_by_hand(sgmm):
    st = gm.new_state(sigma=0.05, patience=1, decay=0.25, sigma_adv=0.2)
    # generation 0: tie for the maximum at 1 and 2; the best's validation -inf ties best_val
    b = gm.boundary(st, [1.0, 5.0, 5.0, 2.0], [10, 11, 12, 13], [9.0, -INF, 7.0, 7.0], [1, 2, 3, 4])
    assert (b.best, b.abest, b.checkpoint) == (1, 0, False)
    assert tuple(b.row.tolist()) == (5.0, -INF, 0.0125, 11, 2, 1, 2)
    s = b.state
    assert (s["gen"], s["no_improve"], s["sigma_mm"], s["sigma_adv"], s["best_val"]) == (1, 0, 0.0125, 0.05, -INF)
    # generation 1: NaN fitness wins the tell on both sides; its validation improves
    b = gm.boundary(s, [3.0, NAN, 4.0], [5, 6, 7], [0.0, -2.5, 0.0], [0, 9, 0])
    assert (b.best, b.abest, b.checkpoint) == (1, 1, True)
    assert np.isnan(b.row["train_f"]) and tuple(b.row.tolist())[1:] == (-2.5, 0.0125, 6, 9, 1, 1)
    s = b.state
    assert (s["gen"], s["no_improve"], s["sigma_mm"], s["best_val"], s["last_val_f"]) == (2, 0, 0.0125, -2.5, -2.5)
    # generation 2: an exact tie with best_val does not improve; patience 1 decays again
    b = gm.boundary(s, [-1.0, -1.0], [1, 2], [-2.5, 99.0], [3, 4])
    assert (b.best, b.abest, b.checkpoint, int(b.row["flags"])) == (0, 0, False, 2)
    assert b.state["sigma_mm"] == 0.0125 * 0.25 and b.state["sigma_adv"] == 0.05 * 0.25 and b.state["gen"] == 3
    # patience 0: an improving generation decays as well (no_improve 0 >= 0)
    b = gm.boundary(gm.new_state(patience=0), [1.0], [0], [1.0], [0])
    assert int(b.row["flags"]) == 3 and b.checkpoint and b.state["sigma_mm"] == 0.025
