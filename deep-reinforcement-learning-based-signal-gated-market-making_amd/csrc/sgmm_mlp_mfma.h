// sgmm_mlp_mfma.h -- the policy MLP on the matrix cores, written once.
//
// The tick-parallel kernels (k_policy_table_mfma / _v3 / _sp in sgmm_table.hip,
// k_frontier_spill in sgmm_frontier.hip) evaluate the policy for 64 samples per
// wave: layer 1 and 3 on the VALU, the H x H layer on v_mfma_f32_16x16x4_f32,
// whose k-ordered fused chain IS the canonical dot-product order.  The stages
// are here; how a kernel orders and overlaps them (its schedule, which is what
// was measured) stays in the kernel.  Lane layout: grp = lane >> 4, col =
// lane & 15; before the transpose a lane holds samples 16 q + col (q = 0..3),
// after it lane n holds sample n.
//
// Also here: the finish of a 64-tick chunk (step maps + per-state rewards ->
// chunk map, path planes, trade counts), shared with the VALU table, and the
// successor byte of the kernels that run one wave per state.
#pragma once

#include "sgmm_rollout.h"

namespace sgmm {

// this lane's tick prices
struct TickPrices {
    double mid, ask, bid, bmax, smin;
};
__device__ __forceinline__ TickPrices load_prices(const sgmm_ticks& tk, int64_t ti) {
    return TickPrices{tk.mid_next[ti], tk.best_ask[ti], tk.best_bid[ti], tk.buy_max[ti], tk.sell_min[ti]};
}

// the policy outputs -> integer offsets (drl_engine.py:38-39) -> the FPT step from inventory inv
__device__ __forceinline__ StepOut policy_step(const sgmm_env_params& p, int32_t inv, float o0, float o1,
                                               const TickPrices& x) {
    const int32_t oa = act_to_int(rintf(o0 * p.act_scale));
    const int32_t ob = act_to_int(rintf(o1 * p.act_scale));
    return ftp_step(p, inv, oa, ob, x.mid, x.ask, x.bid, x.bmax, x.smin);
}

template <int H>
struct MlpMfma {
    static_assert(H % 16 == 0, "the MFMA MLP needs H multiple of 16");
    using L = GenomeLayout<H>;
    static constexpr int NT = H / 16;  // 16-neuron row tiles of layer 2
    static constexpr int KS = H / 4;   // k-steps (4 per MFMA)
    static constexpr int HP = H + 4;   // LDS row pitch (floats) of the transposed activations

    // the signals of samples 16 q + col; tick_of(sample) = its tick index, clamped
    // into the episode (padded samples are discarded later)
    template <class TickOf>
    static __device__ __forceinline__ void load_signals(const sgmm_ticks& tk, int col, TickOf tick_of,
                                                        float (&xs0)[4], float (&xs1)[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t ti = tick_of(16 * q + col);
            xs0[q] = tk.s1n[ti];
            xs1[q] = tk.s2n[ti];
        }
    }

    // layer-2 fragments of a staged genome g (lane-dependent, tile-independent):
    // w2f = A (neuron 16 rt + col, k = 4 i + grp), b2c = C (neurons 16 rt + 4 grp + r)
    static __device__ __forceinline__ void load_w2(const float* g, int grp, int col, float (&w2f)[NT][KS],
                                                   f32x4 (&b2c)[NT]) {
#pragma unroll
        for (int rt = 0; rt < NT; ++rt) {
#pragma unroll
            for (int i = 0; i < KS; ++i) w2f[rt][i] = g[L::W2 + (16 * rt + col) * H + 4 * i + grp];
#pragma unroll
            for (int r = 0; r < 4; ++r) b2c[rt][r] = g[L::B2 + 16 * rt + 4 * grp + r];
        }
    }

    // layer-3 weights interleaved as (W3[0][j], W3[1][j]) pairs; the first 2 H
    // threads of the block store, the caller synchronizes
    static __device__ __forceinline__ void store_w3i(const float* g, float* w3i) {
        if (threadIdx.x < 2 * H) w3i[threadIdx.x] = g[L::W3 + (threadIdx.x & 1) * H + (threadIdx.x >> 1)];
    }

    // layer 1, the part all inventory states share: w1s[i] = W1[k][2] and
    // pre[q][i] = b1[k] + W1[k][0] s1n + W1[k][1] s2n of sample 16 q + col, k = 4 i + grp
    static __device__ __forceinline__ void layer1_pre(const float* g, int grp, const float (&xs0)[4],
                                                      const float (&xs1)[4], float (&w1s)[KS], float (&pre)[4][KS]) {
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            const int k = 4 * i + grp;
            const float a0 = g[L::W1 + 3 * k], a1 = g[L::W1 + 3 * k + 1], bb = g[L::B1 + k];
            w1s[i] = g[L::W1 + 3 * k + 2];
#pragma unroll
            for (int q = 0; q < 4; ++q) pre[q][i] = __builtin_fmaf(a1, xs1[q], __builtin_fmaf(a0, xs0[q], bb));
        }
    }
    // ... and the inventory term x2 = inv / 2 of one state
    static __device__ __forceinline__ void layer1_state(const float (&w1s)[KS], const float (&pre)[4][KS], float x2,
                                                        float (&h1)[KS][4]) {
#pragma unroll
        for (int i = 0; i < KS; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) h1[i][q] = relu(__builtin_fmaf(w1s[i], x2, pre[q][i]));
    }
    // layer 1 of a single state in one go
    static __device__ __forceinline__ void layer1(const float* g, int grp, const float (&xs0)[4],
                                                  const float (&xs1)[4], float x2, float (&h1)[KS][4]) {
        float w1s[KS], pre[4][KS];
        layer1_pre(g, grp, xs0, xs1, w1s, pre);
        layer1_state(w1s, pre, x2, h1);
    }

    // layer 2: H2^T = W2 . H1^T + b2, four 16-sample tiles
    static __device__ __forceinline__ void layer2(const float (&w2f)[NT][KS], const f32x4 (&b2c)[NT],
                                                  const float (&h1)[KS][4], f32x4 (&acc)[4][NT]) {
#pragma unroll
        for (int i = 0; i < KS; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int rt = 0; rt < NT; ++rt)
                    acc[q][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w2f[rt][i], h1[i][q],
                                                                      i == 0 ? b2c[rt] : acc[q][rt], 0, 0, 0);
    }

    // relu(H2) -> LDS as [sample][neuron]: lane n then reads tick n's H activations
    static __device__ __forceinline__ void transpose(const f32x4 (&acc)[4][NT], float* hb, int grp, int col) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int rt = 0; rt < NT; ++rt) {
                f32x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = relu(acc[q][rt][r]);
                *reinterpret_cast<f32x4*>(&hb[(16 * q + col) * HP + 16 * rt + 4 * grp]) = v;
            }
    }

    // layer 3 of this lane's tick: the two canonical output chains from (o0, o1) = b3
    static __device__ __forceinline__ void layer3(const float* hb, const float* w3i, int lane, float& o0, float& o1) {
#pragma unroll
        for (int j4 = 0; j4 < H / 4; ++j4) {
            const f32x4 h = *reinterpret_cast<const f32x4*>(&hb[lane * HP + 4 * j4]);
#pragma unroll
            for (int r2 = 0; r2 < 2; ++r2) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(&w3i[2 * (4 * j4 + 2 * r2)]);
                o0 = __builtin_fmaf(w[0], h[2 * r2], o0);
                o1 = __builtin_fmaf(w[1], h[2 * r2], o1);
                o0 = __builtin_fmaf(w[2], h[2 * r2 + 1], o0);
                o1 = __builtin_fmaf(w[3], h[2 * r2 + 1], o1);
            }
        }
    }
};

// ------------------------------------------------------------------ chunk finish
// One wave, lane = tick of a 64-tick chunk: from each tick's step map and trade
// bits (identity / 0 on padded lanes) and the per-state rewards reward_of(state)
// of this lane's tick, write
//   plane s0 row `row` = the tick's reward along the chunk's path from start state s0,
//   cmaps[ci] = the chunk's transition map, ctr[ci] = the trade count along the
//   path from each start state (8 bits each).
// scanned(excl) runs between the map scan and the planes (a kernel's stamp or fence).
struct NoHook {
    __device__ __forceinline__ void operator()(uint64_t) const {}
};
template <int NSI, class RewardOf, class Scanned = NoHook>
__device__ __forceinline__ void chunk_finish(uint64_t map, uint32_t traded, bool valid, int lane, int nsi,
                                             double* __restrict__ rew, int64_t rs, int64_t row,
                                             uint64_t* __restrict__ cmaps, uint64_t* __restrict__ ctr, uint32_t ci,
                                             RewardOf reward_of, Scanned scanned = Scanned{}) {
    const uint64_t inc = wave_map_scan(map);
    uint64_t excl = shfl_up_u64(inc, 1);
    if (lane == 0) excl = kIdentityMap;
    scanned(excl);
    uint64_t cnt = 0;
#pragma unroll
    for (int s0 = 0; s0 < NSI; ++s0) {
        if (s0 >= nsi) break;
        const uint32_t st = map_get(excl, (uint32_t)s0);
        if (valid) rew[s0 * rs + row] = reward_of(st);
        cnt |= (uint64_t)__popcll(__ballot(valid && ((traded >> st) & 1u))) << (8 * s0);
    }
    if (lane == kWave - 1) {
        cmaps[ci] = inc;
        ctr[ci] = cnt;
    }
}

// ------------------------------------------------------------------ successor byte
// One wave per inventory state: state si's wave leaves its tick's step as
// successor | traded << 7; wave 0 collects the nsi bytes of its lane's tick.
__device__ __forceinline__ uint8_t pack_step(int si, const StepOut& so) {
    return (uint8_t)((si + so.fill_buy - so.fill_sell) | ((so.fill_buy | so.fill_sell) << 7));
}
__device__ __forceinline__ void unpack_steps(const uint8_t (*to_s)[kWave], int lane, int nsi, uint64_t& map,
                                             uint32_t& traded) {
    for (int s = 0; s < nsi; ++s) {
        const uint32_t b = to_s[s][lane];
        map = (map & ~(0xFFull << (8 * s))) | ((uint64_t)(b & 0x7Fu) << (8 * s));
        traded |= (b >> 7) << s;
    }
}

}  // namespace sgmm
