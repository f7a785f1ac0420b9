// sgmm_table.hip -- the policy tables of the fitness path (sgmm_rollout.hip has
// the overview): every (tick, inventory[, adversary flags]) state of a 64-tick
// chunk evaluated in parallel, on the VALU (k_policy_table) or with the H x H
// layer on the matrix cores (k_policy_table_mfma / _v3 / _sp; the MLP stages
// and the chunk finish are in sgmm_mlp_mfma.h), and the walk-order job that
// rides along with the state-parallel table.  rollout_impl reaches them through
// launch_policy_table / launch_walk_reorder (sgmm_rollout.h).
#include "sgmm_mlp_mfma.h"

namespace sgmm {

// ------------------------------------------------------------------ table
// Block = 64 consecutive ticks of one episode x nsi inventory states: wave w
// evaluates the policy and the FPT step for every tick of the block from
// inventory inv_min + w (one lane per (tick, state)).  The genome is
// wave-uniform, so weights arrive by scalar loads straight into the FMAs'
// SGPR operands, each used once (no loop-invariant hoisting, no SGPR spills,
// ~H+16 VGPRs -> full occupancy).  The 64-tick slice of the tick stream is
// staged once in LDS (coalesced) and read by all waves.  Wave 0 then turns the
// per-state fills into the chunk's transition maps.  Outputs:
//   !ARL: per chunk, cmaps[chunk] = the chunk's full transition map and
//         ctr[chunk] = the trade count along the chunk's path from each start
//         state (8 bits per state); per tick, the path planes
//         rew[s * rs + row] = the reward of the tick along the chunk's path
//         that starts in state s (float64);
//    ARL: fills[row] = 2 fill bits per (inventory, sell flag, buy flag) state
//         and rew[state * rs + row] = the step reward from that state.
template <int H, int NSM, bool ARL>
__global__ __launch_bounds__(kChunk * 8) void k_policy_table(
    sgmm_ticks tk, EpArrays ep, const sgmm_env_params* __restrict__ params,
    GenomeSrc src, int32_t inv_min, int32_t nsi, uint64_t* __restrict__ ctr,
    uint64_t* __restrict__ cmaps, uint64_t* __restrict__ fills, double* __restrict__ rew) {
    const int e = blockIdx.y;
    const int32_t T = ep.len[e];
    const int32_t t0 = blockIdx.x * kChunk;
    if (t0 >= T) return;  // block-uniform
    const int w = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    const int ns = ARL ? 4 * nsi : nsi;
    const sgmm_env_params p = params[ep.param[e]];
    __shared__ float gsm[GenomeLayout<H>::N];
    __shared__ float gsa[kAdvParams];
    const int ai = (ARL && ep.adv) ? ep.adv[e] : -1;
    stage_genomes(src, e, ep.genome[e], ai, GenomeLayout<H>::N, gsm, ARL ? gsa : nullptr);
    const float* g = gsm;

    __shared__ float sx[2][kChunk];
    __shared__ double spx[5][kChunk];
    __shared__ uint8_t code[32][kChunk];
    __shared__ double rws[ARL ? 1 : NSM][kChunk];  // !ARL: per-state rewards for the path planes
    __shared__ int32_t lut[2][32];
    // stage the tick slice: column c by wave c % nsi
    const int64_t tbase = ep.tick_off[e] + t0;
    const int nvalid = min(kChunk, T - t0);
    for (int c = w; c < 7; c += nsi) {
        if (lane < nvalid) {
            const int64_t ti = tbase + lane;
            switch (c) {
                case 0: sx[0][lane] = tk.s1n[ti]; break;
                case 1: sx[1][lane] = tk.s2n[ti]; break;
                case 2: spx[0][lane] = tk.mid_next[ti]; break;
                case 3: spx[1][lane] = tk.best_ask[ti]; break;
                case 4: spx[2][lane] = tk.best_bid[ti]; break;
                case 5: spx[3][lane] = tk.buy_max[ti]; break;
                default: spx[4][lane] = tk.sell_min[ti]; break;
            }
        }
    }
    __syncthreads();  // staged genomes
    if (ARL) {
        if ((int)threadIdx.x < ns) {
            const int s = threadIdx.x;
            int32_t da = 0, db = 0;
            if (ai >= 0) adv_delta(gsa, p, inv_min + (s >> 2), (s >> 1) & 1, s & 1, da, db);
            lut[0][s] = da;
            lut[1][s] = db;
        }
    }
    __syncthreads();
    const bool valid = lane < nvalid;
    if (valid) {
        const int32_t inv = inv_min + w;
        float o0, o1;
        mlp_forward<H>(g, sx[0][lane], sx[1][lane], (float)((double)inv / 2.0), o0, o1);
        const int32_t oa = act_to_int(rintf(o0 * p.act_scale));  // drl_engine.py:38-39
        const int32_t ob = act_to_int(rintf(o1 * p.act_scale));
        const double mid = spx[0][lane], ask = spx[1][lane], bid = spx[2][lane];
        const double bmax = spx[3][lane], smin = spx[4][lane];
        const int64_t row = ep.step_off[e] + t0 + lane;
        if (!ARL) {
            const StepOut so = ftp_step(p, inv, oa, ob, mid, ask, bid, bmax, smin);
            code[w][lane] = (uint8_t)(so.fill_buy | (so.fill_sell << 1));
            rws[ARL ? 0 : w][lane] = so.reward;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int s = 4 * w + c;
                const StepOut so = ftp_step(p, inv, (double)oa + (double)lut[0][s],
                                            (double)ob + (double)lut[1][s], mid, ask, bid, bmax, smin);
                code[s][lane] = (uint8_t)(so.fill_buy | (so.fill_sell << 1));
                rew[s * ep.rs + row] = so.reward;  // per-state planes (SoA): coalesced rows
            }
        }
    }
    __syncthreads();
    if (w != 0) return;
    const int64_t row = ep.step_off[e] + t0 + lane;
    if (ARL) {  // the fill codes (the scan derives the chunk transducers from them)
        uint64_t fw = 0;
        for (int s = 0; s < ns; ++s) fw |= (uint64_t)code[s][lane] << (2 * s);
        if (valid) fills[row] = fw;
        return;
    }
    uint64_t map = kIdentityMap;
    uint32_t traded = 0;
    if (valid) {
        for (int s = 0; s < nsi; ++s) {
            const uint32_t c = code[s][lane];
            const uint64_t to = (uint64_t)(s + (int)(c & 1u) - (int)(c >> 1));
            map = (map & ~(0xFFull << (8 * s))) | (to << (8 * s));
            traded |= (uint32_t)(c != 0) << s;
        }
    }
    chunk_finish<NSM>(map, traded, valid, lane, nsi, rew, ep.rs, row, cmaps, ctr,
                      chunk_base(ep.step_off[e], e) + blockIdx.x,
                      [&](uint32_t st) { return rws[ARL ? 0 : st][lane]; });
}

#ifdef SGMM_STAMPS
// diagnostic build only: phase timestamps (s_memtime) of the table kernels per
// wave; slot 7 of a table wave holds s_memrealtime at entry (a clock common to
// all XCDs)
constexpr int kStampWaves = 1 << 16;
__device__ unsigned long long g_tstamps[kStampWaves][8];
__device__ unsigned int g_thwid[kStampWaves][2];  // HW_ID, XCC_ID of each table wave
#define SGMM_TSTAMP(w, k, dep)                                                     \
    do {                                                                           \
        unsigned long long t_;                                                     \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" \
                     : "=s"(t_) : "v"(dep) : "memory");                             \
        if ((threadIdx.x & 63) == 0 && (w) < kStampWaves) g_tstamps[w][k] = t_;    \
    } while (0)
#define SGMM_TSTAMP_REAL(w, k)                                                         \
    do {                                                                               \
        unsigned long long t_;                                                         \
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
        if ((threadIdx.x & 63) == 0 && (w) < kStampWaves) g_tstamps[w][k] = t_;        \
        unsigned h_, x_;                                                               \
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" \
                     : "=s"(h_), "=s"(x_));                                            \
        if ((threadIdx.x & 63) == 0 && (w) < kStampWaves) { g_thwid[w][0] = h_; g_thwid[w][1] = x_; } \
    } while (0)
#else
#define SGMM_TSTAMP(w, k, dep) \
    do {                       \
    } while (0)
#define SGMM_TSTAMP_REAL(w, k) \
    do {                       \
    } while (0)
#endif

// ------------------------------------------------------------------ table on the matrix cores
// gfx950's f32-input MFMA v_mfma_f32_16x16x4_f32 computes, per output, the
// k-ordered fused chain D = fma(a_k3,b_k3, fma(.., fma(a_k0,b_k0, C))) --
// exactly the canonical dot-product order of the numerics contract -- so the
// policy's H x H layer runs on the matrix pipe bit-identically to the
// VALU/oracle chains, with the weights held as compact per-lane fragments
// (loaded once per wave, reused for every tile).
//
// One wave = one 64-tick chunk of one episode; for each inventory state:
//   layer 1 (VALU):  h1[k][n] = relu(b1 + W1[k].(s1n, s2n, inv/2)), the two
//                    signal terms shared by all states;
//   layer 2 (MFMA):  H2^T[j][n] = W2[j][:] . H1^T[:][n] + b2[j], four 16-sample
//                    tiles (A = W2 rows, B = h1 at k = 4i + (lane>>4), C = b2);
//   transpose:       relu(H2) -> LDS as [sample][neuron] (one 16-byte write
//                    per tile and lane);
//   layer 3 (VALU):  lane n = tick n reads its H activations and runs the two
//                    canonical output chains b3[o] + sum_j W3[o][j] h2[j] (the
//                    2-row output would waste 7/8 of a 16-row MFMA tile).
// The lane then holds the policy outputs of its own tick for every state.

template <int H, int NSI, bool ARL>
__global__ __launch_bounds__(kWave * 4, H <= 16 ? 5 : ((ARL && H <= 32) ? 3 : 1)) void k_policy_table_mfma(
    sgmm_ticks tk, EpArrays ep, const sgmm_env_params* __restrict__ params,
    GenomeSrc src, int32_t inv_min, int32_t nsi, uint64_t* __restrict__ ctr,
    uint64_t* __restrict__ cmaps, uint64_t* __restrict__ fills, double* __restrict__ rew) {
    using M = MlpMfma<H>;
    using L = GenomeLayout<H>;
    constexpr int NT = M::NT, KS = M::KS, HP = M::HP;
    const int e = blockIdx.y;
    const int32_t T = ep.len[e];
    const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int32_t t0 = chunk * kChunk;
    if (blockIdx.x * 4 * kChunk >= T) return;  // block-uniform: no wave of this block has ticks
    const int lane = threadIdx.x & (kWave - 1), grp = lane >> 4, col = lane & 15;
    const int ns = ARL ? 4 * nsi : nsi;
    // this wave's tick data, requested before the genome staging so the loads
    // overlap it (indices clamped into the episode: padded samples are discarded)
    float xs0[4], xs1[4];
    M::load_signals(tk, col, [&](int smp) { return ep.tick_off[e] + min(t0 + smp, T - 1); }, xs0, xs1);
    // the episode's genomes -> LDS (all four waves, before any of them leaves)
    __shared__ __attribute__((aligned(16))) float gsm[L::N];
    __shared__ float gsa[kAdvParams];
    const int ai = (ARL && ep.adv) ? ep.adv[e] : -1;
    stage_genomes(src, e, ep.genome[e], ai, L::N, gsm, ARL ? gsa : nullptr);
    __syncthreads();
    __shared__ __attribute__((aligned(8))) float w3i[2 * H];  // read as f32x2 by the packed output chains
    M::store_w3i(gsm, w3i);
    __syncthreads();
    if (t0 >= T) return;  // wave-uniform; no block barriers below
#ifdef SGMM_STAMPS
    const int wslot = e * (int)(gridDim.x * 4) + chunk;
#endif
    SGMM_TSTAMP_REAL(wslot, 7);
    SGMM_TSTAMP(wslot, 0, 0);
    const sgmm_env_params p = params[ep.param[e]];
    const float* g = gsm;
    const int64_t row = ep.step_off[e] + t0 + lane;  // this lane's output row
    __shared__ __attribute__((aligned(16))) float hb_s[4][kWave * HP];
    float* hb = hb_s[threadIdx.x >> 6];

    // ---- per-lane weight fragments (lane-dependent, tile-independent)
    float w2f[NT][KS];
    f32x4 b2c[NT];
    M::load_w2(g, grp, col, w2f, b2c);
    float w1s[KS], pre[4][KS];
    M::layer1_pre(g, grp, xs0, xs1, w1s, pre);
    SGMM_TSTAMP(wslot, 1, w2f[0][0] + w1s[KS - 1] + pre[3][KS - 1] + b2c[0][0]);

    // ---- the policy for every (state, tick) of the chunk, software-pipelined:
    // the layer-2 MFMAs of state si+1 are issued beside the layer-3 chains of
    // state si (which read the activations si left in LDS), then state si+1 is
    // transposed.  One accumulator set, one activation buffer.
    float out0[NSI], out1[NSI];
    f32x4 acc[4][NT];
    // own layers 1 + 2 (the pipeline's shape): layer 1's last term for two tiles
    // per packed fma, the MFMAs of four independent 16-sample chains interleaved
    // with them (k-step outer)
    auto layer12 = [&](int si) {
        const float x2 = (float)((double)(inv_min + si) / 2.0);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int rt = 0; rt < NT; ++rt) acc[q][rt] = b2c[rt];
#pragma unroll
        for (int i = 0; i < KS; ++i)
#pragma unroll
            for (int q = 0; q < 4; q += 2) {
                const f32x2 hh = __builtin_elementwise_fma(f32x2{w1s[i], w1s[i]}, f32x2{x2, x2},
                                                           f32x2{pre[q][i], pre[q + 1][i]});
                const float h1a = relu(hh.x), h1b = relu(hh.y);
#pragma unroll
                for (int rt = 0; rt < NT; ++rt) {
                    acc[q][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w2f[rt][i], h1a, acc[q][rt], 0, 0, 0);
                    acc[q + 1][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w2f[rt][i], h1b, acc[q + 1][rt], 0, 0, 0);
                }
            }
    };
    // (a lambda like layer12, not the bare call: the two inline at different points of
    // the compiler's pipeline, and this kernel's H = 16 instances are within two VGPRs
    // of spilling -- the bare call costs <16, 5, false> 12 bytes of scratch)
    auto transpose = [&]() { M::transpose(acc, hb, grp, col); };
    layer12(0);
    transpose();
#pragma unroll
    for (int si = 0; si < NSI; ++si) {
        out0[si] = out1[si] = 0.0f;
        if (si >= nsi) continue;
        const bool next = si + 1 < nsi;
        if (next) layer12(si + 1);
        // own layer 3: both output chains in one packed fma per neuron
        f32x2 o = {g[L::B3], g[L::B3 + 1]};
#pragma unroll
        for (int j4 = 0; j4 < H / 4; ++j4) {
            const f32x4 h = *reinterpret_cast<const f32x4*>(&hb[lane * HP + 4 * j4]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f32x2 w = *reinterpret_cast<const f32x2*>(&w3i[2 * (4 * j4 + r)]);
                o = __builtin_elementwise_fma(w, f32x2{h[r], h[r]}, o);
            }
        }
        out0[si] = o.x;
        out1[si] = o.y;
        if (next) transpose();
    }
    // this lane's tick prices (loaded after the MLP: registers)
    const TickPrices px = load_prices(tk, ep.tick_off[e] + min(t0 + lane, T - 1));
    SGMM_TSTAMP(wslot, 2, out0[NSI - 1] + out1[0]);

    // ---- FPT step from every state, one lane per tick
    const bool valid = t0 + lane < T;
    __shared__ int32_t lut_s[4][2][32];
    int32_t* lut0 = lut_s[threadIdx.x >> 6][0];
    int32_t* lut1 = lut_s[threadIdx.x >> 6][1];
    if (ARL) {
        if (lane < ns) {
            int32_t da = 0, db = 0;
            if (ai >= 0) adv_delta(gsa, p, inv_min + (lane >> 2), (lane >> 1) & 1, lane & 1, da, db);
            lut0[lane] = da;
            lut1[lane] = db;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    uint64_t map = kIdentityMap;
    uint32_t traded = 0;
    uint64_t fw = 0;
    // [state][lane] rewards, staged in the activation buffer (the MLP is done
    // with it; the asm is a compiler memory barrier: float and double views of
    // the same LDS must not be reordered)
    double* rl = reinterpret_cast<double*>(hb);
    static_assert(NSI * 2 <= HP, "reward staging fits the activation buffer");
    asm volatile("" ::: "memory");
    if (valid) {
#pragma unroll
        for (int si = 0; si < NSI; ++si) {
            if (si >= nsi) break;
            const int32_t inv = inv_min + si;
            if (!ARL) {
                const StepOut so = policy_step(p, inv, out0[si], out1[si], px);
                map = (map & ~(0xFFull << (8 * si))) |
                      ((uint64_t)(si + so.fill_buy - so.fill_sell) << (8 * si));
                traded |= (uint32_t)(so.fill_buy | so.fill_sell) << si;
                rl[si * kWave + lane] = so.reward;
            } else {
                // own step: the 4 (previous fills) states of this inventory differ only by
                // the adversary's delta (wave-uniform: one adversary per episode); states
                // whose delta equals an earlier one's take that step's result
                // (adv_scale 1: deltas in {-1, 0, 1}, mostly shared)
                const int32_t oa = act_to_int(rintf(out0[si] * p.act_scale));  // drl_engine.py:38-39
                const int32_t ob = act_to_int(rintf(out1[si] * p.act_scale));
                int32_t dac[4], dbc[4], fc[4];
                double rc[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int s = 4 * si + c;
                    dac[c] = __builtin_amdgcn_readfirstlane(lut0[s]);
                    dbc[c] = __builtin_amdgcn_readfirstlane(lut1[s]);
                    int dup = -1;
#pragma unroll
                    for (int c2 = c - 1; c2 >= 0; --c2)
                        if (dac[c2] == dac[c] && dbc[c2] == dbc[c]) dup = c2;
                    if (dup < 0) {
                        const StepOut so = ftp_step(p, inv, (double)oa + (double)dac[c],
                                                    (double)ob + (double)dbc[c], px.mid, px.ask, px.bid,
                                                    px.bmax, px.smin);
                        rc[c] = so.reward;
                        fc[c] = so.fill_buy | (so.fill_sell << 1);
                    } else {
                        rc[c] = dup == 0 ? rc[0] : (dup == 1 ? rc[1] : rc[2]);
                        fc[c] = dup == 0 ? fc[0] : (dup == 1 ? fc[1] : fc[2]);
                    }
                    fw |= (uint64_t)fc[c] << (2 * s);
                    rew[s * ep.rs + row] = rc[c];  // per-state planes (SoA): coalesced rows
                }
            }
        }
    }
    if (ARL) {  // the fill codes (the scan derives the chunk transducers from them)
        if (valid) fills[row] = fw;
        return;
    }
    SGMM_TSTAMP(wslot, 3, map + traded);
    chunk_finish<NSI>(
        map, traded, valid, lane, nsi, rew, ep.rs, row, cmaps, ctr, chunk_base(ep.step_off[e], e) + chunk,
        [&](uint32_t st) { return rl[st * kWave + lane]; },
        [&](uint64_t excl) {
            SGMM_TSTAMP(wslot, 4, excl);
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        });
#ifdef SGMM_STAMPS
    SGMM_TSTAMP(wslot, 5, 0);
    SGMM_TSTAMP_REAL(wslot, 6);
#endif
}

// ------------------------------------------------------------------ table v3: one state per MFMA stream
// Same outputs and arithmetic as k_policy_table_mfma (no adversary),
// re-scheduled: one accumulator set; per inventory state a vector block
// (relu + LDS transpose of state si, layer 1 of si+1, layer 3 and the FPT step
// of si) and a pure MFMA block (layer 2 of si+1).  f32 MFMAs and vector ops of
// ONE wave do not overlap on gfx950 (tools/mb/mb_mfma_valu.hip), so the blocks
// are kept apart and the overlap comes from the other waves of the SIMD.
// Every lane computes every state (padded lanes read a clamped tick and are
// masked out of the maps afterwards).  (Round 2's alternative with two
// accumulator sets interleaved, "v3i", and this schedule for the adversary
// table measured slower: tools/experiments/round3_opt_in_paths.patch.)
template <int H, int NSI>
__global__ __launch_bounds__(kWave * 4, H <= 16 ? (NSI <= 5 ? 5 : 4) : 2) void k_policy_table_v3(
    sgmm_ticks tk, EpArrays ep, const sgmm_env_params* __restrict__ params, GenomeSrc src,
    int32_t inv_min, int32_t nsi, uint64_t* __restrict__ ctr, uint64_t* __restrict__ cmaps,
    double* __restrict__ rew) {
    static_assert(H <= 32, "v3 table: H = 16 or 32");
    using M = MlpMfma<H>;
    using L = GenomeLayout<H>;
    constexpr int NT = M::NT, KS = M::KS, HP = M::HP;
    const int e = blockIdx.y;
    const int32_t T = ep.len[e];
    const int wv = threadIdx.x >> 6;
    const int chunk = blockIdx.x * 4 + wv;
    const int32_t t0 = chunk * kChunk;
    if (blockIdx.x * 4 * kChunk >= T) return;  // block-uniform
    const int lane = threadIdx.x & (kWave - 1), grp = lane >> 4, col = lane & 15;
    const int64_t tb = ep.tick_off[e];
    // tick data requested before the genome staging so the loads overlap it
    // (indices clamped into the episode: padded samples are discarded)
    float xs0[4], xs1[4];
    M::load_signals(tk, col, [&](int smp) { return tb + min(t0 + smp, T - 1); }, xs0, xs1);
    const TickPrices px = load_prices(tk, tb + min(t0 + lane, T - 1));
    // the genome is staged in the reward buffer: it is dead once every wave
    // holds its weights in registers (the barrier below).  The LDS saved keeps
    // the H = 16 workgroup at 30.8 KB, so five fit a CU (96 VGPRs: five waves
    // per SIMD; config 2's table 21.3 -> 19.4 us)
    __shared__ __attribute__((aligned(16))) double rl_s[4][NSI][kWave];  // [state][lane] path-plane rewards
    static_assert(sizeof(rl_s) >= sizeof(float) * L::N, "genome fits the reward buffer");
    float* gsm = reinterpret_cast<float*>(&rl_s[0][0][0]);
    stage_genomes(src, e, ep.genome[e], -1, L::N, gsm, nullptr);
    __syncthreads();
    __shared__ __attribute__((aligned(16))) float w3i[2 * H];
    M::store_w3i(gsm, w3i);
    const float* g = gsm;
    float w2f[NT][KS];
    f32x4 b2c[NT];
    M::load_w2(g, grp, col, w2f, b2c);
    float w1s[KS], pre[4][KS];
    M::layer1_pre(g, grp, xs0, xs1, w1s, pre);
    const float b30 = g[L::B3], b31 = g[L::B3 + 1];
    __syncthreads();      // the genome is dead: rl_s holds rewards from here
    if (t0 >= T) return;  // wave-uniform; no block barriers below
#ifdef SGMM_STAMPS
    // slots: 7 realtime at entry, 0 start, 1 weights + layer 1 of state 0,
    // 2 states done, 3 map scan, 4 end, 5 / 6 summed MFMA / vector blocks
    const int wslot = e * (int)(gridDim.x * 4) + chunk;
    unsigned long long st_m = 0, st_v = 0, st_a, st_b;
#define SGMM_V3T(var) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory")
#endif
    SGMM_TSTAMP_REAL(wslot, 7);
    SGMM_TSTAMP(wslot, 0, 0);
    const sgmm_env_params p = params[ep.param[e]];
    __shared__ __attribute__((aligned(16))) float hb_s[4][kWave * HP];
    float* hb = hb_s[wv];
    double* rl = &rl_s[wv][0][0];

    f32x4 acc[4][NT];
    uint64_t map = kIdentityMap;
    uint32_t traded = 0;
    const bool valid = t0 + lane < T;
    const int64_t row = ep.step_off[e] + t0 + lane;
    auto layer3_env = [&](int si) {  // layer 3 of this lane's tick, then its FPT step from state si
        float o0 = b30, o1 = b31;
        M::layer3(hb, w3i, lane, o0, o1);
        const StepOut so = policy_step(p, inv_min + si, o0, o1, px);
        const bool live = si < nsi;  // states past the caps keep the identity byte
        const uint64_t to = live ? (uint64_t)(si + so.fill_buy - so.fill_sell) : (uint64_t)si;
        map = (map & ~(0xFFull << (8 * si))) | (to << (8 * si));
        traded |= (uint32_t)(live && (so.fill_buy | so.fill_sell)) << si;
        rl[si * kWave + lane] = so.reward;
    };
    {
        float h1[KS][4];
        auto layer1 = [&](int si) { M::layer1_state(w1s, pre, (float)((double)(inv_min + si) / 2.0), h1); };
        layer1(0);
        SGMM_TSTAMP(wslot, 1, h1[KS - 1][3] + pre[0][0] + w2f[0][0] + b2c[0][0]);
#ifdef SGMM_STAMPS
        SGMM_V3T(st_b);
#endif
        __builtin_amdgcn_sched_barrier(0);
        M::layer2(w2f, b2c, h1, acc);
#pragma unroll
        for (int si = 0; si < NSI; ++si) {
            __builtin_amdgcn_sched_barrier(0);
#ifdef SGMM_STAMPS
            SGMM_V3T(st_a);
            st_m += st_a - st_b;
#endif
            M::transpose(acc, hb, grp, col);
            if (si + 1 < NSI) layer1(si + 1);
            layer3_env(si);
            __builtin_amdgcn_sched_barrier(0);
#ifdef SGMM_STAMPS
            SGMM_V3T(st_b);
            st_v += st_b - st_a;
#endif
            if (si + 1 < NSI) M::layer2(w2f, b2c, h1, acc);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    SGMM_TSTAMP(wslot, 2, map + traded);
    if (!valid) {  // padded lanes: identity steps, no trades
        map = kIdentityMap;
        traded = 0;
    }
    chunk_finish<NSI>(
        map, traded, valid, lane, nsi, rew, ep.rs, row, cmaps, ctr, chunk_base(ep.step_off[e], e) + chunk,
        [&](uint32_t st) { return rl[st * kWave + lane]; }, [&](uint64_t excl) { SGMM_TSTAMP(wslot, 3, excl); });
#ifdef SGMM_STAMPS
    SGMM_TSTAMP(wslot, 4, 0);
    if (lane == 0 && wslot < kStampWaves) {
        g_tstamps[wslot][5] = st_m;
        g_tstamps[wslot][6] = st_v;
    }
#undef SGMM_V3T
#endif
}

// ------------------------------------------------------------------ walk order feedback
// A launch with whole walks and walks in halves (frontier_plan's four-walk
// rule, config 3: 1 024 whole + 1 536 in halves) ends with its heaviest whole
// walk: the walks of a GA-trained population differ in how long their paths
// stay apart, and the populations differ in how heavy their tails are
// (config 3 after 15 generations: the heaviest whole walk of population 0 ran
// 167 slots / 557 us, population 1's 116; every half walk ended by 430 us;
// profiles/r05_timeline/tlo_*).  After each training launch of
// sgmm_generation_multi_best this kernel ranks the populations by the heaviest
// episode they just ran -- a whole walk's slots x 5, an episode in halves the
// sum of its halves' slots x 4 (the halves' extra chunk starts: ~25 % more
// slots for the same episode) -- and rewrites the order so the next launch
// walks the lightest populations whole and cuts the heaviest into halves.
// Scheduling only: every result is per episode and independent of the order.
// (sgmm_populations::walk_order = NULL -- walk_feedback=False in the engine --
// keeps the caller's order; SGMM_PLAN_REORDER_WEIGHTS sets the two weights.)
// The job (ReorderJob, sgmm_rollout.h) rides along as one extra workgroup of
// the validation table launch that follows (k_policy_table_sp), which hides its
// ~6 us of latency; alone (k_walk_reorder) where that launch takes another path.
__device__ __forceinline__ void walk_reorder_block(const ReorderJob rj) {
    const uint32_t* __restrict__ wslots = rj.wslots;
    int32_t* __restrict__ order = rj.order;
    const int32_t n = rj.n, whole = rj.whole, gtail = rj.gtail, pop_eps = rj.pop_eps;
    const int nt = (int)blockDim.x;
    // an episode in gtail groups has chunks in the first ceil(nch / 64) only (the
    // frontier kernel writes no slot count for an empty group)
    const int cl = frontier_len(max(rj.len, 1), gtail);
    const int gused = min(gtail, (((rj.len + cl - 1) / cl) + kFrontierLanes - 1) / kFrontierLanes);
    __shared__ uint32_t score[kReorderMaxPops];
    __shared__ int32_t rank[kReorderMaxPops];
    const int npop = n / pop_eps;
    if ((int)threadIdx.x < npop) score[threadIdx.x] = 0;
    __syncthreads();
    // four positions per thread in flight: the order loads, then the slot loads (two
    // dependent load rounds per 4 096 positions instead of two per 1 024)
    constexpr int kPer = 4;
    for (int base = 0; base < n; base += nt * kPer) {
        int e[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int pos = base + j * nt + (int)threadIdx.x;
            e[j] = pos < n ? order[pos] : -1;
        }
        uint32_t sc[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {  // the episode's walks' slots at wslots[e * gtail + g]
            const int pos = base + j * nt + (int)threadIdx.x;
            sc[j] = 0;
            if (e[j] < 0) continue;
            if (pos < whole) {
                sc[j] = rj.w_whole * wslots[e[j] * gtail];
            } else {
                uint32_t sum = 0;
                for (int g = 0; g < gused; ++g) sum += wslots[e[j] * gtail + g];
                sc[j] = rj.w_split * sum;
            }
        }
        // one LDS atomic per wave where its 64 positions are one population (the usual
        // case: the order is population blocks), per lane otherwise
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int k = e[j] < 0 ? -1 : e[j] / pop_eps;
            const int k0 = __builtin_amdgcn_readfirstlane(k);
            if (__all(k == k0)) {
                uint32_t m = sc[j];
#pragma unroll
                for (int d = 1; d < kWave; d <<= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, kWave));
                if ((threadIdx.x & (kWave - 1)) == 0 && k0 >= 0) atomicMax(&score[k0], m);
            } else if (k >= 0) {
                atomicMax(&score[k], sc[j]);
            }
        }
    }
    __syncthreads();  // every read of the old order precedes the writes below
    if (threadIdx.x == 0) {  // populations by (score, index), lightest first
        for (int k = 0; k < npop; ++k) rank[k] = k;
        for (int i = 1; i < npop; ++i)
            for (int j = i; j > 0 && score[rank[j]] < score[rank[j - 1]]; --j) {
                const int t = rank[j];
                rank[j] = rank[j - 1];
                rank[j - 1] = t;
            }
    }
    __syncthreads();
    for (int pos = threadIdx.x; pos < n; pos += blockDim.x) order[pos] = rank[pos / pop_eps] * pop_eps + pos % pop_eps;
}
__global__ __launch_bounds__(1024) void k_walk_reorder(ReorderJob rj) { walk_reorder_block(rj); }
// ------------------------------------------------------------------ table, one state per wave (small launches)
// The v3 table's arithmetic with its state loop spread over the workgroup: one
// workgroup per 64-tick chunk, wave si runs layers 1-3 and the FPT step from
// inventory state si, and wave 0 assembles the chunk's map, path planes and
// trade counts from the states' successor bytes and rewards in LDS.  For
// launches with few chunks (the validation rollouts: 5 x 15 chunks at config
// 3) the v3 wave's serial five-state chain is the launch's latency; here it is
// one state deep.  Outputs are identical to v3's (same per-tick arithmetic).
template <int H, int NSI>
__global__ __launch_bounds__(kWave * NSI) void k_policy_table_sp(
    sgmm_ticks tk, EpArrays ep, const sgmm_env_params* __restrict__ params, GenomeSrc src,
    int32_t inv_min, int32_t nsi, uint64_t* __restrict__ ctr, uint64_t* __restrict__ cmaps,
    double* __restrict__ rew, ReorderJob rj) {
    static_assert(H <= 32, "state-parallel table: H = 16 or 32");
    using M = MlpMfma<H>;
    using L = GenomeLayout<H>;
    constexpr int NT = M::NT, KS = M::KS, HP = M::HP;
    if (rj.order && blockIdx.y == gridDim.y - 1) {  // the extra workgroup: the walk-order job
        if (blockIdx.x == 0) walk_reorder_block(rj);
        return;
    }
    const int e = blockIdx.y;
    const int32_t T = ep.len[e];
    const int chunk = blockIdx.x;
    const int32_t t0 = chunk * kChunk;
    if (t0 >= T) return;  // block-uniform
    const int si = threadIdx.x >> 6;  // this wave's inventory state (blockDim = 64 nsi)
    const int lane = threadIdx.x & (kWave - 1), grp = lane >> 4, col = lane & 15;
    const int64_t tb = ep.tick_off[e];
    float xs0[4], xs1[4];
    M::load_signals(tk, col, [&](int smp) { return tb + min(t0 + smp, T - 1); }, xs0, xs1);
    const TickPrices px = load_prices(tk, tb + min(t0 + lane, T - 1));
    __shared__ __attribute__((aligned(16))) float gsm[L::N];
    __shared__ __attribute__((aligned(16))) float w3i[2 * H];
    __shared__ __attribute__((aligned(16))) float hb_s[NSI][kWave * HP];
    __shared__ __attribute__((aligned(16))) double rl_s[NSI][kWave];  // [state][lane] rewards
    __shared__ uint8_t to_s[NSI][kWave];                              // pack_step of [state][lane]
    stage_genomes(src, e, ep.genome[e], -1, L::N, gsm, nullptr);
    __syncthreads();
    M::store_w3i(gsm, w3i);
    const float* g = gsm;
    float w2f[NT][KS];
    f32x4 b2c[NT];
    M::load_w2(g, grp, col, w2f, b2c);
    float h1[KS][4];
    M::layer1(g, grp, xs0, xs1, (float)((double)(inv_min + si) / 2.0), h1);
    float o0 = g[L::B3], o1 = g[L::B3 + 1];
    __syncthreads();  // w3i complete
    const sgmm_env_params p = params[ep.param[e]];
    float* hb = hb_s[si];
    f32x4 acc[4][NT];
    M::layer2(w2f, b2c, h1, acc);
    M::transpose(acc, hb, grp, col);
    M::layer3(hb, w3i, lane, o0, o1);
    const StepOut so = policy_step(p, inv_min + si, o0, o1, px);
    to_s[si][lane] = pack_step(si, so);
    rl_s[si][lane] = so.reward;
    __syncthreads();
    if (si != 0) return;
    // wave 0: the chunk's map, path planes and trade counts (v3's tail)
    const bool valid = t0 + lane < T;
    uint64_t map = kIdentityMap;
    uint32_t traded = 0;
    if (valid) unpack_steps(to_s, lane, nsi, map, traded);
    chunk_finish<NSI>(map, traded, valid, lane, nsi, rew, ep.rs, ep.step_off[e] + t0 + lane, cmaps, ctr,
                      chunk_base(ep.step_off[e], e) + chunk, [&](uint32_t st) { return rl_s[st][lane]; });
}

#undef SGMM_TSTAMP
#undef SGMM_TSTAMP_REAL

// ------------------------------------------------------------------ launches
void launch_walk_reorder(const ReorderJob& job, hipStream_t s) {
    SGMM_LAUNCH(k_walk_reorder, dim3(1), dim3(kScanThreads), 0, s, job);
}

void launch_policy_table(PolicyKernel kind, int hidden, bool arl, int nsi, int max_len, int n_ep,
                         const sgmm_ticks& tk, const EpArrays& ep, const sgmm_env_params* params,
                         const GenomeSrc& src, int32_t inv_min, uint64_t* ctr, uint64_t* cmaps, uint64_t* fills,
                         double* rew, const ReorderJob* rj, hipStream_t s) {
    const int nch = (max_len + kChunk - 1) / kChunk;
    if (kind == PolicyKernel::TableValu) {  // one workgroup per chunk, one wave per inventory state
        const dim3 grid(nch, n_ep), block(kChunk * nsi);
        with_int<8, 16, 32, 64>(hidden, [&](auto h) {
            constexpr int H = decltype(h)::value;
            if (arl)
                SGMM_LAUNCH((k_policy_table<H, 8, true>), grid, block, 0, s, tk, ep, params, src, inv_min, nsi, ctr,
                            cmaps, fills, rew);
            else
                with_int<5, 8>(nsi <= 5 ? 5 : 8, [&](auto n) {
                    SGMM_LAUNCH((k_policy_table<H, decltype(n)::value, false>), grid, block, 0, s, tk, ep, params,
                                src, inv_min, nsi, ctr, cmaps, fills, rew);
                });
        });
        return;
    }
    // the MFMA tables: TableSp and TableV3 for H = 16 / 32 without the adversary,
    // TableMfma for H = 64 and the adversary path
    const dim3 grid((nch + 3) / 4, n_ep), block(kWave * 4);  // 4 chunks (waves) per block
    with_int<16, 32, 64>(hidden, [&](auto h) {
        with_int<5, 8>(nsi <= 5 ? 5 : 8, [&](auto n) {
            constexpr int H = decltype(h)::value, NSI = decltype(n)::value;
            if constexpr (H <= 32) {
                if (kind == PolicyKernel::TableSp) {
                    // rj (may be null): a walk-order job to run as the table's extra workgroup
                    const ReorderJob job = rj ? *rj : ReorderJob{nullptr, nullptr, 0, 0, 0, 1};
                    const dim3 g2(nch, n_ep + (job.order ? 1 : 0)), b2(kWave * nsi);  // one workgroup per chunk, one wave per state
                    SGMM_LAUNCH((k_policy_table_sp<H, NSI>), g2, b2, 0, s, tk, ep, params, src, inv_min, nsi, ctr,
                                cmaps, rew, job);
                    return;
                }
                if (kind == PolicyKernel::TableV3) {
                    SGMM_LAUNCH((k_policy_table_v3<H, NSI>), grid, block, 0, s, tk, ep, params, src, inv_min, nsi,
                                ctr, cmaps, rew);
                    return;
                }
            }
            with_bool(arl, [&](auto a) {
                SGMM_LAUNCH((k_policy_table_mfma<H, NSI, decltype(a)::value>), grid, block, 0, s, tk, ep, params,
                            src, inv_min, nsi, ctr, cmaps, fills, rew);
            });
        });
    });
}

}  // namespace sgmm

#ifdef SGMM_STAMPS
extern "C" int sgmm_debug_thwid(unsigned int* host, int n_waves) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(sgmm::g_thwid), sizeof(unsigned int) * 2 * n_waves);
}
extern "C" int sgmm_debug_tstamps(unsigned long long* host, int n_waves) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(sgmm::g_tstamps), sizeof(unsigned long long) * 8 * n_waves);
}
#endif
