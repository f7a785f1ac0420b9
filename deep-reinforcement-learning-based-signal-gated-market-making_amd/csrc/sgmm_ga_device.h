// sgmm_ga_device.h -- the generation boundary as device code, shared by the
// standalone GA kernels (sgmm_ga.hip) and the tails inside the rollout launches
// (sgmm_scan.hip: tail_run and validation_tail; sgmm_scan.h: population_arrive
// of the lanes scan and of the frontier's fused scan).
//
// Each piece of the boundary's semantics is here once, cut the way the model
// tests/ga_model.py is: tell_commit (ga_model.tell's record), val_commit
// (ga_model.val_update) on a GaSnap of the state, hist_row, regen4 (master <-
// ask(best)), and better / argmax_merge / argmax_key under every argmax.  The
// three argmax schedules -- block_argmax2, ga_step_fused's with its payload,
// tell_wave's blocked loads -- are measured designs and stay apart.
//
// Reference: NeuroEvolution.tell (models/model.py:73-76) and the validation /
// sigma-decay block of DRLEngine.train (Env/drl_engine.py:119-171).
#pragma once

#include "sgmm_device.h"

namespace sgmm {

constexpr int kStepBlock = 1024;

// ---------------------------------------------------------------- records and argmax
// Loads of the fitness records.  HANDOFF: they were stored in this launch by
// other workgroups with write-through (sc1) stores, so every load of them is a
// global sc1 load (MI355X_MICROARCH.md, inter-workgroup visibility, row 1:
// one storing lane per workgroup, agent-scope arrival ticket, the last
// arriver loads) -- no acquire fence, no L2 invalidate.
template <bool HANDOFF, class T>
__device__ __forceinline__ T ld_rec(const T* p) {
    if constexpr (HANDOFF) {
        typedef __attribute__((address_space(1))) const T gT;
        return __hip_atomic_load((gT*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        return *p;
    }
}

// individual i's record in a ShardView
template <bool HANDOFF, class T>
__device__ __forceinline__ T shard_ld(const T* __restrict__ base, ShardView v, int i) {
    if (v.n <= 0) return ld_rec<HANDOFF>(base + i);
    const char* q = reinterpret_cast<const char*>(base) + (int64_t)(i / v.n) * v.stride;
    return ld_rec<HANDOFF>(reinterpret_cast<const T*>(q) + i % v.n);
}

__device__ __forceinline__ void argmax_merge(double& bv, int& bi, double ov, int oi) {
    const bool take = oi >= 0 && (bi < 0 || better(ov, oi, bv, bi));
    bv = take ? ov : bv;
    bi = take ? oi : bi;
}

// order-preserving unsigned key: -0 == +0, NaN above everything
__device__ __forceinline__ uint64_t argmax_key(double f) {
    if (f != f) return ~0ull;
    const uint64_t b = (uint64_t)__double_as_longlong(f == 0.0 ? 0.0 : f);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}

// wave maximum / minimum (wave_ladder: integer data only), uniform
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
    return readlane64(wave_ladder(v, (uint64_t)0, [](uint64_t t, uint64_t x) { return t > x ? t : x; }), kWave - 1);
}
__device__ __forceinline__ int wave_min_i32(int v) {
    return __builtin_amdgcn_readlane(wave_ladder(v, INT32_MAX, [](int t, int x) { return t < x ? t : x; }), kWave - 1);
}

// np.argmax over one wave (first index on ties, NaN first), lanes with
// valid: a key maximum, a ballot of the lanes equal to it.  Returns the
// winning lane (-1: no valid lane) and its value.
__device__ __forceinline__ int wave_argmax_first(double f, bool valid, double& bv) {
    const uint64_t k = valid ? argmax_key(f) : 0ull;
    const uint64_t m = wave_max_u64(k);
    const uint64_t hit = __ballot(valid && k == m);
    const int l = hit ? __ffsll((unsigned long long)hit) - 1 : -1;
    bv = __longlong_as_double((long long)readlane64((uint64_t)__double_as_longlong(f), l < 0 ? 0 : l));
    return l;
}

// first index of the largest key over the wave (lane candidates (key, idx),
// idx < 0: none); -1 when no lane has a candidate
__device__ __forceinline__ int wave_best_index(uint64_t key, int idx) {
    const uint64_t m = wave_max_u64(idx >= 0 ? key : 0ull);  // valid keys are > 0
    const int c = wave_min_i32(idx >= 0 && key == m ? idx : INT32_MAX);
    return c == INT32_MAX ? -1 : c;
}

// np.argmax of fit and of -fit (first index on ties, NaN first) over the
// workgroup: strided scan, wave shuffles, one LDS round over the waves.
// LDS scratch: sv[2*nt] doubles, si[2*nt] ints.
template <bool HANDOFF>
__device__ void block_argmax2(const double* __restrict__ fit, ShardView sv_, int P, int& best,
                              int& abest, double* sv, int* si) {
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const int nw = (nt + kWave - 1) / kWave;
    double bv = 0.0, av = 0.0;
    int bi = -1, aj = -1;
    for (int i = tid; i < P; i += nt) {
        const double f = shard_ld<HANDOFF>(fit, sv_, i);
        argmax_merge(bv, bi, f, i);
        argmax_merge(av, aj, -f, i);
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const double ob = __shfl_down(bv, off, kWave), oa = __shfl_down(av, off, kWave);
        const int oib = __shfl_down(bi, off, kWave), oia = __shfl_down(aj, off, kWave);
        argmax_merge(bv, bi, ob, oib);
        argmax_merge(av, aj, oa, oia);
    }
    if (lane == 0) {
        sv[wv] = bv;
        si[wv] = bi;
        sv[nt + wv] = av;
        si[nt + wv] = aj;
    }
    __syncthreads();
    if (wv == 0) {
        bv = lane < nw ? sv[lane] : 0.0;
        bi = lane < nw ? si[lane] : -1;
        av = lane < nw ? sv[nt + lane] : 0.0;
        aj = lane < nw ? si[nt + lane] : -1;
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            const double ob = __shfl_down(bv, off, kWave), oa = __shfl_down(av, off, kWave);
            const int oib = __shfl_down(bi, off, kWave), oia = __shfl_down(aj, off, kWave);
            argmax_merge(bv, bi, ob, oib);
            argmax_merge(av, aj, oa, oia);
        }
        if (lane == 0) {
            si[0] = bi;
            si[nt] = aj;
        }
    }
    __syncthreads();
    best = si[0];
    abest = si[nt];
}

// ---------------------------------------------------------------- master <- ask(best)
__device__ __forceinline__ void load4(const float* __restrict__ master, int64_t n, int64_t k4, float (&m)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) m[q] = 4 * k4 + q < n ? master[4 * k4 + q] : 0.0f;
}

// parameters 4 k4 .. 4 k4 + 3 of master <- ask(best), from their current values
// m (read before they are overwritten); the new values into copy too when given
__device__ __forceinline__ void regen4(float* __restrict__ master, float* copy, int64_t n, int64_t k4,
                                       const float (&m)[4], float sig, uint64_t seed, uint32_t sid,
                                       uint32_t gen, int best) {
    float z[4];
    normal4(seed, sid, gen, (uint32_t)best, (uint32_t)k4, z);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (4 * k4 + q < n) {
            const float v = ask1(m[q], z[q], sig);
            master[4 * k4 + q] = v;
            if (copy) copy[4 * k4 + q] = v;
        }
}

// by every thread of the workgroup, 4 parameters a thread at a time.  copy:
// ga_step_dev's LDS stage for the next ask; none for the deferred half of the
// tell (validation_tail) and for k_ga_tell
__device__ __forceinline__ void regen_master_block(float* __restrict__ master, float* copy, int64_t n, float sig,
                                                   uint64_t seed, uint32_t sid, uint32_t gen, int best) {
    for (int64_t k4 = threadIdx.x; 4 * k4 < n; k4 += blockDim.x) {
        float m[4];
        load4(master, n, k4, m);
        regen4(master, copy, n, k4, m, sig, seed, sid, gen, best);
    }
}

// dst[0..n) <- src[0..n) by the workgroup
__device__ __forceinline__ void copy_row(float* __restrict__ dst, const float* src, int64_t n) {
    for (int64_t k = threadIdx.x; k < n; k += blockDim.x) dst[k] = src[k];
}

__device__ void ask_rows(const float* lds_master, int64_t n, float sig, uint64_t seed,
                         uint32_t sid, uint32_t gen, int32_t i0, int32_t cnt,
                         float* __restrict__ out) {
    const int64_t nk4 = (n + 3) / 4;
    for (int64_t g = threadIdx.x; g < nk4 * cnt; g += blockDim.x) {
        const int32_t i = (int32_t)(g / nk4);
        const int64_t k4 = g - (int64_t)i * nk4;
        float v[4];
        ask_row4(lds_master, n, sig, seed, sid, gen, (uint32_t)(i0 + i), k4, v);
        for (int q = 0; q < 4; ++q)
            if (4 * k4 + q < n) out[(int64_t)i * n + 4 * k4 + q] = v[q];
    }
}

// ---------------------------------------------------------------- the boundary's bookkeeping
// row `gen` of a population's history, or null
__device__ __forceinline__ sgmm_ga_history* hist_row(sgmm_ga_history* history, int32_t gen, int32_t cap) {
    return history && gen < cap ? history + gen : nullptr;
}

// The state words a boundary reads, as values: a caller loads them where its
// schedule wants them (ga_step_fused: with its other up-front loads).
struct GaSnap {
    int32_t gen, no_improve, patience;
    double sigma_mm, sigma_adv, best_val, decay;
};
__device__ __forceinline__ GaSnap ga_snap(const sgmm_ga_state* st) {
    return GaSnap{st->gen, st->no_improve, st->patience, st->sigma_mm, st->sigma_adv, st->best_val, st->decay};
}

// The tell's record (ga_model.tell; drl_engine.py:119-128): best / adversary
// indices, the best's training record, the history row's training fields.
// One thread.
__device__ __forceinline__ void tell_commit(sgmm_ga_state* __restrict__ st, sgmm_ga_history* __restrict__ hist,
                                            int best, int abest, double tf, int32_t ttr) {
    st->best_idx = best;
    st->adv_best_idx = abest;
    st->last_train_f = tf;
    if (hist) {
        hist->train_f = tf;
        hist->train_trades = ttr;
        hist->best_idx = best;
    }
}

// strictly greater: a tie and NaN never improve (drl_engine.py:130-131)
__device__ __forceinline__ int val_improves(double v, double best_val) { return v > best_val; }

// The validation bookkeeping (ga_model.val_update; drl_engine.py:129-160) on the
// validation record v / vtr of the post-tell master: best_val on improvement,
// sigma decay after `patience` generations without one, the history row's
// validation fields, gen + 1.  One thread; the caller copies the checkpoint.
struct ValOut {
    int improved;
    double sigma_mm, sigma_adv;  // after the decay
};
__device__ __forceinline__ ValOut val_commit(sgmm_ga_state* __restrict__ st, sgmm_ga_history* __restrict__ hist,
                                             const GaSnap& s, double v, int32_t vtr) {
    const int improved = val_improves(v, s.best_val);
    int32_t no_improve = improved ? 0 : s.no_improve + 1;
    double smm = s.sigma_mm, sadv = s.sigma_adv;
    int decayed = 0;
    if (no_improve >= s.patience) {  // drl_engine.py:155-160
        smm *= s.decay;
        sadv *= s.decay;
        no_improve = 0;
        decayed = 1;
    }
    if (improved) st->best_val = v;
    st->sigma_mm = smm;
    st->sigma_adv = sadv;
    st->no_improve = no_improve;
    st->improved = improved;
    st->decayed = decayed;
    st->last_val_f = v;
    st->gen = s.gen + 1;
    if (hist) {
        hist->val_f = v;
        hist->val_trades = vtr;
        hist->sigma_after = smm;
        hist->flags = improved | (decayed << 1);
    }
    return ValOut{improved, smm, sadv};
}

// val_commit and the checkpoint copy master -> best_master on improvement, by
// one workgroup: every thread calls (v identical in all); `flag` is one int of
// LDS scratch.
__device__ __forceinline__ void val_update_dev(sgmm_ga_state* __restrict__ st, double v, int32_t vtr,
                                               const float* __restrict__ master, float* __restrict__ best_master,
                                               int64_t n, sgmm_ga_history* __restrict__ history,
                                               int32_t hist_cap, int* flag) {
    if (threadIdx.x == 0) {
        const GaSnap s = ga_snap(st);
        *flag = val_commit(st, hist_row(history, s.gen, hist_cap), s, v, vtr).improved;
    }
    __syncthreads();
    if (*flag && best_master) copy_row(best_master, master, n);
}

// One generation boundary, executed by one whole workgroup (power-of-two
// size): tell both evolvers, validation bookkeeping, sigma decay, history
// row, and optionally the next generation's ask of [i0, i0+n).  tell_only: the
// tell alone (sgmm_ga_tell_multi; the validation follows in its own launches).
// LDS scratch: sv[2*nt] doubles, si[2*nt] ints, lm[n_mm], la[n_adv] floats.
// HANDOFF: the fitness records come from other workgroups of this launch
// (sc1 loads, see ld_rec).
template <bool HANDOFF>
__device__ void ga_step_dev(sgmm_ga_state* __restrict__ st, const double* __restrict__ fit,
                            const int32_t* __restrict__ trades, const double* __restrict__ vfit,
                            const int32_t* __restrict__ vtrades, int32_t P, ShardView shard,
                            float* __restrict__ master, float* __restrict__ master_adv,
                            float* __restrict__ best_master, int64_t n_mm, int64_t n_adv,
                            uint64_t seed, sgmm_ga_history* __restrict__ history, int32_t hist_cap,
                            float* __restrict__ next_mm, float* __restrict__ next_adv, int32_t i0,
                            int32_t n, double* sv, int* si, float* lm, float* la, bool tell_only = false) {
    const GaSnap s = ga_snap(st);
    const uint32_t gen = (uint32_t)s.gen;
    int best, abest;
    block_argmax2<HANDOFF>(fit, shard, P, best, abest, sv, si);
    __syncthreads();  // sv/si are reused below
    // tell (model.py:73-76; drl_engine.py:119-125), the new masters staged for the next ask
    regen_master_block(master, lm, n_mm, (float)s.sigma_mm, seed, 0u, gen, best);
    if (master_adv) regen_master_block(master_adv, la, n_adv, (float)s.sigma_adv, seed, 1u, gen, abest);
    if (threadIdx.x == 0) {  // every load issued before the first dependent use
        const bool val = !tell_only;
        const double tf = shard_ld<HANDOFF>(fit, shard, best);
        const double v = val ? shard_ld<HANDOFF>(vfit, shard, best) : 0.0;
        const int32_t ttr = trades ? shard_ld<HANDOFF>(trades, shard, best) : 0;
        const int32_t vtr = val && vtrades ? shard_ld<HANDOFF>(vtrades, shard, best) : 0;
        sgmm_ga_history* hist = hist_row(history, s.gen, hist_cap);
        tell_commit(st, hist, best, abest, tf, ttr);
        if (val) {  // validation of the best (drl_engine.py:129-171)
            const ValOut o = val_commit(st, hist, s, v, vtr);
            si[0] = o.improved;
            sv[0] = o.sigma_mm;
            sv[1] = o.sigma_adv;
        }
    }
    if (tell_only) return;
    __syncthreads();
    if (si[0] && best_master) copy_row(best_master, lm, n_mm);
    // ask of the next generation (model.py:65-71) from the new master / sigma
    if (next_mm) ask_rows(lm, n_mm, (float)sv[0], seed, 0u, gen + 1, i0, n, next_mm);
    if (next_adv && master_adv) ask_rows(la, n_adv, (float)sv[1], seed, 1u, gen + 1, i0, n, next_adv);
}

// The fused generation tail's GA step (sgmm_generation: one workgroup, the
// records contiguous, P <= blockDim.x).  The same results as ga_step_dev, laid
// out for latency: every record (sc1), the masters and the state are loaded up
// front, the argmax carries the best individual's validation record through its
// shuffles, and the masters are regenerated from registers.
constexpr int kTailSlots = 4;  // float4 master chunks per thread (n <= 16 * blockDim.x)

#ifdef SGMM_STAMPS
static __device__ unsigned long long g_tail[8];  // diagnostic build: tail phase times (thread 0)
#endif
#if defined(SGMM_STAMPS) && !defined(SGMM_NO_TAIL_STAMPS)
// the clock when `dep` is available (its register dependency only: no memory
// wait), kept in registers and stored once at the end (SGMM_TAIL_FLUSH)
#define SGMM_TAIL_DECL unsigned long long tt_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define SGMM_TAIL_STAMP(k, dep) \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tt_[k]) : "v"(dep) : "memory")
#define SGMM_TAIL_FLUSH                                         \
    do {                                                        \
        if (threadIdx.x == 0)                                   \
            for (int k_ = 0; k_ < 8; ++k_) g_tail[k_] = tt_[k_]; \
    } while (0)
#else
#define SGMM_TAIL_DECL
#define SGMM_TAIL_STAMP(k, dep) \
    do {                        \
    } while (0)
#define SGMM_TAIL_FLUSH \
    do {                \
    } while (0)
#endif

__device__ __forceinline__ void argmax_merge_p(double& bv, int& bi, double& pv, int& pt, int& pvt,
                                               double ov, int oi, double opv, int opt, int opvt) {
    const bool take = oi >= 0 && (bi < 0 || better(ov, oi, bv, bi));
    bv = take ? ov : bv;
    bi = take ? oi : bi;
    pv = take ? opv : pv;
    pt = take ? opt : pt;
    pvt = take ? opvt : pvt;
}

__device__ __forceinline__ void load_master4(const float* __restrict__ m, int64_t n,
                                             float (&r)[kTailSlots][4]) {
#pragma unroll
    for (int j = 0; j < kTailSlots; ++j) load4(m, n, threadIdx.x + (int64_t)j * blockDim.x, r[j]);
}

// master <- ask(best) from the registers m; also into best_copy when given
// (the validation improved: the checkpoint copy, drl_engine.py:133-137)
__device__ __forceinline__ void regen_master_regs(float* __restrict__ master, float* __restrict__ best_copy,
                                                  int64_t n, const float (&m)[kTailSlots][4],
                                                  float sig, uint64_t seed, uint32_t sid,
                                                  uint32_t gen, int best) {
#pragma unroll
    for (int j = 0; j < kTailSlots; ++j) {
        const int64_t k4 = threadIdx.x + (int64_t)j * blockDim.x;
        if (4 * k4 >= n) break;
        regen4(master, best_copy, n, k4, m[j], sig, seed, sid, gen, best);
    }
}

template <bool HANDOFF>
__device__ void ga_step_fused(sgmm_ga_state* __restrict__ st, const double* __restrict__ fit,
                              const int32_t* __restrict__ trades, const double* __restrict__ vfit,
                              const int32_t* __restrict__ vtrades, int32_t P,
                              float* __restrict__ master, float* __restrict__ master_adv,
                              float* __restrict__ best_master, int64_t n_mm, int64_t n_adv,
                              uint64_t seed, sgmm_ga_history* __restrict__ history, int32_t hist_cap,
                              double* sv, int* si) {
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const int nw = (nt + kWave - 1) / kWave;
    SGMM_TAIL_DECL
    // ---- every load first
    double f = 0.0, vf = 0.0;
    int tr = 0, vtr = 0;
    const bool mine = tid < P;
    if (mine) {
        f = ld_rec<HANDOFF>(fit + tid);
        vf = ld_rec<HANDOFF>(vfit + tid);
        if (trades) tr = ld_rec<HANDOFF>(trades + tid);
        if (vtrades) vtr = ld_rec<HANDOFF>(vtrades + tid);
    }
    float mm[kTailSlots][4], ma[kTailSlots][4];
    load_master4(master, n_mm, mm);
    if (master_adv) load_master4(master_adv, n_adv, ma);
    const GaSnap s = ga_snap(st);
    const uint32_t gen = (uint32_t)s.gen;
    const float sig_mm = (float)s.sigma_mm, sig_adv = (float)s.sigma_adv;
    SGMM_TAIL_STAMP(0, f + vf + mm[0][0] + sig_mm);
    // ---- argmax of fit (payload: the validation record) and of -fit: the
    // waves holding records reduce with shuffles, every thread merges their
    // results from LDS
    const int nwa = (P + kWave - 1) / kWave;
    double bv = f, pv = vf, av = -f;
    int bi = mine ? tid : -1, pt = tr, pvt = vtr, aj = bi;
    if (wv < nwa) {
        const int bl = wave_argmax_first(f, mine, bv);
        const int al = wave_argmax_first(-f, mine, av);
        const int src = bl < 0 ? 0 : bl;  // wave-uniform
        pv = __longlong_as_double((long long)readlane64((uint64_t)__double_as_longlong(vf), src));
        pt = __builtin_amdgcn_readlane(tr, src);
        pvt = __builtin_amdgcn_readlane(vtr, src);
        bi = bl < 0 ? -1 : wv * kWave + bl;
        aj = al < 0 ? -1 : wv * kWave + al;
        // per-wave results: sv[0..nw) best, sv[nw..2nw) its validation fitness, sv[2nw..3nw)
        // adversary; si[0..nw) best idx, si[nw..2nw) trades, si[2nw..3nw) val trades,
        // si[3nw..4nw) adversary idx
        if (lane == 0) {
            sv[wv] = bv;
            sv[nw + wv] = pv;
            sv[2 * nw + wv] = av;
            si[wv] = bi;
            si[nw + wv] = pt;
            si[2 * nw + wv] = pvt;
            si[3 * nw + wv] = aj;
        }
    }
    SGMM_TAIL_STAMP(6, bv);
    __syncthreads();
    SGMM_TAIL_STAMP(7, bv);
    bv = sv[0];
    pv = sv[nw];
    av = sv[2 * nw];
    bi = si[0];
    pt = si[nw];
    pvt = si[2 * nw];
    aj = si[3 * nw];
    for (int w = 1; w < nwa; ++w) {
        argmax_merge_p(bv, bi, pv, pt, pvt, sv[w], si[w], sv[nw + w], si[nw + w], si[2 * nw + w]);
        argmax_merge(av, aj, sv[2 * nw + w], si[3 * nw + w]);
    }
    const int best = bi, abest = aj;
    // every thread knows whether the validation improved
    const int improved = val_improves(pv, s.best_val);
    SGMM_TAIL_STAMP(1, best + abest);
    // ---- tell (model.py:73-76; drl_engine.py:119-125), the checkpoint copy
    // of the new master written in the same pass
    regen_master_regs(master, improved ? best_master : nullptr, n_mm, mm, sig_mm, seed, 0u, gen, best);
    if (master_adv) regen_master_regs(master_adv, nullptr, n_adv, ma, sig_adv, seed, 1u, gen, abest);
    SGMM_TAIL_STAMP(2, mm[0][0]);
    if (tid == 0) {  // the tell's record, the validation of the best (drl_engine.py:129-171)
        sgmm_ga_history* hist = hist_row(history, s.gen, hist_cap);
        tell_commit(st, hist, best, abest, bv, pt);
        val_commit(st, hist, s, pv, pvt);
    }
    SGMM_TAIL_STAMP(4, improved);
    SGMM_TAIL_FLUSH;
}

// The tell's argmax and record by ONE WAVE (the last arriver of the lanes and
// fused scans, wave 0 of the scan workgroups; StepArgs mode kStepArgmax): lane l
// holds records l, l + 64, ... (loaded 16 at a time, sc1), the wave's argmax is
// a DPP maximum of the order-preserving key and a DPP minimum of the index among
// equal keys (np.argmax: first index, NaN first), and the best's training record
// comes from its lane's registers.  master <- ask(best) follows in the
// validation launch's tail (regen_master_block).  Same indices and record as
// ga_step_dev.
constexpr int kWaveRec = 16;  // records per lane loaded together

template <bool HANDOFF>
__device__ void tell_wave(sgmm_ga_state* __restrict__ st, const double* __restrict__ fit,
                          const int32_t* __restrict__ trades, int32_t P,
                          sgmm_ga_history* __restrict__ history, int32_t hist_cap) {
    const int lane = threadIdx.x & (kWave - 1);
    const int32_t gen = st->gen;
    // this lane's best (ascending indices: the first wins ties) for fit and
    // -fit, over blocks of kWaveRec records per lane, each block's loads issued
    // together
    double bv = 0.0, av = 0.0;
    int bi = -1, aj = -1;
    int32_t btr = 0;
    for (int r0 = 0; r0 * kWave < P; r0 += kWaveRec) {
        double f[kWaveRec];
        int32_t tr[kWaveRec];
#pragma unroll
        for (int r = 0; r < kWaveRec; ++r) {
            const int i = lane + (r0 + r) * kWave;
            f[r] = i < P ? ld_rec<HANDOFF>(fit + i) : 0.0;
            tr[r] = (i < P && trades) ? ld_rec<HANDOFF>(trades + i) : 0;
        }
#pragma unroll
        for (int r = 0; r < kWaveRec; ++r) {
            const int i = lane + (r0 + r) * kWave;
            if (i < P) {
                const bool tb = bi < 0 || better(f[r], i, bv, bi);
                bv = tb ? f[r] : bv;
                btr = tb ? tr[r] : btr;
                bi = tb ? i : bi;
                argmax_merge(av, aj, -f[r], i);
            }
        }
    }
    const int best = wave_best_index(argmax_key(bv), bi);
    const int abest = wave_best_index(argmax_key(av), aj);
    const int src = (best < 0 ? 0 : best) & (kWave - 1);
    const double tf = __longlong_as_double((long long)readlane64((uint64_t)__double_as_longlong(bv), src));
    const int32_t ttr = __builtin_amdgcn_readlane(btr, src);
    if (lane == 0) tell_commit(st, hist_row(history, gen, hist_cap), best, abest, tf, ttr);
}

}  // namespace sgmm
