// sgmm_scan.h -- the path scan's device pieces, written once.
//
// The second half of a fitness launch turns the policy kernel's chunk records
// into episode records: chunk start states from the chunk maps, the trades and
// the rewards along the path, the reference's sequential float64 sum
// (drl_engine.py:53-54: total = ((0 + r0) + r1) + ...), the idle penalty
// (drl_engine.py:64-65) and, when the launch ends the generation, the tell of
// a population whose last record has arrived.  The scan kernels (k_path_scan,
// k_path_scan_lanes, k_path_scan_arl in sgmm_scan.hip) and the frontier walk
// that sums its own episode (fused_group / fused_finish in sgmm_frontier.hip)
// are built from the pieces here; how a kernel orders and overlaps them (its
// schedule, which is what was measured) stays in the kernel.
#pragma once

#include "sgmm_rollout.h"

namespace sgmm {

// ------------------------------------------------------------------ loaders
// How a scan reads the policy kernel's global output.  Plain: an earlier
// launch wrote it.  Shared: another wave of the same launch may have (the
// fused scan's hand-off), so the loads and stores are write-through (sc1) both
// ways (MI355X_MICROARCH.md, inter-workgroup visibility, row 1) -- a wave's own
// bytes too: its stores drained first, one code path for both.
template <class T>
__device__ __forceinline__ T fused_ld(const T* p) {
    typedef __attribute__((address_space(1))) const T gT;
    return __hip_atomic_load((gT*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class T>
__device__ __forceinline__ void fused_st(T* p, T v) {
    typedef __attribute__((address_space(1))) T gT;
    __hip_atomic_store((gT*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
struct PlainLd {
    template <class T>
    static __device__ __forceinline__ T ld(const T* __restrict__ p) { return *p; }
};
struct SharedLd {
    template <class T>
    static __device__ __forceinline__ T ld(const T* p) { return fused_ld(p); }
};

// ------------------------------------------------------------------ chunk start states and trades
// One round of 64 chunks, lane = chunk: m = this lane's chunk map (the identity
// past the last chunk), s = the state the path enters the round in.  Returns this
// lane's start state and advances s to the state leaving the round.
__device__ __forceinline__ uint32_t chunk_starts(uint64_t m, uint32_t& s, int lane) {
    const uint64_t inc = wave_map_scan(m);
    uint64_t excl = shfl_up_u64(inc, 1);
    if (lane == 0) excl = kIdentityMap;
    const uint32_t st = map_get(excl, s);
    s = map_get(readlane64(inc, kWave - 1), s);
    return st;
}
// the trades along the path from start state st: the frontier kernel's record
// rec (u32[8]), the table's counter word (one byte per start state)
template <class Ld>
__device__ __forceinline__ int frontier_trades(const uint32_t* ctr32, int64_t rec, uint32_t st) {
    return (int)Ld::ld(ctr32 + rec * 8 + st);
}
__device__ __forceinline__ int table_trades(uint64_t k, uint32_t st) { return (int)((k >> (8 * st)) & 0xFFu); }
// the lanes' sum in every lane
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// ------------------------------------------------------------------ frontier plane gather
// The rewards of 4 consecutive ticks of one chunk (frontier_len is a multiple
// of 4) along the path: plane start[c] before the chunk's paths merge (tick
// offset kc), plane p0 after.  t = the first tick, counted from the first chunk
// that start / kin describe, whose rows begin at base; left >= 1 = the ticks
// left in the window (past them the last one is loaded again).  GROUPS: start /
// kin span the episode's chunk groups (false: one group, at most 64 chunks).
template <class Ld, bool GROUPS>
__device__ __forceinline__ void frontier_gather4(double (&r)[4], const double* rew, const uint8_t* start,
                                                 const uint32_t* kin, int64_t base, int CL, int64_t rs, int t,
                                                 int left) {
    const int c = t / CL, u = t - c * CL;
    const uint32_t ki = kin[c];
    const int kc = (int)(ki & kKinfoTick);
    const int64_t pst = start[c], pp0 = ki >> 29;
    const int64_t rb = GROUPS ? base + (int64_t)(c / kFrontierLanes) * CL * kFrontierLanes +
                                    frontier_row(u, c % kFrontierLanes)
                              : base + frontier_row(u, c);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int jj = min(j, left - 1);
        r[j] = Ld::ld(rew + (u + jj >= kc ? pp0 : pst) * rs + rb + (int64_t)jj * kFrontierLanes);
    }
}

// ------------------------------------------------------------------ reference-order float64 chain
// s + v[0] + ... + v[n-1], one dependent add per value in the reference's order;
// v in LDS, 16-byte aligned, 32 values per round trip (71 against 75 us with 16 on
// config 3; 64 need 226 VGPRs).  (Pinning the next values ahead of these adds as
// asm operands measured slower: 99 against 76 us, profiles/r06_seq2_*.)
__device__ __forceinline__ double seq_chain(double s, const double* v, int n) {
    const double2* p = reinterpret_cast<const double2*>(v);
    const int nc = n & ~31;
    int i = 0;
    for (; i < nc; i += 32) {
        double2 x[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = p[i / 2 + j];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            s += x[j].x;
            s += x[j].y;
        }
    }
    for (; i < n; ++i) s += v[i];
    return s;
}

// ------------------------------------------------------------------ episode record
// One lane per episode: the idle penalty of an episode without a trade
// (drl_engine.py:64-65), the record stored write-through; returns the fitness.
__device__ __forceinline__ double finish_record(const sgmm_env_params* __restrict__ params, const EpArrays& ep,
                                                double* fitness, int32_t* trades, int e, double total, int32_t tr) {
    if (tr == 0) total -= params[ep.param[e]].idle_penalty;
    store_record(fitness, trades, e, total, tr);
    return total;
}

// ------------------------------------------------------------------ population arrival and tell
// Every record of a launch with a generation tail takes a ticket of its
// population; the last to arrive runs the GA step and resets the ticket.  The
// records were stored write-through and the last arriver reads them with sc1
// loads, so the hand-off needs no release fence.
// episode e's population k and its n_eps episodes (n_total: the launch's)
__device__ __forceinline__ void population_of(const StepArgs& sa, int e, int n_total, int& k, int& n_eps) {
    n_eps = sa.pop_eps > 0 ? sa.pop_eps : n_total;
    k = sa.pop_eps > 0 ? e / sa.pop_eps : 0;
}
// ONE lane, after it (or its wave: the drain covers every lane) stored nv
// records of population k: true when they were the population's last
__device__ __forceinline__ bool arrival_ticket(const StepArgs& sa, int k, int nv, int n_eps) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return __hip_atomic_fetch_add(&sa.st[k].arrivals, nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == n_eps - nv;
}
// One wave whose lanes stored the records e0 .. e0 + nv - 1 (of one population):
// the ticket, and the last arriver's tell (the argmax, StepArgs mode 3) with the
// population's state, records, masters, key and history.  (The workgroup-wide tail
// of the scan kernels, tail_run in sgmm_scan.hip, serves every mode from its own
// copy of StepArgs: routing its mode 3 through here, or this through a StepArgs
// copy, moved the scan kernels' registers.)
__device__ __forceinline__ void population_arrive(const StepArgs& sa, const double* fitness, const int32_t* trades,
                                                  int e0, int nv, int n_total, int lane) {
    int k, n_eps;
    population_of(sa, e0, n_total, k, n_eps);
    int last = 0;
    if (lane == 0) last = arrival_ticket(sa, k, nv, n_eps);
    if (__shfl(last, 0, kWave)) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // compiler order only: loads after the ticket
        sgmm_ga_state* st = sa.st + k;
        tell_wave<true>(st, fitness + (int64_t)k * n_eps, trades + (int64_t)k * n_eps, sa.P,
                        sa.history ? sa.history + (int64_t)k * sa.hist_cap : nullptr, sa.hist_cap);
        if (lane == 0) st->arrivals = 0;
    }
}

}  // namespace sgmm
