// sgmm_rollout.hip -- the population-rollout hot path on gfx950: the host entry
// points, the launch of a batch (rollout_impl) and the trace / forward / step
// kernels.  The policy kernels are in sgmm_table.hip (the tables; their MFMA MLP
// in sgmm_mlp_mfma.h) and sgmm_frontier.hip (the frontier walk and its spill),
// the path scans, the exact ordered sum and the generation tail in sgmm_scan.hip
// (launch_path_scan; the pieces every scan shares in sgmm_scan.h).
//
// Reference semantics: evaluate_individual (Env/drl_engine.py:9-67) mapped
// over a GA population (drl_engine.py:104-115), FTPEnv.step
// (Env/market_env.py:22-67), TradingPolicy / AdversaryPolicy
// (models/model.py:5-57).
//
// Fitness path (sgmm_rollout_fitness) -- a policy kernel, then a path scan:
//
//  1. policy kernel.  The inventory feedback makes an episode a serial chain,
//     but the policy only sees (signal_t, inventory) and the inventory takes
//     at most 8 values (caps +-2 -> 5), so the per-(tick, state) work can be
//     laid out in parallel:
//     The launch plan picks one of five (PolicyKernel, sgmm_plan.h):
//     - Frontier, k_policy_frontier (many episodes or episodes beyond kMaxLen,
//       H = 16 / 32, no adversary; sgmm_frontier.hip): one wave per walk,
//       lane = chunk, only the states the chunk's paths occupy are evaluated;
//     - the tables evaluate every (tick, inventory[, adversary flags]) state,
//       the H x H layer on v_mfma_f32_16x16x4_f32 (its k-ordered fused chain
//       IS the canonical dot-product order):
//       TableSp, k_policy_table_sp (H = 16 / 32, no adversary, launches of at
//       most kTableSpChunks chunks): one workgroup per chunk, one wave per state;
//       TableV3, k_policy_table_v3 (H = 16 / 32, no adversary, larger
//       launches): one wave per 64 ticks;
//       TableMfma, k_policy_table_mfma (round 1's schedule): H = 64 and the
//       adversary path at H = 16 / 32 / 64;
//     - TableValu, k_policy_table (one lane per (tick, state) on the VALU):
//       H = 8, and any H when forced, the tests' independent cross-check.
//     Output: per chunk its transition byte-map and the trade count along the
//     path from each start state, per tick the path planes (the reward along
//     the chunk's path from each start state).  With the adversary: 2 fill
//     bits per (inventory, previous fills) state (u64) and one float64 reward
//     plane per state.
//
//  2. path scan (launch_path_scan, sgmm_scan.hip; ScanKernel::Fused: inside the
//     frontier walks): chunk start states from the chunk maps, the rewards along
//     the path summed in the reference's sequential float64 order, bit-exact.
//
// Trace path (sgmm_rollout_trace): k_rollout_direct, one wave per episode,
// lane = hidden neuron, the literal step loop (independent second
// implementation; the tests require both paths to agree bit for bit).
#include <atomic>

#include "sgmm_rollout.h"

namespace sgmm {

// ------------------------------------------------------------------ direct (trace) path
struct TraceOut {
    int32_t *off_a, *off_b, *adv_a, *adv_b, *inventory;
    double *cash, *reward, *pnl, *fee_paid;
    uint8_t *fill_buy, *fill_sell;
    float *raw_a, *raw_b;
    double* fitness;
    int32_t* trades;
};

template <int H>
__global__ __launch_bounds__(kWave) void k_rollout_direct(
    sgmm_ticks tk, EpArrays ep, const sgmm_env_params* __restrict__ params,
    const float* __restrict__ mm, int64_t mm_stride, const float* __restrict__ adv,
    int64_t adv_stride, int32_t inv_min, int32_t nsi, TraceOut out) {
    using L = GenomeLayout<H>;
    const int e = blockIdx.x;
    const int lane = threadIdx.x;
    const int32_t T = ep.len[e];
    const int64_t to = ep.tick_off[e], so = ep.step_off[e];
    const sgmm_env_params p = params[ep.param[e]];
    const float* __restrict__ g = mm + (int64_t)ep.genome[e] * mm_stride;
    const int ai = (adv && ep.adv) ? ep.adv[e] : -1;

    __shared__ float sh1[H], sh2[H];
    __shared__ int32_t lut[2][32];
    // lane j < H owns hidden neuron j of both hidden layers
    float w1[3] = {0.f, 0.f, 0.f}, b1 = 0.f, b2 = 0.f, w2[H];
#pragma unroll
    for (int k = 0; k < H; ++k) w2[k] = 0.f;
    if (lane < H) {
        w1[0] = g[L::W1 + 3 * lane];
        w1[1] = g[L::W1 + 3 * lane + 1];
        w1[2] = g[L::W1 + 3 * lane + 2];
        b1 = g[L::B1 + lane];
        b2 = g[L::B2 + lane];
#pragma unroll
        for (int k = 0; k < H; ++k) w2[k] = g[L::W2 + lane * H + k];
    }
    if (ai >= 0 && lane < 4 * nsi) {
        int32_t da, db;
        adv_delta(adv + (int64_t)ai * adv_stride, p, inv_min + (lane >> 2), (lane >> 1) & 1,
                  lane & 1, da, db);
        lut[0][lane] = da;
        lut[1][lane] = db;
    }
    __syncthreads();

    int32_t inv = 0, trades = 0, fbp = 0, fsp = 0;
    double cash = 0.0, total = 0.0;
    for (int32_t t = 0; t < T; ++t) {
        const int64_t ti = to + t;
        const float x0 = tk.s1n[ti], x1 = tk.s2n[ti];
        const float x2 = (float)((double)inv / 2.0);
        if (lane < H) {
            float a = b1;
            a = __builtin_fmaf(w1[0], x0, a);
            a = __builtin_fmaf(w1[1], x1, a);
            a = __builtin_fmaf(w1[2], x2, a);
            sh1[lane] = relu(a);
        }
        __syncthreads();
        if (lane < H) {
            float a = b2;
#pragma unroll
            for (int k = 0; k < H; ++k) a = __builtin_fmaf(w2[k], sh1[k], a);
            sh2[lane] = relu(a);
        }
        __syncthreads();
        float o0 = g[L::B3], o1 = g[L::B3 + 1];
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const float h = sh2[j];
            o0 = __builtin_fmaf(g[L::W3 + j], h, o0);
            o1 = __builtin_fmaf(g[L::W3 + H + j], h, o1);
        }
        const int32_t oa = act_to_int(rintf(o0 * p.act_scale));
        const int32_t ob = act_to_int(rintf(o1 * p.act_scale));
        int32_t da = 0, db = 0;
        if (ai >= 0) {
            const int s = ((inv - inv_min) << 2) | (fsp << 1) | fbp;
            da = lut[0][s];
            db = lut[1][s];
        }
        const StepOut st = ftp_step(p, inv, (double)oa + (double)da, (double)ob + (double)db,
                                    tk.mid_next[ti], tk.best_ask[ti], tk.best_bid[ti], tk.buy_max[ti],
                                    tk.sell_min[ti]);
        cash = apply_cash(cash, st);
        inv = st.inv;
        total += st.reward;
        trades += (st.fill_buy | st.fill_sell);
        fbp = st.fill_buy;
        fsp = st.fill_sell;
        if (lane == 0) {
            const int64_t r = so + t;
            if (out.off_a) out.off_a[r] = oa;
            if (out.off_b) out.off_b[r] = ob;
            if (out.adv_a) out.adv_a[r] = da;
            if (out.adv_b) out.adv_b[r] = db;
            if (out.inventory) out.inventory[r] = inv;
            if (out.cash) out.cash[r] = cash;
            if (out.reward) out.reward[r] = st.reward;
            if (out.pnl) out.pnl[r] = st.pnl;
            if (out.fee_paid) out.fee_paid[r] = st.fee_paid;
            if (out.fill_buy) out.fill_buy[r] = (uint8_t)st.fill_buy;
            if (out.fill_sell) out.fill_sell[r] = (uint8_t)st.fill_sell;
            if (out.raw_a) out.raw_a[r] = o0;
            if (out.raw_b) out.raw_b[r] = o1;
        }
    }
    if (lane == 0) {
        if (trades == 0) total -= p.idle_penalty;
        if (out.fitness) out.fitness[e] = total;
        if (out.trades) out.trades[e] = trades;
    }
}

// ------------------------------------------------------------------ batched primitives
template <int H>
__global__ void k_policy_forward(const float* __restrict__ genomes, int64_t stride,
                                 const int32_t* __restrict__ idx, const float* __restrict__ st,
                                 float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* g = genomes + (int64_t)(idx ? idx[i] : i) * stride;
    float o0, o1;
    mlp_forward<H>(g, st[3 * i], st[3 * i + 1], st[3 * i + 2], o0, o1);
    out[2 * i] = o0;
    out[2 * i + 1] = o1;
}

__global__ void k_adversary_forward(const float* __restrict__ genomes, int64_t stride,
                                    const int32_t* __restrict__ idx, const float* __restrict__ st,
                                    float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* g = genomes + (int64_t)(idx ? idx[i] : i) * stride;
    float o0, o1;
    adv_forward(g, st[3 * i], st[3 * i + 1], st[3 * i + 2], o0, o1);
    out[2 * i] = o0;
    out[2 * i + 1] = o1;
}

__global__ void k_env_step(const sgmm_env_params* __restrict__ params,
                           const int32_t* __restrict__ pidx, int32_t* __restrict__ inventory,
                           double* __restrict__ cash, const int32_t* __restrict__ action,
                           const int32_t* __restrict__ adv_action,
                           const double* __restrict__ mid, const double* __restrict__ ask,
                           const double* __restrict__ bid, const double* __restrict__ bmax,
                           const double* __restrict__ smin, double* __restrict__ reward,
                           double* __restrict__ pnl, double* __restrict__ inv_reward,
                           double* __restrict__ fee_paid, uint8_t* __restrict__ fill_buy,
                           uint8_t* __restrict__ fill_sell, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const sgmm_env_params p = params[pidx ? pidx[i] : 0];
    double oa = (double)action[2 * i], ob = (double)action[2 * i + 1];
    if (adv_action) {  // market_env.py:25-28 (the int64 sum, exact in float64)
        oa += (double)adv_action[2 * i];
        ob += (double)adv_action[2 * i + 1];
    }
    const StepOut so = ftp_step(p, inventory[i], oa, ob, mid[i], ask[i], bid[i], bmax[i], smin[i]);
    inventory[i] = so.inv;
    cash[i] = apply_cash(cash[i], so);
    if (reward) reward[i] = so.reward;
    if (pnl) pnl[i] = so.pnl;
    if (inv_reward) inv_reward[i] = -(p.phi * (double)(so.inv < 0 ? -so.inv : so.inv));
    if (fee_paid) fee_paid[i] = so.fee_paid;
    if (fill_buy) fill_buy[i] = (uint8_t)so.fill_buy;
    if (fill_sell) fill_sell[i] = (uint8_t)so.fill_sell;
}

// ------------------------------------------------------------------ host helpers
static int check_episodes(const sgmm_ticks* tk, const sgmm_episodes* eps, const void* params,
                          const float* mm, int32_t hidden) {
    SGMM_REQUIRE(tk && eps && params && mm, "null ticks/episodes/params/genomes");
    SGMM_REQUIRE(eps->n >= 0, "n episodes < 0");
    SGMM_REQUIRE(supported_hidden(hidden), "hidden=%d unsupported (8,16,32,64)", hidden);
    SGMM_REQUIRE(eps->max_len >= 0, "max_len=%d < 0", eps->max_len);
    SGMM_REQUIRE(eps->inv_min <= 0 && eps->inv_max >= 0 && eps->inv_max - eps->inv_min + 1 <= 8,
                 "inventory range [%d,%d] must contain 0 and span <= 8 values", eps->inv_min,
                 eps->inv_max);
    if (eps->n > 0)
        SGMM_REQUIRE(eps->genome && eps->tick_off && eps->len && eps->step_off && eps->param,
                     "null episode array");
    SGMM_REQUIRE(tk->s1n && tk->s2n && tk->mid_next && tk->best_ask && tk->best_bid &&
                     tk->buy_max && tk->sell_min,
                 "null tick column");
    return SGMM_OK;
}

// SIMDs of the current device (cached per device id; 256 CUs if the query fails)
static int simd_count() {
    constexpr int kMaxDev = 64;
    static std::atomic<int> cache[kMaxDev];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    std::atomic<int>& c = cache[dev < kMaxDev ? dev : kMaxDev - 1];
    int n = c.load(std::memory_order_relaxed);
    if (n == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        n = 4 * cus;
        c.store(n, std::memory_order_relaxed);
    }
    return n;
}

// rs: the plane stride of the batch's workspace layout (WorkspaceLayout::rs)
static EpArrays ep_arrays(const sgmm_episodes* e, bool with_adv, int64_t rs) {
    return EpArrays{e->genome, with_adv ? e->adv : nullptr, e->tick_off, e->len, e->step_off,
                    e->param, rs, e->order, 1, 1, 1, e->n};
}

}  // namespace sgmm

using namespace sgmm;

// The workspace of a batch on the current device under the current knobs
// (workspace_layout, sgmm_plan.h; rollout_impl carves the same layout)
static size_t rollout_ws_bytes(int32_t n_episodes, int64_t total_steps, int32_t nsi, bool arl,
                               const PlanKnobs& knobs) {
    return workspace_layout(n_episodes, total_steps, nsi, arl, simd_count(), knobs).bytes;
}

extern "C" size_t sgmm_rollout_workspace_bytes(int32_t n_episodes, int64_t total_steps, int32_t n_inventory,
                                               int32_t with_adversary) {
    return rollout_ws_bytes(n_episodes, total_steps, n_inventory, with_adversary != 0, plan_knobs());
}

// ABI 3 form: n_states > 8 means the adversary layout with n_states / 4
// inventory values (use sgmm_rollout_workspace_bytes for an adversary batch
// with fewer than 3 inventory values)
extern "C" size_t sgmm_rollout_workspace_size(int32_t n_episodes, int64_t total_steps,
                                              int32_t n_states) {
    if (n_states > 8) return n_states % 4 ? 0 : rollout_ws_bytes(n_episodes, total_steps, n_states / 4, true, plan_knobs());
    return rollout_ws_bytes(n_episodes, total_steps, n_states, false, plan_knobs());
}

extern "C" int sgmm_ordered_sum(const double* values, int64_t n, double init, double* out,
                                void* stream) {
    clear_error();
    SGMM_REQUIRE(out && (values || n == 0) && n >= 0, "bad arguments");
    ProfScope prof("ordered_sum", as_stream(stream));
    launch_ordered_sum(values, n, init, out, as_stream(stream));
    SGMM_LAUNCHED();
    return SGMM_OK;
}

// zero n words (the fused scan's arrival counters)
__global__ __launch_bounds__(1024) void k_zero_u32(uint32_t* __restrict__ p, int32_t n) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) p[i] = 0u;
}

// policy kernel + path scan (+ the generation tail when step.st) for one batch:
// resolves the launch plan once (resolve_plan, sgmm_plan.h: kernels, chunk
// groups, workspace layout) from the entry point's knob snapshot and executes it.
// walk_order: the caller's writable walk order (eps->order points at it) for the
// walk-order feedback; rj_out: a training launch with the feedback hands its job
// here instead of launching it; rj_in: a job to run inside (or before) this launch
static int rollout_impl(const PlanKnobs& knobs, const sgmm_ticks* ticks, const sgmm_episodes* eps,
                        const sgmm_env_params* params, const GenomeSrc& src, bool arl,
                        int32_t hidden, double* fitness, int32_t* trades, void* workspace,
                        size_t workspace_bytes, const StepArgs& step, hipStream_t s,
                        ReorderJob* rj_out = nullptr, const ReorderJob* rj_in = nullptr,
                        int32_t* walk_order = nullptr) {
    SGMM_REQUIRE(fitness && trades, "null fitness/trades output");
    if (eps->n == 0) return SGMM_OK;
    const int32_t nsi = eps->inv_max - eps->inv_min + 1;
    LaunchShape shape;
    shape.n = eps->n;
    shape.max_len = eps->max_len;
    shape.total_steps = eps->total_steps;
    shape.nsi = nsi;
    shape.hidden = hidden;
    shape.arl = arl;
    shape.simds = simd_count();
    shape.tail = step.st != nullptr;
    shape.mode = step.mode;
    shape.pop_eps = step.pop_eps;
    shape.src_pop_eps = src.pop_eps;
    shape.walk_feedback = walk_order && eps->order == walk_order;
    const LaunchPlan plan = resolve_plan(shape, knobs);
    const WorkspaceLayout& ws = plan.ws;
    if (!workspace || workspace_bytes < ws.bytes) {
        set_error("workspace %zu bytes < required %zu", workspace_bytes, ws.bytes);
        return SGMM_ERR_WORKSPACE;
    }
    char* w = reinterpret_cast<char*>(workspace);
    const auto at = [w](size_t off) -> void* { return off == kNoSection ? nullptr : w + off; };
    uint64_t* cmaps = static_cast<uint64_t*>(at(ws.cmaps));
    uint64_t* ctr = static_cast<uint64_t*>(at(ws.ctr));
    uint32_t* kinfo = static_cast<uint32_t*>(at(ws.kinfo));
    uint32_t* wslots = static_cast<uint32_t*>(at(ws.wslots));
    uint32_t* wspill = static_cast<uint32_t*>(at(ws.wspill));
    uint32_t* arrive = static_cast<uint32_t*>(at(ws.arrive));
    FusedHandoff* handoff = static_cast<FusedHandoff*>(at(ws.handoff));
    uint64_t* fills = static_cast<uint64_t*>(at(ws.fills));
    double* rew = static_cast<double*>(at(ws.rew));
    EpArrays ep = ep_arrays(eps, arl, ws.rs);
    const bool fr = plan.policy == PolicyKernel::Frontier;
    if (fr) {
        ep.ngrp = plan.fr.gmax;
        ep.g0 = plan.fr.g0;
        ep.gtail = plan.fr.gtail;
        ep.whole = plan.fr.whole;
    }
    const bool vt = plan.validation;  // the validation launches are profiled separately
    SGMM_REQUIRE(fr || arl || eps->max_len <= kMaxLen,
                 "max_len=%d > %d needs the frontier kernel (hidden 16 or 32) or the adversary path", eps->max_len,
                 kMaxLen);
    SGMM_REQUIRE(!fr || eps->max_len <= kFrontierMaxLen, "max_len=%d > %lld ticks per episode",
                 eps->max_len, (long long)kFrontierMaxLen);
    const ReorderJob* rj_fold = nullptr;
    if (rj_in && rj_in->order) {
        // a walk-order job rides along in this launch's state-parallel table when it takes
        // that path and its workspace use ends below the job's slot counts; otherwise it
        // runs first, before this launch can touch the workspace
        if (plan.policy == PolicyKernel::TableSp && eps->max_len > 0 &&
            reinterpret_cast<const char*>(rj_in->wslots) >= w + ws.bytes) {
            rj_fold = rj_in;
        } else {
            launch_walk_reorder(*rj_in, s);
            SGMM_LAUNCHED();
        }
    }
    if (eps->max_len <= 0) {
        // no ticks: the scan alone writes every episode's (empty) record
    } else if (fr) {
        FrontierArgs fa{*ticks, ep, params, src, eps->inv_min, nsi, cmaps, reinterpret_cast<uint32_t*>(ctr),
                        kinfo, rew, wslots, wspill, plan.spill};
        if (plan.scan == ScanKernel::Fused) {
            fa.fitness = fitness;
            fa.trades = trades;
            fa.hstate = arrive;
            fa.handoff = handoff;
            fa.n_eps = eps->n;
            fa.step = step;
            // the arrival words start at zero (the wave that ends an episode's chain
            // resets its word; a workspace is not zeroed before its first use).  A kernel,
            // not hipMemsetAsync: replayed after other launches, a captured memset
            // node left stale values here (tools/diag_fused2.py, round 6)
            if (plan.fr.gmax > 1)
                SGMM_LAUNCH(k_zero_u32, dim3((eps->n + 1023) / 1024), dim3(1024), 0, s, arrive, eps->n);
        }
        ProfScope prof(vt ? "val_policy_frontier" : "policy_frontier", s);
        if (int rc = launch_policy_frontier(hidden, nsi, (unsigned)plan.fr.waves, plan.fr.ls, s, fa)) return rc;
        if (fa.spill_budget) {
            ProfScope prof2(vt ? "val_frontier_spill" : "frontier_spill", s);
            if (int rc = launch_frontier_spill(hidden, nsi, (unsigned)plan.fr.waves, plan.fr.ls, s, fa)) return rc;
        }
    } else {
        // TableValu, TableSp (with the walk-order job that rides along), TableV3 or TableMfma
        ProfScope prof(vt ? "val_policy_table" : "policy_table", s);
        launch_policy_table(plan.policy, hidden, arl, nsi, eps->max_len, eps->n, *ticks, ep, params, src,
                            eps->inv_min, ctr, cmaps, fills, rew, rj_fold, s);
        SGMM_LAUNCHED();
    }
    // (a fused frontier launch summed every episode and ran the tail itself)
    if (plan.scan != ScanKernel::Fused) {
        ProfScope prof(vt ? "val_path_scan" : "path_scan", s);
        launch_path_scan(plan, ScanArgs{ep, params, eps->inv_min, nsi, eps->n, cmaps, ctr, kinfo, fills, rew, fitness,
                                        trades, step}, s);
    }
    SGMM_LAUNCHED();
    if (plan.reorder) {
        ReorderJob job{wslots, walk_order, eps->n, plan.fr.whole, plan.fr.gtail, src.pop_eps};
        job.w_whole = plan.w_whole;
        job.w_split = plan.w_split;
        job.len = eps->max_len;  // equal-length episodes (LaunchPlan::reorder)
        if (rj_out) {
            *rj_out = job;
        } else {
            launch_walk_reorder(job, s);
            SGMM_LAUNCHED();
        }
    }
    return SGMM_OK;
}

extern "C" int sgmm_rollout_fitness(const sgmm_ticks* ticks, const sgmm_episodes* eps,
                                    const sgmm_env_params* params, const float* mm_genomes,
                                    int64_t mm_stride, int32_t hidden, const float* adv_genomes,
                                    int64_t adv_stride, double* fitness, int32_t* trades,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    clear_error();
    if (int rc = check_episodes(ticks, eps, params, mm_genomes, hidden)) return rc;
    SGMM_REQUIRE(mm_stride >= (int64_t)hidden * hidden + 7 * hidden + 2, "mm_stride too small");
    const bool arl = adv_genomes != nullptr;
    SGMM_REQUIRE(!arl || adv_stride >= kAdvParams, "adv_stride < 74");
    const GenomeSrc src{mm_genomes, mm_stride, adv_genomes, adv_stride, nullptr, nullptr, nullptr, 0, 0};
    return rollout_impl(plan_knobs(), ticks, eps, params, src, arl, hidden, fitness, trades, workspace,
                        workspace_bytes, StepArgs{}, as_stream(stream));
}

extern "C" int sgmm_rollout_fitness_asked(const sgmm_ticks* ticks, const sgmm_episodes* eps,
                                          const sgmm_env_params* params,
                                          const sgmm_asked_population* pop, int32_t hidden,
                                          double* fitness, int32_t* trades, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    clear_error();
    SGMM_REQUIRE(pop && pop->state && pop->master_mm, "null asked population");
    if (int rc = check_episodes(ticks, eps, params, pop->master_mm, hidden)) return rc;
    SGMM_REQUIRE(pop->i0 >= 0, "negative i0");
    const bool arl = pop->master_adv != nullptr;
    const GenomeSrc src{nullptr, 0, nullptr, 0, pop->state, pop->master_mm, pop->master_adv, pop->seed, pop->i0};
    return rollout_impl(plan_knobs(), ticks, eps, params, src, arl, hidden, fitness, trades, workspace,
                        workspace_bytes, StepArgs{}, as_stream(stream));
}

extern "C" int sgmm_generation(const sgmm_ticks* ticks, const sgmm_episodes* eps,
                               const sgmm_env_params* params, sgmm_ga_state* state, float* master_mm,
                               float* master_adv, float* best_master, int32_t hidden, uint64_t seed,
                               int32_t P, double* fitness, int32_t* trades, sgmm_ga_history* history,
                               int32_t history_cap, void* workspace, size_t workspace_bytes,
                               void* stream) {
    clear_error();
    SGMM_REQUIRE(state && master_mm, "null state / master");
    if (int rc = check_episodes(ticks, eps, params, master_mm, hidden)) return rc;
    SGMM_REQUIRE(P > 0 && eps->n == 2 * P, "episodes must be P training + P validation episodes");
    const int64_t n_mm = (int64_t)hidden * hidden + 7 * hidden + 2;
    SGMM_REQUIRE(n_mm <= kMaxStepParams, "genome too large for the fused GA step");
    const bool arl = master_adv != nullptr;
    // one population, its key by value: no per-population strides or seeds
    GenomeSrc src{};
    src.st = state;
    src.master_mm = master_mm;
    src.master_adv = master_adv;
    src.seed = seed;
    StepArgs step{};
    step.st = state;
    step.master_mm = master_mm;
    step.master_adv = master_adv;
    step.best_master = best_master;
    step.n_mm = n_mm;
    step.n_adv = arl ? kAdvGenome : 0;
    step.seed = seed;
    step.history = history;
    step.hist_cap = history_cap;
    step.P = P;
    step.mode = kStepWhole;
    return rollout_impl(plan_knobs(), ticks, eps, params, src, arl, hidden, fitness, trades, workspace,
                        workspace_bytes, step, as_stream(stream));
}

static int check_pops(const sgmm_populations* pops) {
    SGMM_REQUIRE(pops, "null populations");
    SGMM_REQUIRE(pops->n_pop > 0 && pops->P > 0, "n_pop=%d P=%d must be > 0", pops->n_pop, pops->P);
    SGMM_REQUIRE(supported_hidden(pops->hidden), "hidden=%d unsupported (8,16,32,64)", pops->hidden);
    SGMM_REQUIRE(pops->states && pops->masters_mm && pops->seeds, "null states / masters / seeds");
    SGMM_REQUIRE(pops->history_cap >= 0 && (pops->history || pops->history_cap == 0), "history");
    return SGMM_OK;
}

static int64_t pops_n_mm(const sgmm_populations* pops) {
    return (int64_t)pops->hidden * pops->hidden + 7 * pops->hidden + 2;
}

// The asked genomes of K populations: pop_eps episodes per population,
// individual i0 + genome[e] of the episode's population -- or (use_best) its
// tell's argmax, rolled out against no adversary (the deferred validation).
static GenomeSrc pops_src(const sgmm_populations* pops, int32_t pop_eps, int32_t i0, bool use_best) {
    const bool adv = pops->masters_adv != nullptr && !use_best;
    GenomeSrc src{};
    src.st = pops->states;
    src.master_mm = pops->masters_mm;
    src.master_adv = adv ? pops->masters_adv : nullptr;
    src.i0 = i0;
    src.pop_eps = pop_eps;
    src.seeds = pops->seeds;
    src.mm_pstride = pops_n_mm(pops);
    src.adv_pstride = adv ? kAdvGenome : 0;
    src.use_best = use_best ? 1 : 0;
    return src;
}

// The generation tail of K populations of P individuals, pop_eps episodes per
// population in this launch (StepArgs::mode).  kStepValidate, the validation
// bookkeeping alone, touches no adversary master.
static StepArgs pops_step(const sgmm_populations* pops, int32_t P, int32_t pop_eps, int32_t mode) {
    const bool adv = pops->masters_adv != nullptr && mode != kStepValidate;
    StepArgs step{};
    step.st = pops->states;
    step.master_mm = pops->masters_mm;
    step.master_adv = adv ? pops->masters_adv : nullptr;
    step.best_master = pops->best_masters;
    step.n_mm = pops_n_mm(pops);
    step.n_adv = adv ? kAdvGenome : 0;
    step.history = pops->history;
    step.hist_cap = pops->history_cap;
    step.P = P;
    step.pop_eps = pop_eps;
    step.seeds = pops->seeds;
    step.mode = mode;
    return step;
}

extern "C" int sgmm_generation_multi(const sgmm_ticks* ticks, const sgmm_episodes* eps,
                                     const sgmm_env_params* params, const sgmm_populations* pops,
                                     double* fitness, int32_t* trades, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    clear_error();
    if (int rc = check_pops(pops)) return rc;
    const int32_t H = pops->hidden, K = pops->n_pop, P = pops->P;
    if (int rc = check_episodes(ticks, eps, params, pops->masters_mm, H)) return rc;
    SGMM_REQUIRE((int64_t)eps->n == 2LL * K * P,
                 "episodes must be n_pop x (P training + P validation) = %lld, got %d",
                 2LL * K * P, eps->n);
    SGMM_REQUIRE(pops_n_mm(pops) <= kMaxStepParams, "genome too large for the fused GA step");
    return rollout_impl(plan_knobs(), ticks, eps, params, pops_src(pops, 2 * P, 0, false),
                        pops->masters_adv != nullptr, H, fitness, trades, workspace, workspace_bytes,
                        pops_step(pops, P, 2 * P, kStepWhole), as_stream(stream));
}

// Validation of every population's post-tell master (drl_engine.py:129-160):
// val_eps episode k runs masters_mm row val_eps->genome[k] (= k) with no
// adversary; the scan's workgroup k then runs population k's validation
// bookkeeping (validation_tail).  The policy kernel is the table (K episodes).
// deferred: the training launch's tail ran the tell's argmax only
// (kStepArgmax); episode k rolls out population k's best individual from the
// pre-tell master and the scan's workgroup k writes the new master (kStepDeferred)
static int validate_impl(const PlanKnobs& knobs, const sgmm_ticks* ticks, const sgmm_episodes* val_eps,
                         const sgmm_env_params* params, const sgmm_populations* pops, double* val_fitness,
                         int32_t* val_trades, void* workspace, size_t workspace_bytes, hipStream_t s,
                         bool deferred = false, const ReorderJob* rj = nullptr) {
    const int32_t H = pops->hidden, K = pops->n_pop;
    if (int rc = check_episodes(ticks, val_eps, params, pops->masters_mm, H)) return rc;
    SGMM_REQUIRE(val_eps->n == K, "validation episodes must be one per population (%d), got %d", K, val_eps->n);
    GenomeSrc src{};  // the post-tell masters as materialized rows
    src.mm = pops->masters_mm;
    src.mm_stride = pops_n_mm(pops);
    if (deferred) src = pops_src(pops, 1, 0, true);
    return rollout_impl(knobs, ticks, val_eps, params, src, false, H, val_fitness, val_trades, workspace,
                        workspace_bytes, pops_step(pops, 1, 1, deferred ? kStepDeferred : kStepValidate), s, nullptr,
                        rj);
}

extern "C" int sgmm_validate_multi(const sgmm_ticks* ticks, const sgmm_episodes* val_eps,
                                   const sgmm_env_params* params, const sgmm_populations* pops,
                                   double* val_fitness, int32_t* val_trades, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    clear_error();
    if (int rc = check_pops(pops)) return rc;
    return validate_impl(plan_knobs(), ticks, val_eps, params, pops, val_fitness, val_trades, workspace,
                         workspace_bytes, as_stream(stream));
}

extern "C" int sgmm_generation_multi_best(const sgmm_ticks* ticks, const sgmm_episodes* train_eps,
                                          const sgmm_episodes* val_eps, const sgmm_env_params* params,
                                          const sgmm_populations* pops, double* fitness, int32_t* trades,
                                          double* val_fitness, int32_t* val_trades, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    clear_error();
    if (int rc = check_pops(pops)) return rc;
    const int32_t H = pops->hidden, K = pops->n_pop, P = pops->P;
    if (int rc = check_episodes(ticks, train_eps, params, pops->masters_mm, H)) return rc;
    SGMM_REQUIRE((int64_t)train_eps->n == (int64_t)K * P, "training episodes must be n_pop x P = %lld, got %d",
                 (int64_t)K * P, train_eps->n);
    SGMM_REQUIRE(val_eps && val_eps->n == K, "validation episodes must be one per population");
    SGMM_REQUIRE(val_fitness && val_trades, "null validation outputs");
    SGMM_REQUIRE(pops_n_mm(pops) <= kMaxStepParams, "genome too large for the fused GA step");
    const PlanKnobs knobs = plan_knobs();  // one snapshot for both launches
    // the validation batch is checked before anything is enqueued
    if (int rc = check_episodes(ticks, val_eps, params, pops->masters_mm, H)) return rc;
    {
        const int32_t vnsi = val_eps->inv_max - val_eps->inv_min + 1;
        const size_t vneed = rollout_ws_bytes(val_eps->n, val_eps->total_steps, vnsi, false, knobs);
        if (val_eps->n > 0 && (!workspace || workspace_bytes < vneed)) {
            set_error("workspace %zu bytes < required %zu (validation batch)", workspace_bytes, vneed);
            return SGMM_ERR_WORKSPACE;
        }
    }
    hipStream_t s = as_stream(stream);
    ReorderJob job{nullptr, nullptr, 0, 0, 0, 1};
    // the training launch walks the caller's writable walk order when given
    // (the feedback rewrites it); train_eps itself is only read
    sgmm_episodes tr = *train_eps;
    if (pops->walk_order) tr.order = pops->walk_order;
    if (int rc = rollout_impl(knobs, ticks, &tr, params, pops_src(pops, P, 0, false), pops->masters_adv != nullptr, H,
                              fitness, trades, workspace, workspace_bytes, pops_step(pops, P, P, kStepArgmax), s, &job, nullptr,
                              pops->walk_order))
        return rc;
    return validate_impl(knobs, ticks, val_eps, params, pops, val_fitness, val_trades, workspace, workspace_bytes, s,
                         true, &job);
}

extern "C" int sgmm_rollout_fitness_asked_multi(const sgmm_ticks* ticks, const sgmm_episodes* eps,
                                                const sgmm_env_params* params,
                                                const sgmm_populations* pops, int32_t i0,
                                                int32_t n_eps_pop, double* fitness, int32_t* trades,
                                                void* workspace, size_t workspace_bytes,
                                                void* stream) {
    clear_error();
    if (int rc = check_pops(pops)) return rc;
    const int32_t H = pops->hidden, K = pops->n_pop;
    if (int rc = check_episodes(ticks, eps, params, pops->masters_mm, H)) return rc;
    SGMM_REQUIRE(i0 >= 0 && n_eps_pop > 0 && (int64_t)eps->n == (int64_t)K * n_eps_pop,
                 "episodes must be n_pop x n_eps_pop (i0=%d, n_eps_pop=%d, n=%d)", i0, n_eps_pop, eps->n);
    return rollout_impl(plan_knobs(), ticks, eps, params, pops_src(pops, n_eps_pop, i0, false),
                        pops->masters_adv != nullptr, H, fitness, trades, workspace, workspace_bytes,
                        StepArgs{}, as_stream(stream));
}

extern "C" int sgmm_rollout_trace(const sgmm_ticks* ticks, const sgmm_episodes* eps,
                                  const sgmm_env_params* params, const float* mm_genomes,
                                  int64_t mm_stride, int32_t hidden, const float* adv_genomes,
                                  int64_t adv_stride, int32_t* off_a, int32_t* off_b,
                                  int32_t* adv_a, int32_t* adv_b, int32_t* inventory,
                                  double* cash, double* reward, double* pnl_reward,
                                  double* fee_paid, uint8_t* fill_buy, uint8_t* fill_sell,
                                  float* raw_a, float* raw_b, double* fitness, int32_t* trades,
                                  void* stream) {
    clear_error();
    if (int rc = check_episodes(ticks, eps, params, mm_genomes, hidden)) return rc;
    SGMM_REQUIRE(mm_stride >= (int64_t)hidden * hidden + 7 * hidden + 2, "mm_stride too small");
    const bool arl = adv_genomes != nullptr;
    SGMM_REQUIRE(!arl || adv_stride >= 74, "adv_stride < 74");
    if (eps->n == 0) return SGMM_OK;
    const int32_t nsi = eps->inv_max - eps->inv_min + 1;
    TraceOut o{off_a, off_b, adv_a, adv_b, inventory, cash, reward, pnl_reward, fee_paid,
               fill_buy, fill_sell, raw_a, raw_b, fitness, trades};
    const EpArrays ep = ep_arrays(eps, arl, workspace_layout(eps->n, eps->total_steps, nsi, arl, simd_count(), plan_knobs()).rs);
    hipStream_t s = as_stream(stream);
    ProfScope prof("rollout_direct", s);
    switch (hidden) {
        case 8: SGMM_LAUNCH(k_rollout_direct<8>, dim3(eps->n), dim3(kWave), 0, s, *ticks, ep, params, mm_genomes, mm_stride, adv_genomes, adv_stride, eps->inv_min, nsi, o); break;
        case 16: SGMM_LAUNCH(k_rollout_direct<16>, dim3(eps->n), dim3(kWave), 0, s, *ticks, ep, params, mm_genomes, mm_stride, adv_genomes, adv_stride, eps->inv_min, nsi, o); break;
        case 32: SGMM_LAUNCH(k_rollout_direct<32>, dim3(eps->n), dim3(kWave), 0, s, *ticks, ep, params, mm_genomes, mm_stride, adv_genomes, adv_stride, eps->inv_min, nsi, o); break;
        default: SGMM_LAUNCH(k_rollout_direct<64>, dim3(eps->n), dim3(kWave), 0, s, *ticks, ep, params, mm_genomes, mm_stride, adv_genomes, adv_stride, eps->inv_min, nsi, o); break;
    }
    SGMM_LAUNCHED();
    return SGMM_OK;
}

extern "C" int sgmm_policy_forward(const float* genomes, int64_t genome_stride, int32_t hidden,
                                   const int32_t* genome_idx, const float* states, float* out,
                                   int64_t n, void* stream) {
    clear_error();
    SGMM_REQUIRE(genomes && states && out, "null pointer");
    SGMM_REQUIRE(n >= 0, "n < 0");
    SGMM_REQUIRE(supported_hidden(hidden), "hidden=%d unsupported (8,16,32,64)", hidden);
    SGMM_REQUIRE(genome_stride >= (int64_t)hidden * hidden + 7 * hidden + 2, "stride too small");
    if (n == 0) return SGMM_OK;
    const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
    hipStream_t s = as_stream(stream);
    ProfScope prof("policy_forward", s);
    switch (hidden) {
        case 8: SGMM_LAUNCH(k_policy_forward<8>, grid, blk, 0, s, genomes, genome_stride, genome_idx, states, out, n); break;
        case 16: SGMM_LAUNCH(k_policy_forward<16>, grid, blk, 0, s, genomes, genome_stride, genome_idx, states, out, n); break;
        case 32: SGMM_LAUNCH(k_policy_forward<32>, grid, blk, 0, s, genomes, genome_stride, genome_idx, states, out, n); break;
        default: SGMM_LAUNCH(k_policy_forward<64>, grid, blk, 0, s, genomes, genome_stride, genome_idx, states, out, n); break;
    }
    SGMM_LAUNCHED();
    return SGMM_OK;
}

extern "C" int sgmm_adversary_forward(const float* genomes, int64_t genome_stride,
                                      const int32_t* genome_idx, const float* states, float* out,
                                      int64_t n, void* stream) {
    clear_error();
    SGMM_REQUIRE(genomes && states && out, "null pointer");
    SGMM_REQUIRE(n >= 0 && genome_stride >= 74, "bad n or stride");
    if (n == 0) return SGMM_OK;
    ProfScope prof("adversary_forward", as_stream(stream));
    SGMM_LAUNCH(k_adversary_forward, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       as_stream(stream), genomes, genome_stride, genome_idx, states, out, n);
    SGMM_LAUNCHED();
    return SGMM_OK;
}

extern "C" int sgmm_env_step_batch(const sgmm_env_params* params, const int32_t* param_idx,
                                   int32_t* inventory, double* cash, const int32_t* action,
                                   const int32_t* adv_action, const double* mid_next,
                                   const double* best_ask, const double* best_bid,
                                   const double* buy_max, const double* sell_min, double* reward,
                                   double* pnl_reward, double* inventory_reward, double* fee_paid,
                                   uint8_t* fill_buy, uint8_t* fill_sell, int64_t n,
                                   void* stream) {
    clear_error();
    SGMM_REQUIRE(params && inventory && cash && action && mid_next && best_ask && best_bid &&
                     buy_max && sell_min,
                 "null pointer");
    SGMM_REQUIRE(n >= 0, "n < 0");
    if (n == 0) return SGMM_OK;
    ProfScope prof("env_step", as_stream(stream));
    SGMM_LAUNCH(k_env_step, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       as_stream(stream), params, param_idx, inventory, cash, action, adv_action,
                       mid_next, best_ask, best_bid, buy_max, sell_min, reward, pnl_reward,
                       inventory_reward, fee_paid, fill_buy, fill_sell, n);
    SGMM_LAUNCHED();
    return SGMM_OK;
}
