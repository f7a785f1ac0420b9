// sgmm_evaluate.hip -- strategy evaluation on gfx950: per-episode summaries
// without a trace, and the benchmark strategies (FOIC / GLFT) as policies.
//
// Reference semantics:
//   main.py:99-132               run_benchmark_and_save: the quote-rule loop
//   Env/benchmarks.py            FOICPolicy / GLFTPolicy.get_action (host side:
//                                the device reads its values from a table)
//   Env/recorder.py:46           wealth = cash + inventory * mid
//   analytics/mm_analyzer.py     StrategyAnalytics.summary_dict
//   main.py:309-324              get_clean_stats
//
// Two kernels.
//   k_summary_mlp<H>  one wave per episode, the walk of k_rollout_direct
//     (sgmm_rollout.hip): lane j owns hidden neuron j, every dot product the
//     k-ordered fused chain from the bias, so the actions are the trace path's
//     bit for bit.  The trace's 13 stores per step are replaced by the summary
//     accumulators, which live in registers (wave-uniform values); the next
//     tick's columns are fetched one step ahead with vector loads, whose
//     counter (vmcnt) is not the one the LDS exchange waits on, so the fetch
//     stays in flight across the step.
//   k_rule<TRACE>     one lane per episode (64 episodes per wave): a rule
//     episode has no MLP, a step is ~40 float64 operations.  The rule tables
//     sit in LDS as [entry][lane] (conflict-free), indexed by the inventory.
//     TRACE adds the per-step stores of sgmm_rule_trace.
//
// Sharpe ratios: one pass of shifted sums (Moments below); every other field
// is accumulated in the reference's sequential order (include/sgmm.h).
#include <climits>
#include <cmath>

#include "sgmm_device.h"
#include "sgmm_internal.h"

namespace sgmm {

struct EvalEpisodes {
    const int32_t* genome;
    const int64_t* tick_off;
    const int32_t* len;
    const int64_t* step_off;
    const int32_t* param;
    int32_t n;
};

// One-pass mean / variance by shifted sums: the shift is the first value, so
// s and ss sum deviations of the size of the spread, not of the level.
struct Moments {
    double k = 0.0, s = 0.0, ss = 0.0;
    int32_t n = 0;
    __device__ __forceinline__ void add(double x, bool on = true) {
        k = (on && n == 0) ? x : k;
        const double d = x - k;
        s = on ? s + d : s;
        ss = on ? ss + d * d : ss;
        n += on ? 1 : 0;
    }
    __device__ __forceinline__ double mean() const { return k + s / (double)n; }
    // ddof = 1; NaN below two values (pandas' std of one value)
    __device__ __forceinline__ double std() const {
        if (n < 2) return __builtin_nan("");
        const double var = (ss - s * s / (double)n) / (double)(n - 1);
        return sqrt(var > 0.0 ? var : 0.0);
    }
};

// The summary accumulators of one episode (include/sgmm.h, sgmm_episode_summary).
struct SummaryAcc {
    double w0 = 0.0, w_prev = 0.0, w_max = 0.0, dd = 0.0, w_trade = 0.0, total = 0.0;
    int64_t abs_inv = 0;
    int32_t rows = 0, fb = 0, fs = 0;
    Moments steps, trades;

    __device__ __forceinline__ void step(int32_t t, double cash, int32_t inv, double mid,
                                         const StepOut& st) {
        const double w = cash + (double)inv * mid;  // Env/recorder.py:46
        const bool first = t == 0;
        w0 = first ? w : w0;
        steps.add(w - w_prev, !first);              // main.py:314
        w_prev = w;
        w_max = (first || w > w_max) ? w : w_max;   // mm_analyzer.py:20 (cummax)
        const double d = w - w_max;
        dd = (first || d < dd) ? d : dd;            // :21-22
        abs_inv += inv < 0 ? -inv : inv;
        const bool tr = (st.fill_buy | st.fill_sell) != 0;
        trades.add(w - w_trade, tr && rows > 0);    // mm_analyzer.py:40
        w_trade = tr ? w : w_trade;
        rows += tr ? 1 : 0;
        fb += st.fill_buy;
        fs += st.fill_sell;
        total += st.reward;
    }

    __device__ __forceinline__ void finish(sgmm_episode_summary* o, int32_t T, double cash,
                                           int32_t inv, const sgmm_env_params& p) const {
        const double pnl = T > 0 ? w_prev - w0 : 0.0;
        const double map = T > 0 ? (double)abs_inv / (double)T : 0.0;
        o->total_pnl = pnl;
        o->map = map;
        o->pnl_to_map = map == 0.0 ? 0.0 : pnl / map;
        o->max_dd = dd;
        double sh = 0.0;
        if (rows >= 2) {
            const double sd = trades.std();          // NaN with exactly 2 rows
            sh = sd == 0.0 ? 0.0 : trades.mean() / sd;
        }
        o->sharpe_trades = sh;
        o->sharpe_steps = steps.n < 1 ? __builtin_nan("") : steps.mean() / (steps.std() + 1e-9);
        o->pnl_to_map_floor = pnl / (map > 1e-2 ? map : 1e-2);
        o->fitness = rows == 0 ? total - p.idle_penalty : total;
        o->final_cash = cash;
        o->trade_rows = rows;
        o->fills_buy = fb;
        o->fills_sell = fs;
        o->final_inventory = inv;
        o->steps = T;
        o->reserved = 0;
    }
};

// The five float64 columns of one tick.
struct TickRow {
    double mid, ask, bid, bmax, smin;
};
__device__ __forceinline__ TickRow load_row(const sgmm_ticks& tk, int64_t i) {
    return TickRow{tk.mid_next[i], tk.best_ask[i], tk.best_bid[i], tk.buy_max[i], tk.sell_min[i]};
}

// ------------------------------------------------------------------ MLP summary
template <int H>
__global__ __launch_bounds__(kWave) void k_summary_mlp(
    sgmm_ticks tk, EvalEpisodes ep, const sgmm_env_params* __restrict__ params,
    const float* __restrict__ mm, int64_t mm_stride, sgmm_episode_summary* __restrict__ out) {
    using L = GenomeLayout<H>;
    const int e = blockIdx.x;
    const int lane = threadIdx.x;
    const int32_t T = ep.len[e];
    const int64_t to = ep.tick_off[e];
    const sgmm_env_params p = params[ep.param[e]];
    const float* __restrict__ g = mm + (int64_t)ep.genome[e] * mm_stride;

    __shared__ float sh1[H], sh2[H];
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

    // a zero the compiler cannot see through: added to the (wave-uniform) tick
    // index it makes the column loads vector loads, see the file header
    int64_t vz = 0;
    asm volatile("" : "+v"(vz));

    int32_t inv = 0;
    double cash = 0.0;
    SummaryAcc acc;
    float x0 = 0.f, x1 = 0.f;
    TickRow row{};
    if (T > 0) {
        x0 = tk.s1n[to + vz];
        x1 = tk.s2n[to + vz];
        row = load_row(tk, to + vz);
    }
    for (int32_t t = 0; t < T; ++t) {
        // the next tick (the last step fetches its own again: always in range)
        const int64_t tn = to + (t + 1 < T ? t + 1 : t) + vz;
        const float nx0 = tk.s1n[tn], nx1 = tk.s2n[tn];
        const TickRow nrow = load_row(tk, tn);

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
        const StepOut st = ftp_step(p, inv, oa, ob, row.mid, row.ask, row.bid, row.bmax, row.smin);
        cash = apply_cash(cash, st);
        inv = st.inv;
        acc.step(t, cash, inv, row.mid, st);
        x0 = nx0;
        x1 = nx1;
        row = nrow;
    }
    if (lane == 0) acc.finish(out + e, T, cash, inv, p);
}

// ------------------------------------------------------------------ quote rules
// double -> int32 of an already rounded value: saturating, NaN -> INT32_MIN
// (act_to_int's convention)
__device__ __forceinline__ int32_t rule_to_int(double r) {
    if (!(r > -2147483648.0)) return INT32_MIN;  // NaN too
    return r >= 2147483647.0 ? INT32_MAX : (int32_t)r;
}

struct RuleTrace {
    int32_t *off_a, *off_b, *inventory;
    double *cash, *reward, *pnl, *fee_paid;
    uint8_t *fill_buy, *fill_sell;
    double* fitness;
    int32_t* trades;
};

template <bool TRACE>
__global__ __launch_bounds__(kWave) void k_rule(
    sgmm_ticks tk, EvalEpisodes ep, const sgmm_env_params* __restrict__ params,
    const sgmm_quote_rule* __restrict__ rules, int32_t n_rules, int32_t inv_min, int32_t nsi,
    sgmm_episode_summary* __restrict__ out, RuleTrace tr) {
    __shared__ double tab_a[8][kWave], tab_b[8][kWave];
    const int lane = threadIdx.x;
    const int e = blockIdx.x * kWave + lane;
    if (e >= ep.n) return;  // no barrier below: a lane only reads its own table column
    const int64_t to = ep.tick_off[e];
    const sgmm_env_params p = params[ep.param[e]];
    const int32_t gi = ep.genome[e];
    // a rule index outside [0, n_rules) is never read: the episode is not walked
    // (steps = 0 in its summary, no trace rows); n_rules <= 0: unchecked
    const bool known = n_rules <= 0 || (gi >= 0 && gi < n_rules);
    const int32_t T = known ? ep.len[e] : 0;
    const sgmm_quote_rule* __restrict__ r = rules + (known ? gi : 0);
    const int32_t mode = r->mode;
    const double qt = r->quote_tick;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        tab_a[k][lane] = r->ask[k];
        tab_b[k][lane] = r->bid[k];
    }

    int32_t inv = 0, rows = 0;
    double cash = 0.0, total = 0.0;
    SummaryAcc acc;
    TickRow row{};
    if (T > 0) row = load_row(tk, to);
    const int64_t so = TRACE ? ep.step_off[e] : 0;
    for (int32_t t = 0; t < T; ++t) {
        const TickRow nrow = load_row(tk, to + (t + 1 < T ? t + 1 : t));  // one step ahead
        int q = inv - inv_min;
        q = q < 0 ? 0 : (q >= nsi ? nsi - 1 : q);  // p.i_min / p.i_max keep it inside; never index outside
        const double ra = tab_a[q][lane], rb = tab_b[q][lane];
        double fa = ra, fb = rb;
        if (mode == 1) {  // main.py:106-110
            const double mid_p = (row.ask + row.bid) / 2.0;
            fa = ((mid_p + ra) - row.ask) / qt;
            fb = (row.bid - (mid_p - rb)) / qt;
        }
        const int32_t oa = rule_to_int(rint(fa)), ob = rule_to_int(rint(fb));  // :111, :113
        const StepOut st = ftp_step(p, inv, oa, ob, row.mid, row.ask, row.bid, row.bmax, row.smin);
        cash = apply_cash(cash, st);
        inv = st.inv;
        if (TRACE) {
            const int64_t i = so + t;
            total += st.reward;
            rows += st.fill_buy | st.fill_sell;
            if (tr.off_a) tr.off_a[i] = oa;
            if (tr.off_b) tr.off_b[i] = ob;
            if (tr.inventory) tr.inventory[i] = inv;
            if (tr.cash) tr.cash[i] = cash;
            if (tr.reward) tr.reward[i] = st.reward;
            if (tr.pnl) tr.pnl[i] = st.pnl;
            if (tr.fee_paid) tr.fee_paid[i] = st.fee_paid;
            if (tr.fill_buy) tr.fill_buy[i] = (uint8_t)st.fill_buy;
            if (tr.fill_sell) tr.fill_sell[i] = (uint8_t)st.fill_sell;
        } else {
            acc.step(t, cash, inv, row.mid, st);
        }
        row = nrow;
    }
    if (TRACE) {
        if (rows == 0) total -= p.idle_penalty;
        if (tr.fitness) tr.fitness[e] = total;
        if (tr.trades) tr.trades[e] = rows;
    } else {
        acc.finish(out + e, T, cash, inv, p);
    }
}

// ------------------------------------------------------------------ host side
static int check_eval(const sgmm_ticks* tk, const sgmm_episodes* eps, const void* params) {
    SGMM_REQUIRE(tk && eps && params, "null ticks/episodes/params");
    SGMM_REQUIRE(eps->n >= 0, "n episodes < 0");
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

static int check_rules(const sgmm_episodes* eps, const sgmm_quote_rule* rules_host, int32_t n_rules) {
    SGMM_REQUIRE(n_rules >= 0, "n_rules=%d < 0", n_rules);
    SGMM_REQUIRE(!rules_host || n_rules > 0, "rules_host given without n_rules");
    if (!rules_host) return SGMM_OK;
    const int32_t nsi = eps->inv_max - eps->inv_min + 1;
    for (int32_t i = 0; i < n_rules; ++i) {
        const sgmm_quote_rule& r = rules_host[i];
        SGMM_REQUIRE(r.mode == 0 || r.mode == 1, "rule %d: mode=%d (0 or 1)", i, r.mode);
        SGMM_REQUIRE(r.n_inventory == nsi, "rule %d: n_inventory=%d, the episode batch has %d", i,
                     r.n_inventory, nsi);
        SGMM_REQUIRE(r.mode == 0 || r.quote_tick > 0.0, "rule %d: quote_tick=%g must be > 0 in mode 1",
                     i, r.quote_tick);
    }
    return SGMM_OK;
}

static EvalEpisodes eval_eps(const sgmm_episodes* e) {
    return EvalEpisodes{e->genome, e->tick_off, e->len, e->step_off, e->param, e->n};
}

}  // namespace sgmm

using namespace sgmm;

extern "C" int sgmm_rollout_summary(const sgmm_ticks* ticks, const sgmm_episodes* eps,
                                    const sgmm_env_params* params, const float* mm_genomes,
                                    int64_t mm_stride, int32_t hidden, const sgmm_quote_rule* rules,
                                    const sgmm_quote_rule* rules_host, int32_t n_rules,
                                    sgmm_episode_summary* out, void* stream) {
    clear_error();
    if (int rc = check_eval(ticks, eps, params)) return rc;
    SGMM_REQUIRE((mm_genomes != nullptr) != (rules != nullptr),
                 "exactly one of mm_genomes / rules must be given");
    SGMM_REQUIRE(out, "null out");
    if (mm_genomes) {
        SGMM_REQUIRE(supported_hidden(hidden), "hidden=%d unsupported (8,16,32,64)", hidden);
        SGMM_REQUIRE(mm_stride >= (int64_t)hidden * hidden + 7 * hidden + 2, "mm_stride too small");
        SGMM_REQUIRE(!rules_host && n_rules == 0, "rules_host / n_rules without rules");
    } else if (int rc = check_rules(eps, rules_host, n_rules)) {
        return rc;
    }
    if (eps->n == 0) return SGMM_OK;
    const EvalEpisodes ep = eval_eps(eps);
    hipStream_t s = as_stream(stream);
    if (rules) {
        ProfScope prof("summary_rule", s);
        SGMM_LAUNCH(k_rule<false>, dim3((eps->n + kWave - 1) / kWave), dim3(kWave), 0, s, *ticks, ep,
                    params, rules, n_rules, eps->inv_min, eps->inv_max - eps->inv_min + 1, out,
                    RuleTrace{});
        SGMM_LAUNCHED();
        return SGMM_OK;
    }
    ProfScope prof("summary_mlp", s);
    switch (hidden) {
        case 8: SGMM_LAUNCH(k_summary_mlp<8>, dim3(eps->n), dim3(kWave), 0, s, *ticks, ep, params, mm_genomes, mm_stride, out); break;
        case 16: SGMM_LAUNCH(k_summary_mlp<16>, dim3(eps->n), dim3(kWave), 0, s, *ticks, ep, params, mm_genomes, mm_stride, out); break;
        case 32: SGMM_LAUNCH(k_summary_mlp<32>, dim3(eps->n), dim3(kWave), 0, s, *ticks, ep, params, mm_genomes, mm_stride, out); break;
        default: SGMM_LAUNCH(k_summary_mlp<64>, dim3(eps->n), dim3(kWave), 0, s, *ticks, ep, params, mm_genomes, mm_stride, out); break;
    }
    SGMM_LAUNCHED();
    return SGMM_OK;
}

extern "C" int sgmm_rule_trace(const sgmm_ticks* ticks, const sgmm_episodes* eps,
                               const sgmm_env_params* params, const sgmm_quote_rule* rules,
                               const sgmm_quote_rule* rules_host, int32_t n_rules, int32_t* off_a,
                               int32_t* off_b, int32_t* inventory, double* cash, double* reward,
                               double* pnl_reward, double* fee_paid, uint8_t* fill_buy,
                               uint8_t* fill_sell, double* fitness, int32_t* trades, void* stream) {
    clear_error();
    if (int rc = check_eval(ticks, eps, params)) return rc;
    SGMM_REQUIRE(rules, "null rules");
    if (int rc = check_rules(eps, rules_host, n_rules)) return rc;
    if (eps->n == 0) return SGMM_OK;
    hipStream_t s = as_stream(stream);
    ProfScope prof("rule_trace", s);
    SGMM_LAUNCH(k_rule<true>, dim3((eps->n + kWave - 1) / kWave), dim3(kWave), 0, s, *ticks,
                eval_eps(eps), params, rules, n_rules, eps->inv_min,
                eps->inv_max - eps->inv_min + 1, (sgmm_episode_summary*)nullptr,
                RuleTrace{off_a, off_b, inventory, cash, reward, pnl_reward, fee_paid, fill_buy,
                          fill_sell, fitness, trades});
    SGMM_LAUNCHED();
    return SGMM_OK;
}
