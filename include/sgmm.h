/*
 * sgmm.h -- C ABI of the MI355X population-rollout library (libsgmm.so).
 *
 * Drop-in boundary for the hot path of the reference repository
 * (KAS-W/Deep-Reinforcement-Learning-Based-Signal-Gated-Market-Making).
 * The reference has no FFI: its boundary is a set of Python call signatures.
 * Each entry point below names the reference interface it replaces
 * (paths relative to the reference root); INTEGRATION.md shows the
 * Python (ctypes) binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - Every pointer argument is caller-owned DEVICE memory (hipMalloc / torch
 *     CUDA tensors) unless stated otherwise.  No entry point allocates, frees
 *     or synchronises in the hot calls: work is enqueued on `stream`
 *     (a hipStream_t, NULL = default stream) and the call returns.
 *   - Return value: 0 = success, < 0 = error; sgmm_last_error() (thread-local)
 *     describes the last failure.  Argument errors are detected before any
 *     work is enqueued.
 *   - Calls on distinct streams are thread-safe.
 *   - Numerics: prices/cash/reward float64 without FMA contraction (the
 *     reference's operation order, market_env.py:30-58); policy MLP float32
 *     with each dot product evaluated as the k-ordered fused chain starting at
 *     the bias; actions = rint(raw * act_scale) (round half to even, np.round).
 */
#ifndef SGMM_H
#define SGMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGMM_ABI_VERSION 5

enum {
    SGMM_OK = 0,
    SGMM_ERR_ARG = -1,       /* invalid argument (shape, pointer, range) */
    SGMM_ERR_HIP = -2,       /* HIP runtime error */
    SGMM_ERR_WORKSPACE = -3, /* workspace too small */
    SGMM_ERR_UNSUPPORTED = -4
};

/* Per-episode environment constants.
 * FTPEnv.__init__ (Env/market_env.py:8-15) plus the constants
 * evaluate_individual hard-codes (Env/drl_engine.py:39,48,64-65). */
typedef struct sgmm_env_params {
    double  phi;          /* inventory penalty lambda (market_env.py:10) */
    double  tick;         /* tick size (market_env.py:11) */
    double  fee;          /* fee rate (market_env.py:9) */
    double  idle_penalty; /* subtracted from fitness if no trade (drl_engine.py:64-65): 50.0 */
    int32_t i_max;        /* inventory cap (market_env.py:14): 2 */
    int32_t i_min;        /* inventory floor (market_env.py:15): -2 */
    float   act_scale;    /* MM action scale (drl_engine.py:39): 5.0 */
    float   adv_scale;    /* adversary action scale (drl_engine.py:48): 1.0 */
} sgmm_env_params;        /* 48 bytes */

/* The bundle (drl_engine.py:11) as structure-of-arrays device columns,
 * indexed by absolute tick index.  (sgmm_ticks and sgmm_episodes are HOST
 * structs whose members point to device memory.)  s1n/s2n are the normalised signals of
 * drl_engine.py:33-34 (host computes them once per bundle). */
typedef struct sgmm_ticks {
    const float  *s1n;
    const float  *s2n;
    const double *mid_next;
    const double *best_ask;
    const double *best_bid;
    const double *buy_max;
    const double *sell_min;
} sgmm_ticks;

/* A batch of episodes: episode e runs genome row genome[e] (and adversary
 * row adv[e], or -1 for none) over ticks [tick_off[e], tick_off[e]+len[e])
 * with params[param[e]].  step_off = exclusive prefix sum of len (it places
 * each episode's tables in the workspace); total_steps = sum of len.
 * Every episode of one call shares the inventory range [inv_min, inv_max]
 * (at most 8 inventory values; 0 must lie inside).  order (optional, may be
 * NULL) is a permutation of [0, n), longest episode first: the frontier
 * kernel (one wave per episode) starts the longest walks first so short ones
 * fill the tail; results are per episode and do not depend on it. */
typedef struct sgmm_episodes {
    int32_t        n;
    int32_t        max_len;
    int64_t        total_steps;
    int32_t        inv_min;   /* host copy of the (shared) i_min of params */
    int32_t        inv_max;   /* host copy of the (shared) i_max of params */
    const int32_t *genome;
    const int32_t *adv;       /* may be NULL (no adversary anywhere) */
    const int64_t *tick_off;
    const int32_t *len;
    const int64_t *step_off;
    const int32_t *param;
    const int32_t *order;     /* may be NULL: identity (ABI 2) */
} sgmm_episodes;

int         sgmm_abi_version(void);
const char *sgmm_last_error(void);

/* Batched FTPEnv.step over n independent environments.
 * Replaces Env/market_env.py:22-67 (FTPEnv.step).  inventory/cash are
 * updated in place; adv_action may be NULL (no adversary); reward / pnl /
 * inv_reward / fee_paid / fill_* outputs may individually be NULL.
 * params: device array, param_idx[n] (NULL = all use params[0]). */
int sgmm_env_step_batch(const sgmm_env_params *params, const int32_t *param_idx,
                        int32_t *inventory, double *cash,
                        const int32_t *action, const int32_t *adv_action,
                        const double *mid_next, const double *best_ask, const double *best_bid,
                        const double *buy_max, const double *sell_min,
                        double *reward, double *pnl_reward, double *inventory_reward,
                        double *fee_paid, uint8_t *fill_buy, uint8_t *fill_sell,
                        int64_t n, void *stream);

/* Batched TradingPolicy.forward (models/model.py:24-26): out[i] =
 * MLP(genomes[genome_idx[i]], states[i]).  Genome layout = parameters()
 * order W1[H,3] b1[H] W2[H,H] b2[H] W3[2,H] b3[2] (H*H+7H+2 floats).
 * genome_idx may be NULL (row i).  hidden in {8,16,32,64}. */
int sgmm_policy_forward(const float *genomes, int64_t genome_stride, int32_t hidden,
                        const int32_t *genome_idx, const float *states, float *out,
                        int64_t n, void *stream);

/* Batched AdversaryPolicy.forward (models/model.py:49-50): tanh outputs,
 * weights = the first 74 floats of each genome row (model.py:52-57). */
int sgmm_adversary_forward(const float *genomes, int64_t genome_stride,
                           const int32_t *genome_idx, const float *states, float *out,
                           int64_t n, void *stream);

/* Workspace bytes sgmm_rollout_fitness needs for this batch: n_inventory =
 * inv_max - inv_min + 1 inventory values, with_adversary != 0 when the batch
 * runs adversaries (adv_genomes / masters_adv non-NULL). (ABI 4) */
size_t sgmm_rollout_workspace_bytes(int32_t n_episodes, int64_t total_steps, int32_t n_inventory,
                                    int32_t with_adversary);
/* ABI 3 form: n_states = n_inventory, or 4 * n_inventory with the adversary
 * -- read as the adversary layout only when > 8, so an adversary batch with
 * fewer than 3 inventory values must be sized with sgmm_rollout_workspace_bytes. */
size_t sgmm_rollout_workspace_size(int32_t n_episodes, int64_t total_steps, int32_t n_states);

/* THE HOT PATH.  Fitness of every episode of the batch:
 * replaces Env/drl_engine.py:9-67 (evaluate_individual) as mapped by
 * Pool.starmap over the population (drl_engine.py:104-115).
 * fitness[e] = sum of step rewards (sequential float64 order), minus
 * idle_penalty if the episode never traded; trades[e] = steps with a fill.
 * adv_genomes may be NULL (no adversary, eps->adv ignored). */
int sgmm_rollout_fitness(const sgmm_ticks *ticks, const sgmm_episodes *eps,
                         const sgmm_env_params *params,
                         const float *mm_genomes, int64_t mm_stride, int32_t hidden,
                         const float *adv_genomes, int64_t adv_stride,
                         double *fitness, int32_t *trades,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Per-step trace of every episode (the recorder loop of
 * pipeline/agent_trainer.py:144-153 / main.py:63-90 / pipeline/evaluator.py:25-37,
 * batched).  Outputs are indexed by step_off[e] + t; any may be NULL.
 * off_a/off_b: MM action before the adversary; adv_a/adv_b: adversary deltas;
 * inventory/cash: after the step.  Also writes fitness/trades. */
int sgmm_rollout_trace(const sgmm_ticks *ticks, const sgmm_episodes *eps,
                       const sgmm_env_params *params,
                       const float *mm_genomes, int64_t mm_stride, int32_t hidden,
                       const float *adv_genomes, int64_t adv_stride,
                       int32_t *off_a, int32_t *off_b, int32_t *adv_a, int32_t *adv_b,
                       int32_t *inventory, double *cash, double *reward, double *pnl_reward,
                       double *fee_paid, uint8_t *fill_buy, uint8_t *fill_sell,
                       float *raw_a, float *raw_b,
                       double *fitness, int32_t *trades, void *stream);

/* ------------------------------------------------------------------------
 * Strategy evaluation: the benchmark strategies as policies, and per-episode
 * summaries without a trace (main.py:99-132, 206-210, 300-324;
 * analytics/mm_analyzer.py:5-56).
 * ------------------------------------------------------------------------ */

/* An inventory-indexed quote rule: the action is a function of the current
 * inventory and the tick's best ask / bid, no MLP (Env/benchmarks.py through
 * main.py:104-113).  The host evaluates the strategy's get_action(inventory)
 * for every inventory value (pow / log / sqrt stay there); the device does the
 * per-tick arithmetic, all float64, unfused, with q = inventory - inv_min:
 *   mode 0 (main.py:113, FOIC)   off_a = (int)rint(ask[q]), off_b = (int)rint(bid[q])
 *   mode 1 (main.py:106-111, GLFT)
 *       mid_p = (best_ask + best_bid) / 2.0
 *       off_a = (int)rint(((mid_p + ask[q]) - best_ask) / quote_tick)
 *       off_b = (int)rint((best_bid - (mid_p - bid[q])) / quote_tick)
 * rint rounds half to even (np.round); the conversion to int32 saturates and
 * maps NaN to INT32_MIN.  The reference converts to a 64-bit int, so rounded
 * offsets outside the int32 range are outside the parity domain. */
typedef struct sgmm_quote_rule {      /* one rule = one "genome" row */
    int32_t mode;                     /* 0: tick offsets, 1: mid-relative price offsets */
    int32_t n_inventory;              /* entries used, = inv_max - inv_min + 1, <= 8 */
    double  quote_tick;               /* mode 1: the divisor of main.py:109-110 (0.001 there) */
    double  ask[8], bid[8];           /* indexed by inventory - inv_min */
} sgmm_quote_rule;                    /* 144 bytes */

/* What StrategyAnalytics.summary_dict (analytics/mm_analyzer.py:12-56) and
 * get_clean_stats (main.py:309-324) report of one backtest frame, with
 * w[t] = cash_t + inventory_t * mid[t] after step t (the recorder's wealth,
 * Env/recorder.py:46) and T = steps:
 *   total_pnl = w[T-1] - w[0];  max_dd = min_t (w[t] - max_{u<=t} w[u]);
 *   map = (sum_t |inventory_t|) / T (integer sum);
 *   pnl_to_map = map == 0 ? 0 : total_pnl / map;
 *   pnl_to_map_floor = total_pnl / max(map, 1e-2);
 *   trade_rows = steps with a fill on either side, fills_* the per-side sums;
 *   sharpe_trades: over the wealth differences between consecutive trade rows,
 *     0 with fewer than 2 trade rows, NaN with exactly 2, 0 if std == 0, else
 *     mean / std (ddof = 1);
 *   sharpe_steps = mean(dw) / (std(dw, ddof = 1) + 1e-9) over the T-1 step
 *     differences (NaN for T <= 2);
 *   fitness = the reward sum in sequential order, minus idle_penalty when
 *     trade_rows == 0 (sgmm_rollout_fitness's value); final_cash /
 *     final_inventory = the last cash_t / inventory_t.
 * Every field but the two Sharpes is accumulated in the reference's
 * sequential float64 order and is bit-exact.  The Sharpes use one pass of
 * shifted sums (shift = the first difference x0: s = sum (x - x0), ss = sum
 * (x - x0)^2, mean = x0 + s / n, var = max(ss - s * s / n, 0) / (n - 1)),
 * within 1e-9 relative of the reference's two-pass value.  An episode of
 * length 0 reports zeros (NaN sharpe_steps). */
typedef struct sgmm_episode_summary {
    double total_pnl, map, pnl_to_map, max_dd, sharpe_trades, sharpe_steps,
           pnl_to_map_floor, fitness, final_cash;
    int32_t trade_rows, fills_buy, fills_sell, final_inventory, steps, reserved;
} sgmm_episode_summary;               /* 96 bytes */

/* Summary of every episode of the batch, nothing written per step.  Exactly
 * one of mm_genomes (TradingPolicy rows, as sgmm_rollout_trace: hidden in
 * {8,16,32,64}, row stride mm_stride) and rules must be given; with rules,
 * eps->genome[e] indexes rules, hidden / mm_stride are ignored and every
 * rule's n_inventory must be eps->inv_max - eps->inv_min + 1 (rules is DEVICE
 * memory: n_rules > 0 HOST copies may be passed in rules_host to have
 * n_inventory, mode and quote_tick checked before the launch; NULL skips the
 * check; with n_rules > 0 an episode whose genome[e] is outside [0, n_rules)
 * is not walked and reports steps = 0).  No adversary (eps->adv is ignored): the reference's evaluation
 * never runs one.  out: [eps->n].  One launch, no workspace. */
int sgmm_rollout_summary(const sgmm_ticks *ticks, const sgmm_episodes *eps,
                         const sgmm_env_params *params,
                         const float *mm_genomes, int64_t mm_stride, int32_t hidden,
                         const sgmm_quote_rule *rules, const sgmm_quote_rule *rules_host,
                         int32_t n_rules, sgmm_episode_summary *out, void *stream);

/* Per-step trace of rule episodes (main.py:99-132 run_benchmark_and_save,
 * batched): sgmm_rollout_trace's outputs without the adversary / raw columns,
 * indexed by step_off[e] + t; any may be NULL.  rules / rules_host / n_rules as
 * sgmm_rollout_summary. */
int sgmm_rule_trace(const sgmm_ticks *ticks, const sgmm_episodes *eps,
                    const sgmm_env_params *params, const sgmm_quote_rule *rules,
                    const sgmm_quote_rule *rules_host, int32_t n_rules,
                    int32_t *off_a, int32_t *off_b, int32_t *inventory, double *cash,
                    double *reward, double *pnl_reward, double *fee_paid,
                    uint8_t *fill_buy, uint8_t *fill_sell,
                    double *fitness, int32_t *trades, void *stream);

/* ------------------------------------------------------------------------
 * Hypothesis tests of the evaluation stage (main.py:227-297): Diebold-Mariano
 * (H1), Durbin-Watson (H2) and the moving-block bootstrap of the per-step
 * Sharpe ratio (H3), batched over many series.
 *
 * A SERIES BATCH is (values, off, n_series): device doubles and a device
 * int64 array of n_series + 1 offsets, series s = values[off[s] .. off[s+1]).
 * off_host is an optional HOST copy of off (as rules_host above): when given,
 * off_host[0] >= 0, non-decreasing offsets and series lengths below 2^31 are
 * checked before any HIP call; NULL skips the check (a series whose offsets
 * decrease is then read as empty).
 *
 * THE LANE SUM.  Every sum of these entry points is evaluated in one fixed
 * order, which analytics.py restates in numpy: element i of the summed
 * sequence belongs to lane i mod 64; a lane adds its elements in increasing
 * i, starting from 0.0; the 64 lane values are combined by the xor butterfly
 * d = 32, 16, 8, 4, 2, 1 (v += v[lane ^ d]).  A mean is that sum divided once
 * by the count.  All float64, nothing fused.
 * ------------------------------------------------------------------------ */

/* wealth[step_off[e] + t] = cash[.] + (double)inventory[.] * mid_next[tick_off[e] + t]
 * for every step of the batch (Env/recorder.py:46; the unfused expression of
 * the episode summaries), from the cash / inventory columns of
 * sgmm_rollout_trace or sgmm_rule_trace.  eps->step_off must be the exclusive
 * prefix sum of eps->len.  One launch. */
int sgmm_trace_wealth(const sgmm_ticks *ticks, const sgmm_episodes *eps,
                      const int32_t *inventory, const double *cash, double *wealth,
                      void *stream);

/* statsmodels' durbin_watson (main.py:247): out[s] = sum_{t>=1} (e[t] - e[t-1])^2
 * / sum_t e[t]^2, both lane sums (numerator element i = t - 1).  An empty
 * series gives 0/0 = NaN, length 1 gives 0 / e^2.  out: double[n_series]. */
int sgmm_durbin_watson(const double *values, const int64_t *off, const int64_t *off_host,
                       int32_t n_series, double *out, void *stream);

typedef struct sgmm_dm_result {
    double  stat;      /* mean_d / sqrt(var_d / n) */
    double  p_value;   /* 2 * (1 - Phi(|stat|)) */
    double  mean_d, var_d;
    int64_t n;
} sgmm_dm_result;      /* 40 bytes */

/* dm_test (main.py:228-236) of each series: actual, pred1, pred2 are series
 * batches over the same off; pred2 may be NULL (zeros, the naive forecast of
 * main.py:242).  crit 0 (MSE): e = (actual - pred)^2, crit 1 (MAD): e =
 * |actual - pred|.  d = e1 - e2; mean_d = lane sum / n; var_d = lane sum of
 * (d - mean_d)^2 divided by n - 1 (np.var, ddof = 1, two passes; NaN for
 * n < 2); stat = mean_d / sqrt(var_d / n); p_value = 2 * (1 - Phi(|stat|))
 * with Phi(x) = 0.5 * erfc((-x) / sqrt(2.0)).  NaN inputs propagate.  The
 * reference's h argument is unused there and has no counterpart here. */
int sgmm_dm_test(const double *actual, const double *pred1, const double *pred2,
                 const int64_t *off, const int64_t *off_host, int32_t n_series, int32_t crit,
                 sgmm_dm_result *out, void *stream);

enum {
    SGMM_MBB_CLAMPED = 1,      /* a caller's start lay outside [0, n - block_size] */
    SGMM_MBB_NOT_RESAMPLED = 2 /* n <= block_size: the plain Sharpe ratio, no bootstrap */
};

typedef struct sgmm_mbb_result {
    double  mean_sr, ci_lo, ci_hi;
    int32_t n_returns;        /* returns left after the NaN drop */
    int32_t num_blocks;       /* n_returns / block_size, 0 when not resampled */
    int32_t zero_replicates;  /* replicates equal to 0 (std <= 1e-9 or NaN) */
    int32_t flags;            /* SGMM_MBB_* */
} sgmm_mbb_result;            /* 40 bytes */

/* get_mbb_sharpe (main.py:251-285) of each WEALTH series: the moving-block
 * bootstrap of the per-step Sharpe ratio, 1 <= n_boot <= 4096 replicates of
 * n / block_size blocks of block_size >= 1 returns.
 *   - returns: r[t] = w[t+1] / w[t] - 1 (a division, then a subtraction); NaN
 *     entries are dropped in order, +-inf is kept (pct_change().dropna() for a
 *     NaN-free wealth; pandas forward-fills a NaN wealth, which is outside the
 *     parity domain).  n = the number kept.  `returns` is caller-owned device
 *     memory for off[n_series] doubles, distinct from wealth: series s's
 *     returns are left at returns[off[s] .. off[s] + n).
 *   - n <= block_size (n = 0 included): sr = mean / std if std > 1e-9 else 0
 *     over the returns; mean_sr = ci_lo = ci_hi = sr; flags has
 *     SGMM_MBB_NOT_RESAMPLED; every replicate slot of boot is set to sr.
 *   - otherwise replicate b concatenates blocks r[start .. start + block_size)
 *     for its num_blocks starts; its value is mean / std (np.std: ddof = 0,
 *     two passes, lane sums over the replicate's elements) if std > 1e-9,
 *     else 0 -- a NaN std (an inf in the replicate) compares false and gives 0.
 *     mean_sr = lane sum of the replicates / n_boot; ci_lo / ci_hi = the 2.5
 *     and 97.5 percentiles by numpy's linear rule: virtual index v = (n_boot -
 *     1) * (2.5 / 100) resp. (97.5 / 100), a = sorted[floor v], b = the next
 *     one, t = v - floor v, value = a + (b - a) * t, or b - (b - a) * (1 - t)
 *     when t >= 0.5; NaN if any replicate is NaN.
 *   - starts: device int32 [n_series][n_boot][starts_stride], starts_stride >=
 *     every resampled series' num_blocks; a start outside [0, n - block_size]
 *     is clamped into it and SGMM_MBB_CLAMPED is set -- nothing outside the
 *     series is ever read.  starts = NULL: block j of replicate b of series s
 *     takes output j % 4 of Philox4x32-10 with counter words (j / 4, b, s, 2)
 *     and key words (seed & 0xffffffff, seed >> 32) -- the generator of
 *     sgmm_ga_ask, stream id 2 -- and start = ((uint64_t)word * (uint64_t)(n -
 *     block_size + 1)) >> 32, whose bias is at most (n - block_size + 1) / 2^32.
 *   - boot: caller-owned device double[n_series][n_boot], every replicate's
 *     value (it carries them from the replicate launch to the percentile
 *     launch, so it is not optional).  starts_out: optional device int32 in the
 *     layout of starts, the starts actually used; entries past num_blocks are
 *     not written.  starts and starts_out need off_host: their row stride is
 *     checked against every series' possible block count before the launch.
 * Three launches on `stream` (returns, replicates, percentiles), no
 * cross-workgroup waits. */
int sgmm_mbb_sharpe(const double *wealth, const int64_t *off, const int64_t *off_host,
                    int32_t n_series, int32_t block_size, int32_t n_boot,
                    const int32_t *starts, int64_t starts_stride, uint64_t seed,
                    sgmm_mbb_result *out, double *boot, int32_t *starts_out, double *returns,
                    void *stream);

/* NeuroEvolution.ask (models/model.py:65-71) on device:
 * out[i,k] = master[k] + z(seed, stream_id, gen, i0+i, k) * (float)sigma,
 * z ~ N(0,1) from Philox4x32-10 + Box-Muller (counter-based, so any rank can
 * regenerate any individual).  sigma and gen are read ON DEVICE from `state`
 * (stream_id 0: sigma_mm, 1: sigma_adv; gen = state->gen), so a generation's
 * launches have fixed arguments and can be captured once in a HIP graph and
 * replayed.  out row stride out_stride.
 *
 * The stream is a contract (it is what lets any rank regenerate any individual;
 * tests/ga_model.py restates it in numpy):
 *   - parameter k of individual j takes output k % 4 of the Philox4x32-10 block
 *     with counter words (k / 4, j, (uint32_t)gen, stream_id) and key words
 *     (seed & 0xffffffff, seed >> 32); j = i0 + i is the global index;
 *   - the four raw words r0..r3 become float32 uniforms
 *       u0 = min(((float)r0 + 1) * 2^-32, 1)  in (0, 1],   u1 = (float)r1 * 2^-32,
 *     and u2, u3 likewise from r2, r3 ((float)r rounds to nearest: every word
 *     >= 0xffffff80 gives u0 = 1, z = 0);
 *   - outputs 0, 1 = m * cos(2 pi u1), m * sin(2 pi u1) with m = sqrt(-2 ln u0),
 *     outputs 2, 3 the same from (u2, u3), evaluated in float32 (logf, sqrtf,
 *     sincospif); |z| <= sqrt(64 ln 2) = 6.66;
 *   - out = master + (z * (float)sigma): a float32 multiply, then a float32 add
 *     (model.py:69-70), never fused. */
/* Device GA bookkeeping state (DRLEngine.train locals, drl_engine.py:84-89,
 * 143-160).  Initialise with sgmm_ga_state_init. */
typedef struct sgmm_ga_state {
    double  sigma_mm;      /* NeuroEvolution.sigma of the MM evolver */
    double  sigma_adv;     /* ... of the adversary evolver */
    double  best_val;      /* best_val_reward (-inf at start) */
    double  last_train_f;  /* best train fitness of the last generation */
    double  last_val_f;    /* validation reward of the last generation */
    int32_t no_improve;    /* no_improvement_gens */
    int32_t best_idx;      /* argmax of the last generation */
    int32_t adv_best_idx;  /* argmax of -fitness (adversary tell) */
    int32_t gen;           /* generations completed */
    int32_t improved;      /* last generation improved the validation reward */
    int32_t decayed;       /* last generation decayed sigma */
    int32_t patience;      /* 15 (drl_engine.py:155) */
    int32_t arrivals;      /* internal: workgroup arrival counter of a launch's generation tail (0 between launches) */
    double  decay;         /* 0.5 (drl_engine.py:156) */
} sgmm_ga_state;           /* 80 bytes */

/* History row written per generation (drl_engine.py:163-167). */
typedef struct sgmm_ga_history {
    double  train_f;
    double  val_f;
    double  sigma_after;
    int32_t train_trades;
    int32_t val_trades;
    int32_t best_idx;
    int32_t flags;         /* bit0 improved (checkpoint saved), bit1 sigma decayed */
} sgmm_ga_history;         /* 40 bytes */

int sgmm_ga_state_init(sgmm_ga_state *state, double sigma, int32_t patience, double decay,
                       void *stream);

int sgmm_ga_ask(const float *master, int64_t n_params, const sgmm_ga_state *state,
                uint32_t stream_id, uint64_t seed, int32_t i0, int32_t n,
                float *out, int64_t out_stride, void *stream);

/* NeuroEvolution.tell for both evolvers (model.py:73-76, drl_engine.py:119-125):
 * best = first index of max(fitness) (np.argmax; NaN counts as max),
 * adv_best = first index of max(-fitness).  The new master rows are written
 * into master_mm / master_adv either by copying row best of `pop_mm` /
 * `pop_adv` (host-supplied populations, may be NULL) or, when the pop
 * pointer is NULL, by regenerating the ask() of that index in place
 * (same seed/stream/gen as the ask).  P = global population size.
 * history: array of history_cap rows; row state->gen is written. */
int sgmm_ga_tell(sgmm_ga_state *state, const double *fitness, const int32_t *trades, int32_t P,
                 float *master_mm, const float *pop_mm, int64_t pop_mm_stride,
                 float *master_adv, const float *pop_adv, int64_t pop_adv_stride,
                 int64_t n_params_mm, int64_t n_params_adv, uint64_t seed,
                 sgmm_ga_history *history, int32_t history_cap, void *stream);

/* Validation bookkeeping after the best individual's validation rollout
 * (drl_engine.py:129-171): val_fitness/val_trades are read at index
 * state->best_idx when use_best_index (validation evaluated for the whole
 * population), else at 0.  On improvement master_mm is copied to best_master
 * (the checkpoint slot).  Applies sigma decay, completes history row
 * state->gen, then advances state->gen. */
int sgmm_ga_val_update(sgmm_ga_state *state, const double *val_fitness,
                       const int32_t *val_trades, int32_t use_best_index,
                       const float *master_mm, float *best_master, int64_t n_params_mm,
                       sgmm_ga_history *history, int32_t history_cap, void *stream);

/* One generation boundary in a single launch (single process or after the
 * fitness all-gather): tell (as sgmm_ga_tell, masters regenerated in place),
 * validation bookkeeping with the validation fitness of the whole population
 * (as sgmm_ga_val_update with use_best_index), then -- if next_pop_mm is not
 * NULL -- the ask() of the NEXT generation for individuals [i0, i0+n) with the
 * updated sigma (as sgmm_ga_ask; next_pop_adv likewise when master_adv).
 * Meant for modest P * n_params (one workgroup); use the separate entry points
 * for large populations.
 * Sharded inputs (multi-GPU, after an all-gather of per-rank records): with
 * shard_n > 0 the value of individual i in each of the four population arrays
 * is read at byte offset (i / shard_n) * shard_stride + (i % shard_n) *
 * sizeof(element) from its pointer; shard_n <= 0 means plain contiguous
 * arrays.  Every rank runs the same step on the gathered records, so masters
 * and sigma stay identical without a broadcast. */
int sgmm_ga_step(sgmm_ga_state *state, const double *fitness, const int32_t *trades,
                 const double *val_fitness, const int32_t *val_trades, int32_t P,
                 int32_t shard_n, int64_t shard_stride, float *master_mm, float *master_adv, float *best_master,
                 int64_t n_params_mm, int64_t n_params_adv, uint64_t seed,
                 sgmm_ga_history *history, int32_t history_cap,
                 float *next_pop_mm, float *next_pop_adv, int32_t i0, int32_t n, void *stream);

/* The current generation's ask() population, never materialized: episode e
 * evaluates individual i0 + genome[e] (adversary: i0 + adv[e], -1 = none)
 * whose genome is master + sigma * N(0,1) with the state's sigma and
 * generation -- exactly the rows sgmm_ga_ask would write -- generated inside
 * the rollout kernels (models/model.py:65-71 fused into drl_engine.py:104-115). */
typedef struct sgmm_asked_population {
    const sgmm_ga_state *state;
    const float *master_mm;   /* [genome_size(hidden)] */
    const float *master_adv;  /* [1250] or NULL (no adversary) */
    uint64_t seed;
    int32_t i0;               /* first individual of this rank's shard */
    int32_t pad_;
} sgmm_asked_population;     /* 40 bytes */

/* sgmm_rollout_fitness over the asked population (multi-rank shards: the
 * results then go through the all-gather and sgmm_ga_step). */
int sgmm_rollout_fitness_asked(const sgmm_ticks *ticks, const sgmm_episodes *eps,
                               const sgmm_env_params *params, const sgmm_asked_population *pop,
                               int32_t hidden, double *fitness, int32_t *trades, void *workspace,
                               size_t workspace_bytes, void *stream);

/* One whole generation of DRLEngine.train on one process
 * (Env/drl_engine.py:92-171): the asked population's P training episodes
 * (eps 0..P-1, individual = genome[e]) and P validation episodes (eps
 * P..2P-1) in one rollout, and the generation boundary of sgmm_ga_step
 * (tell both evolvers, validation bookkeeping, sigma decay, history row
 * state->gen) run by the rollout's last workgroup.  fitness/trades: [2P].
 * Two kernel launches, no host synchronization; genome_size(hidden) <= 4096. */
int sgmm_generation(const sgmm_ticks *ticks, const sgmm_episodes *eps,
                    const sgmm_env_params *params, sgmm_ga_state *state, float *master_mm,
                    float *master_adv, float *best_master, int32_t hidden, uint64_t seed,
                    int32_t P, double *fitness, int32_t *trades, sgmm_ga_history *history,
                    int32_t history_cap, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * Several GA populations advanced together: one DRLEngine.train per
 * inventory penalty phi (the lambda sweep of pipeline/agent_trainer.py:136-137
 * called per phi at main.py:39-45; checkpoints/688981/agent_best_val_{phi}.pth)
 * or per asset (agent_trainer.py:168-173).  Population k keeps its own
 * master, sigma schedule, no-improvement counter, best validation reward,
 * history and Philox key -- exactly the state of an independent DRLEngine
 * run with seed seeds[k], so K populations in one launch reproduce K
 * separate runs bit for bit.  A HOST struct whose members point to device
 * memory; rows are contiguous per population.
 * ------------------------------------------------------------------------ */
typedef struct sgmm_populations {
    int32_t n_pop;              /* K */
    int32_t P;                  /* individuals per population (global, all ranks) */
    int32_t hidden;             /* TradingPolicy hidden width (every population) */
    int32_t history_cap;        /* history rows per population */
    sgmm_ga_state *states;      /* [K] (sgmm_ga_state_init each) */
    float *masters_mm;          /* [K][H*H+7H+2] */
    float *masters_adv;         /* [K][1250] or NULL (no adversary) */
    float *best_masters;        /* [K][H*H+7H+2] checkpoint slots (drl_engine.py:144-150) */
    const uint64_t *seeds;      /* [K] device: per-population Philox key */
    sgmm_ga_history *history;   /* [K][history_cap] */
    /* (ABI 5) optional, may be NULL: [K*P] device, the frontier kernel's walk
     * order of the TRAINING episodes for sgmm_generation_multi_best, read and
     * REWRITTEN on the device after each training launch (the walk-order
     * feedback; scheduling only, results do not depend on it).  The caller
     * seeds it with a permutation (e.g. a copy of train_eps->order), owns it
     * for the session and must not share it between concurrent calls.  NULL:
     * no feedback, train_eps->order is only read.  Every other entry point
     * ignores it.  The library never writes any sgmm_episodes array. */
    int32_t *walk_order;
} sgmm_populations;             /* 72 bytes */

/* One generation of K populations on one process.  Episodes: population k
 * owns episodes [2Pk, 2Pk+P) (training, individual genome[e]) and
 * [2Pk+P, 2P(k+1)) (validation, individual genome[e]); each episode's
 * params[param[e]] carries that population's phi / tick / fee.  The last
 * workgroup of each population runs its generation boundary (sgmm_ga_step).
 * fitness/trades: [K*2P], population-major.  Two kernel launches.
 * n_pop = 1 is sgmm_generation with seed = seeds[0]. */
int sgmm_generation_multi(const sgmm_ticks *ticks, const sgmm_episodes *eps,
                          const sgmm_env_params *params, const sgmm_populations *pops,
                          double *fitness, int32_t *trades, void *workspace,
                          size_t workspace_bytes, void *stream);

/* A rank's shard of K asked populations (multi-GPU): population k owns
 * episodes [k*n_eps_pop, (k+1)*n_eps_pop) of the batch, individual
 * i0 + genome[e] of population k; fitness/trades [eps->n]. */
int sgmm_rollout_fitness_asked_multi(const sgmm_ticks *ticks, const sgmm_episodes *eps,
                                     const sgmm_env_params *params, const sgmm_populations *pops,
                                     int32_t i0, int32_t n_eps_pop, double *fitness,
                                     int32_t *trades, void *workspace, size_t workspace_bytes,
                                     void *stream);

/* One generation of K populations in the reference's order
 * (Env/drl_engine.py:92-171): the asked populations' training episodes
 * (train_eps: population k owns [kP, (k+1)P), individual genome[e]), the
 * tell of both evolvers in the training scan's tail (per population, its
 * last workgroup), then ONE validation episode per population on its new
 * master (sgmm_validate_multi) -- instead of validating every individual in
 * the training launch (sgmm_generation_multi).  Four kernel launches;
 * fitness/trades [K*P] (training), val_fitness/val_trades [K].  The workspace
 * must hold the larger of the two batches: sgmm_rollout_workspace_bytes(n,
 * steps, n_inventory, with_adversary) of each, with_adversary = masters_adv !=
 * NULL for the training batch and 0 for the validation batch.  With
 * pops->walk_order set, the training launch walks in that order and, when the
 * frontier kernel cuts some training episodes into halves (2.5-4 episodes per
 * SIMD) and the populations' episodes are of equal length, rewrites it on the
 * device after the launch so the next generation walks the lightest
 * populations whole (scheduling only: results do not depend on the order).
 * train_eps is read-only. */
int sgmm_generation_multi_best(const sgmm_ticks *ticks, const sgmm_episodes *train_eps,
                               const sgmm_episodes *val_eps, const sgmm_env_params *params,
                               const sgmm_populations *pops, double *fitness, int32_t *trades,
                               double *val_fitness, int32_t *val_trades, void *workspace,
                               size_t workspace_bytes, void *stream);

/* Validation of each population's current master (drl_engine.py:129-160),
 * after a tell (sgmm_ga_tell_multi, or the tail of sgmm_generation_multi_best):
 * val_eps holds one episode per population, episode k with genome[k] = k (row
 * k of masters_mm) and no adversary.  Then per population: improvement test
 * (strictly greater), checkpoint copy into best_masters, sigma decay, the
 * history row's validation fields, gen + 1.  Two kernel launches. */
int sgmm_validate_multi(const sgmm_ticks *ticks, const sgmm_episodes *val_eps,
                        const sgmm_env_params *params, const sgmm_populations *pops,
                        double *val_fitness, int32_t *val_trades, void *workspace,
                        size_t workspace_bytes, void *stream);

/* The tell of sgmm_ga_step_multi alone (NeuroEvolution.tell of both
 * evolvers, model.py:73-76, drl_engine.py:119-125): argmax, masters
 * regenerated, best index / training record into the state and history;
 * sgmm_validate_multi completes the generation (multi-GPU: every rank runs
 * both on the gathered training records). */
int sgmm_ga_tell_multi(const sgmm_populations *pops, const double *fitness, const int32_t *trades,
                       int64_t fit_pop_stride, int64_t trades_pop_stride, int32_t shard_n,
                       int64_t shard_stride, void *stream);

/* sgmm_ga_step for each of the K populations (one workgroup each, one
 * launch): population k reads its records at byte offset k * fit_pop_stride
 * from fitness / val_fitness and k * trades_pop_stride from trades /
 * val_trades, with the shard addressing of sgmm_ga_step (shard_n,
 * shard_stride) inside. */
int sgmm_ga_step_multi(const sgmm_populations *pops, const double *fitness, const int32_t *trades,
                       const double *val_fitness, const int32_t *val_trades,
                       int64_t fit_pop_stride, int64_t trades_pop_stride, int32_t shard_n,
                       int64_t shard_stride, void *stream);

/* Sequential float64 sum init + values[0] + values[1] + ... (device array,
 * result written to *out on the stream): the episode total of
 * Env/drl_engine.py:53 (total_reward += reward), evaluated in parallel and
 * bit-identical to the sequential loop.  The rollout uses the same routine. */
int sgmm_ordered_sum(const double *values, int64_t n, double init, double *out, void *stream);

/* ------------------------------------------------------------------------
 * Signal-bundle builder: raw snapshot / trade streams
 * of many trading days -> event bars -> SGU2 input windows -> per-step
 * bundle.  One workgroup per day.  Columns of day d occupy rows
 * [off[d], off[d+1]) and must be sorted by trade_time within the day (the
 * reference sorts with DataFrame.sort_values, HFTLoader.py:29-30).
 * ------------------------------------------------------------------------ */
typedef struct sgmm_day_streams {
    int32_t n_days;
    int32_t pad_;
    int64_t tick_total;        /* rows of the trade columns */
    const int64_t *snap_off;   /* [n_days + 1] */
    const int64_t *snap_time;  /* HHMMSSmmm */
    const double *bid, *ask, *bidvol, *askvol;  /* bidprice1 askprice1 bidvol1 askvol1 */
    const int64_t *tick_off;   /* [n_days + 1] */
    const int64_t *tick_time;
    const double *price, *volume;
    const int32_t *side;       /* +1 buy, -1 sell */
} sgmm_day_streams;            /* 104 bytes */

/* Event bars of every day, day d's events at rows snap_off[d] .. +n_events[d]
 * (capacity: the snapshot rows).  Columns as HFTMarketBase.event_df after the
 * as-of join (HFTLoader.py:26-63); statistics are NaN before the first trade. */
typedef struct sgmm_event_bars {
    int32_t *n_events;         /* [n_days] */
    int64_t *trade_time;
    double *ask, *bid, *p_buy_max, *p_sell_min, *v_buy_sum, *v_sell_sum, *vol_sum, *trade_count,
        *vwap_num;
} sgmm_event_bars;             /* 88 bytes */

size_t sgmm_event_bars_workspace_size(int64_t total_ticks);

/* HFTMarketBase (loaders/HFTLoader.py:26-63) for every day. */
int sgmm_event_bars_build(const sgmm_day_streams *in, const sgmm_event_bars *out, void *workspace,
                          size_t workspace_bytes, void *stream);

/* SGU2DataPro.gen_dataset(event_step=19, time_steps=10) (HFTLoader.py:139-169)
 * for every day: windows of day d at rows win_off[d] .. +n_windows[d] of
 * X[., 10] / y (float32).  At most 4096 bars (19-event groups) per day. */
int sgmm_bar_windows(const sgmm_event_bars *ev, int32_t n_days, const int64_t *snap_off,
                     const int64_t *win_off, float *X, float *y, int32_t *n_windows,
                     int64_t max_bars_per_day, void *stream);

/* load_signals_bundle's step loop (pipeline/agent_trainer.py:45-78): day d
 * uses its last n_samples[d] sampled events (every 19th) and writes
 * n_samples[d]-1 steps at step_off[d]: mid at the next sample, ask/bid at the
 * sample, buy_max/sell_min over the inclusive .loc window between samples. */
int sgmm_step_bundle(const sgmm_event_bars *ev, int32_t n_days, const int64_t *snap_off,
                     const int32_t *n_samples, const int64_t *step_off, int32_t max_steps,
                     double *mid, double *ask, double *bid, double *buy_max, double *sell_min,
                     void *stream);

/* ------------------------------------------------------------------------
 * SGU1: the feature table and boosted-tree inference
 * ------------------------------------------------------------------------ */

/* SGU1DataPro.gen_dataset(event_step=19) (HFTLoader.py:66-126) for every day,
 * one workgroup per day.  Rows of day d are row_off[d] .. +n_rows[d] (the
 * caller leaves room for one row per bar); n_rows[d] is the day's bar count,
 * 0 below 6 bars, -1 above 4096 bars (nothing is written then).  X is the
 * float32 matrix xgboost builds from the table, feature-major: feature f of
 * row r at X[f * ld + r], f in the order f_trades_{1,2,3,5,10},
 * f_vwap_{1,3,5}, f_slope_{1,3,5}, f_lag_rr_{1..5}, f_spread, f_vol_imb,
 * f_total_vol, f_hour.  label[ld]: the float64 label column.  F64[20 * ld]:
 * the table before the cast, same layout, or NULL.  Domain: positive finite
 * quotes (NaN trade statistics are inside it).  The rolling means are pandas'
 * sliding Kahan means bit for bit; the slopes are closed forms within
 * 4 * 2^-52 * max|mid| of the exact least-squares slope (np.polyfit is not
 * reproduced bit for bit; a flat window gives exactly +0.0). */
int sgmm_sgu1_features(const sgmm_event_bars *ev, int32_t n_days, const int64_t *snap_off,
                       const int64_t *row_off, int64_t max_bars_per_day, int64_t ld, float *X,
                       double *label, double *F64, int32_t *n_rows, void *stream);

/* Bytes of a packed forest: n_trees complete binary trees of `depth`
 * (1..6, else 0), each 2^depth - 1 internal nodes in level order (children of
 * k: 2k+1 left, 2k+2 right) of { float thr; uint32 word } -- word bits 0-4 the
 * feature, bit 31 set when a NaN feature goes left -- followed by 2^depth
 * float leaves, left to right.  A leaf above `depth` fills its whole subtree. */
size_t sgmm_sgu1_forest_bytes(int32_t depth, int32_t n_trees);

/* xgboost's CPU predictor for reg:squarederror over a packed forest in device
 * memory (16-byte aligned): out[r] = base_score, then += the leaf of tree
 * 0, 1, ... n_trees-1 in float32, in that order; at a node x[feat] < thr goes
 * left, otherwise right, NaN the default side.  X as sgmm_sgu1_features
 * writes it (20 features, ld >= n_rows).  leaves[n_rows, n_trees]: position
 * 0 .. 2^depth - 1 of the leaf each tree ends in, or NULL.  The kernel masks
 * the feature to 5 bits over a 32-column staging, so no blob content indexes
 * out of bounds.  depth > 6: SGMM_ERR_UNSUPPORTED. */
int sgmm_sgu1_predict(const void *forest_blob, size_t blob_bytes, int32_t depth, int32_t n_trees,
                      float base_score, const float *X, int64_t ld, int64_t n_rows, float *out,
                      int32_t *leaves, void *stream);

/* ------------------------------------------------------------------------
 * SGU2 inference
 * ------------------------------------------------------------------------ */

/* SGU2.predict (models/GateUnits.py:116-120): SGU2Model.forward in eval mode
 * (GateUnits.py:42-54 -- nn.LSTM(1, hidden) over each window, last hidden
 * state, Linear(hidden, 1)) for n windows X[n, time_steps, 1] (float32, the
 * windows of sgmm_bar_windows).  weights: float32 in state_dict order --
 * lstm.weight_ih_l0[4H,1], lstm.weight_hh_l0[4H,H], lstm.bias_ih_l0[4H],
 * lstm.bias_hh_l0[4H], fc.weight[1,H], fc.bias[1].  mean/std: the float32
 * StandardScaler3D fit (utils/scaler.py:9-18; agent_trainer.py:43 scales
 * before predict), applied in the kernel, or both NULL for unscaled input.
 * out: float32[n].  hidden in {10, 16, 32}. */
int sgmm_sgu2_forward(const float *weights, int32_t hidden, const float *X, int64_t n,
                      int32_t time_steps, const float *mean, const float *std, float *out,
                      void *stream);

/* ------------------------------------------------------------------------
 * SGU2 training (models/GateUnits.py:66-114 driven by
 * pipeline/sgu_trainer.py:91-112): whole fits in one launch, one workgroup
 * per fit.  Weights and Adam moments stay in LDS for the whole fit; every
 * epoch, minibatch, the validation pass, early stopping and the history run
 * on the device.  Fits are independent: K fits in one launch equal K launches
 * of one fit bit for bit, and the same inputs give the same bits on every run.
 *
 * Per minibatch: SGU2Model.forward in train mode (the sgmm_sgu2_forward
 * recurrence in its operation order, with a tanh that is accurate relative to
 * small arguments too, since the gradients are products with h; then
 * h_T * keep * 5 -- Dropout(0.8) -- then fc), MSE with the
 * mean over the minibatch, full BPTT in float32 and one torch.optim.Adam step
 * (defaults: betas 0.9 / 0.999, eps 1e-8; bias corrections in float64).  A
 * minibatch of more than 256 samples is walked in chunks of 256.  The last
 * minibatch of an epoch may be partial (drop_last=False).  Per epoch: eval
 * forward over the validation windows, train_loss[e] = sum of the minibatch
 * losses / number of minibatches, val_loss[e] = MSE (NaN when nv == 0); an
 * improvement is val_loss < best (strict, so NaN never improves); the fit stops
 * when `patience` epochs in a row did not improve (GateUnits.py:101-109).
 *
 * Schedule: the sample at position i of epoch e and the keep mask of its
 * hidden unit j.  Given explicitly (perm / keep), or generated from `seed`
 * with Philox4x32-10 (key = seed low word, seed high word):
 *   keep(e, i, j) = word (j & 3) of counter (j >> 2, i, e, 4) < 858993459
 *                   (= floor(0.2 * 2^32): keep with probability 0.2);
 *   perm(e, i): with b = max(2, bit length of n - 1), a = b / 2, c = b - a,
 *     x -> F(x): six rounds r = 0..5 of { L = x >> c; R = x & (2^c - 1);
 *     L ^= word 0 of counter (R, r, e, 3) & (2^a - 1); x = (R << a) | L },
 *     a bijection of [0, 2^b); perm = F applied to i until the value is < n
 *     (cycle walking: an exact permutation of [0, n)).
 * Stream ids 3 and 4 do not collide with the GA's (0, 1) or the bootstrap's (2).
 * ------------------------------------------------------------------------ */
typedef struct sgmm_sgu2_task {
    const float   *X_train;      /* [n, time_steps] windows */
    const float   *y_train;      /* [n] labels */
    const float   *X_val;        /* [nv, time_steps]; may be NULL when nv == 0 */
    const float   *y_val;        /* [nv] */
    float         *weights;      /* [P] sgmm_sgu2_forward layout: initial in, final out */
    float         *best_weights; /* [P] or NULL: the weights after the best epoch
                                    (written at each improvement; untouched if none) */
    const int32_t *perm;         /* [epochs, n] or NULL (Philox) */
    const uint8_t *keep;         /* [epochs, n, hidden] 0 / 1, or NULL (Philox) */
    double        *train_loss;   /* [epochs]; rows >= epochs_run are not written */
    double        *val_loss;     /* [epochs] */
    int32_t       *epochs_run;   /* [1] */
    int32_t       *best_epoch;   /* [1]; -1 when no epoch improved */
    int64_t        n;            /* training windows, 1 .. 2^31 - 1 */
    int64_t        nv;           /* validation windows, >= 0 */
    uint64_t       seed;         /* Philox key of the generated schedule */
    double         lr;           /* Adam learning rate */
} sgmm_sgu2_task;                /* 128 bytes */

/* Bytes of workspace for n_tasks fits (per fit: 256 samples x time_steps x
 * (6 hidden + 1) float32 activations for the backward pass).  A pure function
 * of its arguments; 0 for unsupported arguments. */
size_t sgmm_sgu2_train_workspace_bytes(int32_t hidden, int32_t time_steps, int32_t n_tasks);

/* n_tasks fits in one launch.  tasks: DEVICE array of records whose members
 * point to device memory; tasks_host: the HOST copy of the same records, read
 * for the argument checks (as rules_host of sgmm_rollout_summary).  mean / std:
 * the float32 StandardScaler3D fit applied to train and validation windows in
 * the kernel, or both NULL.  Labels are multiplied by label_scale
 * (sgu_trainer.py:55).  batch in 1..1024, epochs >= 0, patience >= 1,
 * time_steps >= 1, hidden in {10, 16, 32}. */
int sgmm_sgu2_train(const sgmm_sgu2_task *tasks, const sgmm_sgu2_task *tasks_host, int32_t n_tasks,
                    int32_t hidden, int32_t time_steps, int32_t batch, int32_t epochs, int32_t patience,
                    const float *mean, const float *std, float label_scale, void *workspace,
                    size_t workspace_bytes, void *stream);

/* One minibatch of the trainer's device code: X[n, time_steps], y[n], n in
 * 1..1024 -> loss[1] (MSE, mean over n) and its gradient grad[P] in the weight
 * layout.  keep: [n, hidden] 0 / 1 (train mode: h_T * keep * 5) or NULL (eval
 * mode, no dropout).  workspace: sgmm_sgu2_train_workspace_bytes(hidden,
 * time_steps, 1) bytes. */
int sgmm_sgu2_loss_grad(const float *weights, int32_t hidden, const float *X, const float *y, int32_t n,
                        int32_t time_steps, const uint8_t *keep, const float *mean, const float *std,
                        float label_scale, float *loss, float *grad, void *workspace,
                        size_t workspace_bytes, void *stream);

/* The schedule `seed` yields: perm[epochs, n] and keep[epochs, n, hidden]
 * (either may be NULL).  Passed back as a task's explicit schedule they
 * reproduce the Philox run bit for bit. */
int sgmm_sgu2_schedule(uint64_t seed, int64_t n, int32_t hidden, int32_t epochs, int32_t *perm,
                       uint8_t *keep, void *stream);

/* ------------------------------------------------------------------------
 * SGU1 training: histogram gradient-boosted trees for
 * reg:squarederror, whole fits in one launch, one workgroup per fit.  This is
 * a deterministic trainer of its own built from xgboost's objective, gain,
 * weight, node-numbering and early-stopping rules; it is NOT xgboost's
 * trainer (the cuts are not its weighted quantile sketch).  Every reduction
 * over rows is an integer sum, so the result does not depend on thread order,
 * the number of tasks of the launch or the order of the rows.
 *
 * Per round t, with pred = base_score before round 0:
 *   g_i = pred_i - y_i (float32) over the training rows, m = max |g_i|.
 *   m == 0: the tree is one leaf of value +0.  Otherwise, with e the binary
 *   exponent of m (2^(e-1) <= m < 2^e), s = 40 - e and
 *   q_i = (int64) rint((double) g_i * 2^s); the hessian is 1 per row.
 *   A node has Q = sum q_i and H = its row count;
 *   G = (double) Q * 2^-s; T(G) = G - alpha if G > alpha, G + alpha if
 *   G < -alpha, else 0; gain(G, H) = T(G) * T(G) / (H + lambda).
 *   A candidate split of a node is (feature f, cut j, missing side): rows with
 *   x_f < cuts[f][j] go left, NaN rows go to the missing side; the missing
 *   side is tried both ways only where the node has NaN rows of f (otherwise
 *   right).  It is valid when H_L >= min_child_weight and
 *   H_R >= min_child_weight; its score is (gain(L) + gain(R)) - gain(node).
 *   The best candidate has the largest score, ties to the lowest feature, then
 *   the lowest cut, then missing-right; the node splits iff that score is
 *   > gamma and > 1e-6.  Growth is depth-wise up to max_depth; node ids are
 *   xgboost's (root 0; the children of the split nodes of a level are
 *   allocated in increasing parent id, left then right).
 *   w = -T(G) / (H + lambda); a leaf's value is (float)(eta * w); base_weight
 *   is (float) w at a split node and the leaf value at a leaf; loss_change is
 *   (float) score at a split node and 0 at a leaf; sum_hessian is H.
 *   pred_i += leaf(i) in float32 for training and validation rows (the
 *   tree-order sum of sgmm_sgu1_predict).
 *   Metric over the validation rows: r_i = pred_i - y_i (float32), e2 the
 *   binary exponent of max |r_i|, s2 = 20 - e2,
 *   SSE = sum rint((double) r_i * 2^s2)^2 (int64),
 *   rmse = sqrt((double) SSE * 2^(-2 s2) / n_val), 0 when max |r_i| == 0:
 *   within about 2^-20 relative of the plain RMSE, the price of a sum that
 *   has no order.
 *   Early stopping as xgboost's: best_iteration is the first round with a
 *   strictly lower rmse; with early_stopping_rounds > 0 the fit ends after the
 *   round t with t - best_iteration >= early_stopping_rounds, so it holds
 *   best_iteration + early_stopping_rounds + 1 trees.
 * ------------------------------------------------------------------------ */
typedef struct sgmm_sgu1_task {
    const float   *X_train;      /* [20, ld_train] feature-major (sgmm_sgu1_features' layout) */
    const float   *y_train;      /* [ld_train] finite labels, indexed by row */
    const int32_t *rows_train;   /* [n_train] rows of X_train / y_train */
    const float   *X_val;        /* [20, ld_val]; the three may be NULL when n_val == 0 */
    const float   *y_val;        /* [ld_val] */
    const int32_t *rows_val;     /* [n_val] */
    const float   *cuts;         /* [20, 256]: cuts[256 f + j], j < n_cuts[f], strictly increasing */
    const int32_t *n_cuts;       /* [20], each 0 .. max_bin - 1 */
    void          *workspace;    /* sgmm_sgu1_train_workspace_bytes(n_train, n_val) bytes, 256-aligned;
                                    it begins with float pred[n_train + n_val], the running predictions
                                    of the training rows then the validation rows, final on return */
    /* outputs; node arrays hold n_estimators trees at a stride of 2^(max_depth + 1) - 1 nodes,
       ids past a tree's node count are filled with -1 (children) and 0 */
    int32_t       *left;         /* child ids, -1 at a leaf */
    int32_t       *right;
    int32_t       *feature;      /* 0 at a leaf */
    float         *value;        /* the cut of a split node, the value of a leaf */
    uint8_t       *default_left;
    float         *base_weight;
    float         *loss_change;
    float         *sum_hessian;
    int32_t       *tree_nodes;   /* [n_estimators] nodes per tree */
    double        *val_rmse;     /* [n_estimators]; rounds >= n_trees are not written */
    int32_t       *n_trees;      /* [1] */
    int32_t       *best_iteration; /* [1]; -1 when n_val == 0 */
    double        *best_score;   /* [1]; NaN when n_val == 0 */
    int64_t        ld_train;
    int64_t        ld_val;
    int32_t        n_train;      /* 1 .. 2^20 */
    int32_t        n_val;        /* 0 .. 2^23 - 1: the metric's SSE adds n_val squares of |v| <= 2^20
                                    (|r| < 2^e2, so |rint(r 2^s2)| <= 2^20) in int64, and
                                    n_val * 2^40 < 2^63 exactly when n_val <= 2^23 - 1 */
    int32_t        max_depth;    /* 1 .. 6 */
    int32_t        n_estimators; /* >= 0 */
    int32_t        early_stopping_rounds; /* 0 = off; must be 0 when n_val == 0 */
    int32_t        max_bin;      /* 2 .. 256 */
    float          base_score;
    float          reserved;
    double         min_child_weight;
    double         eta;
    double         lambda;
    double         alpha;
    double         gamma;
} sgmm_sgu1_task;                /* 264 bytes */

/* Workspace bytes of one fit (predictions, gathered labels, the uint8 bin
 * matrix with a missing mask per row, the row -> node map); a multiple of
 * 256; 0 for n_train < 1 or n_val < 0. */
size_t sgmm_sgu1_train_workspace_bytes(int64_t n_train, int64_t n_val);

/* n_tasks fits in one launch (tasks: DEVICE records, tasks_host: their HOST
 * copy for the argument checks).  A first kernel bins the rows of every task
 * against its cuts (bin = number of cuts <= x, NaN to a missing bin) and
 * gathers the labels; the second runs the fits.  The kernels clamp every row,
 * bin, node and cut index they read from device memory, so malformed index
 * lists or cuts cannot address outside their arrays; the labels must be
 * finite and the rows inside ld (the caller checks both, they live on the
 * device).  SGMM_ERR_ARG before any launch for: max_depth outside 1..6,
 * max_bin outside 2..256, n_train outside 1..2^20, n_val outside
 * 0..2^23-1 (beyond it the metric's int64 sum of squares could pass 2^63),
 * early_stopping_rounds < 0 or > 0 with n_val == 0, negative or non-finite
 * eta / lambda / alpha / gamma / min_child_weight, lambda == 0 with
 * min_child_weight == 0, a NULL member. */
int sgmm_sgu1_train(const sgmm_sgu1_task *tasks, const sgmm_sgu1_task *tasks_host, int32_t n_tasks,
                    void *stream);

/* ------------------------------------------------------------------------
 * Launch-plan overrides (ABI 5), for tests and A/B experiments.  The shipped
 * library reads no environment variable; its launch plan (policy kernel,
 * chunk groups, lane split, scan width, spill budget) follows the measured
 * rules documented in DESIGN.md unless overridden here.  Overrides are
 * process-wide and apply to launches ENQUEUED after the call (a captured HIP
 * graph keeps the plan it was captured with); set them before building
 * workspaces, since the workspace size follows the plan.  value < 0 restores
 * the default rule.  sgmm_plan_set returns 0 or SGMM_ERR_ARG (unknown knob);
 * sgmm_plan_get returns the override, -1 for the default rule, or INT32_MIN for
 * an unknown knob.  (A build with -DSGMM_EXPERIMENTS also takes the initial
 * values from the SGMM_* environment variables named in DESIGN.md.)
 * ------------------------------------------------------------------------ */
enum {
    SGMM_PLAN_POLICY_PATH = 0,   /* 0 auto, 1 frontier, 2 MFMA table, 3 VALU table */
    SGMM_PLAN_GROUPS = 1,        /* frontier chunk groups per episode, 1..16 */
    SGMM_PLAN_LANE_SPLIT = 2,    /* frontier waves per walk: 1, 2 or 4 */
    SGMM_PLAN_TAIL = 3,          /* 0: no split tail walks (every walk whole) */
    SGMM_PLAN_FOUR = 4,          /* 0: no four-walk rule */
    SGMM_PLAN_MIN_EPS = 5,       /* frontier kernel from this many episodes */
    SGMM_PLAN_TABLE_SP = 6,      /* 0 / 1: state-parallel table off / forced */
    SGMM_PLAN_SCAN_THREADS = 7,  /* path-scan workgroup: 64, 256, 512 or 1024 */
    SGMM_PLAN_REORDER_WEIGHTS = 8, /* walk-order scores: whole << 8 | split */
    SGMM_PLAN_SPILL = 9,         /* frontier spill deadline, us after a walk's start (0: off) */
    SGMM_PLAN_SEQ_SUM = 10,      /* path-scan episode sums: 0 exact parallel method, 1 sequential chain */
    SGMM_PLAN_FUSED_SCAN = 11,   /* frontier launches: 0 separate path scan, 1 scans fused into the walks */
    SGMM_PLAN_LANES_SCAN = 12,   /* frontier path scan: 1 = 2-4 episodes per workgroup, chains in lanes (2 / 4 force
                                    the count); 0 = one episode per wave */
    SGMM_PLAN_N = 13
};
int sgmm_plan_set(int32_t knob, int32_t value);
int sgmm_plan_get(int32_t knob);

/* Kernel timing for benchmarks / diagnostics (not on by default).
 * While enabled, every kernel the library launches is bracketed by a pair of
 * hipEvents recorded on its stream.  sgmm_profile_read waits for the recorded
 * events, writes up to max_kinds entries (name[i] = names + 48*i,
 * NUL-terminated; total_ms[i]; count[i]) and clears the record.  Returns the
 * number of kernel kinds written, or < 0 on error. */
int sgmm_profile_enable(int enable);
int sgmm_profile_read(int max_kinds, char *names, double *total_ms, int64_t *count);

#ifdef __cplusplus
}
#endif

#endif /* SGMM_H */
