// sgmm_hypothesis.hip -- the hypothesis tests of the evaluation stage on gfx950:
// Diebold-Mariano, Durbin-Watson and the moving-block bootstrap of the per-step
// Sharpe ratio, batched over many series, plus the wealth column of a trace.
//
// Reference semantics:
//   main.py:228-236   dm_test
//   main.py:247       statsmodels' durbin_watson (the textbook ratio)
//   main.py:251-285   get_mbb_sharpe
//   Env/recorder.py:46  wealth = cash + inventory * mid
//
// Kernels.
//   k_trace_wealth    one thread per step; the episode of a step is found by a
//     binary search of step_off.
//   k_series_tests    one wave per series: the DM moments (two passes) or the
//     two DW sums.
//   k_mbb_returns     one workgroup per series: r = w[t+1] / w[t] - 1, the
//     non-NaN values compacted in order (ballot + popcount inside a wave, the
//     four wave counts through LDS).
//   k_mbb_replicates  one wave per replicate, four replicates per workgroup.
//     A lane keeps the start of one block in a register (64 blocks per round)
//     and the wave fetches them with a lane shuffle, so a row of 64 elements is
//     64 consecutive doubles of a block (two blocks where a row crosses a
//     boundary).  The series' returns are read 2 * n_boot times from L2 / L1;
//     the kernel is bound by its vector instructions, not by those reads
//     (DESIGN 10.1).
//   k_mbb_reduce      one workgroup per series: the replicates' mean, then a
//     bitonic sort in LDS (padded with +inf to a power of two) and numpy's two
//     linear-rule percentiles; the n <= block_size branch is evaluated here.
//
// Every sum is the LANE SUM of include/sgmm.h: element i in lane i mod 64, a
// lane adds in increasing i from 0.0, the lanes are combined by the xor
// butterfly 32, 16, ..., 1.  analytics.py restates it in numpy.
#include <climits>
#include <cmath>

#include "sgmm_device.h"
#include "sgmm_internal.h"

namespace sgmm {

constexpr int kHypThreads = 256;
constexpr int kHypWaves = kHypThreads / kWave;
constexpr int kMaxBoot = 4096;
constexpr int kRows = 4;  // rows of 64 elements a replicate wave loads before it adds them

__device__ __forceinline__ double lane_combine(double v) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// lane sum of f(0) .. f(n - 1); every lane of the wave must call it
template <class F>
__device__ __forceinline__ double lane_sum(int64_t n, int lane, F f) {
    double acc = 0.0;
    for (int64_t i = lane; i < n; i += kWave) acc += f(i);
    return lane_combine(acc);
}

struct Series {
    int64_t a, n;
};
// offsets that decrease read as an empty series
__device__ __forceinline__ Series series_at(const int64_t* __restrict__ off, int s) {
    const int64_t a = off[s], b = off[s + 1];
    return Series{a, b > a ? b - a : 0};
}

// mean / std if std > 1e-9 else 0 (main.py:259-260, 278-282): a NaN std compares false
__device__ __forceinline__ double sharpe_of(double mean, double var) {
    const double sd = sqrt(var);
    return sd > 1e-9 ? mean / sd : 0.0;
}

// ------------------------------------------------------------------ wealth
__global__ __launch_bounds__(kHypThreads) void k_trace_wealth(
    const double* __restrict__ mid, const int64_t* __restrict__ tick_off,
    const int32_t* __restrict__ len, const int64_t* __restrict__ step_off, int32_t n_eps,
    int64_t total, const int32_t* __restrict__ inv, const double* __restrict__ cash,
    double* __restrict__ w) {
    const int64_t g = (int64_t)blockIdx.x * kHypThreads + threadIdx.x;
    if (g >= total) return;
    int lo = 0, hi = n_eps;  // the last episode with step_off <= g: empty ones share their successor's
    while (hi - lo > 1) {
        const int m = lo + (hi - lo) / 2;
        if (step_off[m] <= g) lo = m; else hi = m;
    }
    const int64_t t = g - step_off[lo];
    if (t < 0 || t >= len[lo]) return;  // step_off is not the prefix sum of len: nothing read
    w[g] = cash[g] + (double)inv[g] * mid[tick_off[lo] + t];  // Env/recorder.py:46
}

// ------------------------------------------------------------------ DM / DW
struct SeriesTests {
    const double *a, *p1, *p2;
    const int64_t* off;
    int32_t n_series, mode;  // 0: DM on MSE, 1: DM on MAD, 2: DW
    double* dw;
    sgmm_dm_result* dm;
};

__global__ __launch_bounds__(kHypThreads) void k_series_tests(SeriesTests q) {
    const int s = blockIdx.x * kHypWaves + threadIdx.x / kWave;
    const int lane = threadIdx.x % kWave;
    if (s >= q.n_series) return;  // whole waves leave; no barrier below
    const Series sr = series_at(q.off, s);
    const double* __restrict__ a = q.a + sr.a;
    if (q.mode == 2) {  // sum (e[t] - e[t-1])^2 / sum e[t]^2
        const double num = lane_sum(sr.n - 1, lane, [&](int64_t i) {
            const double d = a[i + 1] - a[i];
            return d * d;
        });
        const double den = lane_sum(sr.n, lane, [&](int64_t i) { return a[i] * a[i]; });
        if (lane == 0) q.dw[s] = num / den;
        return;
    }
    const double* __restrict__ p1 = q.p1 + sr.a;
    const double* __restrict__ p2 = q.p2 ? q.p2 + sr.a : nullptr;
    const bool mse = q.mode == 0;
    auto d_at = [&](int64_t i) {  // main.py:229-231
        const double x = a[i];
        const double u = x - p1[i], v = x - (p2 ? p2[i] : 0.0);
        const double e1 = mse ? u * u : fabs(u), e2 = mse ? v * v : fabs(v);
        return e1 - e2;
    };
    const double nd = (double)sr.n;
    const double mean = lane_sum(sr.n, lane, d_at) / nd;
    const double ss = lane_sum(sr.n, lane, [&](int64_t i) {
        const double c = d_at(i) - mean;
        return c * c;
    });
    const double var = sr.n < 2 ? __builtin_nan("") : ss / (double)(sr.n - 1);  // ddof = 1
    const double stat = mean / sqrt(var / nd);
    const double p = 2.0 * (1.0 - 0.5 * erfc((-fabs(stat)) / sqrt(2.0)));
    if (lane == 0) q.dm[s] = sgmm_dm_result{stat, p, mean, var, sr.n};
}

// ------------------------------------------------------------------ bootstrap: returns
__global__ __launch_bounds__(kHypThreads) void k_mbb_returns(
    const double* __restrict__ w, const int64_t* __restrict__ off, int32_t block_size,
    double* __restrict__ returns, sgmm_mbb_result* __restrict__ out) {
    __shared__ int32_t wave_cnt[kHypWaves];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid % kWave, wv = tid / kWave;
    const Series sr = series_at(off, s);
    const int64_t m = sr.n > 0 ? sr.n - 1 : 0;  // pct_change's first row is NaN: dropped
    const double* __restrict__ ws = w + sr.a;
    double* __restrict__ rs = returns + sr.a;
    int64_t kept = 0;  // uniform over the workgroup
    for (int64_t base = 0; base < m; base += kHypThreads) {
        const int64_t i = base + tid;
        double r = 0.0;
        bool keep = false;
        if (i < m) {
            r = ws[i + 1] / ws[i] - 1.0;
            keep = r == r;  // dropna: NaN goes, +-inf stays
        }
        const uint64_t mask = __ballot(keep);
        if (lane == 0) wave_cnt[wv] = __popcll(mask);
        __syncthreads();
        int32_t before = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int k = 0; k < kHypWaves; ++k) {
            const int32_t c = wave_cnt[k];
            before += k < wv ? c : 0;
            total += c;
        }
        if (keep) rs[kept + before] = r;  // kept + before <= i: inside the series' slots
        kept += total;
        __syncthreads();  // wave_cnt is rewritten by the next round
    }
    if (tid == 0) {
        const int32_t n = (int32_t)kept;
        const int32_t nb = n > block_size ? n / block_size : 0;  // main.py:258, 264
        out[s] = sgmm_mbb_result{0.0, 0.0, 0.0, n, nb, 0, nb ? 0 : SGMM_MBB_NOT_RESAMPLED};
    }
}

// ------------------------------------------------------------------ bootstrap: replicates
__global__ __launch_bounds__(kHypThreads) void k_mbb_replicates(
    const double* __restrict__ returns, const int64_t* __restrict__ off, int32_t bs, int32_t n_boot,
    int32_t tiles, const int32_t* __restrict__ starts, int64_t stride, uint64_t seed,
    sgmm_mbb_result* out, double* __restrict__ boot, int32_t* __restrict__ starts_out) {
    const int s = blockIdx.x / tiles;
    const int b = (blockIdx.x % tiles) * kHypWaves + threadIdx.x / kWave;
    const int lane = threadIdx.x % kWave;
    if (b >= n_boot) return;  // whole waves leave; no barrier below
    const int32_t n = out[s].n_returns, nb = out[s].num_blocks;
    if (nb == 0) return;  // not resampled: k_mbb_reduce fills the row
    const double* __restrict__ r = returns + off[s];
    const int32_t span = n - bs;  // the largest start; >= 1 here
    const int64_t row = ((int64_t)s * n_boot + b) * stride;
    const int32_t q64 = kWave / bs, r64 = kWave % bs;
    bool clamped = false;

    // the start of block 64 c + lane (0 past the last block: never used)
    auto round_starts = [&](int32_t c, bool first) {
        const int32_t j = c * kWave + lane;
        int32_t st = 0;
        if (j < nb) {
            if (starts) {
                const int32_t v = starts[row + j];
                st = v < 0 ? 0 : (v > span ? span : v);
                clamped |= v != st;
            } else {
                const U4 x = philox4x32_10(U4{(uint32_t)(j >> 2), (uint32_t)b, (uint32_t)s, 2u},
                                           (uint32_t)seed, (uint32_t)(seed >> 32));
                const uint32_t word = (j & 2) ? ((j & 1) ? x.w : x.z) : ((j & 1) ? x.y : x.x);
                st = (int32_t)(((uint64_t)word * (uint64_t)(span + 1)) >> 32);
            }
            if (first && starts_out) starts_out[row + j] = st;
        }
        return st;
    };
    // lane sum over the replicate's nb * bs elements of x (first) or (x - mean)^2.
    // A round covers 64 blocks = 64 * bs elements, a multiple of 64, so element
    // i of the replicate sits in lane i mod 64 in every round.  Round 0's starts
    // (all of them up to 64 blocks) are drawn once and kept for both passes.
    const int32_t st0 = round_starts(0, true);
    auto pass = [&](double mean, bool first) {
        double acc = 0.0;
        for (int32_t c = 0; c * kWave < nb; ++c) {
            const int32_t st = c == 0 ? st0 : round_starts(c, first);
            const int32_t blocks = nb - c * kWave < kWave ? nb - c * kWave : kWave;
            const int32_t elems = blocks * bs;      // <= nb * bs <= n: fits
            int32_t jl = lane / bs, o = lane % bs;  // block within the round, offset within the block
            // kRows rows of 64 elements at a time, without a branch: a lane past the end
            // loads r[0] and adds nothing, so the rows' shuffles and loads are issued
            // back to back and only then added, in row order.  Every lane shuffles.
            for (int32_t e0 = 0; e0 < elems; e0 += kRows * kWave) {
                double x[kRows];
                bool in[kRows];
#pragma unroll
                for (int k = 0; k < kRows; ++k) {
                    const int32_t sj = __shfl(st, jl & (kWave - 1));
                    in[k] = e0 + k * kWave + lane < elems;  // then jl < blocks: sj in [0, n - bs], sj + o < n
                    x[k] = r[in[k] ? sj + o : 0];
                    jl += q64;
                    o += r64;
                    const bool wrap = o >= bs;
                    o -= wrap ? bs : 0;
                    jl += wrap ? 1 : 0;
                }
#pragma unroll
                for (int k = 0; k < kRows; ++k) {
                    const double d = x[k] - mean;
                    const double v = first ? x[k] : d * d;
                    acc = in[k] ? acc + v : acc;
                }
            }
        }
        return lane_combine(acc);
    };
    const double cnt = (double)((int64_t)nb * bs);
    const double mean = pass(0.0, true) / cnt;
    const double var = pass(mean, false) / cnt;  // np.std: ddof = 0
    if (lane == 0) boot[(int64_t)s * n_boot + b] = sharpe_of(mean, var);
    if (__any(clamped) && lane == 0) atomicOr(&out[s].flags, SGMM_MBB_CLAMPED);
}

// ------------------------------------------------------------------ bootstrap: percentiles
// numpy sorts NaN last
__device__ __forceinline__ bool sorts_after(double a, double b) { return a > b || (a != a && b == b); }

__global__ __launch_bounds__(kHypThreads) void k_mbb_reduce(
    const double* __restrict__ returns, const int64_t* __restrict__ off, int32_t n_boot,
    sgmm_mbb_result* __restrict__ out, double* __restrict__ boot) {
    __shared__ double sh[kMaxBoot];
    __shared__ double sh_mean;
    __shared__ int32_t sh_zero, sh_nan;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid % kWave;
    sgmm_mbb_result* __restrict__ o = out + s;
    const int32_t n = o->n_returns, nb = o->num_blocks;
    double* __restrict__ bt = boot + (int64_t)s * n_boot;

    if (nb == 0) {  // main.py:258-261: the plain ratio over the returns, no bootstrap
        if (tid < kWave) {
            const double* __restrict__ r = returns + off[s];
            const double nd = (double)n;
            const double mean = lane_sum(n, lane, [&](int64_t i) { return r[i]; }) / nd;
            const double var = lane_sum(n, lane, [&](int64_t i) {
                const double d = r[i] - mean;
                return d * d;
            }) / nd;
            if (lane == 0) sh_mean = sharpe_of(mean, var);  // n = 0: NaN std -> 0
        }
        __syncthreads();
        const double sr = sh_mean;
        for (int32_t b = tid; b < n_boot; b += kHypThreads) bt[b] = sr;
        if (tid == 0) {
            o->mean_sr = o->ci_lo = o->ci_hi = sr;
            o->zero_replicates = sr == 0.0 ? n_boot : 0;
        }
        return;
    }

    int32_t P = 1;
    while (P < n_boot) P <<= 1;
    for (int32_t i = tid; i < P; i += kHypThreads) sh[i] = i < n_boot ? bt[i] : __builtin_inf();
    if (tid < kWave) {  // np.mean(boot_srs) in replicate order, and the zero / NaN counts
        int32_t zeros = 0, nans = 0;
        double acc = 0.0;
        for (int32_t i = lane; i < n_boot; i += kWave) {
            const double v = bt[i];
            acc += v;
            zeros += v == 0.0;
            nans += v != v;
        }
        acc = lane_combine(acc);
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) {
            zeros += __shfl_xor(zeros, d);
            nans += __shfl_xor(nans, d);
        }
        if (lane == 0) {
            sh_mean = acc / (double)n_boot;
            sh_zero = zeros;
            sh_nan = nans;
        }
    }
    __syncthreads();
    for (int32_t k = 2; k <= P; k <<= 1) {
        for (int32_t j = k >> 1; j > 0; j >>= 1) {
            for (int32_t i = tid; i < P; i += kHypThreads) {
                const int32_t l = i ^ j;
                if (l > i) {
                    const double a = sh[i], c = sh[l];
                    if (sorts_after(a, c) == ((i & k) == 0)) {
                        sh[i] = c;
                        sh[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        auto percentile = [&](double q) {  // numpy's linear rule (_quantile, _lerp)
            const double v = (double)(n_boot - 1) * q;
            const double fl = floor(v);
            const int32_t lo = (int32_t)fl, hi = lo + 1 < n_boot ? lo + 1 : n_boot - 1;
            const double t = v - fl, a = sh[lo], c = sh[hi], diff = c - a;
            return t >= 0.5 ? c - diff * (1.0 - t) : a + diff * t;
        };
        const bool has_nan = sh_nan != 0;
        o->mean_sr = sh_mean;
        o->ci_lo = has_nan ? __builtin_nan("") : percentile(2.5 / 100.0);
        o->ci_hi = has_nan ? __builtin_nan("") : percentile(97.5 / 100.0);
        o->zero_replicates = sh_zero;
    }
}

// ------------------------------------------------------------------ host side
static int check_series(bool values_ok, const int64_t* off, const int64_t* off_host, int32_t n_series) {
    SGMM_REQUIRE(n_series >= 0, "n_series=%d < 0", n_series);
    if (n_series == 0) return SGMM_OK;
    SGMM_REQUIRE(off, "null off");
    if (off_host) {
        SGMM_REQUIRE(off_host[0] >= 0, "off[0]=%lld < 0", (long long)off_host[0]);
        for (int32_t s = 0; s < n_series; ++s) {
            SGMM_REQUIRE(off_host[s + 1] >= off_host[s], "off decreases at series %d", s);
            SGMM_REQUIRE(off_host[s + 1] - off_host[s] < INT32_MAX, "series %d is too long", s);
        }
    }
    // an all-empty batch has nothing to point at
    SGMM_REQUIRE(values_ok || (off_host && off_host[n_series] == off_host[0]), "null series values");
    return SGMM_OK;
}

static inline dim3 wave_grid(int32_t n_series) { return dim3((n_series + kHypWaves - 1) / kHypWaves); }

}  // namespace sgmm

using namespace sgmm;

extern "C" int sgmm_trace_wealth(const sgmm_ticks* ticks, const sgmm_episodes* eps,
                                 const int32_t* inventory, const double* cash, double* wealth,
                                 void* stream) {
    clear_error();
    SGMM_REQUIRE(ticks && eps, "null ticks/episodes");
    SGMM_REQUIRE(eps->n >= 0 && eps->total_steps >= 0, "n episodes / total_steps < 0");
    if (eps->n == 0 || eps->total_steps == 0) return SGMM_OK;
    SGMM_REQUIRE(eps->tick_off && eps->len && eps->step_off, "null episode array");
    SGMM_REQUIRE(ticks->mid_next, "null tick column");
    SGMM_REQUIRE(inventory && cash && wealth, "null inventory/cash/wealth");
    const int64_t blocks = (eps->total_steps + kHypThreads - 1) / kHypThreads;
    SGMM_REQUIRE(blocks <= INT32_MAX, "total_steps too large");
    hipStream_t s = as_stream(stream);
    ProfScope prof("trace_wealth", s);
    SGMM_LAUNCH(k_trace_wealth, dim3((uint32_t)blocks), dim3(kHypThreads), 0, s, ticks->mid_next,
                eps->tick_off, eps->len, eps->step_off, eps->n, eps->total_steps, inventory, cash, wealth);
    SGMM_LAUNCHED();
    return SGMM_OK;
}

extern "C" int sgmm_durbin_watson(const double* values, const int64_t* off, const int64_t* off_host,
                                  int32_t n_series, double* out, void* stream) {
    clear_error();
    if (int rc = check_series(values != nullptr, off, off_host, n_series)) return rc;
    if (n_series == 0) return SGMM_OK;
    SGMM_REQUIRE(out, "null out");
    hipStream_t s = as_stream(stream);
    ProfScope prof("series_tests", s);
    SGMM_LAUNCH(k_series_tests, wave_grid(n_series), dim3(kHypThreads), 0, s,
                SeriesTests{values, nullptr, nullptr, off, n_series, 2, out, nullptr});
    SGMM_LAUNCHED();
    return SGMM_OK;
}

extern "C" int sgmm_dm_test(const double* actual, const double* pred1, const double* pred2,
                            const int64_t* off, const int64_t* off_host, int32_t n_series,
                            int32_t crit, sgmm_dm_result* out, void* stream) {
    clear_error();
    SGMM_REQUIRE(crit == 0 || crit == 1, "crit=%d (0: MSE, 1: MAD)", crit);
    if (int rc = check_series(actual && pred1, off, off_host, n_series)) return rc;
    if (n_series == 0) return SGMM_OK;
    SGMM_REQUIRE(out, "null out");
    hipStream_t s = as_stream(stream);
    ProfScope prof("series_tests", s);
    SGMM_LAUNCH(k_series_tests, wave_grid(n_series), dim3(kHypThreads), 0, s,
                SeriesTests{actual, pred1, pred2, off, n_series, crit, nullptr, out});
    SGMM_LAUNCHED();
    return SGMM_OK;
}

extern "C" int sgmm_mbb_sharpe(const double* wealth, const int64_t* off, const int64_t* off_host,
                               int32_t n_series, int32_t block_size, int32_t n_boot,
                               const int32_t* starts, int64_t starts_stride, uint64_t seed,
                               sgmm_mbb_result* out, double* boot, int32_t* starts_out,
                               double* returns, void* stream) {
    clear_error();
    SGMM_REQUIRE(block_size >= 1 && block_size <= (1 << 30), "block_size=%d outside [1, 2^30]", block_size);
    SGMM_REQUIRE(n_boot >= 1 && n_boot <= kMaxBoot, "n_boot=%d outside [1, %d]", n_boot, kMaxBoot);
    if (int rc = check_series(wealth != nullptr, off, off_host, n_series)) return rc;
    if (starts || starts_out) {
        // the rows of starts / starts_out are sized on the host: the lengths must be known here
        SGMM_REQUIRE(off_host, "starts / starts_out need off_host");
        SGMM_REQUIRE(starts_stride >= 1, "starts_stride=%lld < 1", (long long)starts_stride);
        for (int32_t s = 0; s < n_series; ++s) {
            const int64_t len = off_host[s + 1] - off_host[s];
            const int64_t n_max = len > 0 ? len - 1 : 0;  // before the NaN drop
            SGMM_REQUIRE(n_max <= block_size || n_max / block_size <= starts_stride,
                         "starts_stride=%lld < the %lld blocks series %d may have",
                         (long long)starts_stride, (long long)(n_max / block_size), s);
        }
    }
    if (n_series == 0) return SGMM_OK;
    SGMM_REQUIRE(out && boot, "null out / boot");
    SGMM_REQUIRE(returns || (off_host && off_host[n_series] == off_host[0]), "null returns");
    SGMM_REQUIRE(returns != wealth || !wealth, "returns must not alias wealth");
    const int32_t tiles = (n_boot + kHypWaves - 1) / kHypWaves;
    SGMM_REQUIRE((int64_t)n_series * tiles <= INT32_MAX, "n_series * n_boot too large");
    hipStream_t s = as_stream(stream);
    {
        ProfScope prof("mbb_returns", s);
        SGMM_LAUNCH(k_mbb_returns, dim3(n_series), dim3(kHypThreads), 0, s, wealth, off, block_size,
                    returns, out);
        SGMM_LAUNCHED();
    }
    {
        ProfScope prof("mbb_replicates", s);
        SGMM_LAUNCH(k_mbb_replicates, dim3(n_series * tiles), dim3(kHypThreads), 0, s, returns, off,
                    block_size, n_boot, tiles, starts, starts_stride, seed, out, boot, starts_out);
        SGMM_LAUNCHED();
    }
    {
        ProfScope prof("mbb_reduce", s);
        SGMM_LAUNCH(k_mbb_reduce, dim3(n_series), dim3(kHypThreads), 0, s, returns, off, n_boot, out,
                    boot);
        SGMM_LAUNCHED();
    }
    return SGMM_OK;
}
