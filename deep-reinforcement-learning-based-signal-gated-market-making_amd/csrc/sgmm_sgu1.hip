// sgmm_sgu1.hip -- SGU1 on gfx950: the per-bar feature
// table of SGU1DataPro.gen_dataset(19) and boosted-tree inference over it.
//
// Reference semantics:
//   feature table  loaders/HFTLoader.py:66-126: per 19-event bar a label, the
//                  trade count, vwap, closing mid, volume imbalance, opening
//                  spread, volume and hour; then rolling sums / means / slopes
//                  and lags of them, shift(1), ffill().bfill().dropna().
//                  Inside the domain (positive finite quotes) NaN arises only
//                  from the shifts, so the filling is "leading rows take the
//                  first valid value" and a day keeps all of its bars when it
//                  has at least 6 of them (f_lag_rr_5 is all NaN below that).
//   rolling mean   pandas' sliding Kahan roll_mean (window/aggregations.pyx):
//                  one running sum per window with separate add and remove
//                  compensations, not a fresh mean per window.
//   slope          np.polyfit(arange(m), y, 1)[0] restated in closed form on
//                  differences (exactly +0.0 on a flat window); LAPACK's SVD
//                  is not reproduced bit for bit.
//   forest         xgboost's CPU predictor for reg:squarederror: float32
//                  base_score, then `pred += leaf` per tree in order; at a node
//                  x[feat] < thr goes left, NaN takes the default side.
#include <cmath>

#include "sgmm_bars_device.h"
#include "sgmm_device.h"
#include "sgmm_internal.h"

namespace sgmm {

constexpr int kSgu1Features = 20;

// pandas' roll_mean(values, window w, min_periods 1) at every index, NaN-free
// input: the serial chain of one lane.  out(i, mean_i) is called in order.
template <class Out>
__device__ __forceinline__ void roll_mean_chain(const double* v, int n, int w, Out out) {
    double sum = 0.0, c_add = 0.0, c_rm = 0.0, prev = n > 0 ? v[0] : 0.0;
    int nobs = 0, neg = 0, same = 0;
    for (int i = 0; i < n; ++i) {
        if (i >= w) {  // remove_mean of the value that leaves the window
            const double x = v[i - w];
            const double y = -x - c_rm;
            const double t = sum + y;
            c_rm = t - sum - y;
            sum = t;
            nobs -= 1;
            neg -= signbit(x) ? 1 : 0;
        }
        {  // add_mean
            const double x = v[i];
            const double y = x - c_add;
            const double t = sum + y;
            c_add = t - sum - y;
            sum = t;
            nobs += 1;
            neg += signbit(x) ? 1 : 0;
            same = x == prev ? same + 1 : 1;
            prev = x;
        }
        double r = sum / (double)nobs;  // calc_mean
        if (same >= nobs) r = prev;
        else if (neg == 0 && r < 0.0) r = 0.0;
        else if (neg == nobs && r > 0.0) r = 0.0;
        out(i, r);
    }
}

// least-squares slope of y[0..m-1] against 0..m-1, m <= 5
__device__ __forceinline__ double slope_closed(const double* y, int m) {
    switch (m) {
    case 2: return y[1] - y[0];
    case 3: return (y[2] - y[0]) / 2.0;
    case 4: return (3.0 * (y[3] - y[0]) + (y[2] - y[1])) / 10.0;
    case 5: return (2.0 * (y[4] - y[0]) + (y[3] - y[1])) / 10.0;
    default: return 0.0;
    }
}

// One workgroup per day.  Row r of the table is bar r; column f of row r goes
// to X[f * ld + row_off[d] + r] (float32) and F64 (the table before the cast).
__global__ __launch_bounds__(kDayBlock) void k_sgu1_features(sgmm_event_bars ev, const int64_t* snap_off,
                                                             const int64_t* row_off, int64_t ld, float* X,
                                                             double* label_out, double* F64,
                                                             int32_t* n_rows) {
    __shared__ double tr[kMaxBars];
    __shared__ double vwap[kMaxBars];
    __shared__ double mid[kMaxBars];
    __shared__ double lab[kMaxBars];
    const int d = blockIdx.x, tid = threadIdx.x;
    const int64_t e0 = snap_off[d];
    const int n_ev = ev.n_events[d];
    const int nb = n_ev > kEventStep ? (n_ev - kEventStep + kEventStep - 1) / kEventStep : 0;  // len(range(0, n-19, 19))
    if (nb > kMaxBars || nb < 6) {  // never index past the LDS arrays; below 6 bars dropna leaves no row
        if (tid == 0) n_rows[d] = nb > kMaxBars ? -1 : 0;
        return;
    }
    const int64_t r0 = row_off[d];
    auto put = [&](int f, int r, double v) {
        const int64_t o = (int64_t)f * ld + r0 + r;
        X[o] = (float)v;
        if (F64) F64[o] = v;
    };
    // shift(1) then bfill: the value of bar b is the feature of row b + 1, and of row 0 when b = 0
    auto put_shifted = [&](int f, int b, double v) {
        if (b + 1 < nb) put(f, b + 1, v);
        if (b == 0) put(f, 0, v);
    };
    for (int b = tid; b < nb; b += kDayBlock) {
        const int64_t a = e0 + (int64_t)b * kEventStep;
        const double bmax = nan_max_run(ev.p_buy_max + a, kEventStep);
        const double smin = nan_min_run(ev.p_sell_min + a, kEventStep);
        const double am = skipna_mean_19(ev.ask + a);
        const double bm = skipna_mean_19(ev.bid + a);
        double x;
        if (bmax == bmax && smin == smin) x = bmax - smin;
        else if (smin == smin) x = am - smin;
        else if (bmax == bmax) x = bmax - bm;
        else x = am - bm;
        const double l = rint(x * 1e4) / 1e4;  // round(label, 4)
        const double vol = skipna_sum_19(ev.vol_sum + a);
        tr[b] = skipna_sum_19(ev.trade_count + a);
        vwap[b] = skipna_sum_19(ev.vwap_num + a) / (vol + 1e-9);
        mid[b] = (ev.ask[a + kEventStep - 1] + ev.bid[a + kEventStep - 1]) / 2.0;
        lab[b] = l;
        label_out[r0 + b] = l;
        put_shifted(16, b, ev.ask[a] - ev.bid[a]);
        put_shifted(17, b, (skipna_sum_19(ev.v_buy_sum + a) - skipna_sum_19(ev.v_sell_sum + a)) / (vol + 1e-9));
        put_shifted(18, b, vol);
        put(19, b, (double)(ev.trade_time[a] / 10000000));
    }
    __syncthreads();
    // f_vwap_3 / f_vwap_5: one lane of wave 0 and one of wave 1 walk the day
    if (tid == 0 || tid == kWave) {
        const int w = tid == 0 ? 3 : 5, f = tid == 0 ? 6 : 7;
        roll_mean_chain(vwap, nb, w, [&](int i, double r) { put_shifted(f, i, r); });
    }
    for (int r = tid; r < nb; r += kDayBlock) {
        const int p = r > 0 ? r - 1 : 0;
        const int win[5] = {1, 2, 3, 5, 10};
        double s = 0.0;
        int k = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {  // f_trades_p: integers below 2^53, any order is exact
            for (; k < win[j]; ++k) s += p - k >= 0 ? tr[p - k] : 0.0;
            put(j, r, s);
        }
        put(5, r, vwap[p]);  // a window of 1 is set up afresh at every index: the value itself
        put(8, r, 0.0);      // get_slope of one point
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int sw = j == 0 ? 3 : 5;
            const int m = p + 1 < sw ? p + 1 : sw;
            double y[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) y[i] = i < m ? mid[p - m + 1 + i] : 0.0;
            put(9 + j, r, slope_closed(y, m));
        }
#pragma unroll
        for (int L = 1; L <= 5; ++L) put(10 + L, r, lab[r - L > 0 ? r - L : 0]);
    }
    if (tid == 0) n_rows[d] = nb;
}

// ---------------------------------------------------------------- forest
// Packed forest: every tree a complete binary tree of depth D, internal node k
// with children 2k+1 / 2k+2.  Per tree 2^D - 1 nodes of {float thr, uint32
// word} (word: bits 0-4 the feature, bit 31 default-left), then 2^D leaf floats.
constexpr int kForestBlock = 256;
constexpr int kForestCols = 32;            // 5 feature bits: any word indexes inside the staging
constexpr int kForestLdsWords = 30 * 1024; // 120 KiB of forest beside the 32 KiB of features
#ifndef SGMM_FOREST_ILP
#define SGMM_FOREST_ILP 16
#endif
constexpr int kForestIlp = SGMM_FOREST_ILP;  // trees walked at once

__host__ __device__ constexpr int forest_tree_words(int D) { return 3 * (1 << D) - 2; }

// W trees from LDS word offset `base` on: the W walks advance level by level
// together (W independent chains of dependent LDS reads); the leaves are added
// in tree order
template <int D, int W>
__device__ __forceinline__ void forest_walk(const uint32_t* forest, int base, const float* xcol, float& pred,
                                            int32_t* leaves) {
    constexpr int TW = forest_tree_words(D), NI = (1 << D) - 1;
    int k[W];
#pragma unroll
    for (int j = 0; j < W; ++j) k[j] = 0;
#pragma unroll
    for (int l = 0; l < D; ++l) {
        uint2 nd[W];
#pragma unroll
        for (int j = 0; j < W; ++j) nd[j] = *reinterpret_cast<const uint2*>(forest + base + j * TW + 2 * k[j]);
        float x[W];
#pragma unroll
        for (int j = 0; j < W; ++j) x[j] = xcol[(nd[j].y & (kForestCols - 1)) * kForestBlock];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const bool left = x[j] != x[j] ? (nd[j].y >> 31) != 0 : x[j] < __uint_as_float(nd[j].x);
            k[j] = 2 * k[j] + (left ? 1 : 2);
        }
    }
    float leaf[W];
#pragma unroll
    for (int j = 0; j < W; ++j) leaf[j] = __uint_as_float(forest[base + j * TW + NI + k[j]]);  // 2*NI + (k - NI)
#pragma unroll
    for (int j = 0; j < W; ++j) {
        pred = pred + leaf[j];
        if (leaves) leaves[j] = k[j] - NI;
    }
}

// One thread per row; the forest is walked in LDS-sized chunks of whole trees
// with the float32 partial sum carried in a register.
template <int D>
__global__ __launch_bounds__(kForestBlock) void k_sgu1_forest(const uint32_t* blob, int n_trees, float base_score,
                                                              const float* X, int64_t ld, int64_t n_rows,
                                                              float* out, int32_t* leaves) {
    // an even number of trees per chunk: TW is even, so every chunk starts 16-byte aligned in the blob
    constexpr int TW = forest_tree_words(D), kChunk = (kForestLdsWords / TW) & ~1;
    __shared__ __attribute__((aligned(16))) uint32_t forest[kForestLdsWords];
    __shared__ float xs[kForestCols * kForestBlock];
    const int tid = threadIdx.x;
    const int64_t row = (int64_t)blockIdx.x * kForestBlock + tid;
    const bool live = row < n_rows;
#pragma unroll
    for (int f = 0; f < kForestCols; ++f)
        xs[f * kForestBlock + tid] = (live && f < kSgu1Features) ? X[(int64_t)f * ld + row] : 0.0f;
    float pred = base_score;
    int32_t* lv = (leaves && live) ? leaves + row * (int64_t)n_trees : nullptr;
    for (int t0 = 0; t0 < n_trees; t0 += kChunk) {
        const int nt = n_trees - t0 < kChunk ? n_trees - t0 : kChunk;
        __syncthreads();  // the previous chunk is done with (and xs is written)
        const uint4* src = reinterpret_cast<const uint4*>(blob + (int64_t)t0 * TW);
        const int words = nt * TW;  // TW is even and the blob 16-byte aligned: whole uint4 then a uint2 tail
        for (int i = tid; i < words / 4; i += kForestBlock) reinterpret_cast<uint4*>(forest)[i] = src[i];
        if ((words & 3) && tid == 0)
            reinterpret_cast<uint2*>(forest)[words / 2 - 1] = reinterpret_cast<const uint2*>(src)[words / 2 - 1];
        __syncthreads();
        int t = 0;
        for (; t + kForestIlp <= nt; t += kForestIlp) {
            forest_walk<D, kForestIlp>(forest, t * TW, xs + tid, pred, lv);
            if (lv) lv += kForestIlp;
        }
        for (; t < nt; ++t) {
            forest_walk<D, 1>(forest, t * TW, xs + tid, pred, lv);
            if (lv) lv += 1;
        }
    }
    if (live) out[row] = pred;
}

}  // namespace sgmm

using namespace sgmm;

extern "C" int sgmm_sgu1_features(const sgmm_event_bars* ev, int32_t n_days, const int64_t* snap_off,
                                  const int64_t* row_off, int64_t max_bars_per_day, int64_t ld, float* X,
                                  double* label, double* F64, int32_t* n_rows, void* stream) {
    clear_error();
    SGMM_REQUIRE(ev && snap_off && row_off && X && label && n_rows, "null argument");
    SGMM_REQUIRE(max_bars_per_day <= kMaxBars, "more than %d bars per day", kMaxBars);
    SGMM_REQUIRE(ld >= 0, "ld < 0");
    if (n_days <= 0) return SGMM_OK;
    ProfScope prof("sgu1_features", as_stream(stream));
    SGMM_LAUNCH(k_sgu1_features, dim3(n_days), dim3(kDayBlock), 0, as_stream(stream), *ev, snap_off, row_off, ld,
                X, label, F64, n_rows);
    SGMM_LAUNCHED();
    return SGMM_OK;
}

extern "C" size_t sgmm_sgu1_forest_bytes(int32_t depth, int32_t n_trees) {
    if (depth < 1 || depth > 6 || n_trees < 0) return 0;
    return (size_t)n_trees * forest_tree_words(depth) * sizeof(uint32_t);
}

extern "C" int sgmm_sgu1_predict(const void* forest_blob, size_t blob_bytes, int32_t depth, int32_t n_trees,
                                 float base_score, const float* X, int64_t ld, int64_t n_rows, float* out,
                                 int32_t* leaves, void* stream) {
    clear_error();
    SGMM_REQUIRE(depth >= 1 && n_trees >= 0 && n_rows >= 0, "depth < 1, n_trees < 0 or n_rows < 0");
    if (depth > 6) {
        set_error("forest depth %d > 6", depth);
        return SGMM_ERR_UNSUPPORTED;
    }
    if (n_rows == 0) return SGMM_OK;
    SGMM_REQUIRE(X && out && ld >= n_rows, "null X / out or ld < n_rows");
    SGMM_REQUIRE(n_trees == 0 || forest_blob, "null forest");
    SGMM_REQUIRE((reinterpret_cast<uintptr_t>(forest_blob) & 15) == 0, "forest blob is not 16-byte aligned");
    SGMM_REQUIRE(blob_bytes >= sgmm_sgu1_forest_bytes(depth, n_trees), "forest blob of %zu bytes < %zu (depth %d, %d trees)",
                 blob_bytes, sgmm_sgu1_forest_bytes(depth, n_trees), depth, n_trees);
    SGMM_REQUIRE((n_rows + kForestBlock - 1) / kForestBlock <= 0x7fffffffLL, "too many rows");
    const dim3 grid((unsigned)((n_rows + kForestBlock - 1) / kForestBlock));
    ProfScope prof("sgu1_forest", as_stream(stream));
    with_int<1, 2, 3, 4, 5, 6>(depth, [&](auto dc) {
        SGMM_LAUNCH(k_sgu1_forest<decltype(dc)::value>, grid, dim3(kForestBlock), 0, as_stream(stream),
                    reinterpret_cast<const uint32_t*>(forest_blob), n_trees, base_score, X, ld, n_rows, out, leaves);
    });
    SGMM_LAUNCHED();
    return SGMM_OK;
}
