// sgmm_bars_device.h -- the per-bar reductions of the 19-event groups
// (loaders/HFTLoader.py:70-96 and :131-145), shared by the SGU2 window kernel
// (sgmm_bundle.hip) and the SGU1 feature table (sgmm_sgu1.hip).
#pragma once

#include <cmath>

#include "sgmm_device.h"

namespace sgmm {

constexpr int kDayBlock = 1024;
constexpr int kEventStep = 19;
constexpr int kMaxBars = 4096;  // bars per day held in LDS (4096 * 19 events)

// numpy's float64 add.reduce of 19 values with NaN counted as 0 (what pandas'
// nansum / nanmean hand it): for n in [8, 128) 8 strided accumulators,
// combined pairwise, then the tail in order.  count: the non-NaN values.
__device__ __forceinline__ double nan0_pairwise_sum_19(const double* a, int& count) {
    auto q = [&](int j) -> double {
        const double x = a[j];
        const bool ok = x == x;
        count += ok ? 1 : 0;
        return ok ? x : 0.0;
    };
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = q(j);
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = r[j] + q(8 + j);
    double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    s = s + q(16);
    s = s + q(17);
    s = s + q(18);
    return s;
}

// pandas' Series.mean of 19 quotes (nanops.nanmean, skipna): the sum above
// divided by the number of non-NaN quotes; NaN when there is none.  A call,
// not inlined: with both means inlined k_bar_windows holds 38 quotes at once
// and spills at the 128 VGPRs a 1024-thread block leaves it (66 and none so)
inline __device__ __noinline__ double skipna_mean_19(const double* a) {
    int count = 0;
    const double s = nan0_pairwise_sum_19(a, count);
    return count > 0 ? s / count : NAN;
}

// pandas' Series.sum of 19 values (nanops.nansum, skipna, min_count 0)
inline __device__ __noinline__ double skipna_sum_19(const double* a) {
    int count = 0;
    return nan0_pairwise_sum_19(a, count);
}

__device__ __forceinline__ double nan_max_run(const double* a, int n) {
    double m = NAN;
    for (int i = 0; i < n; ++i)
        if (a[i] == a[i]) m = (m != m || a[i] > m) ? a[i] : m;
    return m;
}

__device__ __forceinline__ double nan_min_run(const double* a, int n) {
    double m = NAN;
    for (int i = 0; i < n; ++i)
        if (a[i] == a[i]) m = (m != m || a[i] < m) ? a[i] : m;
    return m;
}

}  // namespace sgmm
