// sgmm_internal.h -- host-side helpers shared by the C-ABI translation units.
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <type_traits>

#include "../../include/sgmm.h"
#include "sgmm_plan.h"

namespace sgmm {

void set_error(const char* fmt, ...);
void clear_error();

#define SGMM_REQUIRE(cond, ...)                     \
    do {                                            \
        if (!(cond)) {                              \
            ::sgmm::set_error(__VA_ARGS__);         \
            return SGMM_ERR_ARG;                    \
        }                                           \
    } while (0)

#define SGMM_HIP(call)                                                              \
    do {                                                                            \
        hipError_t err_ = (call);                                                   \
        if (err_ != hipSuccess) {                                                   \
            ::sgmm::set_error("%s failed: %s", #call, hipGetErrorString(err_));     \
            return SGMM_ERR_HIP;                                                    \
        }                                                                           \
    } while (0)

#define SGMM_LAUNCHED()                                                             \
    do {                                                                            \
        hipError_t err_ = hipGetLastError();                                        \
        if (err_ != hipSuccess) {                                                   \
            ::sgmm::set_error("kernel launch failed: %s", hipGetErrorString(err_)); \
            return SGMM_ERR_HIP;                                                    \
        }                                                                           \
    } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Kernel-timing hooks (sgmm_profile_enable).  prof_begin returns a slot
// (or -1 when profiling is off) that prof_end closes on the same stream.
// A kernel launched inside the scope with SGMM_LAUNCH takes the slot's events
// into its own dispatch (hipExtLaunchKernel), so the slot then times the kernel
// itself rather than the span between two stream markers.
int prof_begin(const char* kind, hipStream_t s);
void prof_end(int slot, hipStream_t s);
bool prof_take_events(hipEvent_t* start, hipEvent_t* stop);

#define SGMM_LAUNCH(kernel, grid, block, lds, stream, ...)                                       \
    do {                                                                                         \
        hipEvent_t ev_a_, ev_b_;                                                                 \
        if (::sgmm::prof_take_events(&ev_a_, &ev_b_))                                            \
            hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, ev_a_, ev_b_, 0, __VA_ARGS__); \
        else                                                                                     \
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                   \
    } while (0)

struct ProfScope {
    int slot;
    hipStream_t s;
    ProfScope(const char* kind, hipStream_t st) : slot(prof_begin(kind, st)), s(st) {}
    ~ProfScope() { prof_end(slot, s); }
};

inline bool supported_hidden(int h) { return h == 8 || h == 16 || h == 32 || h == 64; }

// Runtime value -> template argument: with_int<16, 32, 64>(hidden, [&](auto h) {
// ... kernel<decltype(h)::value> ... }) calls f with IntC<V> of the V that equals
// v (of the last V when none does); with_bool likewise with std::bool_constant.
template <int N>
struct IntC {
    static constexpr int value = N;
};
template <int V0, int... Vs, class F>
inline void with_int(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) f(IntC<V0>{});
    else if (v == V0) f(IntC<V0>{});
    else with_int<Vs...>(v, f);
}
template <class F>
inline void with_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// Snapshot of the launch-plan overrides (SGMM_PLAN_*, -1 = the default rule):
// taken once per C-ABI entry, so every launch of the call follows one plan
// (sgmm_plan_set; the -DSGMM_EXPERIMENTS build seeds them from SGMM_* variables)
PlanKnobs plan_knobs();

}  // namespace sgmm
