// sgmm_sgu2_device.h -- device code shared by SGU2 inference (sgmm_sgu2.hip)
// and SGU2 training (sgmm_sgu2_train.hip): the gate non-linearities on the
// transcendental unit and the flat weight layout of sgmm_sgu2_forward.
#pragma once

#include "sgmm_device.h"

namespace sgmm {

typedef float f32x2 __attribute__((ext_vector_type(2)));
// constant address space: wave-uniform loads through it become s_load
typedef const __attribute__((address_space(4))) float* CFloatPtr;
constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ float sigmoid_fast(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-x * kLog2e));
}

__device__ __forceinline__ float tanh_fast(float x) {
    return fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(2.0f * kLog2e * x)), 1.0f);
}

// state_dict order: lstm.weight_ih_l0[4H,1], lstm.weight_hh_l0[4H,H],
// lstm.bias_ih_l0[4H], lstm.bias_hh_l0[4H], fc.weight[1,H], fc.bias[1]
template <int H>
struct Sgu2Layout {
    static constexpr int G = 4 * H;
    static constexpr int W_IH = 0, W_HH = G, B_IH = W_HH + G * H, B_HH = B_IH + G, FC_W = B_HH + G, FC_B = FC_W + H;
    static constexpr int P = FC_B + 1;
};

constexpr bool sgu2_hidden_ok(int h) { return h == 10 || h == 16 || h == 32; }

}  // namespace sgmm
