// sgmm_sgu2_train.hip -- SGU2 training on gfx950: whole fits in one launch.
//
// Reference semantics:
//   models/GateUnits.py:66-114   SGU2.train: DataLoader(shuffle=True), Adam,
//                                MSELoss, validation pass, early stopping
//   models/GateUnits.py:42-54    SGU2Model.forward in train mode: LSTM ->
//                                Dropout(0.8) on the last hidden state -> fc
//   pipeline/sgu_trainer.py:91-112  the driver (scaler, label scale 10000)
//
// One workgroup of 256 threads per fit, no communication between workgroups.
// Weights, Adam moments and the minibatch gradient live in LDS for the whole
// fit.  A minibatch is walked in chunks of 256 samples:
//   1. one thread per sample: forward recurrence (k_sgu2's operation order,
//      weights read from LDS as broadcasts; tanh_rel instead of tanh_fast, see
//      there), activations i, f, g, o, c, h and the input written to the
//      workspace as planes of 256 floats ([t][slot][sample], coalesced), then
//      BPTT down the same planes; the gate planes are overwritten with the
//      pre-activation gradients delta_t.  The loops over the hidden units are
//      real loops: what they index (c, the new h, dL/dc, dL/dh) sits in LDS
//      columns private to the thread.
//   2. gradient reduction: wave w owns gate w's rows of W_hh / W_ih / b.  A
//      lane accumulates delta_t[r] * h_{t-1}[k] over its samples (lane, lane +
//      64, ...) and all t in a fixed order, then the 64 lanes are summed by a
//      fixed xor butterfly -- the same bits on every run.
// After the last chunk every thread applies torch.optim.Adam's update to its
// parameters.  The loop nest is bounded by epochs x ceil(n / batch).
#include <cmath>

#include "sgmm_internal.h"
#include "sgmm_sgu2_device.h"

namespace sgmm {

constexpr int kTrainBlock = 256;
constexpr int kMaxBatch = 1024;
constexpr uint32_t kStreamPerm = 3u, kStreamKeep = 4u;  // Philox stream ids (0, 1: GA; 2: bootstrap)
constexpr uint32_t kKeepBelow = 858993459u;             // floor(0.2 * 2^32)

// ---------------------------------------------------------------- schedule
__device__ __forceinline__ int perm_bits(int64_t n) {
    int b = 64 - __builtin_clzll((unsigned long long)(n - 1) | 1ull);
    if (n - 1 == 0) b = 0;
    return b < 2 ? 2 : b;
}

// position i of epoch e -> sample index: a six-round unbalanced Feistel
// bijection of [0, 2^b), walked until it lands in [0, n)
__device__ __forceinline__ int32_t philox_perm(uint64_t seed, uint32_t epoch, int64_t n, int b, uint32_t i) {
    const int a = b / 2, c = b - a;
    const uint32_t mask_a = (1u << a) - 1u, mask_c = (1u << c) - 1u;
    uint32_t x = i;
    for (uint32_t walk = 0; walk < (1u << b); ++walk) {  // a cycle of the bijection is at most 2^b long
#pragma unroll 1
        for (uint32_t r = 0; r < 6; ++r) {
            uint32_t L = x >> c;
            const uint32_t R = x & mask_c;
            L ^= philox4x32_10(U4{R, r, epoch, kStreamPerm}, (uint32_t)seed, (uint32_t)(seed >> 32)).x & mask_a;
            x = (R << a) | L;
        }
        if ((int64_t)x < n) break;
    }
    return (int32_t)x;
}

template <int H>
__device__ __forceinline__ void philox_keep(uint64_t seed, uint32_t epoch, uint32_t i, float (&keep)[H]) {
#pragma unroll
    for (int q = 0; q < (H + 3) / 4; ++q) {
        const U4 r = philox4x32_10(U4{(uint32_t)q, i, epoch, kStreamKeep}, (uint32_t)seed, (uint32_t)(seed >> 32));
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (4 * q + u < H) keep[4 * q + u] = w[u] < kKeepBelow ? 1.0f : 0.0f;
    }
}

__global__ __launch_bounds__(kTrainBlock) void k_sgu2_schedule(uint64_t seed, int64_t n, int hidden, int epochs,
                                                               int32_t* __restrict__ perm,
                                                               uint8_t* __restrict__ keep) {
    const int64_t idx = (int64_t)blockIdx.x * kTrainBlock + threadIdx.x;
    if (idx >= n * epochs) return;
    const uint32_t e = (uint32_t)(idx / n), i = (uint32_t)(idx % n);
    if (perm) perm[idx] = philox_perm(seed, e, n, perm_bits(n), i);
    if (keep) {
        float k[32];
        philox_keep<32>(seed, e, i, k);
        for (int j = 0; j < hidden; ++j) keep[idx * hidden + j] = (uint8_t)k[j];
    }
}

// ---------------------------------------------------------------- one sample
// plane (t, slot) of the chunk workspace at this thread's sample: a uniform
// plane base (scalar registers) plus the thread index
template <int H>
__device__ __forceinline__ float& plane(float* ws, int t, int slot) {
    return (ws + ((size_t)t * (6 * H + 1) + slot) * kTrainBlock)[threadIdx.x];
}

// tanh with a RELATIVE error of a few ulps at every magnitude.  tanh_fast (1 -
// 2 / (1 + e^2x), what inference uses) is accurate to ~1e-7 absolutely, which
// for a small cell state c is a large relative error of h = o * tanh(c) -- and
// the weight gradients are products with h (dW_hh = delta (x) h_{t-1}): measured
// 8 ulps of the gradient's scale against float64 autograd at T = 2.  Below 1/4
// the odd Taylor polynomial through x^9 (next term 1.4e-3 x^11: < 1e-8
// relative), above it (1 - e) / (1 + e) with e = e^(-2|x|), the same hardware
// exp2 / rcp; NaN and +-inf propagate as in tanh_fast.
__device__ __forceinline__ float tanh_rel(float x) {
    const float ax = fabsf(x), x2 = ax * ax;
    const float e = __builtin_amdgcn_exp2f(-2.0f * kLog2e * ax);
    const float big = (1.0f - e) * __builtin_amdgcn_rcpf(1.0f + e);
    const float small =
        ax * fmaf(x2, fmaf(x2, fmaf(x2, fmaf(x2, 62.0f / 2835.0f, -17.0f / 315.0f), 2.0f / 15.0f), -1.0f / 3.0f), 1.0f);
    return copysignf(ax < 0.25f ? small : big, x);
}

// Row r of the gate pre-activations, in k_sgu2's operation order (weights in LDS)
template <int H>
__device__ __forceinline__ float gate_row(const float* w, int r, float xt, const float (&h)[H]) {
    using L = Sgu2Layout<H>;
    const float* wr = w + L::W_HH + r * H;
    f32x2 acc = {0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k + 1 < H; k += 2) acc = __builtin_elementwise_fma(f32x2{wr[k], wr[k + 1]}, f32x2{h[k], h[k + 1]}, acc);
    float hh = acc.x + acc.y;
    if (H & 1) hh = fmaf(wr[H - 1], h[H - 1], hh);
    return fmaf(w[L::W_IH + r], xt, w[L::B_IH + r]) + (hh + w[L::B_HH + r]);
}

// Per-thread vectors that are indexed by a run-time unit j live in LDS as
// columns vec[which][j][thread] (conflict-free, private to the thread): the
// unit loops are real loops, so the code and the live registers stay small at
// every H (a fully unrolled step keeps 4H*H weights in flight and spills).
template <int H>
__device__ __forceinline__ float& col(float* vec, int which, int j) {
    return vec[(which * H + j) * kTrainBlock + threadIdx.x];
}

// the recurrence of k_sgu2; STORE keeps what BPTT needs.  vec: c (0), new h (1)
template <int H, bool STORE>
__device__ __forceinline__ void lstm_forward(const float* w, const float* __restrict__ x, int T, bool scaled, float mu,
                                             float sd, float* ws, float* vec, float (&h)[H]) {
#pragma unroll
    for (int j = 0; j < H; ++j) {
        h[j] = 0.0f;
        col<H>(vec, 0, j) = 0.0f;
    }
    for (int t = 0; t < T; ++t) {
        const float xt = scaled ? (x[t] - mu) / sd : x[t];
#pragma unroll 1
        for (int j = 0; j < H; ++j) {
            const float ig = sigmoid_fast(gate_row<H>(w, j, xt, h)), fg = sigmoid_fast(gate_row<H>(w, H + j, xt, h));
            const float gg = tanh_rel(gate_row<H>(w, 2 * H + j, xt, h));
            const float og = sigmoid_fast(gate_row<H>(w, 3 * H + j, xt, h));
            const float c = fmaf(fg, col<H>(vec, 0, j), ig * gg);
            const float hn = og * tanh_rel(c);
            col<H>(vec, 0, j) = c;
            col<H>(vec, 1, j) = hn;
            if constexpr (STORE) {
                plane<H>(ws, t, j) = ig;
                plane<H>(ws, t, H + j) = fg;
                plane<H>(ws, t, 2 * H + j) = gg;
                plane<H>(ws, t, 3 * H + j) = og;
                plane<H>(ws, t, 4 * H + j) = c;
                plane<H>(ws, t, 5 * H + j) = hn;
            }
        }
#pragma unroll
        for (int j = 0; j < H; ++j) h[j] = col<H>(vec, 1, j);
        if constexpr (STORE) plane<H>(ws, t, 6 * H) = xt;
    }
}

// BPTT of one sample: gate planes i, f, g, o of every step are replaced by the
// gradients of the gate pre-activations.  vec: dL/dc (0), dL/dh_t (1, set by
// the caller to dL/dh_T).  dL/dh_{t-1} = W_hh^T delta_t, accumulated unit by
// unit in the row order j, H+j, 2H+j, 3H+j.
template <int H>
__device__ __forceinline__ void lstm_backward(const float* w, int T, float* ws, float* vec) {
    using L = Sgu2Layout<H>;
#pragma unroll
    for (int j = 0; j < H; ++j) col<H>(vec, 0, j) = 0.0f;
    for (int t = T - 1; t >= 0; --t) {
        float dn[H];
#pragma unroll
        for (int k = 0; k < H; ++k) dn[k] = 0.0f;
        // blocks of J units: the block's 6J plane reads are issued together (one
        // L2 latency per block, not per unit; one wave per SIMD hides none of it)
        constexpr int J = (H % 8 == 0) ? 8 : 5;
        static_assert(H % J == 0, "unit blocks");
#pragma unroll 1
        for (int j0 = 0; j0 < H; j0 += J) {
            float ig[J], fg[J], gg[J], og[J], ct[J], cp[J];
#pragma unroll
            for (int u = 0; u < J; ++u) {
                ig[u] = plane<H>(ws, t, j0 + u);
                fg[u] = plane<H>(ws, t, H + j0 + u);
                gg[u] = plane<H>(ws, t, 2 * H + j0 + u);
                og[u] = plane<H>(ws, t, 3 * H + j0 + u);
                ct[u] = plane<H>(ws, t, 4 * H + j0 + u);
                cp[u] = t > 0 ? plane<H>(ws, t - 1, 4 * H + j0 + u) : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < J; ++u) {
                const int j = j0 + u;
                const float tc = tanh_rel(ct[u]);
                const float dh = col<H>(vec, 1, j);
                const float dcj = fmaf(dh * og[u], 1.0f - tc * tc, col<H>(vec, 0, j));
                const float d[4] = {(dcj * gg[u]) * (ig[u] * (1.0f - ig[u])), (dcj * cp[u]) * (fg[u] * (1.0f - fg[u])),
                                    (dcj * ig[u]) * (1.0f - gg[u] * gg[u]), (dh * tc) * (og[u] * (1.0f - og[u]))};
                col<H>(vec, 0, j) = dcj * fg[u];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    plane<H>(ws, t, q * H + j) = d[q];
                    const float* wr = w + L::W_HH + (q * H + j) * H;
#pragma unroll
                    for (int k = 0; k < H; ++k) dn[k] = fmaf(wr[k], d[q], dn[k]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < H; ++k) col<H>(vec, 1, k) = dn[k];
    }
}

// ---------------------------------------------------------------- workgroup
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// fixed-order tree over the 256 threads; every thread gets the sum
__device__ __forceinline__ float block_sum(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = kTrainBlock / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const float out = red[0];
    __syncthreads();
    return out;
}

// grad += the chunk's gradient (cnt samples whose delta / h / x planes are in ws)
template <int H>
__device__ __forceinline__ void reduce_chunk(float* grad, const float* __restrict__ ws, const float* sdy, int T,
                                             int cnt) {
    using L = Sgu2Layout<H>;
    constexpr int R = H == 10 ? 10 : (H == 16 ? 8 : 4);  // rows per pass: each pass re-reads the h planes
    static_assert(H % R == 0, "row passes");
    constexpr int PL = 6 * H + 1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int rr = 0; rr < H; rr += R) {
        const int r0 = wave * H + rr;
        float acc[R][H], ax[R], ab[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            ax[i] = ab[i] = 0.0f;
#pragma unroll
            for (int k = 0; k < H; ++k) acc[i][k] = 0.0f;
        }
        for (int s = lane; s < cnt; s += 64) {
#pragma unroll 2
            for (int t = 0; t < T; ++t) {
                float d[R];
                const float xv = ws[((size_t)t * PL + 6 * H) * kTrainBlock + s];
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    d[i] = ws[((size_t)t * PL + r0 + i) * kTrainBlock + s];
                    ab[i] += d[i];
                    ax[i] = fmaf(d[i], xv, ax[i]);
                }
                if (t > 0) {
#pragma unroll
                    for (int k = 0; k < H; ++k) {
                        const float hk = ws[((size_t)(t - 1) * PL + 5 * H + k) * kTrainBlock + s];
#pragma unroll
                        for (int i = 0; i < R; ++i) acc[i][k] = fmaf(d[i], hk, acc[i][k]);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const float sx = wave_sum(ax[i]), sb = wave_sum(ab[i]);
            if (lane == 0) {
                grad[L::W_IH + r0 + i] += sx;
                grad[L::B_IH + r0 + i] += sb;
                grad[L::B_HH + r0 + i] += sb;
            }
#pragma unroll
            for (int k = 0; k < H; ++k) {
                const float sk = wave_sum(acc[i][k]);
                if (lane == k) grad[L::W_HH + (r0 + i) * H + k] += sk;
            }
        }
    }
    if (wave == 0) {  // fc: the c planes of the last step hold the dropped-out h_T
        float af[H], afb = 0.0f;
#pragma unroll
        for (int k = 0; k < H; ++k) af[k] = 0.0f;
        for (int s = lane; s < cnt; s += 64) {
            const float dy = sdy[s];
            afb += dy;
#pragma unroll
            for (int k = 0; k < H; ++k)
                af[k] = fmaf(dy, ws[((size_t)(T - 1) * PL + 4 * H + k) * kTrainBlock + s], af[k]);
        }
        const float sb = wave_sum(afb);
        if (lane == 0) grad[L::FC_B] += sb;
#pragma unroll
        for (int k = 0; k < H; ++k) {
            const float sk = wave_sum(af[k]);
            if (lane == k) grad[L::FC_W + k] += sk;
        }
    }
}

struct Sgu2Data {
    const float* X;
    const float* y;
    int T;
    bool scaled;
    float mu, sd, label_scale;
};

enum { kKeepNone = 0, kKeepArray = 1, kKeepPhilox = 2 };

// One minibatch: positions pos0 .. pos0 + cnt - 1 of the epoch.  Adds the
// gradient to grad (LDS, zero on entry) and returns the loss to every thread.
// perm: the epoch's explicit permutation, or NULL with perm_philox, or NULL for
// the identity; keep: the epoch's explicit masks [n, H] when keep_mode is kKeepArray.
template <int H>
__device__ __forceinline__ float minibatch_grad(const float* w, float* grad, float* red, float* sdy, float* vec,
                                                const Sgu2Data& D,
                                                const int32_t* __restrict__ perm, bool perm_philox, int perm_b,
                                                int64_t n, const uint8_t* __restrict__ keep, int keep_mode,
                                                uint64_t seed, uint32_t epoch, int64_t pos0, int cnt, float* ws) {
    using L = Sgu2Layout<H>;
    const int tid = threadIdx.x;
    float sq = 0.0f;
    for (int c0 = 0; c0 < cnt; c0 += kTrainBlock) {
        const int ccnt = min(kTrainBlock, cnt - c0);
        if (tid < ccnt) {
            const int64_t pos = pos0 + c0 + tid;
            const int64_t idx = perm ? (int64_t)perm[pos]
                                     : perm_philox ? (int64_t)philox_perm(seed, epoch, n, perm_b, (uint32_t)pos) : pos;
            float kp[H];
            if (keep_mode == kKeepPhilox) {
                philox_keep<H>(seed, epoch, (uint32_t)pos, kp);
            } else {
#pragma unroll
                for (int j = 0; j < H; ++j) kp[j] = keep_mode == kKeepArray ? (float)keep[pos * H + j] : 1.0f;
            }
            const float drop = keep_mode == kKeepNone ? 1.0f : 5.0f;
            float h[H];
            lstm_forward<H, true>(w, D.X + idx * D.T, D.T, D.scaled, D.mu, D.sd, ws, vec, h);
            float yv = 0.0f;
#pragma unroll
            for (int k = 0; k < H; ++k) {
                h[k] = h[k] * kp[k] * drop;
                yv = fmaf(w[L::FC_W + k], h[k], yv);
            }
            const float err = (yv + w[L::FC_B]) - D.y[idx] * D.label_scale;
            sq += err * err;
            const float dy = 2.0f * err / (float)cnt;
            sdy[tid] = dy;
#pragma unroll
            for (int k = 0; k < H; ++k) col<H>(vec, 1, k) = (dy * w[L::FC_W + k]) * (kp[k] * drop);
            lstm_backward<H>(w, D.T, ws, vec);
#pragma unroll
            for (int k = 0; k < H; ++k) plane<H>(ws, D.T - 1, 4 * H + k) = h[k];
        }
        __syncthreads();
        reduce_chunk<H>(grad, ws, sdy, D.T, ccnt);
        __syncthreads();
    }
    return block_sum(sq, red) / (float)cnt;
}

template <int H>
struct TrainLds {
    static constexpr int P = Sgu2Layout<H>::P;
    float w[P], m[P], v[P], grad[P];
    float red[kTrainBlock], sdy[kTrainBlock];
    float vec[2 * H * kTrainBlock];  // per-thread columns, see col()
};

struct TrainShared {
    int hidden, T, batch, epochs, patience;
    const float* mean;
    const float* std_;
    float label_scale;
    float* workspace;
    size_t ws_stride;  // floats per fit
};

template <int H>
__global__ __launch_bounds__(kTrainBlock) void k_sgu2_train(const sgmm_sgu2_task* __restrict__ tasks, TrainShared S) {
    constexpr int P = Sgu2Layout<H>::P;
    using L = Sgu2Layout<H>;
    __shared__ TrainLds<H> lds;
    const int tid = threadIdx.x;
    const sgmm_sgu2_task tk = tasks[blockIdx.x];
    float* ws = S.workspace + (size_t)blockIdx.x * S.ws_stride;
    for (int p = tid; p < P; p += kTrainBlock) {
        lds.w[p] = tk.weights[p];
        lds.m[p] = lds.v[p] = lds.grad[p] = 0.0f;
    }
    __syncthreads();
    const bool scaled = S.mean != nullptr;
    Sgu2Data D{tk.X_train, tk.y_train, S.T, scaled, scaled ? S.mean[0] : 0.0f, scaled ? S.std_[0] : 1.0f,
               S.label_scale};
    const int64_t n = tk.n, nv = tk.nv;
    const int perm_b = perm_bits(n);
    const int64_t nb = (n + S.batch - 1) / S.batch;
    const float lerp_w = (float)(1.0 - 0.9), sq_w = (float)(1.0 - 0.999);
    float best = INFINITY;
    int best_epoch = -1, trigger = 0, epochs_run = 0;
    int64_t step = 0;
    for (int e = 0; e < S.epochs; ++e) {
        double loss_sum = 0.0;
        const int32_t* perm_e = tk.perm ? tk.perm + (int64_t)e * n : nullptr;
        const uint8_t* keep_e = tk.keep ? tk.keep + (int64_t)e * n * H : nullptr;
        for (int64_t b = 0; b < nb; ++b) {
            const int64_t pos0 = b * S.batch;
            const int cnt = (int)min((int64_t)S.batch, n - pos0);
            const float loss = minibatch_grad<H>(lds.w, lds.grad, lds.red, lds.sdy, lds.vec, D, perm_e, true, perm_b, n, keep_e,
                                                 keep_e ? kKeepArray : kKeepPhilox, tk.seed, (uint32_t)e, pos0, cnt,
                                                 ws);
            loss_sum += (double)loss;
            // torch.optim.Adam, default settings, torch's operation order
            ++step;
            const double bc1 = 1.0 - pow(0.9, (double)step), bc2 = 1.0 - pow(0.999, (double)step);
            const float neg_step = (float)(-(tk.lr / bc1)), bc2_sqrt = (float)sqrt(bc2);
            for (int p = tid; p < P; p += kTrainBlock) {
                const float g = lds.grad[p];
                lds.grad[p] = 0.0f;
                const float m = lds.m[p] + lerp_w * (g - lds.m[p]);
                const float v = lds.v[p] * 0.999f + (sq_w * g) * g;
                lds.m[p] = m;
                lds.v[p] = v;
                lds.w[p] = lds.w[p] + (neg_step * m) / (sqrtf(v) / bc2_sqrt + 1e-8f);
            }
            __syncthreads();
        }
        // validation: eval-mode forward, no dropout
        float sq = 0.0f;
        for (int64_t i = tid; i < nv; i += kTrainBlock) {
            float h[H];
            lstm_forward<H, false>(lds.w, tk.X_val + i * S.T, S.T, scaled, D.mu, D.sd, nullptr, lds.vec, h);
            float yv = 0.0f;
#pragma unroll
            for (int k = 0; k < H; ++k) yv = fmaf(lds.w[L::FC_W + k], h[k], yv);
            const float err = (yv + lds.w[L::FC_B]) - tk.y_val[i] * S.label_scale;
            sq += err * err;
        }
        const float val = block_sum(sq, lds.red) / (float)nv;  // 0 / 0 = NaN when nv == 0
        if (tid == 0) {
            tk.train_loss[e] = loss_sum / (double)nb;
            tk.val_loss[e] = (double)val;
        }
        epochs_run = e + 1;
        if (val < best) {
            best = val;
            best_epoch = e;
            trigger = 0;
            if (tk.best_weights)
                for (int p = tid; p < P; p += kTrainBlock) tk.best_weights[p] = lds.w[p];
        } else if (++trigger >= S.patience) {
            break;
        }
    }
    for (int p = tid; p < P; p += kTrainBlock) tk.weights[p] = lds.w[p];
    if (tid == 0) {
        tk.epochs_run[0] = epochs_run;
        tk.best_epoch[0] = best_epoch;
    }
}

template <int H>
__global__ __launch_bounds__(kTrainBlock) void k_sgu2_loss_grad(const float* __restrict__ weights,
                                                                const float* __restrict__ X,
                                                                const float* __restrict__ y, int n, int T,
                                                                const uint8_t* __restrict__ keep,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ std_, float label_scale,
                                                                float* __restrict__ loss, float* __restrict__ grad,
                                                                float* ws) {
    constexpr int P = Sgu2Layout<H>::P;
    __shared__ float w[P], g[P], red[kTrainBlock], sdy[kTrainBlock], vec[2 * H * kTrainBlock];
    const int tid = threadIdx.x;
    const bool scaled = mean != nullptr;
    const Sgu2Data D{X, y, T, scaled, scaled ? mean[0] : 0.0f, scaled ? std_[0] : 1.0f, label_scale};
    for (int p = tid; p < P; p += kTrainBlock) {
        w[p] = weights[p];
        g[p] = 0.0f;
    }
    __syncthreads();
    const float l = minibatch_grad<H>(w, g, red, sdy, vec, D, nullptr, false, 2, n, keep, keep ? kKeepArray : kKeepNone, 0,
                                      0, 0, n, ws);
    for (int p = tid; p < P; p += kTrainBlock) grad[p] = g[p];
    if (tid == 0) loss[0] = l;
}

size_t fit_workspace_floats(int hidden, int T) { return (size_t)kTrainBlock * (size_t)T * (size_t)(6 * hidden + 1); }

}  // namespace sgmm

using namespace sgmm;

extern "C" size_t sgmm_sgu2_train_workspace_bytes(int32_t hidden, int32_t time_steps, int32_t n_tasks) {
    if (!sgu2_hidden_ok(hidden) || time_steps < 1 || n_tasks < 1) return 0;
    return fit_workspace_floats(hidden, time_steps) * sizeof(float) * (size_t)n_tasks;
}

extern "C" int sgmm_sgu2_train(const sgmm_sgu2_task* tasks, const sgmm_sgu2_task* tasks_host, int32_t n_tasks,
                               int32_t hidden, int32_t time_steps, int32_t batch, int32_t epochs, int32_t patience,
                               const float* mean, const float* std_, float label_scale, void* workspace,
                               size_t workspace_bytes, void* stream) {
    clear_error();
    SGMM_REQUIRE(tasks && tasks_host, "null tasks / tasks_host");
    SGMM_REQUIRE(n_tasks >= 1, "n_tasks %d < 1", n_tasks);
    SGMM_REQUIRE(sgu2_hidden_ok(hidden), "hidden %d not in {10, 16, 32}", hidden);
    SGMM_REQUIRE(time_steps >= 1, "time_steps %d < 1", time_steps);
    SGMM_REQUIRE(batch >= 1 && batch <= kMaxBatch, "batch %d not in 1..%d", batch, kMaxBatch);
    SGMM_REQUIRE(epochs >= 0 && patience >= 1, "epochs %d < 0 or patience %d < 1", epochs, patience);
    SGMM_REQUIRE((mean == nullptr) == (std_ == nullptr), "mean and std must both be given or both NULL");
    for (int32_t k = 0; k < n_tasks; ++k) {
        const sgmm_sgu2_task& t = tasks_host[k];
        SGMM_REQUIRE(t.n >= 1 && t.n <= INT32_MAX, "task %d: n %lld not in 1..2^31-1 (no training windows)", k,
                     (long long)t.n);
        SGMM_REQUIRE(t.nv >= 0, "task %d: negative nv", k);
        SGMM_REQUIRE(t.X_train && t.y_train, "task %d: null training windows / labels", k);
        SGMM_REQUIRE(t.nv == 0 || (t.X_val && t.y_val), "task %d: null validation windows / labels", k);
        SGMM_REQUIRE(t.weights, "task %d: null weights", k);
        SGMM_REQUIRE(t.train_loss && t.val_loss && t.epochs_run && t.best_epoch, "task %d: null output", k);
    }
    const size_t need = sgmm_sgu2_train_workspace_bytes(hidden, time_steps, n_tasks);
    SGMM_REQUIRE(workspace, "null workspace");
    if (workspace_bytes < need) {
        set_error("workspace %zu < %zu bytes", workspace_bytes, need);
        return SGMM_ERR_WORKSPACE;
    }
    const TrainShared S{hidden,       time_steps, batch, epochs, patience, mean, std_, label_scale,
                        (float*)workspace, fit_workspace_floats(hidden, time_steps)};
    const dim3 grid((unsigned)n_tasks), block(kTrainBlock);
    ProfScope prof("sgu2_train", as_stream(stream));
    with_int<10, 16, 32>(hidden, [&](auto h) {
        SGMM_LAUNCH(k_sgu2_train<decltype(h)::value>, grid, block, 0, as_stream(stream), tasks, S);
    });
    SGMM_LAUNCHED();
    return SGMM_OK;
}

extern "C" int sgmm_sgu2_loss_grad(const float* weights, int32_t hidden, const float* X, const float* y, int32_t n,
                                   int32_t time_steps, const uint8_t* keep, const float* mean, const float* std_,
                                   float label_scale, float* loss, float* grad, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    clear_error();
    SGMM_REQUIRE(weights && X && y, "null weights / windows / labels");
    SGMM_REQUIRE(loss && grad, "null loss / grad");
    SGMM_REQUIRE(sgu2_hidden_ok(hidden), "hidden %d not in {10, 16, 32}", hidden);
    SGMM_REQUIRE(time_steps >= 1, "time_steps %d < 1", time_steps);
    SGMM_REQUIRE(n >= 1 && n <= kMaxBatch, "batch %d not in 1..%d", n, kMaxBatch);
    SGMM_REQUIRE((mean == nullptr) == (std_ == nullptr), "mean and std must both be given or both NULL");
    const size_t need = sgmm_sgu2_train_workspace_bytes(hidden, time_steps, 1);
    SGMM_REQUIRE(workspace, "null workspace");
    if (workspace_bytes < need) {
        set_error("workspace %zu < %zu bytes", workspace_bytes, need);
        return SGMM_ERR_WORKSPACE;
    }
    ProfScope prof("sgu2_loss_grad", as_stream(stream));
    with_int<10, 16, 32>(hidden, [&](auto h) {
        hipLaunchKernelGGL(k_sgu2_loss_grad<decltype(h)::value>, dim3(1), dim3(kTrainBlock), 0, as_stream(stream),
                           weights, X, y, (int)n, (int)time_steps, keep, mean, std_, label_scale, loss, grad,
                           (float*)workspace);
    });
    SGMM_LAUNCHED();
    return SGMM_OK;
}

extern "C" int sgmm_sgu2_schedule(uint64_t seed, int64_t n, int32_t hidden, int32_t epochs, int32_t* perm,
                                  uint8_t* keep, void* stream) {
    clear_error();
    SGMM_REQUIRE(n >= 1 && n <= INT32_MAX, "n %lld not in 1..2^31-1", (long long)n);
    SGMM_REQUIRE(sgu2_hidden_ok(hidden), "hidden %d not in {10, 16, 32}", hidden);
    SGMM_REQUIRE(epochs >= 0, "negative epochs");
    if (epochs == 0 || (!perm && !keep)) return SGMM_OK;
    const int64_t total = n * epochs;
    SGMM_REQUIRE(total / kTrainBlock < INT32_MAX, "schedule of %lld elements is too large", (long long)total);
    ProfScope prof("sgu2_schedule", as_stream(stream));
    hipLaunchKernelGGL(k_sgu2_schedule, dim3((unsigned)((total + kTrainBlock - 1) / kTrainBlock)), dim3(kTrainBlock), 0,
                       as_stream(stream), seed, n, (int)hidden, (int)epochs, perm, keep);
    SGMM_LAUNCHED();
    return SGMM_OK;
}
