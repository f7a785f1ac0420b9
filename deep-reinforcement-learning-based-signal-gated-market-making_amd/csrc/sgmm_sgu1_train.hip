// sgmm_sgu1_train.hip -- SGU1 training on gfx950: histogram
// gradient-boosted trees for reg:squarederror, a whole fit per workgroup, one
// task per block, K tasks per launch (as k_sgu2_train).
//
// The contract is stated in include/sgmm.h above sgmm_sgu1_task.  What keeps
// it free of any order: gradients are quantised to int64 against the round's
// largest |g|, histograms hold integer sums and counts (LDS integer atomics),
// the split search runs in float64 from those integers in one fixed operation
// order, and the metric is an integer sum of squares.  No floating-point
// atomic anywhere.
//
// LDS: 40 histogram slots of 257 bins (256 value bins and the missing bin), an
// int64 sum and an int32 count each (123 360 bytes).  A level of nn nodes is
// searched in passes over the features, 40 / nn features per pass: all 20 in
// one pass for the first two levels, one feature per pass at the 32 nodes of
// level 5.  D sizes the node tables (2^(D+1) - 1 ids); the histogram tile is
// the same for every D.
#include <cmath>

#include "sgmm_device.h"
#include "sgmm_internal.h"

namespace sgmm {

constexpr int kTrF = 20;             // features
constexpr int kTrBins = 257;         // 256 value bins + the missing bin
constexpr int kTrMissing = 256;
constexpr int kTrSlots = 40;         // (node, feature) histograms in LDS
constexpr int kTrBlock = 1024;
constexpr int kTrWaves = kTrBlock / 64;
constexpr int kTrCutStride = 256;
constexpr int kTrLevelNodes = 32;    // nodes of the deepest searched level (depth 6: level 5)
constexpr int kTrMaxVal = (1 << 23) - 1;  // validation rows: n_val * (2^20)^2 < 2^63 in the metric's int64 sum
constexpr int kBinBlock = 256;
constexpr int kNoCand = 0x7fffffff;

struct Sgu1Ws {
    float* pred;
    float* y;
    uint32_t* miss;
    uint8_t* pos;
    uint8_t* bins;  // [20, n]
};

__host__ __device__ inline size_t pad4(size_t v) { return (v + 3) & ~(size_t)3; }

__host__ __device__ inline Sgu1Ws ws_views(void* p, size_t n) {
    char* c = static_cast<char*>(p);
    Sgu1Ws w;
    w.pred = reinterpret_cast<float*>(c);
    w.y = reinterpret_cast<float*>(c + 4 * n);
    w.miss = reinterpret_cast<uint32_t*>(c + 8 * n);
    w.pos = reinterpret_cast<uint8_t*>(c + 12 * n);
    w.bins = reinterpret_cast<uint8_t*>(c + 12 * n + pad4(n));
    return w;
}

inline size_t ws_bytes(size_t n) { return (12 * n + pad4(n) + (size_t)kTrF * n + 255) & ~(size_t)255; }

__device__ __forceinline__ int clamp_cuts(int nc, int max_bin) {
    const int cap = max_bin - 1 < kTrCutStride - 1 ? max_bin - 1 : kTrCutStride - 1;
    return nc < 0 ? 0 : (nc > cap ? cap : nc);
}

// One thread per row of a task (training rows, then validation rows): gather
// the label, start the prediction at base_score, bin the 20 features.
__global__ __launch_bounds__(kBinBlock) void k_sgu1_bin(const sgmm_sgu1_task* __restrict__ tasks) {
    const sgmm_sgu1_task tk = tasks[blockIdx.y];
    const int64_t ntr = tk.n_train, n = ntr + (int64_t)tk.n_val;
    const Sgu1Ws w = ws_views(tk.workspace, (size_t)n);
    for (int64_t i = (int64_t)blockIdx.x * kBinBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBinBlock) {
        const bool tr = i < ntr;
        const float* X = tr ? tk.X_train : tk.X_val;
        const float* yv = tr ? tk.y_train : tk.y_val;
        const int64_t ld = tr ? tk.ld_train : tk.ld_val;
        int64_t r = tr ? tk.rows_train[i] : tk.rows_val[i - ntr];
        r = r < 0 ? 0 : (r >= ld ? ld - 1 : r);  // never outside the table
        w.y[i] = yv[r];
        w.pred[i] = tk.base_score;
        w.pos[i] = 0;
        uint32_t miss = 0;
        for (int f = 0; f < kTrF; ++f) {
            const float x = X[(int64_t)f * ld + r];
            int lo = 0;
            if (x != x) {
                miss |= 1u << f;
            } else {  // number of cuts <= x
                int hi = clamp_cuts(tk.n_cuts[f], tk.max_bin);
                const float* c = tk.cuts + f * kTrCutStride;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (c[mid] <= x) lo = mid + 1;
                    else hi = mid;
                }
            }
            w.bins[(int64_t)f * n + i] = (uint8_t)lo;
        }
        w.miss[i] = miss;
    }
}

// binary exponent of a positive float32 minus one: floor(log2 m), subnormals included
__device__ __forceinline__ int floor_log2f(float m) {
    const uint32_t b = __float_as_uint(m) & 0x7fffffffu;
    const int E = (int)(b >> 23);
    return E ? E - 127 : (31 - __clz((int)b)) - 149;
}

__device__ __forceinline__ long long quantise(float g, int s) { return (long long)rint(ldexp((double)g, s)); }

template <class T, class Op>
__device__ __forceinline__ T block_reduce(T v, T* scratch, Op op) {
    const int tid = threadIdx.x;
    scratch[tid] = v;
    __syncthreads();
    for (int s = kTrBlock / 2; s > 0; s >>= 1) {
        if (tid < s) scratch[tid] = op(scratch[tid], scratch[tid + s]);
        __syncthreads();
    }
    const T r = scratch[0];
    __syncthreads();
    return r;
}

struct SplitParams {
    double mcw, lambda, alpha;
};

__device__ __forceinline__ double soft(double G, double alpha) {
    return G > alpha ? G - alpha : (G < -alpha ? G + alpha : 0.0);
}

__device__ __forceinline__ double gain(long long Q, int H, int s, const SplitParams& P) {
    const double t = soft(ldexp((double)Q, -s), P.alpha);
    return t * t / ((double)H + P.lambda);
}

__device__ __forceinline__ double weight(long long Q, int H, int s, const SplitParams& P) {
    return -soft(ldexp((double)Q, -s), P.alpha) / ((double)H + P.lambda);
}

struct Best {
    double score;
    int cand;  // ((feature * 256 + cut) << 1) | default_left: the lower, the earlier in the tie order (better())
    long long QL;
    int HL;
};

template <int D>
__global__ __launch_bounds__(kTrBlock) void k_sgu1_train(const sgmm_sgu1_task* __restrict__ tasks) {
    constexpr int NN = (2 << D) - 1;
    __shared__ unsigned long long hsum[kTrSlots * kTrBins];
    __shared__ int hcnt[kTrSlots * kTrBins];
    __shared__ unsigned long long scratch[kTrBlock];
    __shared__ long long nQ[NN];
    __shared__ int nH[NN], nLeft[NN], nRight[NN], nFeat[NN], nCut[NN], nDl[NN];
    __shared__ float nVal[NN], nBw[NN], nLc[NN];
    __shared__ double bScore[kTrLevelNodes], sScore[kTrSlots];
    __shared__ long long bQL[kTrLevelNodes], sQL[kTrSlots];
    __shared__ int bCand[kTrLevelNodes], bHL[kTrLevelNodes], sCand[kTrSlots], sHL[kTrSlots];
    __shared__ int ncut[kTrF];
    __shared__ int s_next;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const sgmm_sgu1_task tk = tasks[blockIdx.x];
    const int ntr = tk.n_train, nv = tk.n_val, n = ntr + nv;
    const Sgu1Ws w = ws_views(tk.workspace, (size_t)n);
    const int Dt = tk.max_depth < 1 ? 1 : (tk.max_depth > D ? D : tk.max_depth);
    const int NNt = (2 << Dt) - 1;
    const SplitParams P{tk.min_child_weight, tk.lambda, tk.alpha};
    if (tid < kTrF) ncut[tid] = clamp_cuts(tk.n_cuts[tid], tk.max_bin);
    __syncthreads();

    auto fmax_op = [](float a, float b) { return a > b ? a : b; };
    auto add_op = [](long long a, long long b) { return a + b; };
    auto make_leaf = [&](int node, int s) {
        const float v = (float)(tk.eta * weight(nQ[node], nH[node], s, P));
        nLeft[node] = nRight[node] = -1;
        nFeat[node] = nCut[node] = nDl[node] = 0;
        nVal[node] = nBw[node] = v;
        nLc[node] = 0.0f;
    };

    double best_score = INFINITY;
    int best_it = -1, n_trees = 0;
    for (int t = 0; t < tk.n_estimators; ++t) {
        // ---- gradients: the round's scale
        float m = 0.0f;
        for (int i = tid; i < n; i += kTrBlock) {
            w.pos[i] = 0;
            if (i < ntr) m = fmax_op(m, fabsf(w.pred[i] - w.y[i]));
        }
        m = block_reduce(m, reinterpret_cast<float*>(scratch), fmax_op);
        int count = 1;
        if (!(m > 0.0f)) {  // every gradient is zero: one +0 leaf
            if (tid == 0) {
                nQ[0] = 0;
                nH[0] = ntr;
                nLeft[0] = nRight[0] = -1;
                nFeat[0] = nCut[0] = nDl[0] = 0;
                nVal[0] = nBw[0] = nLc[0] = 0.0f;
            }
            __syncthreads();
        } else {
            const int s = 40 - (floor_log2f(m) + 1);
            long long q0 = 0;
            for (int i = tid; i < ntr; i += kTrBlock) q0 += quantise(w.pred[i] - w.y[i], s);
            q0 = block_reduce(q0, reinterpret_cast<long long*>(scratch), add_op);
            if (tid == 0) {
                nQ[0] = q0;
                nH[0] = ntr;
            }
            __syncthreads();
            int lo = 0, hi = 1;
            for (int level = 0; level < Dt && lo < hi; ++level) {
                const int nn = hi - lo;  // <= 2^level <= 32
                const int FT = kTrSlots / nn < kTrF ? kTrSlots / nn : kTrF;
                if (tid < nn) {
                    bScore[tid] = -INFINITY;
                    bCand[tid] = kNoCand;
                    bQL[tid] = 0;
                    bHL[tid] = 0;
                }
                for (int f0 = 0; f0 < kTrF; f0 += FT) {
                    const int nf = kTrF - f0 < FT ? kTrF - f0 : FT;
                    const int nslots = nn * nf;  // <= 40
                    for (int k = tid; k < nslots * kTrBins; k += kTrBlock) {
                        hsum[k] = 0;
                        hcnt[k] = 0;
                    }
                    __syncthreads();
                    // ---- histograms of the level's nodes, features f0 .. f0 + nf - 1
                    for (int i = tid; i < ntr; i += kTrBlock) {
                        const unsigned p = (unsigned)((int)w.pos[i] - lo);
                        if (p >= (unsigned)nn) continue;
                        const unsigned long long q = (unsigned long long)quantise(w.pred[i] - w.y[i], s);
                        const uint32_t miss = w.miss[i];
                        for (int ff = 0; ff < nf; ++ff) {
                            const int f = f0 + ff;
                            const int b = (miss >> f) & 1u ? kTrMissing : (int)w.bins[(int64_t)f * n + i];
                            const int k = ((int)p * nf + ff) * kTrBins + b;
                            atomicAdd(&hsum[k], q);
                            atomicAdd(&hcnt[k], 1);
                        }
                    }
                    __syncthreads();
                    // ---- prefix over the value bins: bin j then holds the rows with x < cut j
                    if (tid < nslots) {
                        unsigned long long a = 0;
                        int c = 0;
                        for (int b = 0; b < kTrMissing; ++b) {
                            a += hsum[tid * kTrBins + b];
                            c += hcnt[tid * kTrBins + b];
                            hsum[tid * kTrBins + b] = a;
                            hcnt[tid * kTrBins + b] = c;
                        }
                    }
                    __syncthreads();
                    // ---- candidates: one wave per slot, lanes over the cuts
                    for (int slot = wave; slot < nslots; slot += kTrWaves) {
                        const int node = lo + slot / nf, f = f0 + slot % nf, base = slot * kTrBins;
                        const long long NQ = nQ[node], MQ = (long long)hsum[base + kTrMissing];
                        const int NH = nH[node], MH = hcnt[base + kTrMissing];
                        const double gN = gain(NQ, NH, s, P);
                        Best mine{-INFINITY, kNoCand, 0, 0};
                        auto consider = [&](long long QL, int HL, int cand) {
                            const int HR = NH - HL;
                            if (!((double)HL >= P.mcw && (double)HR >= P.mcw)) return;
                            const double sc = (gain(QL, HL, s, P) + gain(NQ - QL, HR, s, P)) - gN;
                            if (better(sc, cand, mine.score, mine.cand)) mine = Best{sc, cand, QL, HL};
                        };
                        for (int j = lane; j < ncut[f]; j += 64) {
                            const long long QL = (long long)hsum[base + j];
                            const int HL = hcnt[base + j], cand = (f * kTrCutStride + j) << 1;
                            consider(QL, HL, cand);
                            if (MH > 0) consider(QL + MQ, HL + MH, cand | 1);
                        }
                        double sc = mine.score;
                        int cd = mine.cand;
                        for (int off = 32; off > 0; off >>= 1) {
                            const double osc = __shfl_xor(sc, off);
                            const int ocd = __shfl_xor(cd, off);
                            if (better(osc, ocd, sc, cd)) {
                                sc = osc;
                                cd = ocd;
                            }
                        }
                        if (cd == kNoCand) {
                            if (lane == 0) {
                                sScore[slot] = -INFINITY;
                                sCand[slot] = kNoCand;
                            }
                        } else if (mine.cand == cd) {  // candidates are distinct: one lane owns the winner
                            sScore[slot] = mine.score;
                            sCand[slot] = mine.cand;
                            sQL[slot] = mine.QL;
                            sHL[slot] = mine.HL;
                        }
                    }
                    __syncthreads();
                    // ---- a node's best over the pass's features, lower features first
                    if (tid < nn) {
                        for (int ff = 0; ff < nf; ++ff) {
                            const int slot = tid * nf + ff;
                            if (sCand[slot] != kNoCand && sScore[slot] > bScore[tid]) {
                                bScore[tid] = sScore[slot];
                                bCand[tid] = sCand[slot];
                                bQL[tid] = sQL[slot];
                                bHL[tid] = sHL[slot];
                            }
                        }
                    }
                    __syncthreads();
                }
                // ---- decide the level: ids in increasing parent id, left then right
                if (tid == 0) {
                    int next = hi;
                    for (int k = 0; k < nn; ++k) {
                        const int node = lo + k;
                        const bool split = bCand[k] != kNoCand && bScore[k] > tk.gamma && bScore[k] > 1e-6 &&
                                           next + 2 <= NNt;
                        if (!split) {
                            make_leaf(node, s);
                            continue;
                        }
                        const int c = bCand[k], f = (c >> 9) % kTrF, j = (c >> 1) & (kTrCutStride - 1);
                        nLeft[node] = next;
                        nRight[node] = next + 1;
                        nFeat[node] = f;
                        nCut[node] = j;
                        nDl[node] = c & 1;
                        nVal[node] = tk.cuts[f * kTrCutStride + j];
                        nBw[node] = (float)weight(nQ[node], nH[node], s, P);
                        nLc[node] = (float)bScore[k];
                        nQ[next] = bQL[k];
                        nH[next] = bHL[k];
                        nQ[next + 1] = nQ[node] - bQL[k];
                        nH[next + 1] = nH[node] - bHL[k];
                        next += 2;
                    }
                    s_next = next;
                }
                __syncthreads();
                // ---- rows to their children (training and validation rows)
                for (int i = tid; i < n; i += kTrBlock) {
                    const int p = w.pos[i];
                    if ((unsigned)(p - lo) >= (unsigned)nn || nLeft[p] < 0) continue;
                    const int f = nFeat[p];
                    const bool left = (w.miss[i] >> f) & 1u ? nDl[p] != 0 : (int)w.bins[(int64_t)f * n + i] <= nCut[p];
                    w.pos[i] = (uint8_t)(left ? nLeft[p] : nRight[p]);
                }
                lo = hi;
                hi = s_next;
                __syncthreads();
            }
            if (tid < hi - lo) make_leaf(lo + tid, s);  // the nodes of the last level
            count = hi;
            __syncthreads();
        }
        // ---- the tree, the predictions
        {
            const int64_t o = (int64_t)t * NNt;
            for (int k = tid; k < NNt; k += kTrBlock) {
                const bool live = k < count;
                tk.left[o + k] = live ? nLeft[k] : -1;
                tk.right[o + k] = live ? nRight[k] : -1;
                tk.feature[o + k] = live ? nFeat[k] : 0;
                tk.value[o + k] = live ? nVal[k] : 0.0f;
                tk.default_left[o + k] = live ? (uint8_t)nDl[k] : (uint8_t)0;
                tk.base_weight[o + k] = live ? nBw[k] : 0.0f;
                tk.loss_change[o + k] = live ? nLc[k] : 0.0f;
                tk.sum_hessian[o + k] = live ? (float)nH[k] : 0.0f;
            }
            if (tid == 0) tk.tree_nodes[t] = count;
        }
        float mr = 0.0f;
        for (int i = tid; i < n; i += kTrBlock) {
            const int p = w.pos[i];
            const float pr = w.pred[i] + nVal[p < count ? p : 0];
            w.pred[i] = pr;
            if (i >= ntr) mr = fmax_op(mr, fabsf(pr - w.y[i]));
        }
        n_trees = t + 1;
        if (nv > 0) {
            // ---- the metric and early stopping
            mr = block_reduce(mr, reinterpret_cast<float*>(scratch), fmax_op);
            double rmse = 0.0;
            if (mr > 0.0f) {
                const int s2 = 20 - (floor_log2f(mr) + 1);
                long long sse = 0;
                for (int i = ntr + tid; i < n; i += kTrBlock) {
                    const long long v = quantise(w.pred[i] - w.y[i], s2);
                    sse += v * v;
                }
                sse = block_reduce(sse, reinterpret_cast<long long*>(scratch), add_op);
                rmse = sqrt(ldexp((double)sse, -2 * s2) / (double)nv);
            }
            if (tid == 0) tk.val_rmse[t] = rmse;
            if (rmse < best_score) {
                best_score = rmse;
                best_it = t;
            } else if (tk.early_stopping_rounds > 0 && t - best_it >= tk.early_stopping_rounds) {
                break;
            }
        } else {
            __syncthreads();  // the node tables are rewritten by the next round
        }
    }
    if (tid == 0) {
        tk.n_trees[0] = n_trees;
        tk.best_iteration[0] = best_it;
        tk.best_score[0] = best_it >= 0 ? best_score : (double)NAN;
    }
}

}  // namespace sgmm

using namespace sgmm;

extern "C" size_t sgmm_sgu1_train_workspace_bytes(int64_t n_train, int64_t n_val) {
    if (n_train < 1 || n_val < 0 || n_train + n_val > INT32_MAX) return 0;
    return ws_bytes((size_t)(n_train + n_val));
}

extern "C" int sgmm_sgu1_train(const sgmm_sgu1_task* tasks, const sgmm_sgu1_task* tasks_host, int32_t n_tasks,
                               void* stream) {
    clear_error();
    SGMM_REQUIRE(tasks && tasks_host, "null tasks / tasks_host");
    SGMM_REQUIRE(n_tasks >= 1 && n_tasks <= 65535, "n_tasks %d not in 1..65535", n_tasks);
    int depth = 1;
    int64_t rows = 1;
    auto ok = [](double v) { return std::isfinite(v) && v >= 0.0; };
    for (int32_t k = 0; k < n_tasks; ++k) {
        const sgmm_sgu1_task& t = tasks_host[k];
        SGMM_REQUIRE(t.max_depth >= 1 && t.max_depth <= 6, "task %d: max_depth %d not in 1..6", k, t.max_depth);
        SGMM_REQUIRE(t.max_bin >= 2 && t.max_bin <= 256, "task %d: max_bin %d not in 2..256", k, t.max_bin);
        SGMM_REQUIRE(t.n_train >= 1 && t.n_train <= (1 << 20), "task %d: n_train %d not in 1..2^20", k, t.n_train);
        // the metric's int64 sum of n_val squares of |v| <= 2^20 stays below 2^63 up to 2^23 - 1 rows
        SGMM_REQUIRE(t.n_val >= 0 && t.n_val <= kTrMaxVal, "task %d: n_val %d not in 0..2^23-1", k, t.n_val);
        SGMM_REQUIRE(t.n_estimators >= 0, "task %d: negative n_estimators", k);
        SGMM_REQUIRE(t.early_stopping_rounds >= 0, "task %d: negative early_stopping_rounds", k);
        SGMM_REQUIRE(t.early_stopping_rounds == 0 || t.n_val > 0,
                     "task %d: early_stopping_rounds needs validation rows", k);
        SGMM_REQUIRE(std::isfinite(t.eta) && ok(t.lambda) && ok(t.alpha) && ok(t.gamma) && ok(t.min_child_weight) &&
                         std::isfinite(t.base_score),
                     "task %d: eta / lambda / alpha / gamma / min_child_weight / base_score negative or not finite", k);
        SGMM_REQUIRE(t.lambda > 0.0 || t.min_child_weight > 0.0, "task %d: lambda and min_child_weight both 0", k);
        SGMM_REQUIRE(t.X_train && t.y_train && t.rows_train && t.ld_train >= 1, "task %d: null training table", k);
        SGMM_REQUIRE(t.n_val == 0 || (t.X_val && t.y_val && t.rows_val && t.ld_val >= 1),
                     "task %d: null validation table", k);
        SGMM_REQUIRE(t.cuts && t.n_cuts, "task %d: null cuts", k);
        SGMM_REQUIRE(t.workspace && (reinterpret_cast<uintptr_t>(t.workspace) & 255) == 0,
                     "task %d: null or unaligned workspace", k);
        SGMM_REQUIRE(t.left && t.right && t.feature && t.value && t.default_left && t.base_weight && t.loss_change &&
                         t.sum_hessian && t.tree_nodes && t.val_rmse && t.n_trees && t.best_iteration && t.best_score,
                     "task %d: null output", k);
        depth = t.max_depth > depth ? t.max_depth : depth;
        rows = (int64_t)t.n_train + t.n_val > rows ? (int64_t)t.n_train + t.n_val : rows;
    }
    {
        ProfScope prof("sgu1_bin", as_stream(stream));
        int64_t gx = (rows + kBinBlock - 1) / kBinBlock;
        gx = gx > 4096 ? 4096 : gx;
        SGMM_LAUNCH(k_sgu1_bin, dim3((unsigned)gx, (unsigned)n_tasks), dim3(kBinBlock), 0, as_stream(stream), tasks);
        SGMM_LAUNCHED();
    }
    ProfScope prof("sgu1_train", as_stream(stream));
    with_int<1, 2, 3, 4, 5, 6>(depth, [&](auto dc) {
        SGMM_LAUNCH(k_sgu1_train<decltype(dc)::value>, dim3((unsigned)n_tasks), dim3(kTrBlock), 0, as_stream(stream),
                    tasks);
    });
    SGMM_LAUNCHED();
    return SGMM_OK;
}
