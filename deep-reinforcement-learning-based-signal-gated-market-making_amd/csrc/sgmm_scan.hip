// sgmm_scan.hip -- the path scans: the second half of a fitness launch.
//
// The policy kernel (sgmm_table.hip, sgmm_frontier.hip) left per chunk its
// transition byte-map and the trade count along the path from each start state,
// per tick the path planes.  The scan kernels here (ScanKernel, sgmm_plan.h:
// Wave = k_path_scan, one workgroup or one wave per episode; Lanes =
// k_path_scan_lanes, 2-4 episodes per workgroup; Arl = k_path_scan_arl, the
// adversary's state machine) turn them into the episode records, the rewards
// summed in the reference's sequential float64 order (bit-exact: the plain chain
// or exact_sum_window), and run the generation tail when the launch ends the
// generation.  launch_path_scan executes the plan's scan for rollout_impl
// (sgmm_rollout.hip); the pieces shared with the frontier walk's own scan
// (ScanKernel::Fused, sgmm_frontier.hip) are in sgmm_scan.h.
//
// Reference semantics: evaluate_individual (Env/drl_engine.py:9-67), its reward
// sum (drl_engine.py:53-54) and idle penalty (drl_engine.py:64-65).
#include <algorithm>
#include <climits>

#include "sgmm_scan.h"

namespace sgmm {

// ------------------------------------------------------------------ adversary state machine
// State (inventory, previous sell fill, previous buy fill) = 4 * inv_index + 2 fs + fb
// (drl_engine.py:42-45, 62-63); a tick's 2-bit code is fill_buy | fill_sell << 1.
__device__ __forceinline__ int next_state_arl(int s, int code) {
    const int fb = code & 1, fs = code >> 1;
    return (((s >> 2) + fb - fs) << 2) | (fs << 1) | fb;
}
// one tick of the walk from state s over the tick's 2-bit fill codes f (state x
// at bits 2x): next_state_arl with the inventory step as a byte lookup
// (code 0, 1, 2, 3 -> 0, +4, -4, 0 on s & ~3) and the trade count
__device__ __forceinline__ int arl_step(int s, uint64_t f, int& cnt) {
    const int c = (int)(f >> (2 * s)) & 3;
    cnt += c != 0;
    const int d = __builtin_amdgcn_sbfe(0x00FC0400, 8 * c, 8);
    return ((s + d) & ~3) | c;
}

#ifdef SGMM_STAMPS
// diagnostic build only: phase timestamps (s_memtime) of the scan kernel per
// episode (the table kernels keep their own per wave, sgmm_table.hip)
__device__ unsigned long long g_stamps[4096][16];
#define SGMM_STAMP(e, k)                                                           \
    do {                                                                           \
        unsigned long long t_;                                                     \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
        if (threadIdx.x == 0 && (e) < 4096) g_stamps[e][k] = t_;                   \
    } while (0)
#else
#define SGMM_STAMP(e, k) \
    do {                 \
    } while (0)
#endif

// ------------------------------------------------------------------ exact ordered sum
// The episode total is the reference's sequential float64 sum
// (drl_engine.py:53: total = ((0 + r0) + r1) + ...).  It is evaluated in
// parallel, bit-exactly, from one property of IEEE addition: while the running
// sum S stays inside one binade [2^e, 2^(e+1)) (either sign) it is an integer
// multiple M of u = 2^(e-52), and fl(S + r) = (M + rint(r/u)) * u exactly as
// long as the exact S + r stays inside the binade and r/u is not a tie (x.5).
// So a stretch of ticks that keeps one binade adds up as 64-bit integers.
//
// A window of 4 NT values, cut into NT/4 blocks of 16 values, one block per
// lane of the first NT/256 waves:
//   a. float32 approximate block starts (wave scan + the waves' totals);
//   b. per block: the binade predicted from its approximate start, its integer
//      steps d = rint(r/u), their prefix range and a flag for ties / huge
//      steps / a predicted range near the binade's edges.  Blocks of one wave
//      that share a predicted binade form a run; every block gets the record
//      of the rest of its run (segmented suffix min / max of the integer
//      prefixes, the run's integer sum, its end); wave 0 extends each wave's
//      head record over the following waves;
//   c. one lane walks the blocks from the exact S, kept as (binade, integer
//      M) between fallback blocks: if S's binade is the block's prediction
//      and M plus the run's prefix range stays strictly inside [2^52, 2^53),
//      the whole rest of the run is added as one integer; otherwise the block
//      is added with the reference's float64 additions and the walk moves to
//      the next block.
// Every accepted shortcut is exact by the property above, so the result is
// the sequential sum bit for bit.  On a bench episode the walk takes ~10
// fallback blocks (the sum's doublings: ticks 2, 3, 6, 16, 22, 43, 85, ...)
// and ~11 run jumps.
constexpr int kSumBlk = 16;
constexpr int kSumTpt = 4;          // rewards gathered per path-scan thread
constexpr int kScanWin = kScanThreads * kSumTpt;
constexpr int64_t kMLo = (1LL << 52) + 1, kMHi = (1LL << 53) - 1;
constexpr int32_t kZeroRun = INT32_MAX;  // a block's prediction: all its values are +-0.0
constexpr int kHeadBlocks = 8;           // blocks added the reference way when a sum starts at +0.0
constexpr int64_t kEdge = 1LL << 40;  // prediction margin at the binade edges (2^-12 relative)
static_assert(kChunk % kSumTpt == 0, "a thread's ticks lie in one chunk");

// S = M * 2^(e-52) with |M| in [2^52, 2^53); false unless S is normal with
// |e| <= 900 (the shortcut's range: 2^(52-e) and its inverse stay normal)
__device__ __forceinline__ bool binade_of(double s, int& e, int64_t& m) {
    const int64_t bits = __double_as_longlong(s);
    const int be = (int)((bits >> 52) & 0x7FF);
    e = be - 1023;
    const int64_t mag = (bits & 0xFFFFFFFFFFFFFLL) | (1LL << 52);
    m = bits < 0 ? -mag : mag;
    return be >= 1023 - 900 && be <= 1023 + 900;
}

__device__ __forceinline__ double from_binade(int64_t m, int e) {
    const int64_t mag = m < 0 ? -m : m;  // in [2^52, 2^53)
    const int64_t bits = ((int64_t)(e + 1023) << 52) | (mag - (1LL << 52));
    return __longlong_as_double(m < 0 ? (bits | INT64_MIN) : bits);
}

__device__ __forceinline__ double uniform_f64(double v) {
    const long long b = __double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)b >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

__device__ __forceinline__ int64_t uniform_i64(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ double pow2(int k) {  // k in [-1022, 1023]
    return __longlong_as_double((int64_t)(k + 1023) << 52);
}

__device__ __forceinline__ int64_t shfl_i64(int64_t v, int src) {
    const int lo = __shfl((int)(uint32_t)v, src, kWave);
    const int hi = __shfl((int)(uint32_t)((uint64_t)v >> 32), src, kWave);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// inclusive float32 prefix sum over the wave (DPP row shifts + row broadcasts)
__device__ __forceinline__ float wave_scan_add_f32(float v) {
#define SGMM_FSTEP(CTRL, RM) \
    v += __int_as_float((int)dpp32<CTRL, RM>(0u, (uint32_t)__float_as_int(v)));
    SGMM_FSTEP(0x111, 0xF) SGMM_FSTEP(0x112, 0xF) SGMM_FSTEP(0x114, 0xF)
    SGMM_FSTEP(0x118, 0xF) SGMM_FSTEP(0x142, 0xA) SGMM_FSTEP(0x143, 0xC)
#undef SGMM_FSTEP
    return v;
}

// the walk's view of block b: the rest of its run [b, rend)
struct SumRec {
    int64_t mn, mx;  // min / max of the integer prefixes over the run, relative to b's start
    int64_t dsum;    // integer sum of blocks b .. rend-1
    int32_t be;      // predicted binade (INT32_MIN: none, tie, huge step, or past the end)
    int32_t rend;    // first block after b (window index) with another prediction, or the wave's end
};

template <int NT>
struct SumLds {
    SumRec rec[NT / 4];
    float w_ap[NT / kWave];
    double S;
};

// All NT threads call once sel[0, n) holds the window's values (n <= 4 NT)
// and a barrier has passed; returns S + sel[0] + ... + sel[n-1] in sequential
// float64 order in every thread.  S must be the same in every thread.  Ends
// with a barrier (sel may then be refilled).
// A block without a prediction takes the rest of its run with it: one loop of
// reference additions, no walk step per block (see the walk below).
template <int NT>
__device__ __forceinline__ double exact_sum_window(const double* sel, int n, double S, SumLds<NT>& L,
                                                   bool seq = false) {
    static_assert(NT % (4 * kWave) == 0, "whole block waves");
    if (seq) {
        // the plain sequential chain: wave 0's lanes add the window from LDS
        // broadcast reads in the reference's order.  Faster than the parallel
        // method below where its fallbacks are many or its window phases are not
        // hidden (the one-wave scans of thousands of GA-trained episodes, the
        // validation scans); the launch plan chooses (LaunchPlan::seq_sum).
        // seq_chain (sgmm_scan.h) spelled out: called here it moved the SGPR spills
        // of eight k_path_scan instantiations (DESIGN, "One path scan")
        if (threadIdx.x < kWave) {
            double s = S;
            const double2* p = reinterpret_cast<const double2*>(sel);
            const int nc = n & ~31;
            int i = 0;
            for (; i < nc; i += 32) {
                double2 v[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) v[j] = p[i / 2 + j];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    s += v[j].x;
                    s += v[j].y;
                }
            }
            for (; i < n; ++i) s += sel[i];
            if (threadIdx.x == 0) L.S = s;
        }
        __syncthreads();
        return L.S;
    }
    constexpr int NB = NT / 4;         // 16-value blocks per window
    constexpr int NWB = NB / kWave;    // waves holding one block per lane
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
    const int b = tid;                 // this lane's block (waves < NWB)
    const int i0 = b * kSumBlk;
    const bool blk = wv < NWB;         // wave-uniform
    const bool live = blk && i0 < n;
    double r[kSumBlk];
    float fex = 0.0f;
    if (blk) {
        // the block's values; the last block padded with -0.0 in LDS (x + -0.0
        // == x for every x, -0.0 and NaN included), so a fallback block always
        // adds 16 values
#pragma unroll
        for (int j = 0; j < kSumBlk; j += 2) {
            const double2 v = live ? *reinterpret_cast<const double2*>(sel + i0 + j) : double2{0.0, 0.0};
            r[j] = i0 + j < n ? v.x : 0.0;
            r[j + 1] = i0 + j + 1 < n ? v.y : 0.0;
        }
        if (live && i0 + kSumBlk > n)
            for (int j = n - i0; j < kSumBlk; ++j) const_cast<double*>(sel)[i0 + j] = -0.0;
        // a. approximate block starts (binade predictions only: float32 is enough)
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < kSumBlk; ++j) a += r[j];
        const float fv = (float)a;
        const float finc = wave_scan_add_f32(fv);
        fex = finc - fv;
        if (lane == kWave - 1) L.w_ap[wv] = finc;
    }
    __syncthreads();
    SGMM_STAMP(blockIdx.x, 8);
    if (blk) {
        float woff = 0.0f;  // the preceding block waves' totals (broadcast reads, in order)
#pragma unroll
        for (int k = 0; k < NWB; ++k) woff += k < wv ? L.w_ap[k] : 0.0f;
        // b. integer steps of the block in its predicted binade
        int eb = 0;
        int64_t ma = 0;  // the approximate start's mantissa
        const bool fast = live && binade_of(S + (double)(woff + fex), eb, ma);
        const double sc52 = pow2(52 - (fast ? eb : 0));
        bool bad = !fast;
        int64_t P = 0, mn = INT64_MAX, mx = INT64_MIN;
        // rint by the 1.5 * 2^52 shifter: for |q| < 2^51, q + 1.5 * 2^52 lands
        // in [2^52, 2^53) (ulp 1), so the addition rounds q half-to-even and the
        // integer is the difference of the bit patterns; a tie is |rint(q) - q|
        // == 0.5 (exact: both are multiples of ulp(q) <= 1/4).  Larger steps
        // leave the binade anyway: the block is flagged.
        constexpr double kShift = 0x1.8p52;
#pragma unroll
        for (int j = 0; j < kSumBlk; ++j) {
            const double qv = r[j] * sc52;
            const double t = qv + kShift;
            const bool bj = !(fabs(qv) < 0x1p51) || fabs((t - kShift) - qv) == 0.5;
            const bool use = fast && i0 + j < n;
            bad |= use && bj;
            const int64_t d = (use && !bj) ? __double_as_longlong(t) - __double_as_longlong(kShift) : 0;
            P += d;
            mn = min(mn, P);
            mx = max(mx, P);
        }
        // a block whose predicted prefix comes within 2^-12 of the binade's
        // edges (the float32 start's error is far below that) most likely
        // crosses it: no prediction, so the runs before it stay fast and it is
        // added the reference way
        const bool edge = fast && (ma > 0 ? (ma + mx > kMHi - kEdge || ma + mn < kMLo + kEdge)
                                          : (ma + mn < -kMHi + kEdge || ma + mx > -kMLo - kEdge));
        // a block of exact zeros (either sign) leaves any S unchanged (S is
        // never -0.0: the sum starts at +0.0 and round-to-nearest cancels to
        // +0.0), whatever its binade -- runs of them are skipped whole, which is
        // what keeps an idle individual's walk (S = 0 for the whole episode:
        // every block was a fallback) as short as a trading one's
        bool allz = true;
#pragma unroll
        for (int j = 0; j < kSumBlk; ++j) allz &= r[j] == 0.0;
        const int32_t be = allz ? kZeroRun : (fast && !bad && !edge) ? eb : INT32_MIN;
#ifdef SGMM_STAMPS
        {   // why blocks have no prediction: [6] += no binade | bad step << 20 | binade edge << 40, [7] += zero blocks
            const unsigned long long nf = __popcll(__ballot(live && !allz && !fast));
            const unsigned long long nb = __popcll(__ballot(live && !allz && fast && bad));
            const unsigned long long ne = __popcll(__ballot(live && !allz && fast && !bad && edge));
            const unsigned long long nz = __popcll(__ballot(live && allz));
            if (lane == 0 && blockIdx.x < 4096) {
                atomicAdd(&g_stamps[blockIdx.x][6], nf | nb << 20 | ne << 40);
                atomicAdd(&g_stamps[blockIdx.x][7], nz);
            }
        }
#endif
        // block sums -> wave-local exclusive prefix zl
        const uint64_t zinc = wave_scan_add((uint64_t)P);
        const int64_t zl = (int64_t)(zinc - (uint64_t)P);
        const int64_t wtot = (int64_t)readlane64(zinc, kWave - 1);
        // runs inside the wave: a block starts a run when its prediction
        // differs from the previous block's
        const int32_t bprev = __shfl_up(be, 1, kWave);
        const uint64_t starts = __ballot(lane == 0 || be != bprev);
        const uint64_t later = lane == kWave - 1 ? 0ull : starts & (~0ull << (lane + 1));
        const int rq = later ? __ffsll((unsigned long long)later) - 1 : kWave;
        // segmented suffix min / max of the in-wave prefix extremes over [lane, rq)
        int64_t amn = zl + mn, amx = zl + mx;
        // inside each 16-lane row by DPP row shifts (lane i reads lane i + d of its
        // row: no LDS round trip), then across rows from the three row heads
        // (readlane): a lane whose run goes on into row k > its row takes row k's
        // head, which covers [16k, min(rq, 16k + 16)) of the same run
        {
            const int rl_ = lane & 15;
#define SGMM_SEG_STEP(D)                                                                   \
    {                                                                                      \
        const int64_t omn = (int64_t)dpp64<0x100 + D>((uint64_t)INT64_MAX, (uint64_t)amn); \
        const int64_t omx = (int64_t)dpp64<0x100 + D>((uint64_t)INT64_MIN, (uint64_t)amx); \
        if (rl_ + D < 16 && lane + D < rq) {                                               \
            amn = min(amn, omn);                                                           \
            amx = max(amx, omx);                                                           \
        }                                                                                  \
    }
            SGMM_SEG_STEP(1) SGMM_SEG_STEP(2) SGMM_SEG_STEP(4) SGMM_SEG_STEP(8)
#undef SGMM_SEG_STEP
            const int row = lane >> 4;
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                const int64_t hmn = (int64_t)readlane64((uint64_t)amn, 16 * k);
                const int64_t hmx = (int64_t)readlane64((uint64_t)amx, 16 * k);
                if (row < k && rq > 16 * k) {
                    amn = min(amn, hmn);
                    amx = max(amx, hmx);
                }
            }
        }
        const int64_t zr = shfl_i64(zl, min(rq, kWave - 1));
        SumRec rc;
        rc.mn = amn - zl;
        rc.mx = amx - zl;
        rc.dsum = (rq < kWave ? zr : wtot) - zl;
        rc.be = be;
        rc.rend = wv * kWave + rq;
        L.rec[b] = rc;
    }
    __syncthreads();
    SGMM_STAMP(blockIdx.x, 9);
    // c. the walk (wave 0, scalar control flow, every lane carries S)
    if (wv == 0) {
        const int nblk = (n + kSumBlk - 1) / kSumBlk;
        // runs across waves: the head record of wave w (its run starts at the
        // wave's first block) is extended over the following waves while each
        // is one run with the same prediction -- a segmented suffix scan of
        // (min, max, sum) over the heads, lanes w < NT/64
        constexpr int NW = NT / (4 * kWave);  // block waves
        if (lane < NW) {
            const SumRec h = L.rec[lane * kWave];
            const int32_t bnext = __shfl_down(h.be, 1, kWave);
            const bool link = lane + 1 < NW && h.rend == (lane + 1) * kWave && bnext == h.be;
            const uint64_t brk = __ballot(!link) & ((1ull << NW) - 1);
            const uint64_t atl = brk & (~0ull << lane);  // the first break at or after this wave
            const int k = __ffsll((unsigned long long)atl) - 1;
            int64_t mn = h.mn, mx = h.mx, ds = h.dsum;
            int32_t re = h.rend;
#pragma unroll
            for (int d = 1; d < NW; d <<= 1) {
                const int src = min(lane + d, NW - 1);
                const int64_t omn = shfl_i64(mn, src), omx = shfl_i64(mx, src), ods = shfl_i64(ds, src);
                const int32_t ore = __shfl(re, src, kWave);
                if (lane + d <= k) {
                    mn = min(mn, ds + omn);
                    mx = max(mx, ds + omx);
                    ds += ods;
                    re = ore;
                }
            }
            SumRec& hw = L.rec[lane * kWave];
            hw.mn = mn;
            hw.mx = mx;
            hw.dsum = ds;
            hw.rend = re;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#ifdef SGMM_STAMPS
        unsigned long long n_iter = 0, n_slow = 0;
#endif
        // One lane walks, carrying S as (binade e, integer M) between
        // fallback blocks: a run jump is integer work only (M += the run's
        // sum), S is rebuilt as a double just for a fallback block's reference
        // additions.  Both possible next records (pos + 1 and the run end) are
        // requested as soon as the current one arrives.
        constexpr int NB = NT / 4;
        // the walk is the episode's serial chain: first call on its SIMD's issue
        // while it runs (the other waves there are in their window phases)
        __builtin_amdgcn_s_setprio(3);
        if (lane == 0 && nblk > 0) {
            int pos = 0;
            int e = 0;
            int64_t M = 0;
            bool ib = binade_of(S, e, M);  // S = M * 2^(e-52) exactly while ib
            // an episode's sum starts at +0.0 and doubles every few ticks at first
            // (ticks 2, 3, 6, 16, 22, 43, 85, ...): its first kHeadBlocks blocks
            // are walk steps that almost all fall back, so they are added the
            // reference way in one loop
            if (__double_as_longlong(S) == 0) {
                const int pe = min(kHeadBlocks, nblk);
                const double2* hp = reinterpret_cast<const double2*>(sel);
                double s = S;
                for (int b = 0; b < pe; ++b) {
                    double2 v[kSumBlk / 2];
#pragma unroll
                    for (int j = 0; j < kSumBlk / 2; ++j) v[j] = hp[b * (kSumBlk / 2) + j];
#pragma unroll
                    for (int j = 0; j < kSumBlk / 2; ++j) {
                        s += v[j].x;
                        s += v[j].y;
                    }
                }
#ifdef SGMM_STAMPS
                n_slow += pe;
#endif
                S = s;
                ib = binade_of(s, e, M);
                pos = pe;
            }
            SumRec cur = L.rec[min(pos, NB - 1)];
            while (pos < nblk) {
#ifdef SGMM_STAMPS
                ++n_iter;
#endif
                const SumRec rn = L.rec[min(pos + 1, NB - 1)];
                const SumRec rj = L.rec[min(cur.rend, NB - 1)];
                // (a zero run is skipped unless S is -0.0: only the API's init can make it so)
                // every term evaluated, combined bitwise: no branch per term on the
                // walk's serial chain (the short-circuit form compiled to 4-5 branches;
                // measured the same, profiles/r04_ab/r04af*)
                const int64_t lo_ = M + cur.mn, hi_ = M + cur.mx;
                const bool pos_ok = (lo_ >= kMLo) & (hi_ <= kMHi);
                const bool neg_ok = (hi_ <= -kMLo) & (lo_ >= -kMHi);
                const bool zero_ok = (cur.be == kZeroRun) & (ib | (__double_as_longlong(S) != INT64_MIN));
                const bool ok = zero_ok | (ib & (cur.be == e) & (M > 0 ? pos_ok : neg_ok));
                const int64_t Mj = M + cur.dsum;
                const int pj = cur.rend;
                // a block without a prediction is added the reference way whatever
                // S is, and so is the rest of its run (every block of [pos, rend)
                // has none): the whole streak in one loop of 8 values per LDS
                // round trip (a sum crossing zero or sitting on a binade edge makes
                // such streaks: the slowest episodes' walks were 70-171 one-block
                // fallbacks)
                const bool streak = !ok && cur.be == INT32_MIN;
                const int pend = streak ? min(pj, nblk) : pos + 1;
                if (!ok) {  // blocks [pos, pend) the reference way (the last block padded with -0.0)
#ifdef SGMM_STAMPS
                    n_slow += pend - pos;
#endif
                    const double2* vp = reinterpret_cast<const double2*>(sel + pos * kSumBlk);
                    double2 v[kSumBlk / 2];
#pragma unroll
                    for (int j = 0; j < kSumBlk / 2; ++j) v[j] = vp[j];
                    double s = ib ? from_binade(M, e) : S;
#pragma unroll
                    for (int j = 0; j < kSumBlk / 2; ++j) {
                        s += v[j].x;
                        s += v[j].y;
                    }
                    // the rest of a streak, 8 values per LDS round trip
                    const double2* __restrict__ sp = vp + kSumBlk / 2;
                    const double2* const se = vp + (pend - pos) * (kSumBlk / 2);
                    for (; sp < se; sp += 4) {
                        const double2 a = sp[0], b = sp[1], c = sp[2], d = sp[3];
                        s += a.x;
                        s += a.y;
                        s += b.x;
                        s += b.y;
                        s += c.x;
                        s += c.y;
                        s += d.x;
                        s += d.y;
                    }
                    S = s;
                    ib = binade_of(s, e, M);
                }
                // both successors' records were requested before the decision
                // (a streak ends at the run's end: its record is rj)
                const bool to_end = ok || streak;
                M = ok ? Mj : M;
                pos = ok ? pj : pend;
                // field by field: a whole-struct select was lowered to a scratch
                // round trip per step
                cur.mn = to_end ? rj.mn : rn.mn;
                cur.mx = to_end ? rj.mx : rn.mx;
                cur.dsum = to_end ? rj.dsum : rn.dsum;
                cur.be = to_end ? rj.be : rn.be;
                cur.rend = to_end ? rj.rend : rn.rend;
                if (pos >= nblk) break;
            }
            L.S = ib ? from_binade(M, e) : S;
        }
#ifdef SGMM_STAMPS
        if (threadIdx.x == 0 && blockIdx.x < 4096) { g_stamps[blockIdx.x][13] += n_iter; g_stamps[blockIdx.x][14] += n_slow; }
#endif
        if (lane == 0 && nblk == 0) L.S = S;
        __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();
    SGMM_STAMP(blockIdx.x, 10);
    return L.S;
}

// LDS bytes the tail needs (aliased onto the kernel's dynamic LDS)
static inline size_t step_lds_bytes(int threads, const StepArgs& sa) {
    return (size_t)threads * 2 * (sizeof(double) + sizeof(int)) +
           sizeof(float) * (size_t)(sa.n_mm + (sa.master_adv ? sa.n_adv : 0));
}

// Thread 0 stored the workgroup's record with store_record.  It drains the
// stores, takes an arrival ticket (agent-scope atomic); the workgroup that
// draws the last ticket reads every record with sc1 loads (ga_step_dev
// <HANDOFF = true>) -- MI355X_MICROARCH.md inter-workgroup visibility, row 1
// -- runs the GA step and resets the ticket for the next launch.  e = the
// episode whose record was stored (its population's ticket), n_total = the
// launch's episodes (one population when pop_eps == 0).
// The GA step of population k once all its records are stored (the last
// arriver's part of generation_tail; the fused frontier launch's cleanup runs
// it directly).
__device__ __forceinline__ void tail_run(const StepArgs& sa0, const double* fitness0, const int32_t* trades0, unsigned char* lds,
                         int k, int n_eps) {
    StepArgs sa = sa0;
    sa.st = sa0.st + k;
    sa.master_mm = sa0.master_mm + (int64_t)k * sa0.n_mm;
    if (sa0.master_adv) sa.master_adv = sa0.master_adv + (int64_t)k * sa0.n_adv;
    if (sa0.best_master) sa.best_master = sa0.best_master + (int64_t)k * sa0.n_mm;
    if (sa0.history) sa.history = sa0.history + (int64_t)k * sa0.hist_cap;
    if (sa0.seeds) sa.seed = sa0.seeds[k];
    const double* fitness = fitness0 + (int64_t)k * n_eps;
    const int32_t* trades = trades0 + (int64_t)k * n_eps;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // compiler order only: loads after the ticket
    SGMM_STAMP(blockIdx.x, 4);
#ifdef SGMM_STAMPS
    if (threadIdx.x == 0) g_stamps[4095][0] = g_stamps[blockIdx.x][4];
#endif
    const int nt = blockDim.x;
    double* sv = reinterpret_cast<double*>(lds);
    int* si = reinterpret_cast<int*>(sv + 2 * nt);
    float* lm = reinterpret_cast<float*>(si + 2 * nt);
    float* la = lm + sa.n_mm;
    if (sa.mode == kStepArgmax) {
        if (threadIdx.x < kWave) tell_wave<true>(sa.st, fitness, trades, sa.P, sa.history, sa.hist_cap);
    } else if (sa.P <= nt && sa.n_mm <= 16 * nt && sa.n_adv <= 16 * nt)
        ga_step_fused<true>(sa.st, fitness, trades, fitness + sa.P, trades + sa.P, sa.P, sa.master_mm,
                            sa.master_adv, sa.best_master, sa.n_mm, sa.n_adv, sa.seed, sa.history,
                            sa.hist_cap, sv, si);
    else
        ga_step_dev<true>(sa.st, fitness, trades, fitness + sa.P, trades + sa.P, sa.P, ShardView{0, 0},
                          sa.master_mm, sa.master_adv, sa.best_master, sa.n_mm, sa.n_adv, sa.seed,
                          sa.history, sa.hist_cap, nullptr, nullptr, 0, 0, sv, si, lm, la);
    if (threadIdx.x == 0) sa.st->arrivals = 0;
    SGMM_STAMP(blockIdx.x, 5);
}

__device__ __forceinline__ void generation_tail(const StepArgs& sa0, const double* fitness0, const int32_t* trades0,
                                unsigned char* lds, int* s_last, int e, int n_total) {
    // this episode's population (one arrival ticket per population)
    int k, n_eps;
    population_of(sa0, e, n_total, k, n_eps);
    if (threadIdx.x == 0) *s_last = arrival_ticket(sa0, k, 1, n_eps);
    __syncthreads();
    if (!*s_last) return;
    tail_run(sa0, fitness0, trades0, lds, k, n_eps);
}

// The validation launch's tail (StepArgs::mode 2): episode k holds the
// validation record (v, vtr: thread 0's values) of population k's post-tell
// master and runs its bookkeeping -- no other episode's record is needed.
__device__ __forceinline__ void validation_tail(const StepArgs& sa, double v, int32_t vtr, int* flag, int k) {
    __syncthreads();  // flag aliases LDS the caller has just read
    if (sa.mode == kStepDeferred) {
        // the deferred tell: master <- ask(best) with the generation's sigma and
        // counter (the bookkeeping below decays sigma and advances gen)
        const sgmm_ga_state* st = sa.st + k;
        const uint32_t gen = (uint32_t)st->gen;
        const int best = st->best_idx, abest = st->adv_best_idx;
        const float smm = (float)st->sigma_mm, sadv = (float)st->sigma_adv;
        const uint64_t seed = sa.seeds ? sa.seeds[k] : sa.seed;
        regen_master_block(sa.master_mm + (int64_t)k * sa.n_mm, nullptr, sa.n_mm, smm, seed, 0u, gen, best);
        if (sa.master_adv)
            regen_master_block(sa.master_adv + (int64_t)k * sa.n_adv, nullptr, sa.n_adv, sadv, seed, 1u, gen, abest);
        __syncthreads();  // the new master before the checkpoint copy reads it
    }
    val_update_dev(sa.st + k, v, vtr, sa.master_mm + (int64_t)k * sa.n_mm,
                   sa.best_master ? sa.best_master + (int64_t)k * sa.n_mm : nullptr, sa.n_mm,
                   sa.history ? sa.history + (int64_t)k * sa.hist_cap : nullptr, sa.hist_cap, flag);
}

// ------------------------------------------------------------------ path scan (no adversary)
// Per episode (one workgroup, or one wave of the fused frontier launch):
//   1. wave 0: chunk start states from a wave-level scan of the chunk maps,
//      and the episode's trades: each chunk's count along the path from its
//      start state (8 bits per start state, written by the table);
//   2. every thread: the rewards of its 4 ticks from the path plane of their
//      chunk's start state (one coalesced row per chunk) -> LDS;
//   3. the rewards' sequential float64 sum, bit-exact (exact_sum_window).
// FR: the frontier kernel's chunks (frontier_len(T, nw) ticks, 64 per wave,
// records e * 256 + c, u32 trade counts, kinfo = merge tick | p0 << 29).
// TPB < NT: a TPB-thread workgroup with NT's window and block layout (TPB =
// 64, NT = 256: one wave -- the only one exact_sum_window<256> gives blocks
// to -- gathers 1024 values, so many more episodes run per CU).
template <int NT>
struct ScanShared {
    double* sel;          // [NT * kSumTpt] the window (the last block padded in place)
    SumLds<NT>* L;
    uint8_t* start;       // chunk start states
    uint32_t* kin;        // FR: the chunks' merge info
    int* red;             // trades, then the tail's "last arriver" flag
    unsigned char* tail;  // generation-tail scratch (aliases sel)
};

template <int NSM, int NT, bool FR, int TPB>
__device__ __forceinline__ void scan_episode(int e, int nw, const EpArrays& ep, const sgmm_env_params* __restrict__ params,
                                             int32_t inv_min, const uint64_t* __restrict__ cmaps,
                                             const uint64_t* __restrict__ ctr, const uint32_t* __restrict__ kinfo,
                                             const double* __restrict__ rew, double* __restrict__ fitness,
                                             int32_t* __restrict__ trades_out, const StepArgs& step, int n_total,
                                             const ScanShared<NT>& sh) {
    static_assert(TPB == NT || (TPB == kWave && NT == 4 * kWave), "TPB = NT or one wave with NT = 256");
    constexpr int kWin = NT * kSumTpt;
    double* sel = sh.sel;
    uint8_t* start = sh.start;
    uint32_t* kin = sh.kin;
    const int32_t T = ep.len[e];
    const int64_t so = ep.step_off[e];
    // FR: records laid out for nw (ep.ngrp) groups; the episode's own group
    // count is in its first record
    const int64_t cb = FR ? frontier_rec(e, nw, 0) : (int64_t)chunk_base(so, e);
    const int nwe = (FR && T > 0) ? (int)kinfo_groups(kinfo[cb]) : 1;
    const int CL = FR ? frontier_len(T, nwe) : kChunk;
    const int nch = (T + CL - 1) / CL;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    SGMM_STAMP(e, 0);
    if (tid < kWave) {  // chunk start states, 64 chunks per round, carried across rounds
        uint32_t s = (uint32_t)(-inv_min);
        int tr = 0;
        for (int c0 = 0; c0 < nch; c0 += kWave) {
            const int c = c0 + lane;
            const uint64_t m = c < nch ? cmaps[cb + c] : kIdentityMap;
            const uint64_t k = (!FR && c < nch) ? ctr[cb + c] : 0;
            const uint32_t st = chunk_starts(m, s, lane);
            if (c < nch) start[c] = (uint8_t)st;
            if (FR) {
                if (c < nch) {
                    tr += frontier_trades<PlainLd>(reinterpret_cast<const uint32_t*>(ctr), cb + c, st);
                    kin[c] = kinfo[cb + c];
                }
            } else {
                tr += table_trades(k, st);
            }
        }
        tr = wave_sum_i32(tr);
        if (lane == 0) *sh.red = tr;
    }
    __syncthreads();
    SGMM_STAMP(e, 1);
#ifdef SGMM_STAMPS
    // per episode, summed over the windows: 11 gather cycles, 12 sum cycles,
    // 15 windows; 13 / 14 walk iterations / fallback blocks
    unsigned long long sw_a, sw_b, sw_g = 0, sw_s = 0, sw_n = 0;
    if (tid == 0 && e < 4096) g_stamps[e][13] = g_stamps[e][14] = g_stamps[e][6] = g_stamps[e][7] = 0;
#define SGMM_SW(var) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory")
#endif
    double S = 0.0;  // exact running sum (identical in every thread between windows)
    // a window's rewards: each thread's NT / TPB groups of kSumTpt ticks (4
    // ticks of one chunk, CL % kSumTpt == 0) gathered into registers; the next
    // window's loads are issued before this window's exact sum, so their
    // latency hides behind the sum's serial walk
    double r[NT / TPB][kSumTpt];
    auto gather = [&](int w0) {
        const int n = min(kWin, T - w0);
#pragma unroll
        for (int g = 0; g < NT / TPB; ++g) {
            const int i0 = (g * TPB + tid) * kSumTpt;
            if (i0 < n) {
                if (FR) {
                    frontier_gather4<PlainLd, true>(r[g], rew, start, kin, frontier_base(so, e, nw), CL, ep.rs, w0 + i0,
                                                    n - i0);
                } else {
                    const double* __restrict__ src = rew + (int64_t)start[(w0 + i0) / kChunk] * ep.rs + so + w0 + i0;
#pragma unroll
                    for (int j = 0; j < kSumTpt; ++j) r[g][j] = src[min(j, n - 1 - i0)];
                }
            }
        }
    };
    if (T > 0) gather(0);
    for (int w0 = 0; w0 < T; w0 += kWin) {
        const int n = min(kWin, T - w0);
#ifdef SGMM_STAMPS
        SGMM_SW(sw_a);
#endif
#pragma unroll
        for (int g = 0; g < NT / TPB; ++g) {
            const int i0 = (g * TPB + tid) * kSumTpt;
#pragma unroll
            for (int j = 0; j < kSumTpt; ++j)
                if (i0 + j < n) sel[i0 + j] = r[g][j];
        }
        __syncthreads();
        SGMM_STAMP(e, 2);
#ifdef SGMM_STAMPS
        SGMM_SW(sw_b);
        sw_g += sw_b - sw_a;
#endif
        if (w0 + kWin < T) gather(w0 + kWin);  // in flight during the sum
        S = exact_sum_window<NT>(sel, n, S, *sh.L, ep.seq_sum != 0);
#ifdef SGMM_STAMPS
        SGMM_SW(sw_a);
        sw_s += sw_a - sw_b;
        sw_n += 1;
#endif
    }
#ifdef SGMM_STAMPS
    if (tid == 0 && e < 4096) {
        g_stamps[e][11] = sw_g;
        g_stamps[e][12] = sw_s;
        g_stamps[e][15] = sw_n;
    }
#undef SGMM_SW
#endif
    SGMM_STAMP(e, 3);
    int tr = 0;  // thread 0's record (the tails read it there only)
    double total = S;
    if (tid == 0) {
        tr = *sh.red;
        total = finish_record(params, ep, fitness, trades_out, e, total, tr);
    }
    if (step.st) {
        if (step.mode == kStepValidate || step.mode == kStepDeferred) validation_tail(step, total, tr, sh.red, e);
        else generation_tail(step, fitness, trades_out, sh.tail, sh.red, e, n_total);
    }
}

// one workgroup per episode (the table path, and the frontier path unfused)
template <int NSM, int NT, bool FR, int TPB = NT>
__global__ __launch_bounds__(TPB) void k_path_scan(
    EpArrays ep, const sgmm_env_params* __restrict__ params, int32_t inv_min,
    const uint64_t* __restrict__ cmaps, const uint64_t* __restrict__ ctr,
    const uint32_t* __restrict__ kinfo, const double* __restrict__ rew, double* __restrict__ fitness,
    int32_t* __restrict__ trades_out, StepArgs step) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ SumLds<NT> L;
    __shared__ uint8_t start_t[FR ? 1 : kMaxLen / kChunk];
    __shared__ int red_trades;
    const int e = blockIdx.x;
    // frontier chunks (64 per group): their start states and merge info follow
    // the window in the dynamic LDS (scan_lds_bytes)
    uint8_t* start = FR ? lds + NT * kSumTpt * sizeof(double) : start_t;
    uint32_t* kin = reinterpret_cast<uint32_t*>(lds + NT * kSumTpt * sizeof(double) + kFrontierLanes * ep.ngrp);
    const ScanShared<NT> sh{reinterpret_cast<double*>(lds), &L, start, kin, &red_trades, lds};
    scan_episode<NSM, NT, FR, TPB>(e, FR ? ep.ngrp : 1, ep, params, inv_min, cmaps, ctr, kinfo, rew, fitness, trades_out,
                                   step, (int)gridDim.x, sh);
}

// ------------------------------------------------------------------ path scan, W episodes per workgroup
// The frontier path scan for many episodes, the sums as sequential chains: wave w
// of the workgroup takes episode e0 + w through the scan's first two phases (chunk
// start states and trades; the rewards of its path, kLanesWin ticks per window,
// into LDS row w, padded with -0.0), and wave 0 adds the W windows, lane w episode
// e0 + w, one dependent v_add_f64 advancing all W chains.  The one-wave scan ran
// one chain per wave on all 64 lanes: with 2-3 scans per SIMD its float64 adds
// shared the vector pipe (trained config 3: ~20 cycles per tick and episode,
// against ~10 for a lone chain, tools/mb_trained_timeline.py SCAN=1).  x + -0.0 == x
// for every x, so the padding leaves each episode's sum its reference-order chain.
// The generation tail: the workgroup's W records, one arrival of W (the tell's
// argmax, StepArgs mode 3, when its last population record arrives).
// W and the window measured (profiles/r06_lanes/, scan of config 3 / of config 5's
// 1-of-8 shard): W = 16 57.8 / 40.5 us, 8 59.5 / 33.9, 4 55.5 / 31.1, 2 53.5 / 33.5;
// 1024-tick windows 56.5-59.6 / 33.8 (one episode per wave: 72.2 / 37.5)
constexpr int kLanesWin = 512;              // ticks per window
constexpr int kLanesPitch = kLanesWin + 2;  // doubles per LDS row (16-byte bank offset per row)
static size_t lanes_scan_lds(int ngrp, int w) {
    return (size_t)w * kLanesPitch * sizeof(double) + (size_t)w * kFrontierLanes * ngrp * (sizeof(uint32_t) + 1) + 64;
}
template <int NSM, int kLanesW>
__global__ __launch_bounds__(kWave * kLanesW) void k_path_scan_lanes(
    EpArrays ep, const sgmm_env_params* __restrict__ params, int32_t inv_min, const uint64_t* __restrict__ cmaps,
    const uint32_t* __restrict__ ctr32, const uint32_t* __restrict__ kinfo, const double* __restrict__ rew,
    double* __restrict__ fitness, int32_t* __restrict__ trades_out, StepArgs step, int32_t n) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int nw = ep.ngrp;
    double* win = reinterpret_cast<double*>(lds);  // [kLanesW][kLanesPitch]
    uint32_t* kin_all = reinterpret_cast<uint32_t*>(win + kLanesW * kLanesPitch);
    uint8_t* start_all = reinterpret_cast<uint8_t*>(kin_all + kLanesW * kFrontierLanes * nw);
    __shared__ int32_t red_s[kLanesW];
    __shared__ int32_t len_s[kLanesW];
    const int w = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & (kWave - 1));
    const int e0 = (int)blockIdx.x * kLanesW, e = e0 + w;
    constexpr int wc = 0;  // the chain wave (rotating it over the SIMDs measured no different)
    SGMM_STAMP(blockIdx.x, 0);
#ifdef SGMM_STAMPS
    if (threadIdx.x == 0 && blockIdx.x < 4096) g_stamps[blockIdx.x][12] = 0;
#endif
    const bool has = e < n;
    const int32_t T = has ? ep.len[e] : 0;
    uint32_t* kin = kin_all + w * kFrontierLanes * nw;
    uint8_t* start = start_all + w * kFrontierLanes * nw;
    double* row = win + w * kLanesPitch;
    // 1. (wave w) chunk start states and the trades along the path
    const int64_t cb = frontier_rec(has ? e : 0, nw, 0);
    const int nwe = T > 0 ? (int)kinfo_groups(kinfo[cb]) : 1;
    const int CL = frontier_len(T, nwe);
    const int nch = T > 0 ? (T + CL - 1) / CL : 0;
    {
        uint32_t s = (uint32_t)(-inv_min);
        int tr = 0;
        for (int c0 = 0; c0 < nch; c0 += kWave) {
            const int c = c0 + lane;
            const uint64_t m = c < nch ? cmaps[cb + c] : kIdentityMap;
            const uint32_t st = chunk_starts(m, s, lane);
            if (c < nch) {
                start[c] = (uint8_t)st;
                kin[c] = kinfo[cb + c];
                tr += frontier_trades<PlainLd>(ctr32, cb + c, st);
            }
        }
        tr = wave_sum_i32(tr);
        if (lane == 0) {
            red_s[w] = tr;
            len_s[w] = T;
        }
    }
    __syncthreads();
    SGMM_STAMP(blockIdx.x, 1);
    int tmax = 0;
#pragma unroll
    for (int i = 0; i < kLanesW; ++i) tmax = max(tmax, len_s[i]);
    // 2. windows: every wave gathers its episode's next window while wave 0 adds
    const int64_t base = frontier_base(has ? ep.step_off[e] : 0, has ? e : 0, nw);
    constexpr int kG = kLanesWin / (4 * kWave);
    double r[kG][4];
    auto gather = [&](int w0) {
        const int cnt = min(kLanesWin, T - w0);  // <= 0 past the episode's end
#pragma unroll
        for (int q = 0; q < kG; ++q) {
            const int i0 = (q * kWave + lane) * 4;
            if (i0 < cnt)
                frontier_gather4<PlainLd, true>(r[q], rew, start, kin, base, CL, ep.rs, w0 + i0, cnt - i0);
        }
    };
    gather(0);
    double S = 0.0;  // wave 0, lane v < kLanesW: episode e0 + v
    const double* mine = win + min(lane, kLanesW - 1) * kLanesPitch;
    for (int w0 = 0; w0 < tmax; w0 += kLanesWin) {
        const int cnt = T - w0;
#pragma unroll
        for (int q = 0; q < kG; ++q) {
            const int i0 = (q * kWave + lane) * 4;
            double2 a, b;
            a.x = i0 < cnt ? r[q][0] : -0.0;
            a.y = i0 + 1 < cnt ? r[q][1] : -0.0;
            b.x = i0 + 2 < cnt ? r[q][2] : -0.0;
            b.y = i0 + 3 < cnt ? r[q][3] : -0.0;
            *reinterpret_cast<double2*>(row + i0) = a;
            *reinterpret_cast<double2*>(row + i0 + 2) = b;
        }
        __syncthreads();
#ifdef SGMM_STAMPS
        if (w0 == 0) SGMM_STAMP(blockIdx.x, 2);
        unsigned long long ch0;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(ch0)::"memory");
#endif
        if (w0 + kLanesWin < T) gather(w0 + kLanesWin);
        if (w == wc) {
            // this window's length over the workgroup's episodes
            const int m = min(kLanesWin, tmax - w0);
            S = seq_chain(S, mine, m);
#ifdef SGMM_STAMPS
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            unsigned long long ch1;
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(ch1)::"memory");
            if (threadIdx.x == 0 && blockIdx.x < 4096) g_stamps[blockIdx.x][12] += ch1 - ch0;
#endif
        }
        __syncthreads();  // the windows are read before the next ones are written
    }
    SGMM_STAMP(blockIdx.x, 3);
    // 3. records (the chain wave, lane v: episode e0 + v) and the generation tail
    if (w == wc) {
        const int nv = min(kLanesW, n - e0);
        if (lane < nv) finish_record(params, ep, fitness, trades_out, e0 + lane, S, red_s[lane]);
        if (step.st) population_arrive(step, fitness, trades_out, e0, nv, n, lane);
    }
    SGMM_STAMP(blockIdx.x, 4);
}

// ------------------------------------------------------------------ ordered sum (standalone)
// init + x[0] + x[1] + ... in sequential float64 order, one workgroup.
__global__ __launch_bounds__(kScanThreads) void k_ordered_sum(const double* __restrict__ x, int64_t n,
                                                              double init, double* __restrict__ out) {
    __shared__ __align__(16) double sel[kScanWin];
    __shared__ SumLds<kScanThreads> L;
    double S = init;
    for (int64_t w0 = 0; w0 < n; w0 += kScanWin) {
        const int m = (int)min((int64_t)kScanWin, n - w0);
        for (int i = threadIdx.x; i < m; i += kScanThreads) sel[i] = x[w0 + i];
        __syncthreads();
        S = exact_sum_window<kScanThreads>(sel, m, S, L);
    }
    if (threadIdx.x == 0) *out = S;
}

// ------------------------------------------------------------------ path scan (adversary)
// 4 nsi-state machine (inventory x previous fill flags).  Per episode, one
// NT-thread workgroup, segment by segment (kSeg ticks = 128 pieces of 32), the
// state entering a segment carried over -- no bound on the episode length:
//   1. the segment's fill codes -> LDS (coalesced);
//   2. every (piece, start state) pair walks its piece over the LDS codes (8
//      per round trip): the piece's transducer, end state and trade count per
//      start state (all NT threads: 3 rounds of 32 steps at config 4, where
//      one serial walker per table wave cost the table ~25 us; 64-tick pieces
//      took 2 rounds of 64 steps, and twice as long in step 4);
//   3. the end maps chained by pointer jumping (log2(128) rounds over all
//      (piece, state) pairs) -> each piece's start state; trades = the sum of
//      every piece's count from its start state;
//   4. one thread per piece walks its 32 ticks from the start state and
//      records the state of every tick;
//   5. every thread gathers its ticks' rewards from the per-state planes
//      rew[state * rs + row] (independent loads: one latency per segment;
//      consecutive ticks in one state are consecutive addresses);
//   6. the exact sequential float64 sum (exact_sum_window).
// Dynamic LDS: [kSeg u64 codes / f64 rewards][kSeg states][2][128][ns] maps
// [128][ns] trade counts [128] starts.
constexpr int kArlSub = 32;                 // ticks per transducer piece (half a table chunk)
constexpr int kSegChunks = kSeg / kArlSub;  // pieces per segment
static size_t arl_scan_lds(int ns) { return (size_t)kSeg * 9 + (size_t)3 * kSegChunks * ns + kSegChunks; }
template <int NT>
__global__ __launch_bounds__(NT) void k_path_scan_arl(
    EpArrays ep, const sgmm_env_params* __restrict__ params, int32_t inv_min, int32_t nsi,
    const uint64_t* __restrict__ fills, const double* __restrict__ rew,
    double* __restrict__ fitness, int32_t* __restrict__ trades_out, StepArgs step) {
    extern __shared__ __align__(16) unsigned char lds[];
    uint64_t* fl = reinterpret_cast<uint64_t*>(lds);  // the segment's fill codes, then
    double* sel = reinterpret_cast<double*>(lds);     // its rewards (the codes are dead by then)
    uint8_t* stt = lds + kSeg * sizeof(double);       // [kSeg] the state at each tick
    const int ns = 4 * nsi;
    uint8_t* jm = stt + kSeg;                         // [2][segch][ns] jump maps (double-buffered)
    uint8_t* tr = jm + 2 * kSegChunks * ns;           // [segch][ns] trades from each start state
    uint8_t* start = tr + kSegChunks * ns;            // [segch]
    __shared__ SumLds<NT> L;
    __shared__ int red_trades;
    const int e = blockIdx.x;
    const int32_t T = ep.len[e];
    const int64_t so = ep.step_off[e];
    const uint64_t* __restrict__ F = fills + so;
    const int tid = threadIdx.x;
    if (tid == 0) red_trades = 0;
    SGMM_STAMP(e, 0);
    int carry = (-inv_min) << 2;  // the state entering the segment (episode start: inventory 0, no fills)
    int my_trades = 0;
    double total = 0.0;
    for (int seg0 = 0; seg0 < T; seg0 += kSeg) {
        const int segn = min(kSeg, T - seg0);
        const int segch = (segn + kArlSub - 1) / kArlSub;
        for (int i = tid; i < segn; i += NT) fl[i] = F[seg0 + i];
        __syncthreads();
        SGMM_STAMP(e, 1);
        // chunk k's transducer from start state s (padded ticks: none, the walk stops at the chunk's end)
        for (int i = tid; i < segch * ns; i += NT) {
            const int k = i / ns;
            int st = i - k * ns, cnt = 0;
            const int ta = k * kArlSub, tb = min(segn, ta + kArlSub);
            if (tb - ta == kArlSub) {  // a whole piece: no per-tick bound check
#pragma unroll 1
                for (int t8 = ta; t8 < tb; t8 += 8) {
                    uint64_t f[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) f[j] = fl[t8 + j];
#pragma unroll
                    for (int j = 0; j < 8; ++j) st = arl_step(st, f[j], cnt);
                }
            } else
            for (int t8 = ta; t8 < tb; t8 += 8) {
                uint64_t f[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = fl[t8 + j];  // < kSeg: in the buffer
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (t8 + j < tb) {
                        const int c = (int)(f[j] >> (2 * st)) & 3;
                        cnt += c != 0;
                        st = next_state_arl(st, c);
                    }
            }
            jm[i] = (uint8_t)st;
            tr[i] = (uint8_t)cnt;
        }
        __syncthreads();
        SGMM_STAMP(e, 6);
        // jm[k][s] = state after chunks k-2^r+1 .. k from state s at chunk k-2^r+1's start
        int cur = 0;
        for (int d = 1; d < segch; d <<= 1) {
            const uint8_t* a = jm + cur * segch * ns;
            uint8_t* b = jm + (cur ^ 1) * segch * ns;
            for (int i = tid; i < segch * ns; i += NT) {
                const int k = i / ns, st = i - k * ns;
                b[i] = k >= d ? a[k * ns + a[(k - d) * ns + st]] : a[i];
            }
            cur ^= 1;
            __syncthreads();
        }
        // start of chunk k = the inclusive prefix of chunks 0 .. k-1 applied to the carry
        const uint8_t* pre = jm + cur * segch * ns;
        for (int k = tid; k < segch; k += NT) {
            const int st = k == 0 ? carry : pre[(k - 1) * ns + carry];
            start[k] = (uint8_t)st;
            my_trades += tr[k * ns + st];
        }
        __syncthreads();
        SGMM_STAMP(e, 7);
        carry = pre[(segch - 1) * ns + carry];
        if (tid < segch) {  // piece tid's state path
            int st = start[tid];
            const int ta = tid * kArlSub, tb = min(segn, ta + kArlSub);
            if (tb - ta == kArlSub) {  // a whole piece: no per-tick bound check
                int unused = 0;
#pragma unroll 1
                for (int t8 = ta; t8 < tb; t8 += 8) {
                    uint64_t f[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) f[j] = fl[t8 + j];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        stt[t8 + j] = (uint8_t)st;
                        st = arl_step(st, f[j], unused);
                    }
                }
            } else
            for (int t8 = ta; t8 < tb; t8 += 8) {
                uint64_t f[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = fl[t8 + j];
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (t8 + j < tb) {
                        stt[t8 + j] = (uint8_t)st;
                        st = next_state_arl(st, (int)(f[j] >> (2 * st)) & 3);
                    }
            }
        }
        __syncthreads();  // the codes are dead: sel takes their place
        SGMM_STAMP(e, 11);
        for (int i = tid; i < segn; i += NT) sel[i] = rew[(int64_t)stt[i] * ep.rs + so + seg0 + i];
        __syncthreads();
        SGMM_STAMP(e, 12);
        for (int k = 0; k < segn; k += 4 * NT)  // windows of 4 values per thread
            total = exact_sum_window<NT>(sel + k, min(4 * NT, segn - k), total, L, ep.seq_sum != 0);
    }
    const int w = wave_sum_i32(my_trades);
    if ((tid & (kWave - 1)) == 0 && w) atomicAdd(&red_trades, w);
    __syncthreads();
    if (tid == 0) finish_record(params, ep, fitness, trades_out, e, total, red_trades);
    SGMM_STAMP(e, 3);
    if (step.st) generation_tail(step, fitness, trades_out, lds, &red_trades, e, (int)gridDim.x);
}

// ------------------------------------------------------------------ launches
void launch_path_scan(const LaunchPlan& plan, const ScanArgs& a, hipStream_t s) {
    const bool fr = plan.policy == PolicyKernel::Frontier;
    const int nt = plan.scan_threads;
    const dim3 grid(plan.scan_grid), block(nt);
    EpArrays ep = a.ep;
    ep.seq_sum = plan.seq_sum;
    if (plan.scan == ScanKernel::Arl) {
        size_t lds = arl_scan_lds(4 * a.nsi);
        if (a.step.st) lds = std::max(lds, step_lds_bytes(nt, a.step));
        if (nt == kScanThreads)
            SGMM_LAUNCH(k_path_scan_arl<kScanThreads>, grid, block, lds, s, ep, a.params, a.inv_min, a.nsi, a.fills,
                        a.rew, a.fitness, a.trades, a.step);
        else
            SGMM_LAUNCH(k_path_scan_arl<kScanBlock>, grid, block, lds, s, ep, a.params, a.inv_min, a.nsi, a.fills,
                        a.rew, a.fitness, a.trades, a.step);
    } else if (plan.scan == ScanKernel::Lanes) {
        const int lw = plan.lanes_w;
        const size_t lds = lanes_scan_lds(ep.ngrp, lw);
        with_int<5, 8>(a.nsi <= 5 ? 5 : 8, [&](auto n) {
            with_int<2, 4>(lw, [&](auto lw_) {
                SGMM_LAUNCH((k_path_scan_lanes<decltype(n)::value, decltype(lw_)::value>), grid, block, lds, s, ep,
                            a.params, a.inv_min, a.cmaps, reinterpret_cast<const uint32_t*>(a.ctr), a.kinfo, a.rew,
                            a.fitness, a.trades, a.step, a.n);
            });
        });
    } else {
        size_t lds = (size_t)(nt == kWave ? 4 * kWave : nt) * kSumTpt * sizeof(double) +  // the window
                     (fr ? (size_t)5 * kFrontierLanes * ep.ngrp : 0);  // chunk start states + merge info
        if (a.step.st) lds = std::max(lds, step_lds_bytes(nt, a.step));
        // one wave runs the 256-thread window and block layout (k_path_scan<NSM, 256, FR, 64>)
        with_int<5, 8>(a.nsi <= 5 ? 5 : 8, [&](auto n) {
            with_bool(fr, [&](auto f) {
                with_int<kWave, kScanThreads, 512, 256>(nt, [&](auto t) {
                    constexpr int TPB = decltype(t)::value, NT = TPB == kWave ? 4 * kWave : TPB;
                    SGMM_LAUNCH((k_path_scan<decltype(n)::value, NT, decltype(f)::value, TPB>), grid, block, lds, s, ep,
                                a.params, a.inv_min, a.cmaps, a.ctr, a.kinfo, a.rew, a.fitness, a.trades, a.step);
                });
            });
        });
    }
}

void launch_ordered_sum(const double* values, int64_t n, double init, double* out, hipStream_t s) {
    SGMM_LAUNCH(k_ordered_sum, dim3(1), dim3(kScanThreads), 0, s, values, n, init, out);
}

}  // namespace sgmm

#ifdef SGMM_STAMPS
extern "C" int sgmm_debug_stamps(unsigned long long* host, int n_eps) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(sgmm::g_stamps), sizeof(unsigned long long) * 16 * n_eps);
}
extern "C" int sgmm_debug_tail(unsigned long long* host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(sgmm::g_tail), sizeof(unsigned long long) * 8);
}
#endif
