// sgmm_plan.h -- the launch plan of a rollout batch: which policy kernel and
// path scan run, the frontier kernel's chunk groups, and the workspace layout,
// resolved once per launch from (shape, knobs, SIMD count).
//
// Pure host arithmetic: no HIP header, so a plain C++17 compiler builds it
// (tests/plan_check.cpp).  Every rule lives here and nowhere else;
// rollout_impl (sgmm_rollout.hip) executes the LaunchPlan it is given, and the
// workspace-size entry points report WorkspaceLayout::bytes.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/sgmm.h"

// frontier_pad / frontier_len are shared with the kernels
#if defined(__HIPCC__)
#define SGMM_PLAN_HD __host__ __device__ __forceinline__
#else
#define SGMM_PLAN_HD inline
#endif

namespace sgmm {

constexpr int kWave = 64;
constexpr int kChunk = 64;          // ticks per chunk in the path scan
constexpr int kScanBlock = 256;
constexpr int kMaxLen = 1 << 17;    // max ticks per episode of the no-adversary table path (its scan's LDS chunk tables)
constexpr int kFrontierLanes = 64;     // chunks per wave (one per lane)
constexpr int kFrontierMaxWaves = 16;  // waves (64-chunk groups) per episode
constexpr int64_t kFrontierMaxLen = (int64_t)kFrontierLanes * 65532;  // ticks: chunks (multiples of 4) below 2^16 ticks, 16-bit trade counts
constexpr int kFusedMaxGroups = 2;  // fused path scan: at most two groups per episode
constexpr int kFusedHandoffBytes = 16;  // sizeof(FusedHandoff), sgmm_rollout.h
constexpr int kScanThreads = 1024;  // path-scan workgroup
constexpr int kScanAt1024 = 256;  // path-scan workgroup: 1024 threads up to this many episodes,
constexpr int kScanAt512 = 512;   // 256 up to this many, one wave above
constexpr int kScanArlAt1024 = 1024;  // adversary path scan: 1024 threads up to this many, kScanBlock above
constexpr int kLanesW = 4;          // episodes per lanes-scan workgroup (the plan picks 2 or 4 per launch)
constexpr int kReorderMaxPops = 64;

// ticks per chunk with nw waves (64 nw chunks) per episode
SGMM_PLAN_HD int frontier_len(int T, int nw) {
    const int c = (T + kFrontierLanes * nw - 1) / (kFrontierLanes * nw);
    return c < 4 ? 4 : (c + 3) & ~3;  // a multiple of 4: a scan thread's 4 ticks stay in one chunk
}
// the episode's block of plane rows: nw groups of frontier_len(T, nw) x 64 rows
// <= T + 256 nw rows (T rounded up to 64 nw chunks of a multiple of 4),
// starting on a 128-byte line (16 rows), so blocks at step_off + pad e
// (rounded up to 16, pad = 256 nw + 16) never overlap and no two episodes
// share a line; the plane stride covers total_steps + pad n (plane_stride).
// Group g's rows start at base + g * CL * 64 (frontier_row within the group)
SGMM_PLAN_HD int64_t frontier_pad(int nw) { return 256LL * nw + 16; }

// ------------------------------------------------------------------ inputs
// One value per SGMM_PLAN_* knob (sgmm_plan_set), -1 = the default rule.  A
// C-ABI entry snapshots them once (plan_knobs), so one launch sees one plan.
struct PlanKnobs {
    int32_t policy_path = -1;
    int32_t groups = -1;
    int32_t lane_split = -1;
    int32_t tail = -1;
    int32_t four = -1;
    int32_t min_eps = -1;
    int32_t table_sp = -1;
    int32_t scan_threads = -1;
    int32_t reorder_weights = -1;
    int32_t spill = -1;
    int32_t seq_sum = -1;
    int32_t fused_scan = -1;
    int32_t lanes_scan = -1;
};
static_assert(sizeof(PlanKnobs) == SGMM_PLAN_N * sizeof(int32_t), "one field per SGMM_PLAN_* knob");

struct LaunchShape {
    int32_t n = 0;            // episodes
    int32_t max_len = 0;      // ticks of the longest episode
    int64_t total_steps = 0;  // ticks of all episodes
    int32_t nsi = 0;          // inventory values
    int32_t hidden = 0;
    bool arl = false;         // with the adversary
    int32_t simds = 0;        // SIMDs of the device
    // the generation tail (StepArgs): present, its mode and episodes per population
    bool tail = false;
    int32_t mode = 0;
    int32_t pop_eps = 0;
    int32_t src_pop_eps = 0;  // GenomeSrc::pop_eps
    // the walk-order feedback is on: the launch walks the caller's writable
    // order (sgmm_populations::walk_order, not NULL)
    bool walk_feedback = false;
};

// ------------------------------------------------------------------ outputs
// Workspace layout (256-byte aligned sections), per batch of total_steps ticks:
//   no adversary: u64 cmaps[nc] | u64 ctr[nc] (nc = total_steps/64 + n + 1 chunk
//                 slots) | u32 kinfo[n * 64 G] | u32 wslots[n * 64] | u32 wspill[n * 64] |
//                 u32 arrive[n] | FusedHandoff handoff[n] | f64 path planes
//                 rew[n_states][rs] (rs = total_steps + frontier_pad(G) n,
//                 rounded up to 32; G = the frontier plan's gmax)
//   adversary:    u64 fills[total_steps] | f64 rew[n_states][rs] (rs =
//                 total_steps rounded up to 32)
//   (frontier kernel: cmaps / ctr hold u64 maps / u32[8] trade counts at the
//   records e * 64 G + c, kinfo the merge tick | p0 << 29 of each record; the
//   sections are sized for both the table and the frontier layout)
// Byte offsets from the workspace base; kNoSection: not part of this layout.
constexpr size_t kNoSection = ~size_t(0);
struct WorkspaceLayout {
    size_t cmaps = kNoSection, ctr = kNoSection, kinfo = kNoSection, wslots = kNoSection, wspill = kNoSection,
           arrive = kNoSection, handoff = kNoSection, fills = kNoSection, rew = kNoSection;
    int64_t rs = 0;    // plane stride, rew[state * rs + row]
    size_t bytes = 0;  // 0: invalid arguments
};

// The launch's chunk-group plan: g0 groups for the episodes at order positions
// [0, whole), gtail groups for the rest; gmax = the record / padding layout.
struct FrontierPlan {
    int32_t g0, gtail, whole, gmax;
    int64_t waves;  // walks (64-chunk groups)
    int32_t ls;     // waves per walk (lane split, k_policy_frontier<H, NSI, LS>)
};

enum class PolicyKernel { Frontier, TableSp, TableV3, TableMfma, TableValu };
enum class ScanKernel { Fused, Lanes, Wave, Arl };

struct LaunchPlan {
    PolicyKernel policy;
    FrontierPlan fr;       // meaningful for the frontier kernel; gmax also lays out the workspace
    uint32_t spill;        // FrontierArgs::spill_budget (10 ns units, 0: no spill)
    ScanKernel scan;
    int32_t scan_threads;  // the scan's workgroup (Fused: 0, the walks sum)
    int32_t scan_grid;     // its workgroups
    int32_t seq_sum;       // EpArrays::seq_sum
    int32_t lanes_w;       // Lanes: episodes per workgroup
    bool validation;       // a validation launch (tail modes 2 / 4; profiled separately)
    bool reorder;          // the walk-order feedback applies: a ReorderJob follows the scan
    uint32_t w_whole, w_split;  // its score weights
    WorkspaceLayout ws;
};

// ------------------------------------------------------------------ rules
// Chunk groups per episode in the frontier kernel (one wave each).  A walk's
// time is set by its serial chain of ticks, not by its SIMD's load, so when the
// launch has fewer than two walks per SIMD the episodes are cut into 2-4
// groups of 64 chunks of proportionally fewer ticks;
// each extra group pays for tracking every start state of its chunks until
// their paths merge.  SGMM_PLAN_GROUPS = 1..16 forces the count (records and
// plane padding are laid out for the launch's count, frontier_rec / frontier_pad).
constexpr int kFrontierAutoWaves = 8;  // the default rule's cap
inline FrontierPlan frontier_plan(int32_t n, int32_t simds, const PlanKnobs& k) {
    FrontierPlan p{1, 1, std::max(n, 0), 1, std::max<int64_t>(n, 0), 1};
    const int ls_force = k.lane_split;  // tests / experiments: waves per walk
    if (ls_force == 2 || ls_force == 4) p.ls = ls_force;
    {
        const int g = k.groups;
        if (g >= 1 && g <= kFrontierMaxWaves) {
            p.g0 = p.gtail = p.gmax = g;
            p.waves = (int64_t)n * g;
            return p;
        }
    }
    if (n <= 0) return p;
    // two walks per SIMD (measured, config 5's 1-of-8 shard, 1024 episodes of
    // 3600 ticks: 317 / 274 / 313 / 336 us at 1 / 2 / 3 / 4 groups, round 4;
    // 270 / 272 / 331 us at 2 / 4 / 8 groups, round 5; splitting lanes instead,
    // 283-311 us, profiles/r05_small)
    const int64_t S = simds;
    p.g0 = p.gtail = p.gmax = (int32_t)std::max<int64_t>(1, std::min<int64_t>(kFrontierAutoWaves, 2 * S / n));
    // from half as many episodes as SIMDs down, two waves per walk (lane split):
    // four waves per SIMD without more chunk starts (the 1-of-16 shard, 512
    // episodes: frontier + scan 248.5 us at G = 4 with two waves per walk against
    // 255.9 us at G = 8 and 270.6 us at G = 4 with one, profiles/r05_small/ls_*, c5s16_fr4)
    if (n <= S / 2 && ls_force < 0) p.ls = 2;
    // Whole walks are dispatched one per SIMD per run of S waves, so n = a S + r
    // leaves r SIMDs with a walk more than the others, and the walks on those
    // SIMDs end last.  The r episodes at the end of the order are cut into
    // ~S / r groups instead: the last run of waves becomes ~S shorter walks,
    // one per SIMD (1536 = 1024 + 512 -> 1024 whole walks and 512 episodes in 2
    // groups; config 3's 2560 = 2 x 1024 + 512 -> 2048 + 512 in 2 groups took
    // the policy kernel from 547 to 525 us, before the four-walk rule below).
    // SGMM_PLAN_TAIL = 0 keeps every walk whole.
    const bool tail = k.tail != 0;
    const int64_t r = n % S;
    const bool four = k.four != 0;  // SGMM_PLAN_FOUR = 0: no four-walk rule
    if (tail && four && p.g0 == 1 && 2 * n - 4 * S >= S / 2 && n < 4 * S) {
        // from 2.5 episodes per SIMD up to 4: four walks per SIMD, 2n - 4S whole
        // and the rest in halves, one whole and three half walks per SIMD (config
        // 3: 2560 = 1024 whole + 1536 in halves; 660.5-668.0 against 670.3-670.6 us
        // per generation for 2048 whole + 512 in halves, and 690-699 us for all in
        // halves, profiles/r05_ab/ab20_*, ab21_*; whole walks and quarters, 2048 +
        // 512 in four groups, took 683-688 against 649-654 us, profiles/r06_ab/NOTES.md)
        p.whole = (int32_t)(2 * n - 4 * S);
        p.gtail = p.gmax = 2;
    } else if (tail && p.g0 == 1 && n > S && r > 0) {
        const int64_t gt = std::max<int64_t>(1, std::min<int64_t>(kFrontierMaxWaves, (S + r / 2) / r));
        if (gt > 1) {
            p.whole = (int32_t)(n - r);
            p.gtail = p.gmax = (int32_t)gt;
        }
    }
    p.waves = (int64_t)p.whole * p.g0 + (int64_t)(n - p.whole) * p.gtail;
    return p;
}

// plane stride: every tick, plus (no adversary: the frontier kernel may run)
// the frontier layout's padding rows per episode, frontier_pad(G) with G the
// launch's chunk groups; the adversary planes are table rows only
inline int64_t plane_stride(int64_t steps, int32_t n, bool arl, int32_t gmax) {
    const int64_t pad = arl ? 0 : frontier_pad(gmax) * n;
    return (steps + pad + 31) & ~int64_t(31);
}

// The workspace of a batch with nsi inventory values, with or without the
// adversary (then 4 * nsi states: inventory x previous fill flags), laid out
// for gmax chunk groups.  The adversary flag is explicit: 4 * nsi <= 8 for one
// or two inventory values, so a state count alone cannot tell the layouts apart.
// The no-adversary layout serves the table and the frontier kernel alike,
// whichever the launch takes.
inline WorkspaceLayout workspace_layout(int32_t n, int64_t total_steps, int32_t nsi, bool arl, int32_t gmax) {
    WorkspaceLayout L;
    L.rs = plane_stride(total_steps, n, arl, gmax);
    if (total_steps < 0 || nsi <= 0 || nsi > 8 || n < 0) return L;
    size_t at = 0;
    const auto section = [&at](size_t bytes) {
        const size_t off = at;
        at += (bytes + 255) & ~size_t(255);
        return off;
    };
    const size_t steps = (size_t)total_steps, ne = (size_t)n;
    if (arl) {  // fill codes, per-state planes rew[state * rs + row]
        L.fills = section(steps * sizeof(uint64_t));
        L.rew = at;
        L.bytes = at + (size_t)L.rs * (size_t)(4 * nsi) * sizeof(double);
        return L;
    }
    const size_t slots = steps / kChunk + ne + 1;           // the table's chunk slots
    const size_t recs = ne * kFrontierLanes * (size_t)gmax;  // the frontier kernel's chunk records
    L.cmaps = section(std::max(slots, recs) * sizeof(uint64_t));
    L.ctr = section(std::max(slots * sizeof(uint64_t), recs * 8 * sizeof(uint32_t)));
    // u32 kinfo: per chunk record the merge tick | p0 << 29
    L.kinfo = section(recs * sizeof(uint32_t));
    // u32 wslots[n * 64]: the frontier launch's MLP slots per walk, [e * G + group] (G <= 16)
    L.wslots = section(ne * 64 * sizeof(uint32_t));
    // u32 wspill[n * 64]: per frontier wave (<= 16 groups x 4 waves per episode) the
    // tick offset at which it spilled, 0 if it did not
    L.wspill = section(ne * 64 * sizeof(uint32_t));
    // the fused scan's per-episode arrival words and chain hand-offs (FrontierArgs::hstate, handoff)
    L.arrive = section(ne * sizeof(uint32_t));
    L.handoff = section(ne * kFusedHandoffBytes);
    L.rew = at;
    L.bytes = at + (size_t)L.rs * (size_t)nsi * sizeof(double);
    return L;
}
// ... for the chunk groups the default rules and the knobs give n episodes
inline WorkspaceLayout workspace_layout(int32_t n, int64_t total_steps, int32_t nsi, bool arl, int32_t simds,
                                        const PlanKnobs& k) {
    return workspace_layout(n, total_steps, nsi, arl, frontier_plan(n, simds, k).gmax);
}

// Frontier kernel or table: the frontier kernel does ~1/3 of the table's
// matrix work but walks each episode serially (one wave per episode), so it
// needs many episodes to fill the chip; it is also the only path for episodes
// longer than kMaxLen.  SGMM_PLAN_POLICY_PATH forces either,
// SGMM_PLAN_MIN_EPS moves the threshold.  Measured crossover (one rank's
// shard of config 5, H = 32, 3600 ticks, per generation, profiles/r03_c5_shard*):
// 256 episodes table 235 / frontier 363 us, 512: 365 / 435, 1024: 633 / 525,
// 2048: 1078 / 572 -- the lines crossed near 700 episodes.  With 2-4 chunk
// groups per episode (round 4, training launch alone, profiles/r04_ab/r04m_*,
// r04n_*): 256 episodes table 167 / frontier 162 us, 512: 255-263 / 195-204.
constexpr int kFrontierMinEps = 512;
// The one-state-per-wave table for launches of at most kTableSpChunks chunks
// (SGMM_PLAN_TABLE_SP = 0 / 1 forces v3 / it, for A/B and the tests)
constexpr int64_t kTableSpChunks = 256;
// Policy kernel selection, SGMM_PLAN_POLICY_PATH: default = the frontier
// kernel for many episodes, else the f32-MFMA table; 1 / 2 force either; 3
// forces the VALU table (one lane per (tick, state)), an independent
// cross-check in the tests.  Of the MFMA tables, H = 16 / 32 without the
// adversary take k_policy_table_sp or k_policy_table_v3; H = 64 and the
// adversary path k_policy_table_mfma; H = 8 has the VALU table only.
inline PolicyKernel policy_kernel(const LaunchShape& sh, const PlanKnobs& k) {
    const bool h1632 = sh.hidden == 16 || sh.hidden == 32;
    const int path = k.policy_path;
    if (!sh.arl && h1632) {
        if (sh.max_len > kMaxLen || path == 1) return PolicyKernel::Frontier;
        if (path <= 0 && sh.n >= (k.min_eps > 0 ? k.min_eps : kFrontierMinEps)) return PolicyKernel::Frontier;
    }
    if (sh.hidden == 8 || path == 3) return PolicyKernel::TableValu;
    if (sh.arl || !h1632) return PolicyKernel::TableMfma;
    const int64_t nch = (sh.max_len + kChunk - 1) / kChunk;
    const bool sp = k.table_sp >= 0 ? k.table_sp != 0 : nch * sh.n <= kTableSpChunks;
    return sp ? PolicyKernel::TableSp : PolicyKernel::TableV3;
}

inline LaunchPlan resolve_plan(const LaunchShape& sh, const PlanKnobs& k) {
    LaunchPlan p{};
    p.policy = policy_kernel(sh, k);
    p.fr = frontier_plan(sh.n, sh.simds, k);
    p.ws = workspace_layout(sh.n, sh.total_steps, sh.nsi, sh.arl, p.fr.gmax);
    const bool fr = p.policy == PolicyKernel::Frontier;
    p.validation = sh.tail && (sh.mode == 2 || sh.mode == 4);
    const bool plain_tail = !sh.tail || sh.mode == 3;  // no tail, or the tell's argmax only

    // Spill deadline of a frontier launch (FrontierArgs::spill_budget, 10 ns units):
    // SGMM_PLAN_SPILL microseconds after a walk's start, 0 = no spill.  A walk
    // still running then stops once its chunks have <= kSpillTicks ticks left;
    // k_frontier_spill runs the rest tick-parallel.
    if (fr && k.spill > 0 && sh.max_len > 0) p.spill = (uint32_t)std::min<int64_t>((int64_t)k.spill * 100, 0x7FFFFFFF);

    // the launches the walk-order feedback applies to: a training launch (the tell's
    // argmax, mode 3) with a mixed whole / halves plan of one wave per walk, whole
    // populations of equal-length episodes, the caller's writable walk order
    // (sgmm_populations::walk_order; NULL, walk_feedback=False in the engine, keeps the
    // caller's order).  SGMM_PLAN_REORDER_WEIGHTS = whole << 8 | split sets the scores.
    const int P = sh.src_pop_eps;
    p.reorder = fr && sh.tail && sh.mode == 3 && sh.walk_feedback && P > 0 && sh.n % P == 0 && sh.n / P >= 2 &&
                sh.n / P <= kReorderMaxPops && p.fr.ls == 1 && p.fr.g0 == 1 && (p.fr.gtail == 2 || p.fr.gtail == 4) &&
                p.fr.whole > 0 && p.fr.whole < sh.n && sh.total_steps == (int64_t)sh.n * sh.max_len;
    p.w_whole = 5;
    p.w_split = 4;
    if (const int w = k.reorder_weights; w > 0 && (w >> 8) > 0 && (w & 255) > 0) {
        p.w_whole = (uint32_t)(w >> 8) & 63u;
        p.w_split = (uint32_t)w & 63u;
    }

    // The path scan fused into the frontier launch (k_policy_frontier<..., FS>): each
    // walk sums its own episode (the sequential chain) while the launch's longer walks
    // still run, and the last record of a population runs the tell -- no separate
    // scan launch.  Where it applies: one wave per walk, <= kFusedMaxGroups groups, no
    // spill, no tail or the tell's argmax (mode 3), not where the parallel sum is forced.
    // The default takes it for launches of whole walks only (round 6, profiles/r06_fused/,
    // per generation: config 5 1.344-1.360 -> 1.327-1.332 ms, its 1-of-2 shard
    // 0.789-0.794 -> 0.759-0.761, 1-of-4 0.489-0.490 -> 0.469-0.471); with halves the
    // chain hand-offs and the in-kernel sums on SIMDs shared with walks cost more than
    // the separate scan (config 3 0.639-0.641 -> 0.646-0.650, the 1-of-8 shard 0.333 ->
    // 0.372 ms).  SGMM_PLAN_FUSED_SCAN forces it off (0) or on where it applies (1).
    if (fr && sh.max_len > 0 && k.fused_scan != 0 && !p.validation && !p.spill && p.fr.ls == 1 &&
        p.fr.gmax <= kFusedMaxGroups && k.seq_sum != 0 && plain_tail && (k.fused_scan == 1 || p.fr.gmax == 1)) {
        p.scan = ScanKernel::Fused;
        return p;
    }

    // Episode sums of a path scan: the plain sequential chain or the exact parallel
    // binade method (exact_sum_window); both give the reference's bits.  Measured per
    // shape, 20 generations each (profiles/r06_seq/): the sequential chain wins in the
    // one-wave and 4-wave scans of many GA-trained episodes -- config 3 89.0 -> 75.7 us,
    // config 5's 8 192 / 4 096 / 2 048 / 1 024 / 512 episodes 187.9 / 112.8 / 68.0 /
    // 55.9 / 50.7 -> 177.4 / 102.4 / 61.8 / 40.1 / 32.9 us -- and in the validation
    // scans (11.5-12.7 -> 10.3-11.4 us); the parallel method wins where one 16-wave
    // workgroup sums each long episode (config 2 15.7 vs 26.8 us, config 6 18.5 vs
    // 27.0) and in the adversary scan (config 4 39.9 vs 44.9, its 1-of-4 shard 32.5 vs
    // 41.9).  SGMM_PLAN_SEQ_SUM forces either.
    const auto seq_sum = [&](int nt) {
        if (k.seq_sum >= 0) return k.seq_sum != 0;
        return p.validation || (!sh.arl && nt <= 256);
    };
    p.scan_grid = sh.n;
    if (sh.arl) {
        // 16-wave workgroups while one per CU fits (a 4096-tick segment is one
        // exact-sum window), 4-wave ones beyond
        p.scan = ScanKernel::Arl;
        p.scan_threads = sh.n <= kScanArlAt1024 ? kScanThreads : kScanBlock;
        p.seq_sum = seq_sum(p.scan_threads);
        return p;
    }
    // path-scan workgroup size for n episodes (256 CUs): one 16-wave workgroup per
    // CU while they fit, then 8-wave, then 4-wave workgroups --
    // the workgroup shrinks as episodes grow: few episodes get a 16-wave
    // workgroup each (4096-tick windows, the phases spread over the CU);
    // many get 8- or 4-wave ones (2048- / 1024-tick windows), several
    // resident per CU, so the serial walks of different episodes overlap
    // instead of idling the CU (A/B on MI355X: P=64 / 256 / 1024 / 4096).
    // Beyond 512 episodes one-wave workgroups: the exact-sum walk is serial,
    // so many episodes resident per CU beat fewer wider workgroups (config 3:
    // 193 -> 145 us per scan, tools/gpu_sc1.sh; config 5's 1-of-8 shard, 1024
    // episodes: 110 -> 74 us, profiles/r04_ab/r04k_*; round 6: 54.7 against 69.3 /
    // 94.6 us for 256 / 512 threads, profiles/r06_scanw/).  From 257 to 512
    // episodes 4-wave workgroups (1024-tick windows): config 5's 1-of-16 shard
    // (512 episodes) 49.8 against 61.7 us with 512 threads, 52.4 with one wave
    const int t = k.scan_threads;
    const int nt = (t == 64 || t == 256 || t == 512 || t == 1024)
                       ? t
                       : (sh.n <= kScanAt1024 ? kScanThreads : (sh.n <= kScanAt512 ? 256 : kWave));
    p.scan = ScanKernel::Wave;
    p.scan_threads = nt;
    p.seq_sum = seq_sum(nt);

    // The frontier path scan with kLanesW episodes per workgroup and their chains in
    // the lanes of one wave (k_path_scan_lanes): where the one-wave scan would run the
    // sequential chain, with no tail or the tell's argmax (mode 3) and populations of
    // whole workgroups (config 3: scan 72 -> 55.5 us, 0.627-0.639 -> 0.605-0.612 ms
    // per generation; config 5's 1-of-8 shard 37.5 -> 31.1 us).  SGMM_PLAN_LANES_SCAN forces it off (0) or on where it applies (1).
    const int lv = k.lanes_scan;
    if (fr && lv != 0 && p.seq_sum && plain_tail && !(sh.tail && sh.pop_eps > 0 && sh.pop_eps % 4 != 0) &&
        (lv > 0 || nt == kWave)) {
        // episodes per lanes-scan workgroup: 2 from 2 048 episodes, 4 below (config 3 / 2 560
        // episodes: scan 53.5 against 55.5 us; config 5's 1-of-8 shard / 1 024: 31.1 against
        // 33.5 us with 2, profiles/r06_lanes/); SGMM_PLAN_LANES_SCAN = 2 or 4 forces it
        p.scan = ScanKernel::Lanes;
        p.lanes_w = (lv == 2 || lv == 4) ? lv : (sh.n >= 2048 ? 2 : kLanesW);
        p.scan_threads = kWave * p.lanes_w;
        p.scan_grid = (sh.n + p.lanes_w - 1) / p.lanes_w;
    }

    return p;
}

}  // namespace sgmm
