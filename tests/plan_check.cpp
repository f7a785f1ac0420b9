// plan_check.cpp -- host-only driver of csrc/sgmm_plan.h for tests/test_plan.py.
//
// Reads one launch per line from stdin as key=value tokens (shape fields, then
// any SGMM_PLAN_* knob by its binding name), resolves its plan, checks the
// workspace layout against section sizes written out here by hand, and prints
// the plan as one line of key=value tokens.  Exit status 1 on a layout
// violation or an unknown key.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sgmm_plan.h"

using namespace sgmm;

static const char* name_of(PolicyKernel k) {
    switch (k) {
        case PolicyKernel::Frontier: return "Frontier";
        case PolicyKernel::TableSp: return "TableSp";
        case PolicyKernel::TableV3: return "TableV3";
        case PolicyKernel::TableMfma: return "TableMfma";
        case PolicyKernel::TableValu: return "TableValu";
    }
    return "?";
}
static const char* name_of(ScanKernel k) {
    switch (k) {
        case ScanKernel::Fused: return "Fused";
        case ScanKernel::Lanes: return "Lanes";
        case ScanKernel::Wave: return "Wave";
        case ScanKernel::Arl: return "Arl";
    }
    return "?";
}

static bool set_field(LaunchShape& sh, PlanKnobs& k, const std::string& key, long long v) {
    if (key == "n") sh.n = (int32_t)v;
    else if (key == "len") sh.max_len = (int32_t)v;
    else if (key == "steps") sh.total_steps = v;
    else if (key == "nsi") sh.nsi = (int32_t)v;
    else if (key == "H") sh.hidden = (int32_t)v;
    else if (key == "arl") sh.arl = v != 0;
    else if (key == "simds") sh.simds = (int32_t)v;
    else if (key == "tail") sh.tail = v != 0;
    else if (key == "mode") sh.mode = (int32_t)v;
    else if (key == "pop_eps") sh.pop_eps = (int32_t)v;
    else if (key == "src_pop_eps") sh.src_pop_eps = (int32_t)v;
    else if (key == "feedback") sh.walk_feedback = v != 0;
    else if (key == "policy_path") k.policy_path = (int32_t)v;
    else if (key == "groups") k.groups = (int32_t)v;
    else if (key == "lane_split") k.lane_split = (int32_t)v;
    else if (key == "tail_split") k.tail = (int32_t)v;  // SGMM_PLAN_TAIL ("tail" is the shape's generation tail)
    else if (key == "four") k.four = (int32_t)v;
    else if (key == "min_eps") k.min_eps = (int32_t)v;
    else if (key == "table_sp") k.table_sp = (int32_t)v;
    else if (key == "scan_threads") k.scan_threads = (int32_t)v;
    else if (key == "reorder_weights") k.reorder_weights = (int32_t)v;
    else if (key == "spill") k.spill = (int32_t)v;
    else if (key == "seq_sum") k.seq_sum = (int32_t)v;
    else if (key == "fused_scan") k.fused_scan = (int32_t)v;
    else if (key == "lanes_scan") k.lanes_scan = (int32_t)v;
    else return false;
    return true;
}

// Sections start at 0, each on a 256-byte boundary right after the one before
// (whose size is restated here, not taken from the header), and `bytes` is the
// end of the planes.
static bool check_layout(const LaunchShape& sh, const LaunchPlan& p) {
    const WorkspaceLayout& L = p.ws;
    const size_t n = (size_t)sh.n, steps = (size_t)sh.total_steps, G = (size_t)p.fr.gmax;
    struct Sec {
        const char* name;
        size_t off, size;
    };
    std::vector<Sec> secs;
    if (sh.arl) {
        secs = {{"fills", L.fills, steps * 8}, {"rew", L.rew, (size_t)L.rs * 4 * sh.nsi * 8}};
        if (L.cmaps != kNoSection || L.ctr != kNoSection || L.kinfo != kNoSection || L.wslots != kNoSection ||
            L.wspill != kNoSection || L.arrive != kNoSection || L.handoff != kNoSection)
            return std::fprintf(stderr, "adversary layout has a no-adversary section\n"), false;
        if (L.rs != (int64_t)((steps + 31) / 32 * 32)) return std::fprintf(stderr, "adversary rs\n"), false;
    } else {
        const size_t slots = steps / 64 + n + 1, recs = n * 64 * G;
        secs = {{"cmaps", L.cmaps, std::max(slots, recs) * 8},
                {"ctr", L.ctr, std::max(slots * 8, recs * 32)},
                {"kinfo", L.kinfo, recs * 4},
                {"wslots", L.wslots, n * 64 * 4},
                {"wspill", L.wspill, n * 64 * 4},
                {"arrive", L.arrive, n * 4},
                {"handoff", L.handoff, n * 16},
                {"rew", L.rew, (size_t)L.rs * sh.nsi * 8}};
        if (L.fills != kNoSection) return std::fprintf(stderr, "no-adversary layout has fills\n"), false;
        if (L.rs != (int64_t)((steps + (256 * G + 16) * n + 31) / 32 * 32)) return std::fprintf(stderr, "rs\n"), false;
    }
    size_t at = 0;
    for (const Sec& s : secs) {
        if (s.off == kNoSection || s.off % 256 != 0 || s.off != at)
            return std::fprintf(stderr, "section %s at %zu, expected %zu\n", s.name, s.off, at), false;
        at = s.off + s.size;
        if (&s != &secs.back()) at = (at + 255) / 256 * 256;
    }
    if (L.bytes != at) return std::fprintf(stderr, "bytes %zu != end of planes %zu\n", L.bytes, at), false;
    return true;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string tok;
        LaunchShape sh;
        PlanKnobs knobs;
        bool any = false;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos || !set_field(sh, knobs, tok.substr(0, eq), std::atoll(tok.c_str() + eq + 1))) {
                std::fprintf(stderr, "bad token %s\n", tok.c_str());
                return 1;
            }
            any = true;
        }
        if (!any) continue;
        const LaunchPlan p = resolve_plan(sh, knobs);
        if (!check_layout(sh, p)) {
            std::fprintf(stderr, "in: %s\n", line.c_str());
            return 1;
        }
        std::printf("policy=%s g0=%d gtail=%d whole=%d gmax=%d waves=%lld ls=%d spill=%u scan=%s threads=%d grid=%d "
                    "seq_sum=%d lanes_w=%d validation=%d reorder=%d w_whole=%u w_split=%u rs=%lld bytes=%zu\n",
                    name_of(p.policy), p.fr.g0, p.fr.gtail, p.fr.whole, p.fr.gmax, (long long)p.fr.waves, p.fr.ls,
                    p.spill, name_of(p.scan), p.scan_threads, p.scan_grid, p.seq_sum, p.lanes_w, (int)p.validation,
                    (int)p.reorder, p.w_whole, p.w_split, (long long)p.ws.rs, p.ws.bytes);
    }
    return 0;
}
