// ntt_plan.h — the pass plan of a 2^log_n transform (ntt.hip ntt_run): tile, pass count and radices.  Host only, no HIP
// types: tests/ntt_plan_check.cpp walks every (log_n, ZK_OPT_NTT_MAX_RADIX_LOG2) pair through it without a GPU.
#pragma once
#include <stdint.h>

namespace zk {

static constexpr uint32_t NTT_MAX_LOG_N = 26;       // the largest transform the entry points accept
static constexpr uint32_t NTT_MAX_PASSES = 26;      // radix-2 passes of that transform (option value 1): the worst case
static constexpr uint32_t NTT_TILE_LOG_DEFAULT = 9;
static constexpr uint32_t NTT_TILE_LOG_MAX = 11;
static constexpr uint32_t NTT_MAX_RADIX_LOG2 = 11;  // the largest value ZK_OPT_NTT_MAX_RADIX_LOG2 takes

struct NttPlan {
    uint32_t tile_log;              // a workgroup holds 2^tile_log elements in LDS
    uint32_t passes;                // 0: N == 1, nothing to launch
    uint32_t bits[NTT_MAX_PASSES];  // log2 of each pass's radix, first pass first
};

// Radices as even as possible, each <= max_log_r (>= 1), the larger ones first.  Returns the pass count, or -1 when it
// exceeds `cap` entries (nothing is written past bits[cap - 1]).
inline int ntt_plan(uint32_t log_n, uint32_t max_log_r, uint32_t* bits, uint32_t cap = NTT_MAX_PASSES) {
    if (log_n == 0) return 0;
    if (max_log_r == 0) return -1;
    const uint32_t np = (log_n + max_log_r - 1) / max_log_r;
    if (np > cap) return -1;
    uint32_t rem = log_n;
    for (uint32_t p = 0; p < np; p++) {
        bits[p] = (rem + (np - p) - 1) / (np - p);
        rem -= bits[p];
    }
    return (int)np;
}

// The plan: largest radix and tile by transform size.  Measured (tools/ntt_sweep.py, one vector, ms; 3 passes of 2^7 on the 2^9
// tile -> the plan below): 2^15 0.044 -> 0.032, 2^16 0.047 -> 0.034 (two passes of 2^8, tile 2^9); 2^17 0.052 -> 0.043, 2^18 0.076 ->
// 0.051 (two passes of 2^9, tile 2^10); 2^19 0.103 -> 0.079, 2^20 0.174 -> 0.158 (two passes of 2^10, tile 2^11); 2^21 and up stay at
// passes of at most 2^7 (two passes of 2^11 / 2^10 on the 2^11 tile: 0.37 against 0.30 ms — one 32-byte column per tile row).
// An explicit radix (`opt_max_log_r`, ZK_OPT_NTT_MAX_RADIX_LOG2 = 1..11) takes the smallest tile that holds it and is honoured
// for every log_n: up to NTT_MAX_PASSES passes.  `build_tile_log` is the build's ZK_NTT_TILE_LOG: a build that pins another tile
// than the default keeps that tile and the old default radix 2^7 for every size, and clamps an explicit radix to the tile.
// Returns false (nothing to run) for log_n > NTT_MAX_LOG_N or an option value out of range.
inline bool ntt_make_plan(uint32_t log_n, uint32_t opt_max_log_r, NttPlan* out, uint32_t build_tile_log = NTT_TILE_LOG_DEFAULT) {
    if (log_n > NTT_MAX_LOG_N || opt_max_log_r > NTT_MAX_RADIX_LOG2) return false;
    uint32_t tl = build_tile_log, max_r = 7;
    if (opt_max_log_r) {
        max_r = opt_max_log_r;
        if (build_tile_log == NTT_TILE_LOG_DEFAULT) tl = max_r < 9 ? 9 : max_r > NTT_TILE_LOG_MAX ? NTT_TILE_LOG_MAX : max_r;
    } else if (build_tile_log == NTT_TILE_LOG_DEFAULT) {
        if (log_n <= 16) {
            max_r = 8;
        } else if (log_n <= 18) {
            max_r = 9;
            tl = 10;
        } else if (log_n <= 20) {
            max_r = 10;
            tl = 11;
        }
    }
    if (max_r > tl) max_r = tl;
    const int np = ntt_plan(log_n, max_r, out->bits);
    if (np < 0) return false;
    out->tile_log = tl;
    out->passes = (uint32_t)np;
    return true;
}

}  // namespace zk
