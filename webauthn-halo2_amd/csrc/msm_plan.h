// msm_plan.h — the plan rules of the MSM (msm.hip, msm_standard.hip.h, msm_lanes.hip): which window a size takes, which path
// serves it (wide / fused / swept), which sort and scatter the fused plan runs, how its bit sums are split, how many columns one
// pass may hold — and the workspace of a plan: its buffers with their sizes, and how far the launchers of msm.hip reach into them.
// Host only, no HIP types: tests/msm_plan_check.cpp walks every (mode, log n, ZK_OPT_MSM_WINDOW, pass width) through it without
// a GPU, and tests/msm_cases.py restates the rules in Python.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <initializer_list>

namespace zk {

static constexpr uint32_t MSM_MAX_BATCH = 256;       // columns per fixed-base pass at most (MsmBatch, the lanes' result arrays)
static constexpr uint32_t SORT_LDS_BUCKETS = 8192;   // 32 KiB of LDS counters per sort workgroup
static constexpr uint32_t CBINS_MAX = 256;           // coarse bins: buckets / 64 (64 at 13-bit windows, 128 at 14); buckets / 128 on the wide path (256 at 16)
static constexpr uint32_t BITSUM_MAX_SPLIT = 4;      // partial sums per bit of a bucket set at most (msm_bitsum_kernel)
static constexpr uint32_t MSM_WS_MIN_N = 1024;       // the MSM workspaces are at least this many scalars long (get_msm_ws)

inline uint32_t nwin_for(uint32_t c) { return 254 / c + 1; }
// smallest log2(n) that takes 17-bit windows by default.  99 = never: measured end to end (round 4, tools/bench_ab.sh, same box,
// new head in both): 17 bits make the accumulation 6 % shorter (0.627 against 0.666 ms per launch: 15 additions per scalar
// instead of 16) and the proof NOT faster — 94.2 / 94.7 proofs/s against 95.7 / 95.5 at 16 bits, single proof 12.3 against 12.0 ms:
// twice the buckets (65 536) double the row / column sums and the parts of the reduction tail, which run at one or two waves per
// SIMD.  The 17-bit plan stays selectable (ZK_OPT_MSM_WINDOW = 17) and tested.
#ifndef ZK_W17_MIN_LG
#define ZK_W17_MIN_LG 99
#endif
// the wide path (msm_wide.hip.h): 15 / 16 / 17-bit windows over a resident basis.  An entry holds the table index in ib = 24 .. 26
// bits and a fine key of fb = 31 - ib bits (at most 7); the buckets / 2^fb coarse bins must not exceed 512
inline bool msm_wide_shape(uint32_t c, size_t table_stride, uint32_t* ib_out, uint32_t* fb_out) {
    if (c < 15 || c > 17 || table_stride == 0) return false;
    const uint64_t idx = (uint64_t)nwin_for(c) * table_stride;
    uint32_t ib = 24;
    while (((uint64_t)1 << ib) < idx) ib++;
    if (ib > 26) return false;
    const uint32_t fb = 31 - ib > 7 ? 7 : 31 - ib;
    if (((1u << (c - 1)) >> fb) > 512) return false;
    if (ib_out) *ib_out = ib;
    if (fb_out) *fb_out = fb;
    return true;
}
inline bool msm_wide_applies(uint32_t c, size_t table_stride) { return msm_wide_shape(c, table_stride, nullptr, nullptr); }

// fixed-base mode (the resident SRS's window tables); `override_c` is ZK_OPT_MSM_WINDOW
inline uint32_t msm_auto_window(size_t n, uint32_t override_c = 0) {
    uint32_t lg = 0;
    while (((size_t)1 << (lg + 1)) <= n) lg++;
    // measured on MI355X with whole proofs (tools/single_ab.py, tools/window_exp.py, tools/bench_rows.py): the wide path's 16-bit
    // windows at 2^16 .. 2^20 (16 bucket additions per scalar instead of 20 / 22: k = 19 single proof 13.7 -> 12.3 ms, k = 18
    // 10.3 -> 9.2, k = 17 7.5 -> 6.95 ms and 160 -> 169 proofs/s, k = 16 7.4 -> 7.0); below, lg - 5 bits on the 13-bit plan (k = 15:
    // 7.0 ms against 7.6 / 7.9 with 15 / 16 bits); 2^21 and up (window table indexes beyond 24 bits) 15 bits on the swept sort
    // round 4: 16 bits also at 2^21 (table indexes of 25 bits; was: 15 bits on the swept sort); 17 bits only on request (below)
    int c = lg >= 22 ? 15 : (lg == 21 ? 16 : (lg >= ZK_W17_MIN_LG ? 17 : (lg >= 16 ? 16 : (int)lg - 5)));
    if (override_c) c = (int)override_c;  // zk_ctx_set_option(ZK_OPT_MSM_WINDOW)
    if (c < 9) c = 9;
    if (c > 17) c = 17;
    while (c > 15 && !msm_wide_applies(c, n)) c--;  // 16 / 17-bit digits exist on the wide path only
    // the MSM workspaces are at least 1024 scalars long (get_msm_ws), the wide path needs table stride == workspace length:
    // below that a 15 / 16-bit override would build internal-form tables that msm_run reads on the standard path
    if (c >= 15 && n < MSM_WS_MIN_N) c = 14;
    return (uint32_t)c;
}

// arbitrary bases (generic mode: a bucket set per window, host Horner over the windows): the round-2 rule — lg - 6 from 2^19
// (13 bits at 2^19), 12 at 2^16 .. 2^18, lg - 5 below, at most 14 (15 from 2^21)
inline uint32_t msm_auto_window_generic(size_t n) {
    uint32_t lg = 0;
    while (((size_t)1 << (lg + 1)) <= n) lg++;
    int c = lg >= 19 ? (int)lg - 6 : (lg >= 16 ? 12 : (int)lg - 5);
    if (c > 14) c = lg >= 21 ? 15 : 14;
    if (c < 9) c = 9;
    return (uint32_t)c;
}

// length of the workspace that serves n scalars (get_msm_ws): the power of two at or above n, at least MSM_WS_MIN_N
inline size_t msm_ws_len(size_t n) {
    size_t want = 1;
    while (want < n) want <<= 1;
    return want < MSM_WS_MIN_N ? MSM_WS_MIN_N : want;
}

// the fused fixed-base plan of msm_run: digits + histogram in one kernel, every column its own bucket set; bucket sets beyond
// the LDS budget (15-bit windows off the wide path) take the swept sort, one column per pass
inline bool msm_fused(bool fixed, uint32_t nb) { return fixed && nb <= SORT_LDS_BUCKETS; }

// ---- two-level counting sort (msm_standard.hip.h, ZK_SORT2)
#ifndef ZK_SORT2
#define ZK_SORT2 1
#endif
#ifndef ZK_SORT2_MIN_N
#define ZK_SORT2_MIN_N (1u << 18)
#endif
// The two extra launches and the 4096-entry sub-rounds only pay for long columns: single proofs of the k <= 16 rows of
// bench_ecdsa.config are 2-6 % slower with it, k = 17 1-2 %, k >= 18 equal, and batches of k = 19 proofs 4 % faster.
inline bool sort2_applies(bool fused, size_t n, uint32_t nb, uint32_t nwin, size_t table_stride) {
    return ZK_SORT2 && fused && n >= ZK_SORT2_MIN_N && nb >= 64 && (nb >> 6) <= CBINS_MAX &&
           (uint64_t)nwin * table_stride <= (1u << 24);
}

// columns per launch of the one-pass scatter (msm_scatter_fixed_kernel).  Long columns: one launch per column — a column's
// 4-byte stores land in its own ~40 MB of the entry list and combine in the cache; all columns at once thrash it (0.8 ms instead
// of 4 x 0.1 ms at four columns of 2^19).  Short columns: one launch for all (launch-bound otherwise).
inline uint32_t msm_scatter_per_launch(uint32_t n, uint32_t batch) { return n >= (1u << 18) ? 1 : batch; }

// ---- bit sums (msm_bitsum_kernel).  One wave per workgroup.  Measured on the 4 x 2048 multipliers of a 13-bit window
// (tools/ubench_bitsum.hip): workgroups of 512 lanes (one multiplier per lane, a cross-wave step through LDS) 205 us, 256 lanes
// 140, 128 lanes 113, 64 lanes 107 — the hardware packs the waves of a workgroup two or three to a SIMD even on an idle chip,
// each tree step then costs two or three additions, and the others wait at the barrier; a lone wave per workgroup gets a SIMD
// to itself.
inline uint32_t bitsum_threads(uint32_t nb) {
    (void)nb;
    return 64;
}
inline uint32_t bitsum_split(uint32_t nb) {
    uint32_t s = (nb >> 1) / 512;
    if (s < 1) s = 1;
    if (s > BITSUM_MAX_SPLIT) s = BITSUM_MAX_SPLIT;
    return s;
}

// ---- columns per fixed-base pass.  Batching makes the accumulate launch bigger (fuller waves: -15 % per column already at two
// columns of 2^19) and replaces several reduction tails by one longer one; measured best (whole proofs): 2 at 2^19, growing as
// the columns get shorter and launch overheads dominate.  `opt` is ZK_OPT_MSM_BATCH (0 = this rule).
inline uint32_t msm_batch_width(size_t n, uint32_t opt) {
    size_t b = ((size_t)1 << 20) / (n ? n : 1);
    if (opt) b = opt;
    if (b < 1) b = 1;
    if (b > MSM_MAX_BATCH) b = MSM_MAX_BATCH;
    return (uint32_t)b;
}

// The widest pass the fixed-base plan of `c`-bit windows over a resident basis of `table_stride` points takes when `want`
// columns are asked for: msm_run batches columns on the wide path and on the fused plan only — the swept sort (15 bits where
// the wide path does not apply: every SRS from 2^22) runs one column per pass and refuses more.
inline uint32_t msm_max_pass(uint32_t c, size_t table_stride, uint32_t want) {
    if (want < 1) want = 1;
    if (want > MSM_MAX_BATCH) want = MSM_MAX_BATCH;
    const bool wide = msm_wide_applies(c, table_stride) && table_stride == msm_ws_len(table_stride);
    return wide || msm_fused(true, 1u << (c - 1)) ? want : 1;
}

// ---- the geometry the kernels and the workspace share (#ifndef: build-time tuning knobs, tools/ab_variants.sh)
#ifndef ZK_SEG0
#define ZK_SEG0 16
#endif
#ifndef ZK_GA
#define ZK_GA 4
#endif
#ifndef ZK_FCHUNK
#define ZK_FCHUNK 1024
#endif
#ifndef ZK_SORT_SUB
#define ZK_SORT_SUB 4096
#endif
#ifndef ZK_WL
#define ZK_WL 16
#endif
#ifndef ZK_WCUR_STRIDE
#define ZK_WCUR_STRIDE 32
#endif
static constexpr uint32_t CHUNK = 16384;              // scalars per histogram / scatter workgroup of the swept sort
static constexpr uint32_t FCHUNK = ZK_FCHUNK;         // scalars per workgroup (x nwin entries) of the fused heads
static constexpr uint32_t SEG0 = ZK_SEG0;             // entries per accumulate lane
static constexpr uint32_t GA = ZK_GA;                 // slots per first-level gather lane
static constexpr uint32_t PAD = SEG0 * GA;            // bucket ranges are padded to multiples of PAD entries
static constexpr uint32_t SUB = ZK_SORT_SUB;          // entries sorted in LDS at a time
static constexpr uint32_t COARSE_WORDS = 5 * (CBINS_MAX + 1);  // two-level sort: words of a column's header in `coarse`; [blocks][CBINS_MAX] follow
static constexpr uint32_t WL = ZK_WL;                 // wide path: entries per accumulation lane (measured: msm_wide.hip.h)
static constexpr uint32_t WCB = 512;                  // ... coarse bins at most (65 536 buckets / 128, or 32 768 / 64)
static constexpr uint32_t WCUR = ZK_WCUR_STRIDE;      // ... words between two append cursors (one per 128-byte line: msm_wide.hip.h)
static constexpr uint32_t WCUR0 = 5 * (WCB + 1);      // ... first cursor
static constexpr uint32_t WHDR = WCUR0 + WCB * WCUR;  // ... words of a column's header; the workgroups' reserved bases [blocks][WCB] follow
static constexpr uint32_t WCAP_MIN = 2;               // ... slots per part at least: sizes the part lists
static constexpr uint32_t MSM_PARTS_FIXED = 8, MSM_PARTS_GENERIC = 1;  // parts per bucket of the second-level gather

// ---- what the launchers of msm.hip index at most in one pass.  Standard plan, `batch` columns of n scalars (arbitrary bases: 1):
struct MsmStdPass {
    uint32_t slices, nbt, parts, ngroups;  // bucket sets (one per column; per window for arbitrary bases), buckets, parts per bucket, gather groups
    size_t worst, threads, lanes1;         // padded entries, accumulation segments, first-level gather lanes
};
inline MsmStdPass msm_std_pass(bool fixed, uint32_t c, size_t n, uint32_t batch) {
    MsmStdPass p;
    p.slices = fixed ? batch : nwin_for(c);
    p.nbt = p.slices << (c - 1);
    p.parts = fixed ? MSM_PARTS_FIXED : MSM_PARTS_GENERIC;
    p.ngroups = p.nbt * p.parts;
    p.worst = (size_t)batch * n * nwin_for(c) + (size_t)p.nbt * (PAD - 1);
    p.threads = (p.worst + SEG0 - 1) / SEG0;
    p.lanes1 = (p.worst + PAD - 1) / PAD;
    return p;
}
// Wide path: every column owns a region of the entry / lane / slot / part lists, strides fixed by (c, max_n) ...
struct MsmWideDims {
    uint32_t bins, rows;     // coarse bins; the bucket matrix is [rows = nb / 256][256]
    size_t ent_stride;       // entries per column region (multiple of 64)
    uint32_t lane_stride, slot_stride, part_stride;  // accumulation lanes, slots (lanes + buckets), parts per column region
};
inline MsmWideDims msm_wide_dims(uint32_t c, size_t max_n) {
    MsmWideDims d = {};
    uint32_t ib = 0, fb = 0;
    if (!msm_wide_shape(c, max_n, &ib, &fb)) return d;
    const uint32_t nb = 1u << (c - 1);
    d.bins = nb >> fb;
    d.rows = nb >> 8;
    d.ent_stride = (max_n * nwin_for(c) + 63) & ~(size_t)63;
    d.lane_stride = (uint32_t)(d.ent_stride / WL) + 64;
    d.slot_stride = d.lane_stride + nb + 64;
    d.part_stride = ((d.lane_stride + 2 * nb) / WCAP_MIN + nb + 2 * d.bins + 127) & ~63u;
    return d;
}
// ... and per pass of n scalars: accumulation lanes of one column at most; chunks of its binned list (msm_wfinehist /
// msm_wscatter2: one workgroup each); parts: every bin's region is its slots / WCAP + a part per bucket + slack (msm_wscatter1_kernel)
inline uint32_t wide_lanes(uint32_t nwin, size_t n) { return (uint32_t)((n * nwin + WL - 1) / WL); }
inline uint32_t wide_max_chunks(uint32_t nwin, uint32_t bins, size_t n) { return (uint32_t)(((uint64_t)n * nwin + SUB - 1) / SUB) + bins; }
inline uint32_t wide_max_parts(uint32_t nwin, uint32_t nb, uint32_t bins, size_t n, uint32_t WCAP) {
    return (wide_lanes(nwin, n) + 2 * nb) / WCAP + nb + 2 * bins + 64;
}

// ---- the workspace of a plan (msm_workspace_create): fixed when it is made.  A fixed-base workspace over a resident table of
// max_n points runs wide where msm_wide_shape holds; arbitrary bases never do.
enum MsmPlan : uint32_t { MSM_PLAN_WIDE, MSM_PLAN_FIXED, MSM_PLAN_GENERIC };
inline MsmPlan msm_ws_plan(bool fixed, uint32_t c, size_t max_n) {
    return !fixed ? MSM_PLAN_GENERIC : msm_wide_applies(c, max_n) ? MSM_PLAN_WIDE : MSM_PLAN_FIXED;
}
enum MsmBuf : uint32_t {
    WS_COUNTS, WS_ENTRIES, WS_REDO, WS_SLOT_PT, WS_INTER, WS_COARSE,  // every plan (the last two: no arbitrary bases)
    WS_TOTALS, WS_CURSOR, WS_DIGITS, WS_BUCKET_START, WS_BLOCKBASE, WS_PARTIAL, WS_PART, WS_BIT_SUM,  // the standard plan's
    WS_W_TOT0, WS_W_TOT1, WS_W_CUR0, WS_W_CUR1, WS_W_LANE_B, WS_W_BSTART, WS_W_PSTART, WS_W_PBUCKET, WS_W_PART, WS_W_RC,  // the wide path's
    WS_NBUF
};
struct MsmWsLayout {
    struct { size_t count, elem; } buf[WS_NBUF];  // elements and bytes per element; 0: the plan has no such buffer
    uint32_t coarse_stride;                       // words per column in WS_COARSE: the wide header covers the two-level sort's (256 bins)
};
// pt29 / ptx: sizeof(G1X29S) / sizeof(G1X).  Bucket sets are max_batch (fixed base) or nwin (arbitrary bases).  The wide path's
// entries, redo list and slots are its own column regions, not the standard plan's padded list.
inline MsmWsLayout msm_ws_layout(MsmPlan plan, uint32_t c, size_t max_n, uint32_t max_batch, size_t pt29, size_t ptx) {
    MsmWsLayout L = {};
    const auto set = [&L](MsmBuf id, size_t count, size_t elem) { L.buf[id].count = count, L.buf[id].elem = elem; };
    const size_t cols = max_batch, nwin = nwin_for(c), nb = (size_t)1 << (c - 1), nblk = (max_n + FCHUNK - 1) / FCHUNK;
    L.coarse_stride = (uint32_t)(WHDR + nblk * WCB);
    set(WS_COUNTS, 4 * (MSM_MAX_BATCH + 1), 4);
    if (plan != MSM_PLAN_GENERIC) {
        set(WS_INTER, cols * max_n * nwin, 4);
        set(WS_COARSE, cols * L.coarse_stride, 4);
    }
    if (plan == MSM_PLAN_WIDE) {
        const MsmWideDims d = msm_wide_dims(c, max_n);
        set(WS_ENTRIES, cols * d.ent_stride, 4);
        set(WS_REDO, cols * d.lane_stride, 4);
        set(WS_SLOT_PT, cols * d.slot_stride, pt29);
        for (MsmBuf id : {WS_W_TOT0, WS_W_TOT1, WS_W_CUR0, WS_W_CUR1, WS_W_BSTART, WS_W_PSTART}) set(id, cols * nb, 4);
        set(WS_W_LANE_B, cols * d.lane_stride, 4);
        set(WS_W_PBUCKET, cols * d.part_stride, 4);
        set(WS_W_PART, cols * d.part_stride, pt29);
        set(WS_W_RC, cols * (d.rows + 256), pt29);
        return L;
    }
    const bool fixed = plan == MSM_PLAN_FIXED;
    const MsmStdPass p = msm_std_pass(fixed, c, max_n, max_batch);  // the widest, longest pass
    const size_t swept_blocks = (max_n + CHUNK - 1) / CHUNK * nwin, fused_blocks = fixed ? cols * nblk : 0;
    set(WS_ENTRIES, p.worst, 4);
    set(WS_REDO, p.threads + 1, 4);
    set(WS_SLOT_PT, p.threads + 1, pt29);
    set(WS_TOTALS, (size_t)p.nbt + 1, 4);
    set(WS_BUCKET_START, (size_t)p.nbt + 1, 4);
    if (fixed) set(WS_CURSOR, cols * nb, 4);
    set(WS_DIGITS, cols * max_n * nwin, 2);
    set(WS_BLOCKBASE, (swept_blocks > fused_blocks ? swept_blocks : fused_blocks) * nb, 4);
    set(WS_PARTIAL, (p.threads + 1) / GA + 2, pt29);
    set(WS_PART, p.ngroups, pt29);
    set(WS_BIT_SUM, (size_t)p.slices * c * BITSUM_MAX_SPLIT, ptx);
    return L;
}

}  // namespace zk
