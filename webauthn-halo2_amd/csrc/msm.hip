// msm.hip — Pippenger bucket multi-scalar multiplication over BN254 G1 for gfx950.
//
// Device replacement for halo2_proofs `arithmetic::best_multiexp`, reached only
// through `ParamsKZG::{commit, commit_lagrange}` (reference
// call sites halo2-circuits/src/ecc/ecdsa_p256.rs:366-373,416-423,555-562).
// Any correct algorithm yields the same group element, so the result is
// bit-identical to the reference's after affine normalisation.
//
// Layout of the source (round 6; one translation unit — the parts are textual includes that share the constants defined here):
//   msm.hip               behind the kernels the host: the workspace (made for ONE plan: its own buffers only), msm_run (dispatch) ->
//                         msm_run_standard / msm_run_wide (a sort head each, accumulation, tail), msm_collect (redo where the
//                         pass's word asks for it, Horner over the bit sums per result)
//   msm_plan.h            host code without HIP types: the choice of the plan (window by size, wide / fused / swept path, sort and
//                         scatter, bit-sum split, columns per pass), the geometry constants, every plan's workspace layout and
//                         its launchers' reach (walked by tests/msm_plan_check.cpp)
//   msm_wide.hip.h        THE path of every proof of the reference's configurations (2^16 .. 2^21 points over the resident SRS):
//                         15 .. 17-bit windows on precomputed window tables, ONE bucket set per column, a dense two-level sort,
//                         restartable accumulation lanes, the three-kernel reduction tail
//   msm_standard.hip.h    the plans around it: lg n - 5 window bits with digit planes and padded segments below 2^16 points, the
//                         swept sort from 2^22, and arbitrary bases (`zk_msm_bn254`: W windows x 2^(c-1) buckets, host Horner over
//                         the windows) — kernels msm_recode / msm_sort / msm_scatter* / msm_accumulate / msm_gather* / msm_bitsum
//   msm_tables.hip.h      the window tables 2^(c w) P_i and the identity test of a basis
// Two modes:
//   generic   bases are arbitrary (the fine-grained `zk_msm_bn254` seam): W windows of c bits, W x 2^(c-1) buckets;
//   fixed     bases are the resident SRS (`zk_commit`): a table of window multiples 2^(c w) P_i is precomputed once per basis,
//             so every window's digits fall into ONE set of 2^(c-1) buckets — no per-window reduction, no window Horner.
// Load balance does not depend on the scalar distribution: witness columns are dominated by zeros / small values (hot low
// buckets), and an accumulation lane is a fixed number of entries whatever buckets they fall in.
#include <stdlib.h>
#include <string.h>
#include <vector>

// This file's products on the carry-free field keep the source order of their multiply-adds (field29.hip.h ZK_MUL29_ASM):
// the accumulation runs four waves per SIMD (below), enough to hide a serial column, and saves the 64-bit join per column.
// Round 6: = 2, a column part per asm statement instead of a multiply-add per statement — hipcc's hazard recogniser puts an
// s_nop behind every asm statement whose result the next instruction reads (1 358 per mixed addition, 283 now): the lone 2^19
// accumulation 0.572 -> 0.553 / 0.580 -> 0.566 ms, two columns 1.058 -> 1.040 / 1.069 -> 1.033 (profiles/r6_ab_block_asm.txt)
#ifndef ZK_MUL29_ASM
#define ZK_MUL29_ASM 2
#endif
// ... except in the reduction kernels, which run about one wave per SIMD: their additions wait on that serial chain, not on
// issue slots, and take the compiler's form (g1x29_add<false>; tools/tail_times.sh, per lone k = 19 proof: msm_wrowcol
// 1.19 -> 0.98 ms, msm_wbits 1.00 -> 0.59, k = 15: msm_bitsum 1.02 -> 0.75, msm_gather 0.75 -> 0.64; msm_wparts unchanged)
#ifndef ZK_TAIL_SER
#define ZK_TAIL_SER false
#endif
// ... and except the per-bucket T1 (msm_wbucket_kernel), which is chosen only where the chip is loaded: issue slots count there
#ifndef ZK_T1B_SER
#define ZK_T1B_SER true
#endif
// slots a bucket may have for the per-bucket T1 to take it (a uniformly random 2^19 column: 17 .. 19)
#ifndef ZK_T1B_LMAX
#define ZK_T1B_LMAX 24
#endif
#include "ec29.hip.h"
#include "engine.h"

namespace zk {

static constexpr uint32_t SIGN_BIT = 0x80000000u;
static constexpr uint32_t SKIP_ENTRY = 0xffffffffu;  // padding entry (no base)
// wide path: an entry is sign << 31 | first-of-bucket << 30 | delta << 24 | table index (24 bits)
static constexpr uint32_t WIDE_FLAG = 0x40000000u;  // index bits ib = 24 .. 26 (WideGeo): delta field [ib, 30), escape = all ones
// CHUNK, FCHUNK, SEG0, GA, PAD, SUB and the wide path's WL, WCB, WCUR, WHDR, WCAP_MIN: msm_plan.h (with their build-time knobs)
#ifndef ZK_GLANES
#define ZK_GLANES 16
#endif
static constexpr uint32_t GLANES_FIXED = ZK_GLANES;  // lanes per bucket in the second-level gather (fixed-base mode)
#ifndef ZK_GSHARE
#define ZK_GSHARE 64
#endif
static constexpr uint32_t GSHARE = ZK_GSHARE;         // first-level partials per (bucket, part) group; a bucket uses ceil(partials / GSHARE) parts

struct MsmBatch {
    const Fr* s[MSM_MAX_BATCH];
};

// the kernels, by plan (one translation unit: the parts share the constants above)
#include "msm_standard.hip.h"  // 13-bit fused plan (n < 2^16), 15-bit swept sort (n >= 2^22), arbitrary bases
#include "msm_wide.hip.h"    // 15 .. 17-bit windows, one bucket set per column: every proof of the reference's configurations
#include "msm_tables.hip.h"  // window tables

// ------------------------------------------------------------------ host ---

// A workspace is made for ONE plan (msm_plan.h msm_ws_plan) and holds that plan's buffers only; their sizes are msm_ws_layout's,
// and tests/msm_plan_check.cpp proves on the host that no launcher below indexes beyond them.  It runs one pass at a time.
struct MsmWorkspace {
    size_t max_n;
    uint32_t max_batch;         // columns per fixed-base launch this workspace is sized for
    uint32_t c, nwin, nb;       // window bits, windows, buckets per window
    MsmPlan plan;
    bool wide;                  // plan == MSM_PLAN_WIDE: fixed base, and a table stride of max_n has the wide shape (msm_wide_shape)
    // ---- every plan
    uint32_t* counts;           // [4 * (MSM_MAX_BATCH + 1)]
    uint32_t* entries;          // +-base index; standard plan: bucket implied by position, padded per bucket; wide: dense column regions
    uint32_t* redo;             // segments / lanes the unchecked accumulation hands to the checked one
    G1X29S* slot_pt;            // partial sums of the accumulation, in its internal form (ec29.hip.h)
    size_t slot_elems;          // elements of slot_pt
    // two-level sorts (fixed-base plans): entries first grouped by coarse bin in `inter`, then by bucket
    uint32_t* inter;            // [max_batch][max_n * nwin]
    size_t inter_stride;        // entries per column in `inter`
    uint32_t* coarse;           // per column: the header (coarse-bin starts, chunk prefix, append cursors), then [blocks][bins] reserved bases
    uint32_t coarse_stride;     // words per column in `coarse`
    struct Standard {           // ---- msm_standard.hip.h
        uint32_t* totals;       // [bucket sets * nb + 1]
        uint32_t* cursor;       // [max_batch * nb] per-bucket write cursors of the two-level sort's second level (fixed base)
        int16_t* digits;        // [max_batch][nwin][max_n]  (|digit| <= 2^(c-1) <= 16384)
        uint32_t* bucket_start; // [bucket sets * nb + 1]
        uint32_t* blockbase;    // [blocks][nb]
        G1X29S* partial;        // [entries / PAD]
        G1X29S* part;           // [bucket sets * nb * parts]
        G1X* bit_sum;           // [bucket sets * c * BITSUM_MAX_SPLIT]
    } s;
    struct Wide : MsmWideDims { // ---- msm_wide.hip.h: per-column regions, their strides (msm_wide_dims) fixed by (c, max_n)
        WideGeo geo;            // entry layout, coarse bins, the recoding bias
        uint32_t row_bits;      // rows = 2^row_bits
        uint32_t t1_mode;       // T1 (ZK_OPT_MSM_T1): 1 one lane per bucket, otherwise parts + segmented tree
        bool clean;             // the pass counters (totals, cursors, counts) are zero: the previous pass left them so
        // per-bucket totals and level-2 cursors exist twice: pass i counts in set i & 1 while its first kernel — 131 K lanes with
        // to spare (the fine histogram: two thousand workgroups) — zeroes the other set for pass i + 1 (in the 16 waves of the last
        // tail kernel the reset cost 25 us of exposed latency per pass, in H1 13 us)
        uint32_t* tot[2];
        uint32_t* cur[2];
        uint32_t par;
        uint32_t used_cols[2];  // columns of a set that hold counts of its last pass (what the next H1 has to zero)
        uint32_t* lane_b;       // [max_batch][lane_stride] the bucket every lane starts in
        uint32_t* bstart;       // [max_batch][nb] places of the buckets in their column's entry region
        uint32_t* pstart;       // [max_batch][nb] first part of every bucket
        uint32_t* pbucket;      // [max_batch][part_stride] bucket of every part
        G1X29S* part;           // [max_batch][part_stride]
        G1X29S* rc;             // [max_batch][rows + 256] row and column sums of the bucket matrix
    } w;
};

size_t msm_ws_max_n(const MsmWorkspace* ws) { return ws->max_n; }
uint32_t msm_ws_max_batch(const MsmWorkspace* ws) { return ws->max_batch; }
uint32_t msm_ws_window(const MsmWorkspace* ws) { return ws->c; }
void msm_ws_set_t1_mode(MsmWorkspace* ws, uint32_t mode) { ws->w.t1_mode = mode; }

static_assert(sizeof(G1X29S) == 144 && sizeof(G1X) == 128, "tests/msm_plan_check.cpp sums the workspaces' bytes with these");
// where the buffer `id` of the layout lives
static void** msm_ws_slot(MsmWorkspace* ws, MsmBuf id) {
    switch (id) {
        case WS_COUNTS: return (void**)&ws->counts; case WS_ENTRIES: return (void**)&ws->entries; case WS_REDO: return (void**)&ws->redo;
        case WS_SLOT_PT: return (void**)&ws->slot_pt; case WS_INTER: return (void**)&ws->inter; case WS_COARSE: return (void**)&ws->coarse;
        case WS_TOTALS: return (void**)&ws->s.totals; case WS_CURSOR: return (void**)&ws->s.cursor; case WS_DIGITS: return (void**)&ws->s.digits;
        case WS_BUCKET_START: return (void**)&ws->s.bucket_start; case WS_BLOCKBASE: return (void**)&ws->s.blockbase; case WS_PARTIAL: return (void**)&ws->s.partial;
        case WS_PART: return (void**)&ws->s.part; case WS_BIT_SUM: return (void**)&ws->s.bit_sum; case WS_W_TOT0: return (void**)&ws->w.tot[0];
        case WS_W_TOT1: return (void**)&ws->w.tot[1]; case WS_W_CUR0: return (void**)&ws->w.cur[0]; case WS_W_CUR1: return (void**)&ws->w.cur[1];
        case WS_W_LANE_B: return (void**)&ws->w.lane_b; case WS_W_BSTART: return (void**)&ws->w.bstart; case WS_W_PSTART: return (void**)&ws->w.pstart;
        case WS_W_PBUCKET: return (void**)&ws->w.pbucket; case WS_W_PART: return (void**)&ws->w.part; case WS_W_RC: return (void**)&ws->w.rc;
        case WS_NBUF: break;
    }
    return nullptr;
}

MsmWorkspace* msm_workspace_create(size_t max_n, uint32_t c, bool fixed, hipError_t* err, uint32_t max_batch) {
    if (err) *err = hipSuccess;
    if (c == 0) c = msm_auto_window(max_n);
    if (max_batch == 0) max_batch = 1;
    const MsmPlan plan = msm_ws_plan(fixed, c, max_n);
    if (c < 9 || c > 17 || (c >= 16 && plan != MSM_PLAN_WIDE) || max_n == 0 || max_n > ((size_t)1 << 26) || max_batch > MSM_MAX_BATCH) {
        if (err) *err = hipErrorInvalidValue;
        return nullptr;
    }
    MsmWorkspace* ws = new MsmWorkspace();
    ws->max_n = max_n;
    ws->max_batch = max_batch;
    ws->c = c;
    ws->nwin = nwin_for(c);
    ws->nb = 1u << (c - 1);
    ws->plan = plan;
    ws->wide = plan == MSM_PLAN_WIDE;
    const MsmWsLayout L = msm_ws_layout(plan, c, max_n, max_batch, sizeof(G1X29S), sizeof(G1X));
    for (uint32_t id = 0; id < WS_NBUF; id++) {
        const hipError_t e = L.buf[id].elem ? hipMalloc(msm_ws_slot(ws, (MsmBuf)id), L.buf[id].count * L.buf[id].elem) : hipSuccess;
        if (e != hipSuccess) {
            if (err) *err = e;
            msm_workspace_destroy(ws);
            return nullptr;
        }
    }
    ws->slot_elems = L.buf[WS_SLOT_PT].count;
    ws->inter_stride = max_n * ws->nwin;
    ws->coarse_stride = L.coarse_stride;
    if (ws->wide) {
        // the geometry of every pass of this workspace, made once
        static_cast<MsmWideDims&>(ws->w) = msm_wide_dims(c, max_n);
        WideGeo& g = ws->w.geo;
        msm_wide_shape(c, max_n, &g.ib, &g.fb);
        g.c = c;
        g.nwin = ws->nwin;
        g.nb = ws->nb;
        g.bins = ws->w.bins;
        for (uint32_t w = 0; w < ws->nwin; w++) {  // the recoding bias: s + K < 2^254 + 2^(nwin c - 1) (1 + 2^-c + ..) < 2^256
            const uint32_t bit = c - 1 + w * c;
            g.K[bit >> 5] |= 1u << (bit & 31);
        }
        while ((1u << ws->w.row_bits) < ws->w.rows) ws->w.row_bits++;
    }
    return ws;
}

void msm_workspace_destroy(MsmWorkspace* ws) {
    if (!ws) return;
    for (uint32_t id = 0; id < WS_NBUF; id++) hipFree(*msm_ws_slot(ws, (MsmBuf)id));
    delete ws;
}

static MsmBatch msm_columns(const MsmPassArgs& a) {
    MsmBatch mb;
    memset(&mb, 0, sizeof(mb));
    for (uint32_t q = 0; q < a.batch; q++) mb.s[q] = a.columns[q];
    return mb;
}

// the head's hand-off: the tail goes on a.tail behind a.head_done where that is another stream than the head's
static hipError_t msm_tail_stream(const MsmPassArgs& a, hipStream_t* ts) {
    *ts = a.head;
    if (!a.tail || a.tail == a.head) return hipSuccess;
    hipError_t e;
    if ((e = hipEventRecord(a.head_done, a.head)) != hipSuccess) return e;
    if ((e = hipStreamWaitEvent(a.tail, a.head_done, 0)) != hipSuccess) return e;
    *ts = a.tail;
    return hipSuccess;
}

// ---- the wide path's pipeline (msm_wide.hip.h).  The geometry is the workspace's; what depends on the pass (wide_lanes,
// wide_max_chunks, wide_max_parts): msm_plan.h

// H1 + S1 at C-bit windows: the coarse histogram and the first scatter
template <uint32_t C>
static void wide_head(const MsmWorkspace* ws, const MsmPassArgs& a, uint32_t WCAP) {
    const uint32_t n32 = (uint32_t)a.n;
    const dim3 gh((n32 + FCHUNK - 1) / FCHUNK, a.batch);
    const MsmBatch mb = msm_columns(a);
    hipLaunchKernelGGL(msm_whist_kernel<C>, gh, dim3(256), 0, a.head, mb, n32, ws->w.geo, ws->coarse, ws->coarse_stride, ws->counts);
    hipLaunchKernelGGL(msm_wscatter1_kernel<C>, gh, dim3(256), 0, a.head, mb, n32, ws->w.geo, a.table_stride, ws->coarse, ws->coarse_stride,
                       ws->inter, ws->inter_stride, ws->counts, WCAP);
}

// The reduction tail of `batch` columns of n scalars on `ts`, over the counter set `totals` the pass counted in: T1 per part, with
// `per_bucket` behind the per-bucket kernel (ZK_OPT_MSM_T1 = 1: fewer instructions, a longer chain — measured: no gain,
// msm_wide.hip.h), T2, T3.  T3 writes its sums (and the redo count) STRAIGHT into the caller's pinned host buffer: 17 x 128 bytes
// per column over the bus instead of a copy kernel at the end of every pass's chain (host_sums must be device-visible pinned
// memory: the engine's lanes allocate it with hipHostMalloc).  The caller asks hipGetLastError.
static hipError_t wide_tail(MsmWorkspace* ws, uint32_t batch, size_t n, hipStream_t ts, uint32_t* totals, bool per_bucket, G1X* host_sums) {
    const uint32_t nb = ws->nb, WCAP = wcap_for(batch);
    if (n > 0) {
        uint32_t lmin = 0;
        if (per_bucket) {
            lmin = ZK_T1B_LMAX;
            hipLaunchKernelGGL(msm_wbucket_kernel, dim3(nb / 64, batch), dim3(64), 0, ts, ws->slot_pt, ws->w.slot_stride, totals, ws->w.bstart,
                               ws->w.pstart, ws->w.part_stride, nb, ws->w.part, WCAP, lmin);
        }
        hipLaunchKernelGGL(msm_wparts_kernel, dim3((wide_max_parts(ws->nwin, nb, ws->w.bins, n, WCAP) + 63) / 64, batch), dim3(64), 0, ts, ws->slot_pt,
                           ws->w.slot_stride, totals, ws->w.bstart, ws->w.pstart, ws->w.pbucket, ws->w.part_stride, nb, ws->counts, ws->w.part,
                           WCAP, lmin);
    }
    hipLaunchKernelGGL(msm_wrowcol_kernel, dim3(ws->w.rows + 256, batch), dim3(64), 0, ts, ws->w.part, ws->w.part_stride, totals, ws->w.bstart,
                       ws->w.pstart, nb, ws->w.rc, WCAP);
    G1X* out_dev = nullptr;
    const hipError_t e = hipHostGetDevicePointer((void**)&out_dev, host_sums, 0);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(msm_wbits_kernel, dim3(9 + ws->w.row_bits, batch), dim3(64), 0, ts, ws->w.rc, nb, out_dev, ws->counts);
    return hipSuccess;
}

// `a.batch` columns against the resident basis whose window table — in the internal form, msm_build_table(.., internal = true)
// — is a.table
static hipError_t msm_run_wide(MsmWorkspace* ws, const MsmPassArgs& a, MsmPass* pass) {
    const uint32_t c = ws->c, nb = ws->nb, batch = a.batch, WCAP = wcap_for(batch);
    const size_t n = a.n;
    const WideGeo& g = ws->w.geo;
    hipStream_t st = a.head;
    hipError_t e;
#ifdef ZK_MSM_POISON  // debug: a slot / part / row-column sum read without having been written by THIS pass shows
    hipMemsetAsync(ws->slot_pt, 0xA5, ws->slot_elems * sizeof(G1X29S), st);
    hipMemsetAsync(ws->w.part, 0xA5, (size_t)ws->max_batch * ws->w.part_stride * sizeof(G1X29S), st);
    hipMemsetAsync(ws->w.rc, 0xA5, (size_t)ws->max_batch * (ws->w.rows + 256) * sizeof(G1X29S), st);
#endif
    if (!ws->w.clean) {
        // first pass on this workspace (or the previous one did not finish): every later pass finds the counters zeroed by
        // the last tail kernel of the pass before
        const uint32_t all = ws->max_batch * nb;
        uint32_t m = all;
        if (ws->max_batch * WCB > m) m = ws->max_batch * WCB;
        if (4 * (MSM_MAX_BATCH + 1) > m) m = 4 * (MSM_MAX_BATCH + 1);
        hipLaunchKernelGGL(msm_wclear_kernel, dim3((m + 255) / 256), dim3(256), 0, st, ws->w.tot[0], ws->w.cur[0], ws->w.tot[1], ws->w.cur[1],
                           all, ws->counts, ws->coarse, ws->coarse_stride, ws->max_batch);
        ws->w.used_cols[0] = ws->w.used_cols[1] = 0;
    }
    ws->w.clean = false;
    uint32_t* const totals = ws->w.tot[ws->w.par];  // this pass's set of per-bucket counters; H1 zeroes the other one
    uint32_t* const cursor = ws->w.cur[ws->w.par];
    uint32_t* const next_totals = ws->w.tot[ws->w.par ^ 1];
    uint32_t* const next_cursor = ws->w.cur[ws->w.par ^ 1];
    if (n > 0) {
        if (c == 17)
            wide_head<17>(ws, a, WCAP);
        else if (c == 16)
            wide_head<16>(ws, a, WCAP);
        else
            wide_head<15>(ws, a, WCAP);
        const dim3 gc(wide_max_chunks(ws->nwin, ws->w.bins, n) + 1, batch), gl((wide_lanes(ws->nwin, n) + 63) / 64, batch);
        hipLaunchKernelGGL(msm_wfinehist_kernel, gc, dim3(256), 0, st, ws->inter, ws->inter_stride, ws->coarse, ws->coarse_stride, g, totals,
                           next_totals, next_cursor, ws->w.used_cols[ws->w.par ^ 1]);
        hipLaunchKernelGGL(msm_wscatter2_kernel, gc, dim3(256), 0, st, ws->inter, ws->inter_stride, ws->coarse, ws->coarse_stride, g, totals,
                           ws->w.bstart, cursor, ws->entries, ws->w.ent_stride, ws->w.lane_b, ws->w.lane_stride, ws->w.pstart, ws->w.pbucket,
                           ws->w.part_stride, WCAP);
        if (a.events) hipEventRecord(a.events[0], st);
        if (a.bases_may_be_identity) {
            hipLaunchKernelGGL(msm_wacc_kernel, gl, dim3(64), 0, st, ws->entries, ws->w.ent_stride, a.table, ws->counts, ws->w.lane_b,
                               ws->w.lane_stride, ws->w.bstart, nb, ws->slot_pt, ws->w.slot_stride, g.ib);
        } else {
            hipLaunchKernelGGL(msm_wacc_fast_kernel, gl, dim3(64), 0, st, ws->entries, ws->w.ent_stride, a.table, ws->counts, ws->w.lane_b,
                               ws->w.lane_stride, ws->w.bstart, nb, ws->slot_pt, ws->w.slot_stride, ws->redo, g.ib);
        }
        if (a.events) hipEventRecord(a.events[1], st);
    }
    hipStream_t ts;
    if ((e = msm_tail_stream(a, &ts)) != hipSuccess) return e;
    if (a.events && a.events[2]) hipEventRecord(a.events[2], ts);  // the reduction tail (T1 .. T3) alone
    if ((e = wide_tail(ws, batch, n, ts, totals, ws->w.t1_mode == 1, a.host_sums)) != hipSuccess) return e;
    if (a.events && a.events[3]) hipEventRecord(a.events[3], ts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    ws->w.clean = true;
    if (n > 0) {  // (an empty pass neither counts nor zeroes anything)
        ws->w.used_cols[ws->w.par] = batch;
        ws->w.used_cols[ws->w.par ^ 1] = 0;
        ws->w.par ^= 1;  // the next pass counts in the set this one has zeroed
    }
    // the unchecked accumulation's count of lanes to redo follows the sums (the checked loop lists nothing; an empty pass never
    // reset counts[1])
    *pass = MsmPass{MsmPass::WIDE, batch, WIDE_SUMS, c, n, n > 0 && !a.bases_may_be_identity, a.table};
    return hipSuccess;
}

// The unchecked accumulation of the wide path lists the lanes whose sums show an exceptional step; the count travels to the host
// with the pass's sums (msm_wbits_kernel).  Non-zero — a degenerate basis only — and msm_collect calls this: the listed lanes again
// with the checked loop, then the tail again — by parts, whatever the pass's T1 was — on `st`; the pass's workspace is intact
// until the lane's next pass.
static hipError_t msm_wide_redo(MsmWorkspace* ws, const MsmPass& p, hipStream_t st, G1X* host_sums) {
    hipLaunchKernelGGL(msm_wacc_redo_kernel, dim3(256), dim3(64), 0, st, ws->entries, ws->w.ent_stride, p.table, ws->counts, ws->w.lane_b,
                       ws->w.lane_stride, ws->w.bstart, ws->nb, ws->slot_pt, ws->w.slot_stride, ws->redo, ws->w.geo.ib);
    hipError_t e = hipMemsetAsync(ws->counts + 1, 0, 4, st);  // the second tail reports none
    if (e != hipSuccess) return e;
    // the set the pass counted in (the parity has moved on)
    if ((e = wide_tail(ws, p.batch, p.n, st, ws->w.tot[ws->w.par ^ 1], false, host_sums)) != hipSuccess) return e;
    return hipGetLastError();
}

// ---- the standard plan's pipeline (msm_standard.hip.h).  What a pass indexes at most (MsmStdPass): msm_plan.h
// two-level counting sort with coalesced stores (see msm_scatter1_kernel)
static void std_head_sort2(const MsmWorkspace* ws, const MsmPassArgs& a, const MsmStdPass& p) {
    const uint32_t c = ws->c, nwin = ws->nwin, nb = ws->nb, batch = a.batch, n32 = (uint32_t)a.n, stride = (uint32_t)ws->max_n;
    const uint32_t nblk = (n32 + FCHUNK - 1) / FCHUNK;
    hipStream_t st = a.head;
    hipLaunchKernelGGL(msm_recode_hist2_kernel, dim3(nblk, batch), dim3(256), (nb + 256 * 9) * 4, st, msm_columns(a), n32, stride, c,
                       nwin, nb, ws->s.digits, ws->s.totals, ws->coarse, ws->coarse_stride);
    hipLaunchKernelGGL(msm_scan_kernel, dim3(1), dim3(1024), 0, st, ws->s.totals, ws->s.bucket_start, p.nbt, ws->counts);
    hipLaunchKernelGGL(msm_scan_coarse_kernel, dim3(batch), dim3(CBINS_MAX), 0, st, ws->s.totals, nb, ws->coarse, ws->coarse_stride, nb >> 6, 6u);
    hipLaunchKernelGGL(msm_scatter1_kernel, dim3(nblk, batch), dim3(256), 0, st, ws->s.digits, n32, stride, nwin, nb, a.table_stride,
                       ws->coarse, ws->coarse_stride, ws->inter, ws->inter_stride, 6u);
    const uint32_t max_chunks = (uint32_t)(((uint64_t)n32 * nwin + SUB - 1) / SUB) + (nb >> 6);
    hipLaunchKernelGGL(msm_scatter2_kernel, dim3(max_chunks, batch), dim3(256), 0, st, ws->inter, ws->inter_stride, ws->coarse,
                       ws->coarse_stride, nb, ws->s.totals, ws->s.bucket_start, ws->s.cursor, ws->entries, 6u, PAD, (size_t)0, (const uint8_t*)nullptr);
}

// digits + histogram in one kernel, then the one-pass scatter
static void std_head_fused(const MsmWorkspace* ws, const MsmPassArgs& a, const MsmStdPass& p) {
    const uint32_t c = ws->c, nwin = ws->nwin, nb = ws->nb, batch = a.batch, n32 = (uint32_t)a.n, stride = (uint32_t)ws->max_n;
    const uint32_t nblk = (n32 + FCHUNK - 1) / FCHUNK;
    hipStream_t st = a.head;
    hipLaunchKernelGGL(msm_recode_hist_kernel, dim3(nblk, batch), dim3(256), (nb + 256 * 9) * 4, st, msm_columns(a), n32, stride, c,
                       nwin, nb, ws->s.digits, ws->s.totals, ws->s.blockbase);
    hipLaunchKernelGGL(msm_scan_kernel, dim3(1), dim3(1024), 0, st, ws->s.totals, ws->s.bucket_start, p.nbt, ws->counts);
    // long columns: one scatter launch per column (msm_plan.h msm_scatter_per_launch)
    const uint32_t per_launch = msm_scatter_per_launch(n32, batch);
    for (uint32_t q = 0; q < batch; q += per_launch)
        hipLaunchKernelGGL(msm_scatter_fixed_kernel, dim3(nblk, per_launch), dim3(SCAT_T), nb * 4, st,
                           ws->s.digits + (size_t)q * nwin * stride, n32, stride, nwin, nb, a.table_stride,
                           ws->s.totals + (size_t)q * nb, ws->s.bucket_start + (size_t)q * nb,
                           ws->s.blockbase + (size_t)q * nblk * nb, ws->entries);
}

// the swept sort: arbitrary bases, and bucket sets beyond the LDS budget; one column
static void std_head_swept(const MsmWorkspace* ws, const MsmPassArgs& a, const MsmStdPass& p) {
    const uint32_t c = ws->c, nwin = ws->nwin, nb = ws->nb, n32 = (uint32_t)a.n, stride = (uint32_t)ws->max_n;
    const uint32_t nchunks = (n32 + CHUNK - 1) / CHUNK, fixed = a.table ? 1u : 0u;
    const uint32_t sort_lds = (nb < SORT_LDS_BUCKETS ? nb : SORT_LDS_BUCKETS) * 4;
    hipStream_t st = a.head;
    hipLaunchKernelGGL(msm_recode_kernel, dim3((n32 + 255) / 256), dim3(256), 0, st, a.columns[0], n32, stride, c, nwin,
                       ws->s.digits);
    hipLaunchKernelGGL(msm_sort_kernel<false>, dim3(nchunks * nwin), dim3(256), sort_lds, st, ws->s.digits, n32, stride,
                       nchunks, nb, fixed, a.table_stride, ws->s.totals, ws->s.bucket_start, ws->s.blockbase,
                       (uint32_t*)nullptr);
    hipLaunchKernelGGL(msm_scan_kernel, dim3(1), dim3(1024), 0, st, ws->s.totals, ws->s.bucket_start, p.nbt, ws->counts);
    hipLaunchKernelGGL(msm_sort_kernel<true>, dim3(nchunks * nwin), dim3(256), sort_lds, st, ws->s.digits, n32, stride,
                       nchunks, nb, fixed, a.table_stride, ws->s.totals, ws->s.bucket_start, ws->s.blockbase,
                       ws->entries);
    hipLaunchKernelGGL(msm_pad_kernel, dim3((p.nbt + 255) / 256), dim3(256), 0, st, ws->s.totals, ws->s.bucket_start, p.nbt,
                       ws->entries);
}

// the reduction tail on `ts`: the two gather levels, the bit sums and their copy to the host
static hipError_t std_tail(const MsmWorkspace* ws, const MsmPassArgs& a, const MsmStdPass& p, hipStream_t ts, uint32_t bs) {
    const uint32_t c = ws->c, nb = ws->nb;
    if (a.n > 0) {
        hipLaunchKernelGGL(msm_gather1_kernel, dim3((uint32_t)((p.lanes1 + 63) / 64)), dim3(64), 0, ts, ws->slot_pt, ws->counts,
                           ws->s.partial);
        if (a.table)
            hipLaunchKernelGGL(msm_gather_kernel<GLANES_FIXED>, dim3((p.ngroups * GLANES_FIXED + 255) / 256), dim3(256), 0, ts, ws->s.bucket_start,
                               ws->s.partial, p.parts, p.ngroups, ws->s.part);
        else
            hipLaunchKernelGGL(msm_gather_kernel<4>, dim3((p.ngroups * 4 + 255) / 256), dim3(256), 0, ts, ws->s.bucket_start,
                               ws->s.partial, p.parts, p.ngroups, ws->s.part);
    }
    // bit_sum[(w * c + t) * split + q]: partials of G_{w,t}; one wave per workgroup (msm_plan.h bitsum_threads)
    hipLaunchKernelGGL(msm_bitsum_kernel<64>, dim3(p.slices * c * bs), dim3(64), 0, ts, ws->s.part, p.parts, nb, c, bs, ws->s.bucket_start,
                       ws->s.bit_sum);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(a.host_sums, ws->s.bit_sum, (size_t)p.slices * c * bs * sizeof(G1X), hipMemcpyDeviceToHost, ts);
}

// `a.batch` columns against a.table (table[w * table_stride + i] = 2^(c w) P_i), or one column against the arbitrary a.bases
static hipError_t msm_run_standard(MsmWorkspace* ws, const MsmPassArgs& a, MsmPass* pass) {
    const size_t n = a.n;
    const uint32_t c = ws->c, nwin = ws->nwin, nb = ws->nb, batch = a.batch;
    const bool fixed = a.table != nullptr;
    const bool fused = msm_fused(fixed, nb);  // one-kernel digits + histogram; 15-bit windows take the swept sort
    if (!fused && batch != 1) return hipErrorInvalidValue;  // columns are batched on the fused fixed-base path only
    hipStream_t st = a.head;
    const G1Affine* const points = fixed ? a.table : a.bases;
    const MsmStdPass p = msm_std_pass(fixed, c, n, batch);
    const bool sort2 = sort2_applies(fused, n, nb, nwin, a.table_stride);
    // the bucket parts need no reset: the bit sums read only the parts the gather wrote (msm_bitsum_kernel used_parts); an empty
    // MSM runs no gather, so its parts are set to the identity here
#ifdef ZK_MSM_POISON
    hipMemsetAsync(ws->s.part, 0xA5, (size_t)p.ngroups * sizeof(G1X29S), st);  // debug: any part read without being written shows
#endif
    const uint32_t clear_parts = n > 0 ? 0u : p.ngroups;
    uint32_t m = p.nbt + 1;
    if (clear_parts > m) m = clear_parts;
    if (batch * CBINS_MAX > m) m = batch * CBINS_MAX;
    hipLaunchKernelGGL(msm_clear_kernel, dim3((m + 255) / 256), dim3(256), 0, st, ws->s.part, clear_parts, ws->s.totals, p.nbt + 1,
                       ws->counts, ws->s.cursor, sort2 ? p.nbt : 0u, ws->coarse, ws->coarse_stride, sort2 ? batch : 0u);
    if (n > 0) {
        if (sort2)
            std_head_sort2(ws, a, p);
        else if (fused)
            std_head_fused(ws, a, p);
        else
            std_head_swept(ws, a, p);
        if (a.events) hipEventRecord(a.events[0], st);
        if (a.bases_may_be_identity) {
            hipLaunchKernelGGL(msm_accumulate_kernel, dim3((uint32_t)((p.threads + 63) / 64)), dim3(64), 0, st, ws->entries, points,
                               ws->counts, ws->slot_pt);
        } else {
            hipLaunchKernelGGL(msm_accumulate_fast_kernel, dim3((uint32_t)((p.threads + 63) / 64)), dim3(64), 0, st, ws->entries, points,
                               ws->counts, ws->redo, ws->slot_pt);
        }
        if (a.events) hipEventRecord(a.events[1], st);  // the dominant kernel alone (bench.py's roofline)
        if (!a.bases_may_be_identity)
            hipLaunchKernelGGL(msm_accumulate_redo_kernel, dim3(1024), dim3(64), 0, st, ws->entries, points, ws->counts, ws->redo,
                               ws->slot_pt);
    }
    hipStream_t ts;
    const hipError_t e = msm_tail_stream(a, &ts);
    if (e != hipSuccess) return e;
    const uint32_t bs = bitsum_split(nb);
    // fixed-base mode: a result per column from its c bit positions; arbitrary bases: one result from all windows' positions
    *pass = MsmPass{fixed ? MsmPass::FIXED : MsmPass::GENERIC, batch, (fixed ? 1u : nwin) * c * bs, c, n, false, a.table};
    return std_tail(ws, a, p, ts, bs);
}

// One pass: a.table != nullptr selects the fixed-base mode.  The "head" (recode .. accumulate) runs on a.head; the latency-bound
// "tail" (gather, bit sums, D2H) runs on a.tail after a.head_done, so that the caller can put the next MSM's head (or any other
// kernels) on a.head right away.  a.tail == a.head (or none) gives the plain sequential order.  The plan is the workspace's: a
// wide one serves its resident table only, a standard one never runs wide; a fixed-base workspace is not for arbitrary bases.
hipError_t msm_run(MsmWorkspace* ws, const MsmPassArgs& a, MsmPass* pass) {
    if (a.n > ws->max_n || a.batch == 0 || a.batch > ws->max_batch) return hipErrorInvalidValue;
    if (ws->wide) return a.table && a.table_stride == ws->max_n ? msm_run_wide(ws, a, pass) : hipErrorInvalidValue;
    if ((a.table != nullptr) != (ws->plan == MSM_PLAN_FIXED)) return hipErrorInvalidValue;
    return msm_run_standard(ws, a, pass);
}

// The host's finish of one result.  Standard plan: sum over the bit positions pos of 2^pos G_pos (Horner), G_pos in `split`
// partials (bitsum_split) ...
static G1Jac msm_horner(const G1X* bit_sums, uint32_t positions, uint32_t split) {
    G1X acc = G1X::identity();
    for (int q = (int)positions - 1; q >= 0; q--) {
        if (!acc.is_identity()) acc = g1x_dbl(acc);
        for (uint32_t k = 0; k < split; k++) g1x_add(acc, bit_sums[(size_t)q * split + k]);
    }
    return g1x_to_jac(acc);
}

// ... wide path: sum_{t < 9} 2^t S_t (columns of the bucket matrix, weight l + 1) + sum_u 2^(8 + u) S_{9 + u} (rows, weight 256 h)
static G1Jac msm_horner_wide(const G1X* sums, uint32_t row_bits) {
    G1X acc = G1X::identity();
    for (int pos = (int)(8 + row_bits) - 1; pos >= 0; pos--) {
        if (!acc.is_identity()) acc = g1x_dbl(acc);
        if (pos >= 8) g1x_add(acc, sums[9 + (pos - 8)]);
        if (pos <= 8) g1x_add(acc, sums[pos]);
    }
    return g1x_to_jac(acc);
}

hipError_t msm_collect(MsmWorkspace* ws, const MsmPass& p, hipStream_t tail, G1X* host_sums, G1Jac* out, bool* redone) {
    *redone = false;
    if (p.redo_word) {
        uint32_t listed;
        memcpy(&listed, host_sums + (size_t)p.batch * p.sums_per_result, 4);
        if (listed) {
            // a degenerate basis (equal or opposite points): the unchecked accumulation reported lanes to redo with the checked loop
            hipError_t e = msm_wide_redo(ws, p, tail, host_sums);
            if (e == hipSuccess) e = hipStreamSynchronize(tail);
            if (e != hipSuccess) return e;
            *redone = true;
        }
    }
    const uint32_t split = bitsum_split(1u << (p.c - 1));
    for (uint32_t q = 0; q < p.batch; q++) {
        const G1X* sums = host_sums + (size_t)q * p.sums_per_result;
        out[q] = p.plan == MsmPass::WIDE ? msm_horner_wide(sums, ws->w.row_bits) : msm_horner(sums, p.sums_per_result / split, split);
    }
    return hipSuccess;
}

}  // namespace zk
