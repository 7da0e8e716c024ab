// Host-only check of the MSM plan rules (csrc/msm_plan.h): no device is touched.  For both modes, every log n in 0 .. 26, every
// ZK_OPT_MSM_WINDOW in {0, 9 .. 17} and pass widths {default, 1, 3, 256} it prints one line — window, windows, buckets, wide /
// fused / sort2 / per-column scatter, bit-sum split, sweeps of the swept sort, widest pass — which tests/test_msm_plan.py compares
// with the Python restatement (tests/msm_cases.py), and it asserts what the kernels rely on and what the comments promise.
// Then the workspaces: for every workspace get_msm_ws can make (pass widths {default, 1, 3, 8, 256}) it proves that no launcher of
// msm.hip indexes beyond a buffer of the plan's layout (msm_ws_layout), at any length and pass width the workspace admits, and
// prints one `ws ` line with the workspace's bytes and its largest buffer.
#include <cstdio>
#include <cstdlib>
#include "msm_plan.h"
using namespace zk;

static int fails = 0;
#define EXPECT(cond, ...)                                      \
    do {                                                       \
        if (!(cond)) {                                         \
            printf("FAILED line %d: %s: ", __LINE__, #cond);   \
            printf(__VA_ARGS__);                               \
            printf("\n");                                      \
            fails++;                                           \
        }                                                      \
    } while (0)

static const uint32_t OVERRIDES[] = {0, 9, 10, 11, 12, 13, 14, 15, 16, 17};
static const uint32_t WIDTHS[] = {0, 1, 3, 256};
static const uint32_t MAX_LG = 26;

static const uint32_t WS_WIDTHS[] = {0, 1, 3, 8, 256};
static const char* const BUF_NAMES[WS_NBUF] = {"counts", "entries", "redo", "slot_pt", "inter", "coarse", "totals", "cursor", "digits", "bucket_start", "blockbase", "partial",
                                               "part", "bit_sum", "w_tot0", "w_tot1", "w_cur0", "w_cur1", "w_lane_b", "w_bstart", "w_pstart", "w_pbucket", "w_part", "w_rc"};
static const size_t PT29 = 144, PTX = 128;  // sizeof(G1X29S), sizeof(G1X): static_assert in msm.hip

// One pass of `batch` columns of n scalars on the workspace L of (plan, c, max_n): every index the launchers of msm.hip hand
// to a kernel, against the buffer it lands in.  `stride`: the resident table's (fixed-base plans).
static void reach(const char* tag, const MsmWsLayout& L, MsmPlan plan, uint32_t c, size_t max_n, size_t n, uint32_t batch, size_t stride) {
    const size_t nwin = nwin_for(c), nb = (size_t)1 << (c - 1), nblk = (n + FCHUNK - 1) / FCHUNK, B = batch;
    const auto fits = [&](MsmBuf id, size_t need, const char* what) {
        EXPECT(L.buf[id].elem != 0 && need <= L.buf[id].count, "%s c %u max_n %zu n %zu batch %u: %s needs %zu of %zu in %s", tag, c, max_n, n, batch, what, need,
               L.buf[id].count, BUF_NAMES[id]);
    };
    fits(WS_COUNTS, 4 * (B + 1), "the pass counters");
    if (plan == MSM_PLAN_WIDE) {
        const MsmWideDims d = msm_wide_dims(c, max_n);
        const size_t lanes = wide_lanes(nwin, n);
        EXPECT(n * nwin <= d.ent_stride && lanes <= d.lane_stride && lanes + nb <= d.slot_stride, "%s c %u n %zu: a column outgrows its region", tag, c, n);
        EXPECT(d.ent_stride % 64 == 0 && lanes * WL <= d.ent_stride + WL - 1, "%s c %u n %zu: entry region", tag, c, n);
        for (uint32_t wcap = WCAP_MIN; wcap <= 8; wcap++)  // wcap_for: ZK_WCAP_ONE, ZK_WCAP_BATCH (8); T1's grid is rounded up to 64 and guarded
            EXPECT(wide_max_parts(nwin, nb, d.bins, n, wcap) <= d.part_stride, "%s c %u n %zu: %u parts at WCAP %u, stride %u", tag, c, n,
                   wide_max_parts(nwin, nb, d.bins, n, wcap), wcap, d.part_stride);
        EXPECT(d.bins <= WCB && d.rows * 256 == nb, "%s c %u: %u bins, %u rows", tag, c, d.bins, d.rows);
        fits(WS_INTER, (B - 1) * max_n * nwin + n * nwin, "the binned list");
        fits(WS_COARSE, (B - 1) * L.coarse_stride + WHDR + nblk * WCB, "the headers and reserved bases");
        fits(WS_ENTRIES, (B - 1) * d.ent_stride + n * nwin, "the dense entry list");
        fits(WS_REDO, (B - 1) * d.lane_stride + lanes, "one word per lane");
        fits(WS_W_LANE_B, (B - 1) * d.lane_stride + lanes, "the lanes' buckets");
        fits(WS_SLOT_PT, (B - 1) * d.slot_stride + lanes + nb, "slot = lane + bucket");
        for (MsmBuf id : {WS_W_TOT0, WS_W_TOT1, WS_W_CUR0, WS_W_CUR1, WS_W_BSTART, WS_W_PSTART}) fits(id, B * nb, "a word per bucket");
        fits(WS_W_PBUCKET, B * d.part_stride, "the parts' buckets");
        fits(WS_W_PART, B * d.part_stride, "the parts");
        fits(WS_W_RC, B * (d.rows + 256), "row and column sums");
        return;
    }
    const bool fixed = plan == MSM_PLAN_FIXED, fused = msm_fused(fixed, (uint32_t)nb), sort2 = sort2_applies(fused, n, (uint32_t)nb, (uint32_t)nwin, stride);
    if (!fused && batch != 1) return;  // msm_run refuses
    const MsmStdPass p = msm_std_pass(fixed, c, n, batch);
    // (not asserted: p.worst < 2^32.  The kernels count entries in 32 bits, which 256-column passes over 2^20 points and more,
    // reachable with ZK_OPT_MSM_WINDOW <= 14 and ZK_OPT_MSM_BATCH only, exceed — as before this layout existed)
    EXPECT((uint64_t)p.ngroups * 16 < (1ull << 32), "%s c %u n %zu batch %u: 32-bit grid arithmetic", tag, c, n, batch);
    fits(WS_TOTALS, (size_t)p.nbt + 1, "bucket totals");
    fits(WS_BUCKET_START, (size_t)p.nbt + 1, "bucket starts");
    fits(WS_DIGITS, (B - 1) * nwin * max_n + (nwin - 1) * max_n + n, "digit planes");
    fits(WS_ENTRIES, p.worst, "the padded entry list");
    fits(WS_REDO, p.threads, "one word per segment");
    fits(WS_SLOT_PT, p.threads > p.lanes1 * GA ? p.threads : p.lanes1 * GA, "a slot per segment, GA per gather lane");
    fits(WS_PARTIAL, p.lanes1, "first-level partials");
    fits(WS_PART, n > 0 ? p.ngroups : (size_t)p.nbt * p.parts, "bucket parts");
    fits(WS_BIT_SUM, (size_t)p.slices * c * bitsum_split((uint32_t)nb), "bit sums");
    if (sort2) {
        EXPECT(nb / 64 <= CBINS_MAX && COARSE_WORDS <= WHDR && CBINS_MAX <= WCB, "%s c %u: the wide header does not cover the two-level sort's", tag, c);
        fits(WS_CURSOR, p.nbt, "second-level cursors");
        fits(WS_INTER, (B - 1) * max_n * nwin + n * nwin, "the binned list");
        fits(WS_COARSE, (B - 1) * L.coarse_stride + COARSE_WORDS + nblk * CBINS_MAX, "the headers and reserved bases");
    } else if (fused) {
        fits(WS_BLOCKBASE, B * nblk * nb, "per-workgroup bases");
    } else {
        fits(WS_BLOCKBASE, (n + CHUNK - 1) / CHUNK * nwin * nb, "per-workgroup bases of the sweeps");
    }
}

// the workspace get_msm_ws makes for (mode, window, length, columns): its plan's buffers only, every pass inside them
static void workspace(const char* mode, uint32_t lg, uint32_t ov, uint32_t req, bool fixed, uint32_t c, size_t stride, uint32_t cols) {
    const size_t max_n = msm_ws_len((size_t)1 << lg);
    const MsmPlan plan = msm_ws_plan(fixed, c, max_n);
    const MsmWsLayout L = msm_ws_layout(plan, c, max_n, cols, PT29, PTX);
    char tag[64];
    snprintf(tag, sizeof tag, "ws %s lg %u ov %u req %u", mode, lg, ov, req);
    EXPECT((plan == MSM_PLAN_WIDE) == (fixed && msm_wide_applies(c, max_n)), "%s: plan %u", tag, (unsigned)plan);
    EXPECT(plan != MSM_PLAN_WIDE || stride == max_n, "%s: a wide workspace whose table stride is not its length", tag);
    EXPECT(c <= 15 || plan == MSM_PLAN_WIDE, "%s: %u bits on a standard workspace", tag, c);
    size_t bytes = 0;
    uint32_t big = 0;
    for (uint32_t id = 0; id < WS_NBUF; id++) {
        const bool std_only = id >= WS_TOTALS && id <= WS_BIT_SUM, wide_only = id >= WS_W_TOT0;
        const bool want = id < WS_INTER || (plan == MSM_PLAN_WIDE ? !std_only : !wide_only && (fixed || (id != WS_INTER && id != WS_COARSE && id != WS_CURSOR)));
        EXPECT((L.buf[id].elem != 0) == want && (L.buf[id].elem == 0 || L.buf[id].count > 0), "%s: buffer %s %s", tag, BUF_NAMES[id], want ? "missing" : "of another plan");
        bytes += L.buf[id].count * L.buf[id].elem;
        if (L.buf[id].count * L.buf[id].elem > L.buf[big].count * L.buf[big].elem) big = id;
    }
    if (plan == MSM_PLAN_WIDE) {  // the two checks msm_workspace_create used to make on the device path
        const MsmWideDims d = msm_wide_dims(c, max_n);
        EXPECT(cols * d.ent_stride <= L.buf[WS_ENTRIES].count && (size_t)cols * d.slot_stride <= L.buf[WS_SLOT_PT].count, "%s: column regions", tag);
    }
    // the maxima grow with n and with the batch (sums and rounded-up quotients of both): the ends and a few points between
    const size_t ns[] = {0, 1, 1023, max_n / 2, max_n / 2 + 1, (size_t)ZK_SORT2_MIN_N - 1, (size_t)ZK_SORT2_MIN_N, max_n - 1, max_n};
    const uint32_t bs[] = {1, 2, 3, cols / 2, cols};
    for (size_t n : ns)
        for (uint32_t b : bs)
            if (n <= max_n && n <= (stride > max_n ? max_n : (fixed ? stride : max_n)) && b >= 1 && b <= cols) reach(tag, L, plan, c, max_n, n, b, stride);
    static const char* const PLANS[] = {"wide", "fixed", "generic"};
    printf("ws %s lg=%u ov=%u req=%u plan=%s c=%u max_n=%zu cols=%u bytes=%zu largest=%s:%zu\n", mode, lg, ov, req, PLANS[plan], c, max_n, cols, bytes, BUF_NAMES[big],
           L.buf[big].count * L.buf[big].elem);
}

// what every plan must satisfy, whichever path takes it
static void common(const char* mode, uint32_t lg, uint32_t c, uint32_t nwin, uint32_t nb, uint32_t split, bool wide) {
    EXPECT(c >= 9 && c <= 17, "%s lg %u: window %u", mode, lg, c);
    EXPECT(nb == 1u << (c - 1), "%s lg %u: %u buckets at %u bits", mode, lg, nb, c);
    EXPECT(nwin == nwin_for(c) && nwin * c >= 255, "%s lg %u: %u windows of %u bits leave the carry out of the top digit no window", mode, lg, nwin, c);
    EXPECT((nwin - 1) * c <= 254, "%s lg %u: window %u of %u bits starts above the scalar and its carry", mode, lg, nwin - 1, c);
    EXPECT(split >= 1 && split <= BITSUM_MAX_SPLIT, "%s lg %u: bit-sum split %u", mode, lg, split);
    EXPECT(bitsum_threads(nb) == 64, "%s lg %u: the bit sums run one wave per workgroup", mode, lg);
    if (wide) return;  // (the wide path hands back its own 17 row / column sums per column: msm_wide.hip.h WIDE_SUMS)
    // the result buffer of a lane holds MSM_MAX_BATCH x 15 x 4 sums (ctx.hip): c x split per column, nwin x c x split for arbitrary bases
    EXPECT(c * split <= 15 * 4, "%s lg %u: %u sums per result", mode, lg, c * split);
    EXPECT(nwin * c * split <= MSM_MAX_BATCH * 15 * 4, "%s lg %u: %u sums of a generic MSM", mode, lg, nwin * c * split);
}

int main() {
    for (uint32_t lg = 0; lg <= MAX_LG; lg++) {
        const size_t n = (size_t)1 << lg;
        for (uint32_t ov : OVERRIDES) {
            const uint32_t c = msm_auto_window(n, ov);
            const uint32_t nwin = nwin_for(c), nb = 1u << (c - 1);
            const bool wide = msm_wide_applies(c, n) && n == msm_ws_len(n);
            const bool fused = !wide && msm_fused(true, nb);
            const bool sort2 = !wide && sort2_applies(msm_fused(true, nb), n, nb, nwin, n);
            const bool percol = fused && !sort2 && msm_scatter_per_launch((uint32_t)n, 2) == 1;
            const uint32_t split = bitsum_split(nb);
            const uint32_t sweeps = wide || fused ? 0 : (nb + SORT_LDS_BUCKETS - 1) / SORT_LDS_BUCKETS;
            common("fixed", lg, c, nwin, nb, split, wide);
            // 16 / 17-bit digits exist on the wide path only; the standard plan's digits are int16 planes, its entries hold
            // sign << 31 | window * stride + i
            EXPECT(c < 16 || wide, "fixed lg %u override %u: %u bits off the wide path", lg, ov, c);
            EXPECT(wide || nb <= 16384, "fixed lg %u override %u: digits of %u bits do not fit int16", lg, ov, c);
            EXPECT(wide || (uint64_t)nwin * n < (1ull << 31), "fixed lg %u override %u: table index reaches the sign bit", lg, ov);
            if (wide) {
                uint32_t ib = 0, fb = 0;
                EXPECT(msm_wide_shape(c, n, &ib, &fb) && ib >= 24 && ib <= 26 && fb >= 1 && fb <= 7 && ib + fb <= 31, "wide lg %u: ib %u fb %u", lg, ib, fb);
                EXPECT((uint64_t)nwin * n <= (1ull << ib) && (nb >> fb) <= 512, "wide lg %u: %u windows, ib %u, %u bins", lg, nwin, ib, nb >> fb);
                EXPECT(n >= MSM_WS_MIN_N, "wide lg %u: below the workspace floor", lg);
            }
            if (sort2) {
                EXPECT(fused && n >= ZK_SORT2_MIN_N, "sort2 at lg %u override %u", lg, ov);
                EXPECT((uint64_t)nwin * n <= (1u << 24), "sort2 at lg %u override %u: table indexes exceed the 24-bit field", lg, ov);
                EXPECT(nb >= 64 && nb / 64 <= CBINS_MAX, "sort2 at lg %u override %u: %u coarse bins", lg, ov, nb / 64);
            }
            // the fused plan's histogram: nb counters + 256 x 9 limbs of LDS, at most 64 KiB
            EXPECT(!fused || (nb + 256 * 9) * 4 <= 65536, "fixed lg %u override %u: %u LDS bytes", lg, ov, (nb + 256 * 9) * 4);
            // the defaults, as the comments state them
            if (ov == 0) {
                const uint32_t want = lg >= 22 ? 15 : lg >= 16 ? 16 : lg >= 14 ? lg - 5 : 9;
                EXPECT(c == want, "default window at lg %u: %u, the comments say %u", lg, c, want);
                EXPECT(wide == (lg >= 16 && lg <= 21), "default plan at lg %u: wide %d", lg, (int)wide);
                // (why tests/test_gpu_msm_plans.py selects both with ZK_OPT_MSM_WINDOW: no default plan reaches them)
                EXPECT(!sort2 && !percol, "default plan at lg %u reaches sort2 / the per-column scatter", lg);
            }
            if (ov >= 15 && n < MSM_WS_MIN_N) EXPECT(c == 14, "override %u at lg %u: %u bits below the workspace floor", ov, lg, c);
            if (ov >= 9 && ov <= 14) EXPECT(c == ov, "override %u at lg %u gives %u", ov, lg, c);
            for (uint32_t req : WIDTHS) {
                const uint32_t asked = msm_batch_width(n, req);
                const uint32_t pass = msm_max_pass(c, n, asked);
                EXPECT(asked >= 1 && asked <= MSM_MAX_BATCH && (req == 0 || asked == req), "width %u at lg %u: %u", req, lg, asked);
                EXPECT(req != 0 || asked == (lg >= 20 ? 1u : lg <= 12 ? MSM_MAX_BATCH : 1u << (20 - lg)), "default width at lg %u: %u", lg, asked);
                // msm_run refuses batch != 1 off the wide path when the plan is not fused
                EXPECT(pass == (wide || fused ? asked : 1u), "fixed lg %u override %u width %u: widest pass %u", lg, ov, req, pass);
                EXPECT(msm_max_pass(c, n, 0) == 1 && msm_max_pass(c, n, 100000) == (wide || fused ? MSM_MAX_BATCH : 1u), "widest pass out of range, lg %u", lg);
                printf("fixed lg=%u ov=%u req=%u c=%u nwin=%u nb=%u wide=%d fused=%d sort2=%d percol=%d split=%u sweeps=%u pass=%u\n", lg, ov, req, c, nwin,
                       nb, (int)wide, (int)fused, (int)sort2, (int)percol, split, sweeps, pass);
            }
        }
    }
    for (uint32_t lg = 0; lg <= MAX_LG; lg++) {
        const size_t n = (size_t)1 << lg;
        const uint32_t c = msm_auto_window_generic(msm_ws_len(n));
        const uint32_t nwin = nwin_for(c), nb = 1u << (c - 1), split = bitsum_split(nb);
        const uint32_t sweeps = (nb + SORT_LDS_BUCKETS - 1) / SORT_LDS_BUCKETS;
        common("generic", lg, c, nwin, nb, split, false);
        EXPECT(c <= 15 && nb <= 16384, "generic lg %u: %u bits (int16 digit planes)", lg, c);
        EXPECT(!msm_fused(false, nb) && !sort2_applies(msm_fused(false, nb), n, nb, nwin, 0), "generic lg %u takes a fixed-base sort", lg);
        const uint32_t want = lg >= 21 ? 15 : lg == 20 ? 14 : lg == 19 ? 13 : lg >= 16 ? 12 : lg >= 14 ? lg - 5 : 9;
        EXPECT(c == want, "generic window at lg %u: %u, the comments say %u", lg, c, want);
        printf("generic lg=%u ov=0 req=0 c=%u nwin=%u nb=%u wide=0 fused=0 sort2=0 percol=0 split=%u sweeps=%u pass=1\n", lg, c, nwin, nb, split, sweeps);
    }
    // the workspaces get_msm_ws makes: over the resident SRS of 2^lg points (window = the tables', columns = the widest pass of
    // the width asked for), and for arbitrary bases (one column)
    for (uint32_t lg = 0; lg <= MAX_LG; lg++) {
        const size_t n = (size_t)1 << lg;
        for (uint32_t ov : OVERRIDES)
            for (uint32_t req : WS_WIDTHS) {
                const uint32_t c = msm_auto_window(n, ov);
                workspace("fixed", lg, ov, req, true, c, n, msm_max_pass(c, n, msm_batch_width(msm_ws_len(n), req)));
            }
        workspace("generic", lg, 0, 0, false, msm_auto_window_generic(msm_ws_len(n)), 0, 1);
    }
    // arbitrary bases never run wide, though 15-bit windows over 2^21 points have the wide shape
    EXPECT(msm_auto_window_generic(1u << 21) == 15 && msm_wide_applies(15, 1u << 21) && msm_ws_plan(false, 15, 1u << 21) == MSM_PLAN_GENERIC, "generic 2^21");
    // lengths that are no power of two: the workspace is the next one, at least 1024
    EXPECT(msm_ws_len(0) == 1024 && msm_ws_len(1) == 1024 && msm_ws_len(1025) == 2048 && msm_ws_len((1u << 16) + 1) == (1u << 17), "msm_ws_len");
    EXPECT(msm_auto_window(1000) == 9 && msm_auto_window((1u << 16) - 1) == 10 && msm_auto_window((1u << 22) + 5) == 15, "windows of odd lengths");
    // sort2 at its threshold: a column of 2^18 takes it, one of 2^18 - 1 does not (the SRS being 2^19 either way)
    EXPECT(sort2_applies(true, 1u << 18, 4096, 20, 1u << 19) && !sort2_applies(true, (1u << 18) - 1, 4096, 20, 1u << 19), "sort2 threshold");
    EXPECT(!sort2_applies(true, 1u << 20, 4096, 21, 1u << 20) && msm_scatter_per_launch(1u << 20, 3) == 1, "13 bits at 2^20: the per-column scatter");
    EXPECT(msm_scatter_per_launch((1u << 18) - 1, 3) == 3, "short columns: one scatter launch");
    // the 4-partials cap: 14-bit windows would split 8 ways
    EXPECT(bitsum_split(256) == 1 && bitsum_split(1024) == 1 && bitsum_split(2048) == 2 && bitsum_split(4096) == 4 && bitsum_split(8192) == 4, "bit-sum splits");
    printf("msm plan: %d failures\n", fails);
    return fails ? 1 : 0;
}
