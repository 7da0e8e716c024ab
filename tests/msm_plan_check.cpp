// Host-only check of the MSM plan rules (csrc/msm_plan.h): no device is touched.  For both modes, every log n in 0 .. 26, every
// ZK_OPT_MSM_WINDOW in {0, 9 .. 17} and pass widths {default, 1, 3, 256} it prints one line — window, windows, buckets, wide /
// fused / sort2 / per-column scatter, bit-sum split, sweeps of the swept sort, widest pass — which tests/test_msm_plan.py compares
// with the Python restatement (tests/msm_cases.py), and it asserts what the kernels rely on and what the comments promise.
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
