// Host-only check of the NTT pass planner (csrc/ntt_plan.h) over every transform size the entry points accept and every value of
// ZK_OPT_NTT_MAX_RADIX_LOG2: no device is touched.  Usage: ntt_plan_check [capacity] — `capacity` (default: the shared constant
// NTT_MAX_PASSES, the size of the array ntt_run plans into) lets the test show what a smaller array would have overrun.
#include <cstdio>
#include <cstdlib>
#include "ntt_plan.h"
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

// option 0, as the comment in ntt_plan.h states the plans: 8 / 8 on tile 9 up to 2^16, 9 / 9 on tile 10 up to 2^18, 10 / 10 on
// tile 11 up to 2^20, passes of at most 2^7 on tile 9 above
struct Row {
    uint32_t tile, passes, bits[4];
};
static const Row DEFAULT_PLANS[NTT_MAX_LOG_N + 1] = {
    {9, 0, {0, 0, 0, 0}},   // 2^0: nothing to launch
    {9, 1, {1, 0, 0, 0}},   {9, 1, {2, 0, 0, 0}},   {9, 1, {3, 0, 0, 0}},   {9, 1, {4, 0, 0, 0}},
    {9, 1, {5, 0, 0, 0}},   {9, 1, {6, 0, 0, 0}},   {9, 1, {7, 0, 0, 0}},   {9, 1, {8, 0, 0, 0}},
    {9, 2, {5, 4, 0, 0}},   {9, 2, {5, 5, 0, 0}},   {9, 2, {6, 5, 0, 0}},   {9, 2, {6, 6, 0, 0}},
    {9, 2, {7, 6, 0, 0}},   {9, 2, {7, 7, 0, 0}},   {9, 2, {8, 7, 0, 0}},   {9, 2, {8, 8, 0, 0}},    // .. 2^16
    {10, 2, {9, 8, 0, 0}},  {10, 2, {9, 9, 0, 0}},                                                  // 2^17, 2^18
    {11, 2, {10, 9, 0, 0}}, {11, 2, {10, 10, 0, 0}},                                                // 2^19, 2^20
    {9, 3, {7, 7, 7, 0}},   {9, 4, {6, 6, 5, 5}},   {9, 4, {6, 6, 6, 5}},   {9, 4, {6, 6, 6, 6}},
    {9, 4, {7, 6, 6, 6}},   {9, 4, {7, 7, 6, 6}},                                                   // 2^21 .. 2^26
};

int main(int argc, char** argv) {
    static_assert(sizeof(NttPlan().bits) / sizeof(uint32_t) == NTT_MAX_PASSES, "the plan's array is sized by the shared constant");
    const uint32_t capacity = argc > 1 ? (uint32_t)atoi(argv[1]) : NTT_MAX_PASSES;
    for (uint32_t opt = 0; opt <= NTT_MAX_RADIX_LOG2; opt++) {
        for (uint32_t log_n = 0; log_n <= NTT_MAX_LOG_N; log_n++) {
            NttPlan pl;
            const bool ok = ntt_make_plan(log_n, opt, &pl);
            EXPECT(ok, "no plan for option %u, log_n %u", opt, log_n);
            if (!ok) continue;
            EXPECT(pl.passes <= capacity, "option %u, log_n %u: %u passes overrun an array of %u", opt, log_n, pl.passes, capacity);
            EXPECT(pl.tile_log >= NTT_TILE_LOG_DEFAULT && pl.tile_log <= NTT_TILE_LOG_MAX, "option %u, log_n %u: tile %u", opt, log_n, pl.tile_log);
            if (opt) {
                // an explicit radix takes the smallest tile that holds it, and the fewest passes that respect it
                EXPECT(pl.tile_log == (opt < 9 ? 9 : opt), "option %u, log_n %u: tile %u", opt, log_n, pl.tile_log);
                EXPECT(pl.passes == (log_n + opt - 1) / opt, "option %u, log_n %u: %u passes", opt, log_n, pl.passes);
            }
            uint32_t sum = 0;
            for (uint32_t p = 0; p < pl.passes && p < NTT_MAX_PASSES; p++) {
                const uint32_t b = pl.bits[p];
                sum += b;
                EXPECT(b >= 1, "option %u, log_n %u: pass %u has radix 2^%u", opt, log_n, p, b);
                EXPECT(b <= pl.tile_log, "option %u, log_n %u: pass %u radix 2^%u exceeds tile 2^%u", opt, log_n, p, b, pl.tile_log);
                EXPECT(opt == 0 || b <= opt, "option %u, log_n %u: pass %u radix 2^%u exceeds the requested maximum", opt, log_n, p, b);
                EXPECT(p == 0 || b <= pl.bits[p - 1], "option %u, log_n %u: radices not in descending order", opt, log_n);
                EXPECT(pl.bits[0] - b <= 1, "option %u, log_n %u: radices not as even as possible", opt, log_n);
            }
            EXPECT(sum == log_n, "option %u, log_n %u: radices sum to %u", opt, log_n, sum);
            if (opt == 0) {
                const Row& want = DEFAULT_PLANS[log_n];
                EXPECT(pl.tile_log == want.tile && pl.passes == want.passes, "default plan of log_n %u: tile %u, %u passes", log_n, pl.tile_log,
                       pl.passes);
                for (uint32_t p = 0; p < want.passes && p < pl.passes; p++)
                    EXPECT(pl.bits[p] == want.bits[p], "default plan of log_n %u: pass %u is 2^%u, want 2^%u", log_n, p, pl.bits[p], want.bits[p]);
            }
        }
    }
    // out of range: refused, nothing planned
    NttPlan pl;
    EXPECT(!ntt_make_plan(NTT_MAX_LOG_N + 1, 0, &pl), "log_n 27 accepted");
    EXPECT(!ntt_make_plan(10, NTT_MAX_RADIX_LOG2 + 1, &pl), "option 12 accepted");
    // the bounded planner itself: never writes past `cap`
    uint32_t small[3] = {0, 0, 0xDEADBEEFu};
    EXPECT(ntt_plan(9, 1, small, 2) == -1 && small[0] == 0 && small[2] == 0xDEADBEEFu, "ntt_plan wrote past its capacity");
    EXPECT(ntt_plan(9, 5, small, 2) == 2 && small[0] == 5 && small[1] == 4 && small[2] == 0xDEADBEEFu, "ntt_plan(9, 5)");
    // a build that pins another tile keeps it, with the old default radix, and clamps an explicit radix to it
    EXPECT(ntt_make_plan(20, 0, &pl, 10) && pl.tile_log == 10 && pl.passes == 3 && pl.bits[0] == 7, "pinned tile 10, default radix");
    EXPECT(ntt_make_plan(20, 11, &pl, 10) && pl.tile_log == 10 && pl.passes == 2 && pl.bits[0] == 10, "pinned tile 10, radix clamped");
    printf("ntt plan: %d failures\n", fails);
    return fails ? 1 : 0;
}
