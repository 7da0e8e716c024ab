// Host-only check of the shapes of the polynomial kernels (csrc/poly_plan.h): the workgroups, strides and chains of zk_eval and
// zk_eval_batch, the chunks, blocks and scratch layout of zk_kate_division.  No device is touched.
// Usage: poly_plan_check [n ...] — one line per length given (tests/test_poly_cases.py compares them with the Python restatement
// of tests/poly_cases.py), then the walk over every n in 1 .. 2^16 and every n = 2^j + d, j in 16 .. 26, d in -8 .. 8.
#include <cstdio>
#include <cstdlib>
#include "poly_plan.h"
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

struct Shape {
    uint32_t blocks, S, M, wg, live, L, m, nblk, scratch;
};

static Shape shape_of(uint32_t n) {
    Shape s;
    s.blocks = eval_blocks(n);
    s.S = eval_stride(n);
    s.M = eval_batch_per_lane(n);
    s.wg = 0;  // batch workgroups that hold a coefficient, counted as the kernel sees them
    s.live = 0;
    for (uint32_t b = 0; b < s.blocks; b++) {
        const uint32_t lv = eval_batch_live(n, s.M, b);
        if (lv) {
            s.wg++;
            s.live = lv;
        }
    }
    s.L = kd_len(n);
    s.m = kd_chunks(n, s.L);
    s.nblk = kd_blocks(s.m);
    s.scratch = kd_scratch_elems(n);
    return s;
}

static void check(uint32_t n) {
    const Shape s = shape_of(n);
    const uint64_t N = n;
    // ---- zk_eval: lane t < S owns c[t + k S]
    EXPECT(s.blocks >= 1 && s.blocks <= EVAL_MAX_BLOCKS, "n %u: %u workgroups", n, s.blocks);
    EXPECT(s.S == s.blocks * EVAL_LANES, "n %u: stride %u", n, s.S);
    EXPECT((uint64_t)s.S * ((N + s.S - 1) / s.S) >= N, "n %u: the chains of stride %u do not reach n", n, s.S);
    EXPECT(s.blocks + 1 <= EVAL_SMALL_ELEMS, "n %u: %u partial results and the result overrun the context's small", n, s.blocks);
    // ---- zk_eval_batch: workgroup b owns [256 M b, 256 M (b + 1))
    const uint64_t per = (uint64_t)EVAL_LANES * s.M;
    EXPECT(s.M >= 1 && per * s.blocks >= N, "n %u: 256 x %u x %u < n", n, s.M, s.blocks);
    EXPECT(per * s.blocks <= 0xffffffffull, "n %u: the kernel's 32-bit indexes wrap", n);
    EXPECT(s.wg >= 1 && s.wg <= s.blocks, "n %u: %u non-empty workgroups of %u", n, s.wg, s.blocks);
    EXPECT(per * s.wg >= N && per * (s.wg - 1) < N, "n %u: %u non-empty workgroups do not cover [0, n) exactly", n, s.wg);
    // the non-empty ones are the first wg, every one before the last is full, and the lanes' chains add up to the rest
    uint64_t covered = 0;
    for (uint32_t b = 0; b < s.blocks; b++) {
        const uint32_t lv = eval_batch_live(n, s.M, b);
        EXPECT((lv != 0) == (b < s.wg), "n %u: workgroup %u has %u live lanes", n, b, lv);
        if (!lv) continue;
        const uint64_t first = per * b, span = (N - first < per) ? N - first : per;
        EXPECT(first == covered, "n %u: workgroup %u starts at %llu, %llu covered", n, b, (unsigned long long)first, (unsigned long long)covered);
        EXPECT(lv == (span < EVAL_LANES ? span : EVAL_LANES), "n %u: workgroup %u: %u live lanes over %llu coefficients", n, b, lv, (unsigned long long)span);
        uint64_t chains = 0;
        for (uint32_t t = 0; t < lv; t++) chains += (span - 1 - t) / EVAL_LANES + 1;
        EXPECT(chains == span, "n %u: workgroup %u: chains hold %llu of %llu", n, b, (unsigned long long)chains, (unsigned long long)span);
        covered += span;
    }
    EXPECT(covered == N, "n %u: the workgroups cover %llu", n, (unsigned long long)covered);
    // ---- zk_kate_division
    EXPECT(s.L >= KD_L_MIN && (s.L & (s.L - 1)) == 0, "n %u: chunk length %u", n, s.L);
    EXPECT(s.L == KD_L_MIN || kd_blocks(kd_chunks(n, s.L / 2)) > KD_TOP, "n %u: chunk length %u is not the shortest", n, s.L);
    EXPECT((uint64_t)s.m * s.L >= N && (uint64_t)(s.m - 1) * s.L < N, "n %u: %u chunks of %u", n, s.m, s.L);
    EXPECT((uint64_t)s.nblk * KD_BLK >= s.m && (uint64_t)(s.nblk - 1) * KD_BLK < s.m, "n %u: %u blocks for %u chunks", n, s.nblk, s.m);
    EXPECT(s.nblk >= 1 && s.nblk <= KD_TOP, "n %u: %u blocks", n, s.nblk);
    // exponents: tpow[j], j < nblk, is made from ten squarings' worth of bits; zpow[i], i < 256, from eight
    EXPECT(s.nblk - 1 < (1u << 10) && KD_BLK - 1 < (1u << 8), "n %u: a table exponent has more bits than its powers", n);
    // the table workgroups behind the blocks write every entry of tpow
    const uint32_t grid = kd_scan_grid(s.nblk);
    EXPECT(grid > s.nblk && (uint64_t)(grid - s.nblk - 1) * KD_BLK >= s.nblk, "n %u: a grid of %u leaves entries of tpow unwritten", n, grid);
    // layout: (m unused) | suf[m] | agg[nblk] | tpow[nblk] | zpow[256]
    const uint64_t suf = s.m, agg = suf + s.m, tpow = agg + s.nblk, zpow = tpow + s.nblk, end = zpow + KD_BLK;
    EXPECT(end <= s.scratch, "n %u: the layout ends at %llu, the scratch has %u", n, (unsigned long long)end, s.scratch);
    EXPECT((uint64_t)KD_MAX_BATCH * s.scratch <= 0xffffffffull, "n %u: six divisions' scratch wraps 32 bits", n);
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; i++) {
        const uint32_t n = (uint32_t)strtoul(argv[i], nullptr, 10);
        if (n < 1 || n > (1u << 26)) {
            printf("FAILED: length %s out of range\n", argv[i]);
            fails++;
            continue;
        }
        const Shape s = shape_of(n);
        printf("n=%u blocks=%u S=%u M=%u wg=%u live=%u L=%u m=%u nblk=%u scratch=%u\n", n, s.blocks, s.S, s.M, s.wg, s.live, s.L, s.m,
               s.nblk, s.scratch);
        check(n);
    }
    unsigned long walked = 0;
    for (uint32_t n = 1; n <= (1u << 16); n++, walked++) check(n);
    for (uint32_t j = 16; j <= 26; j++)
        for (int d = -8; d <= 8; d++) {
            const uint64_t n = (uint64_t(1) << j) + d;
            if (n <= (1u << 16) || n > (1u << 26)) continue;  // (walked above; above what zk_kate_division accepts)
            check((uint32_t)n);
            walked++;
        }
    // the documented landmarks
    EXPECT(eval_batch_per_lane(1u << 22) == 16 && eval_batch_per_lane((1u << 22) + 1) == 17, "M around 2^22");
    EXPECT(kd_len(1u << 21) == 8 && kd_len((1u << 21) + 1) == 16 && kd_len(1u << 22) == 16 && kd_len(1u << 26) == 256, "KD_L landmarks");
    EXPECT(kd_blocks(kd_chunks(1u << 21, 8)) == 1024 && kd_blocks(kd_chunks((1u << 19) + 1, 8)) == 257, "block landmarks");
    printf("poly plan: %lu lengths walked, %d failures\n", walked, fails);
    return fails ? 1 : 0;
}
