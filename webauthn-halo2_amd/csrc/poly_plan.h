// poly_plan.h — how the polynomial kernels cut an n-coefficient vector: the workgroups, Horner chains and sums of zk_eval and
// zk_eval_batch (poly.hip) and the chunks, blocks and scratch layout of a Kate division (prover_kernels.hip).  No HIP types and
// no device dependency: kernels and launchers include it, and tests/poly_plan_check.cpp walks it on the host (every n up to 2^16
// and around every power of two up to 2^26) without a GPU; tests/poly_cases.py restates it in Python.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZK_PLAN_FN __host__ __device__ inline
#else
#define ZK_PLAN_FN inline
#endif

namespace zk {

// ---------------------------------------------------------------- eval -----
static constexpr uint32_t EVAL_LANES = 256;        // lanes of a workgroup of every kernel here
static constexpr uint32_t EVAL_PER_LANE = 16;      // coefficients per lane up to the cap on the workgroups
static constexpr uint32_t EVAL_MAX_BLOCKS = 1024;  // most workgroups of one evaluation (what the second-level sums take)
static constexpr uint32_t EVAL_SMALL_ELEMS = 2048 + 8;  // the context's `small`: zk_eval's partial results and its result behind them

// workgroups of an evaluation.  scratch of launch_eval: at least eval_blocks(n) + 1 elements; result in scratch[eval_blocks(n)]
ZK_PLAN_FN uint32_t eval_blocks(uint32_t n) {
    uint32_t b = (n + EVAL_LANES * EVAL_PER_LANE - 1) / (EVAL_LANES * EVAL_PER_LANE);
    if (b < 1) b = 1;
    if (b > EVAL_MAX_BLOCKS) b = EVAL_MAX_BLOCKS;
    return b;
}
// zk_eval: lane t of the whole grid owns c[t + m S]
ZK_PLAN_FN uint32_t eval_stride(uint32_t n) { return eval_blocks(n) * EVAL_LANES; }
// zk_eval_batch: a workgroup owns 256 M consecutive coefficients; M = coefficients per lane (16 up to 2^22)
ZK_PLAN_FN uint32_t eval_batch_per_lane(uint32_t n) {
    const uint32_t blocks = eval_blocks(n);
    return (n + blocks * EVAL_LANES - 1) / (blocks * EVAL_LANES);
}
// lanes of batch workgroup b that hold a coefficient (a short last workgroup; 0: the workgroup holds none)
ZK_PLAN_FN uint32_t eval_batch_live(uint32_t n, uint32_t M, uint32_t b) {
    const uint32_t first = b * EVAL_LANES * M;
    const uint32_t left = n - (n < first ? n : first);
    return left < EVAL_LANES ? left : EVAL_LANES;
}

// ------------------------------------------------------- Kate division -----
#ifndef ZK_KD_L
#define ZK_KD_L 8
#endif
// shortest chunk (power of two): 8: 4x the lanes of 32 (a 2^19 division is 65 536 Horner chains of 8 instead of 16 384 of 32:
// -0.1 ms per k=19 proof, -0.3 ms at k=15..17)
static constexpr uint32_t KD_L_MIN = ZK_KD_L;
static constexpr uint32_t KD_BLK = 256;
static constexpr uint32_t KD_TOP = 1024;  // most blocks of a division: every block sums the aggregates above it directly
static constexpr uint32_t KD_MAX_BATCH = 6;  // divisions per launch (SHPLONK / GWC have at most six rotation sets)
// chunks of L coefficients, and blocks of KD_BLK chunks
ZK_PLAN_FN uint32_t kd_chunks(uint32_t n, uint32_t L) { return (n + L - 1) / L; }
ZK_PLAN_FN uint32_t kd_blocks(uint32_t m) { return (m + KD_BLK - 1) / KD_BLK; }
// chunk length of an n-coefficient division: the shortest that keeps the number of blocks within KD_TOP (8 up to 2^21,
// 16 at 2^22, ...)
ZK_PLAN_FN uint32_t kd_len(uint32_t n) {
    uint32_t L = KD_L_MIN;
    while (((n + L - 1) / L + KD_BLK - 1) / KD_BLK > KD_TOP) L <<= 1;
    return L;
}
// per-division scratch: (m unused) | suf[m] | agg[nblk] | tpow[nblk] | zpow[256]
ZK_PLAN_FN uint32_t kd_scratch_elems(uint32_t n) {
    const uint32_t L = kd_len(n), m = (n + L - 1) / L, nblk = (m + KD_BLK - 1) / KD_BLK;
    return 2 * m + 2 * nblk + 256;
}
// workgroups of kd_scan_kernel: one per block, one for zpow, and one per KD_BLK entries of tpow
ZK_PLAN_FN uint32_t kd_scan_grid(uint32_t nblk) { return nblk + 1 + (nblk + KD_BLK - 1) / KD_BLK; }

}  // namespace zk
