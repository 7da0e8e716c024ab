// field_device_check.hip — runs the device forms of csrc/field.hip.h, field29.hip.h, ec.hip.h and ec29.hip.h on operands read
// from a file, one case per lane, and writes the raw result words to a file.  tests/test_gpu_field_device.py generates the
// cases, runs this once per build and compares with big integers and with the limb-exact model (tests/field29_model.py).
//
// One source, several binaries (build.sh): -DZK_MUL29_ASM=0|1|2, -DZK_MUL29_MASKRUN=0|1, -DZK_EC29_SQR=0|1, -DZK_EC29_FUSE=0|1.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I webauthn-halo2_amd/csrc tests/field_device_check.hip -o tests/field_device_check_a2
// Nothing of the library is linked; only the four headers are included.
//
// Case file (32-bit little-endian words): "ZKFC", n, REC_WORDS, 0, then n records of REC_WORDS words:
//   [0] op   [1] modulus (0 = Fr, 1 = Fq)   [2] aux (shuffle offset, chain length)   [3] 0   [4 ..] operand words
// The records are sorted by (op, modulus); every (op, modulus) run is one kernel, launched twice: in blocks of 64 and of 256
// lanes, the last block ragged.  Result file: "ZKFR", n, OUT_WORDS, 2, then the n x OUT_WORDS words of the 64-lane pass and
// those of the 256-lane pass.  Word OUT_WORDS - 1 of every result is DONE | op: a lane that did not run leaves 0xffffffff.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "field.hip.h"
#include "field29.hip.h"
#include "ec.hip.h"
#include "ec29.hip.h"
using namespace zk;

#define CHK(x)                                                                                      \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) {                                                                     \
            fprintf(stderr, "field_device_check: HIP error '%s' at line %d: %s\n", hipGetErrorString(e_), __LINE__, #x); \
            exit(2);                                                                                \
        }                                                                                           \
    } while (0)

constexpr uint32_t REC_WORDS = 100, OPND = 4, OUT_WORDS = 40, DONE = 0x600d0000u;
constexpr uint32_t MAGIC_IN = 0x43464b5au, MAGIC_OUT = 0x52464b5au;  // "ZKFC", "ZKFR"

enum Op : uint32_t {
    // A: field.hip.h
    OP_FE_ADD = 1, OP_FE_SUB, OP_FE_NEG, OP_FE_DBL, OP_FE_MUL, OP_FE_SQR, OP_FE_TO_MONT, OP_FE_FROM_MONT, OP_FE_INV, OP_REDUCE_ONCE,
    OP_REDUCE_ONCE_ASM, OP_FE_LOAD_STORE,
    // B: field29.hip.h
    OP_TO29 = 20, OP_TO29_X32, OP_FROM29, OP_MUL29_S, OP_MUL29_C, OP_SQR29_S, OP_SQR29_C, OP_MUL2ADD29_S, OP_MUL2ADD29_C,
    OP_MUL1ADD29_S, OP_MUL1ADD29_C, OP_MUL4ADD29_S, OP_MUL4ADD29_C, OP_MUL5ADD29_S, OP_MUL5ADD29_C, OP_ADD29, OP_NORM29, OP_IS_ZERO29,
    OP_STD_TO_INTERNAL, OP_INTERNAL_TO_STD,
    OP_SUB29_2_29 = 40, OP_SUB29_3_29, OP_SUB29_4_29, OP_SUB29_5_30, OP_SUB29_6_29, OP_SUB29_7_29, OP_SUB29_7_31, OP_SUB29_8_29,
    OP_SUB29_9_29, OP_SUB29_10_29, OP_SUB29_13_30, OP_SUB29_33_29, OP_SUB29_65_30,
    // C: ec.hip.h
    OP_G1X_DBL = 60, OP_G1X_DBL_AFFINE, OP_G1X_ADD_AFFINE, OP_G1X_ADD, OP_G1X_TO_JAC, OP_G1X_LOAD_STORE,
    // D: ec29.hip.h
    OP_G1X29_FROM_STD = 70, OP_G1X29_TO_STD, OP_G1X29_ADD_AFFINE_CS, OP_G1X29_ADD_AFFINE_CI, OP_G1X29_ADD_AFFINE_NS, OP_G1X29_ADD_AFFINE_NI,
    OP_G1X29_ADD_S, OP_G1X29_ADD_C, OP_G1X29_DBL_RARE, OP_G1X29_LOAD_STORE, OP_MUL29_CALL, OP_INTERNAL_TO_STD_CALL, OP_G1X29_SHFL_DOWN,
    OP_G1X29_CHAIN,
};

#define FIELD_OPS(X)                                                                                                                \
    X(OP_FE_ADD) X(OP_FE_SUB) X(OP_FE_NEG) X(OP_FE_DBL) X(OP_FE_MUL) X(OP_FE_SQR) X(OP_FE_TO_MONT) X(OP_FE_FROM_MONT) X(OP_FE_INV)  \
    X(OP_REDUCE_ONCE) X(OP_REDUCE_ONCE_ASM) X(OP_FE_LOAD_STORE) X(OP_TO29) X(OP_TO29_X32) X(OP_FROM29) X(OP_MUL29_S) X(OP_MUL29_C)  \
    X(OP_SQR29_S) X(OP_SQR29_C) X(OP_MUL2ADD29_S) X(OP_MUL2ADD29_C) X(OP_MUL1ADD29_S) X(OP_MUL1ADD29_C) X(OP_MUL4ADD29_S)           \
    X(OP_MUL4ADD29_C) X(OP_MUL5ADD29_S) X(OP_MUL5ADD29_C) X(OP_ADD29) X(OP_NORM29) X(OP_IS_ZERO29) X(OP_STD_TO_INTERNAL)            \
    X(OP_INTERNAL_TO_STD) X(OP_SUB29_2_29) X(OP_SUB29_3_29) X(OP_SUB29_4_29) X(OP_SUB29_5_30) X(OP_SUB29_6_29) X(OP_SUB29_7_29)     \
    X(OP_SUB29_7_31) X(OP_SUB29_8_29) X(OP_SUB29_9_29) X(OP_SUB29_10_29) X(OP_SUB29_13_30) X(OP_SUB29_33_29) X(OP_SUB29_65_30)
#define CURVE_OPS(X)                                                                                                                \
    X(OP_G1X_DBL) X(OP_G1X_DBL_AFFINE) X(OP_G1X_ADD_AFFINE) X(OP_G1X_ADD) X(OP_G1X_TO_JAC) X(OP_G1X_LOAD_STORE) X(OP_G1X29_FROM_STD) \
    X(OP_G1X29_TO_STD) X(OP_G1X29_ADD_AFFINE_CS) X(OP_G1X29_ADD_AFFINE_CI) X(OP_G1X29_ADD_AFFINE_NS) X(OP_G1X29_ADD_AFFINE_NI)       \
    X(OP_G1X29_ADD_S) X(OP_G1X29_ADD_C) X(OP_G1X29_DBL_RARE) X(OP_G1X29_LOAD_STORE) X(OP_MUL29_CALL) X(OP_INTERNAL_TO_STD_CALL)      \
    X(OP_G1X29_SHFL_DOWN) X(OP_G1X29_CHAIN)

template <class PRM>
__device__ __forceinline__ Fe<PRM> rd_fe(const uint32_t* p) {
    Fe<PRM> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = p[i];
    return r;
}
template <class PRM>
__device__ __forceinline__ void wr_fe(uint32_t* p, const Fe<PRM>& a) {
#pragma unroll
    for (int i = 0; i < 8; i++) p[i] = a.v[i];
}
template <class PRM>
__device__ __forceinline__ Fe29<PRM> rd_29(const uint32_t* p) {
    Fe29<PRM> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = p[i];
    return r;
}
template <class PRM>
__device__ __forceinline__ void wr_29(uint32_t* p, const Fe29<PRM>& a) {
#pragma unroll
    for (int i = 0; i < 9; i++) p[i] = a.l[i];
}

template <int K, bool SER, class PRM>
__device__ __forceinline__ void run_mulk(const uint32_t* in, uint32_t* out) {
    Fe29<PRM> a[K], b[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        a[j] = rd_29<PRM>(in + 9 * j);
        b[j] = rd_29<PRM>(in + 45 + 9 * j);
    }
    wr_29(out, mulKadd29<K, PRM, SER>(a, b));
}

// groups A and B: `in` points at the operand words of the lane's record, `out` at its OUT_WORDS result words (both 16-byte aligned)
template <uint32_t OP, class PRM>
__device__ __forceinline__ void run_field(const uint32_t* in, uint32_t* out) {
    typedef Fe<PRM> F;
    if constexpr (OP == OP_FE_ADD) wr_fe(out, fe_add(rd_fe<PRM>(in), rd_fe<PRM>(in + 8)));
    else if constexpr (OP == OP_FE_SUB) wr_fe(out, fe_sub(rd_fe<PRM>(in), rd_fe<PRM>(in + 8)));
    else if constexpr (OP == OP_FE_NEG) wr_fe(out, fe_neg(rd_fe<PRM>(in)));
    else if constexpr (OP == OP_FE_DBL) wr_fe(out, fe_dbl(rd_fe<PRM>(in)));
    else if constexpr (OP == OP_FE_MUL) wr_fe(out, fe_mul(rd_fe<PRM>(in), rd_fe<PRM>(in + 8)));
    else if constexpr (OP == OP_FE_SQR) wr_fe(out, fe_sqr(rd_fe<PRM>(in)));
    else if constexpr (OP == OP_FE_TO_MONT) wr_fe(out, fe_to_mont(rd_fe<PRM>(in)));
    else if constexpr (OP == OP_FE_FROM_MONT) wr_fe(out, fe_from_mont(rd_fe<PRM>(in)));
    else if constexpr (OP == OP_FE_INV) wr_fe(out, fe_inv(rd_fe<PRM>(in)));
    else if constexpr (OP == OP_REDUCE_ONCE) {
        F a = rd_fe<PRM>(in);
        reduce_once(a);
        wr_fe(out, a);
    } else if constexpr (OP == OP_REDUCE_ONCE_ASM) {
        F a = rd_fe<PRM>(in);
#if defined(__HIP_DEVICE_COMPILE__)
        zk_reduce_once_asm<PRM>(a.v);
#endif
        wr_fe(out, a);
    } else if constexpr (OP == OP_FE_LOAD_STORE) {
        fe_store(reinterpret_cast<F*>(out), fe_load(reinterpret_cast<const F*>(in)));
    } else if constexpr (OP == OP_TO29) wr_29(out, to29(rd_fe<PRM>(in)));
    else if constexpr (OP == OP_TO29_X32) wr_29(out, to29_x32(rd_fe<PRM>(in)));
    else if constexpr (OP == OP_FROM29) wr_fe(out, from29(rd_29<PRM>(in)));
    else if constexpr (OP == OP_MUL29_S) wr_29(out, mul29<PRM, true>(rd_29<PRM>(in), rd_29<PRM>(in + 9)));
    else if constexpr (OP == OP_MUL29_C) wr_29(out, mul29<PRM, false>(rd_29<PRM>(in), rd_29<PRM>(in + 9)));
    else if constexpr (OP == OP_SQR29_S) wr_29(out, sqr29<PRM, true>(rd_29<PRM>(in)));
    else if constexpr (OP == OP_SQR29_C) wr_29(out, sqr29<PRM, false>(rd_29<PRM>(in)));
    else if constexpr (OP == OP_MUL2ADD29_S)
        wr_29(out, mul2add29<PRM, true>(rd_29<PRM>(in), rd_29<PRM>(in + 9), rd_29<PRM>(in + 18), rd_29<PRM>(in + 27)));
    else if constexpr (OP == OP_MUL2ADD29_C)
        wr_29(out, mul2add29<PRM, false>(rd_29<PRM>(in), rd_29<PRM>(in + 9), rd_29<PRM>(in + 18), rd_29<PRM>(in + 27)));
    else if constexpr (OP == OP_MUL1ADD29_S) run_mulk<1, true, PRM>(in, out);
    else if constexpr (OP == OP_MUL1ADD29_C) run_mulk<1, false, PRM>(in, out);
    else if constexpr (OP == OP_MUL4ADD29_S) run_mulk<4, true, PRM>(in, out);
    else if constexpr (OP == OP_MUL4ADD29_C) run_mulk<4, false, PRM>(in, out);
    else if constexpr (OP == OP_MUL5ADD29_S) run_mulk<5, true, PRM>(in, out);
    else if constexpr (OP == OP_MUL5ADD29_C) run_mulk<5, false, PRM>(in, out);
    else if constexpr (OP == OP_ADD29) wr_29(out, add29(rd_29<PRM>(in), rd_29<PRM>(in + 9)));
    else if constexpr (OP == OP_NORM29) wr_29(out, norm29(rd_29<PRM>(in)));
    else if constexpr (OP == OP_IS_ZERO29) out[36] = is_zero29(rd_29<PRM>(in)) ? 1u : 0u;
    else if constexpr (OP == OP_STD_TO_INTERNAL) wr_29(out, std_to_internal(rd_fe<PRM>(in)));
    else if constexpr (OP == OP_INTERNAL_TO_STD) wr_fe(out, internal_to_std(rd_29<PRM>(in)));
#define SUB_CASE(K, E) else if constexpr (OP == OP_SUB29_##K##_##E) wr_29(out, sub29<K, E>(rd_29<PRM>(in), rd_29<PRM>(in + 9)));
    SUB_CASE(2, 29) SUB_CASE(3, 29) SUB_CASE(4, 29) SUB_CASE(5, 30) SUB_CASE(6, 29) SUB_CASE(7, 29) SUB_CASE(7, 31) SUB_CASE(8, 29)
    SUB_CASE(9, 29) SUB_CASE(10, 29) SUB_CASE(13, 30) SUB_CASE(33, 29) SUB_CASE(65, 30)
#undef SUB_CASE
    else static_assert(OP == 0, "not a field op");
}

__device__ __forceinline__ void wr_g1x29(uint32_t* out, const G1X29& a) {
    g1x29_store(reinterpret_cast<G1X29S*>(out), a);
    out[38] = a.inf ? 1u : 0u;
}

template <bool CHECK, bool INTERNAL>
__device__ __forceinline__ void run_add_affine29(const uint32_t* in, uint32_t* out) {
    G1X29 acc = g1x29_load(reinterpret_cast<const G1X29S*>(in));
    const bool ok = g1x29_add_affine<CHECK, INTERNAL>(acc, rd_fe<FqParams>(in + 36), rd_fe<FqParams>(in + 44));
    wr_g1x29(out, acc);
    out[36] = ok ? 1u : 0u;
    out[37] = is_zero29(acc.zz) ? 1u : 0u;
}

// groups C and D
template <uint32_t OP>
__device__ __forceinline__ void run_curve(const uint32_t* in, uint32_t aux, uint32_t* out) {
    if constexpr (OP == OP_G1X_DBL) g1x_store(reinterpret_cast<G1X*>(out), g1x_dbl(g1x_load(reinterpret_cast<const G1X*>(in))));
    else if constexpr (OP == OP_G1X_DBL_AFFINE)
        g1x_store(reinterpret_cast<G1X*>(out), g1x_dbl_affine(rd_fe<FqParams>(in), rd_fe<FqParams>(in + 8)));
    else if constexpr (OP == OP_G1X_ADD_AFFINE) {
        G1X acc = g1x_load(reinterpret_cast<const G1X*>(in));
        g1x_add_affine(acc, rd_fe<FqParams>(in + 32), rd_fe<FqParams>(in + 40));
        g1x_store(reinterpret_cast<G1X*>(out), acc);
    } else if constexpr (OP == OP_G1X_ADD) {
        G1X acc = g1x_load(reinterpret_cast<const G1X*>(in));
        g1x_add(acc, g1x_load(reinterpret_cast<const G1X*>(in + 32)));
        g1x_store(reinterpret_cast<G1X*>(out), acc);
    } else if constexpr (OP == OP_G1X_TO_JAC) {
        const G1Jac j = g1x_to_jac(g1x_load(reinterpret_cast<const G1X*>(in)));
        wr_fe(out, j.x);
        wr_fe(out + 8, j.y);
        wr_fe(out + 16, j.z);
    } else if constexpr (OP == OP_G1X_LOAD_STORE) g1x_store(reinterpret_cast<G1X*>(out), g1x_load(reinterpret_cast<const G1X*>(in)));
    else if constexpr (OP == OP_G1X29_FROM_STD) wr_g1x29(out, g1x29_from_std(g1x_load(reinterpret_cast<const G1X*>(in))));
    else if constexpr (OP == OP_G1X29_TO_STD)
        g1x_store(reinterpret_cast<G1X*>(out), g1x29_to_std(g1x29_load(reinterpret_cast<const G1X29S*>(in))));
    else if constexpr (OP == OP_G1X29_ADD_AFFINE_CS) run_add_affine29<true, false>(in, out);
    else if constexpr (OP == OP_G1X29_ADD_AFFINE_CI) run_add_affine29<true, true>(in, out);
    else if constexpr (OP == OP_G1X29_ADD_AFFINE_NS) run_add_affine29<false, false>(in, out);
    else if constexpr (OP == OP_G1X29_ADD_AFFINE_NI) run_add_affine29<false, true>(in, out);
    else if constexpr (OP == OP_G1X29_ADD_S || OP == OP_G1X29_ADD_C) {
        G1X29 acc = g1x29_load(reinterpret_cast<const G1X29S*>(in));
        const G1X29 b = g1x29_load(reinterpret_cast<const G1X29S*>(in + 36));
        g1x29_add<OP == OP_G1X29_ADD_S>(acc, b);
        wr_g1x29(out, acc);
    } else if constexpr (OP == OP_G1X29_DBL_RARE) {
        G1X29 acc = g1x29_load(reinterpret_cast<const G1X29S*>(in));
        g1x29_dbl_rare(acc);
        wr_g1x29(out, acc);
    } else if constexpr (OP == OP_G1X29_LOAD_STORE) wr_g1x29(out, g1x29_load(reinterpret_cast<const G1X29S*>(in)));
    else if constexpr (OP == OP_MUL29_CALL) wr_29(out, mul29_call(rd_29<FqParams>(in), rd_29<FqParams>(in + 9)));
    else if constexpr (OP == OP_INTERNAL_TO_STD_CALL) wr_fe(out, internal_to_std_call(rd_29<FqParams>(in)));
    else if constexpr (OP == OP_G1X29_CHAIN) {
        // aux steps of g1x29_add_affine from the identity over the record's five affine points, cyclically
        G1X29 acc = g1x29_identity();
        uint32_t ok = 1;
        for (uint32_t k = 0; k < aux; k++) {
            const uint32_t* pt = in + 16 * (k % 5);
            ok &= g1x29_add_affine(acc, rd_fe<FqParams>(pt), rd_fe<FqParams>(pt + 8)) ? 1u : 0u;
        }
        g1x_store(reinterpret_cast<G1X*>(out), g1x29_to_std(acc));
        out[36] = ok;
    } else static_assert(OP == 0, "not a curve op");
}

// one case per lane; `first` is the run's first record, `count` its length; the launch's last block is ragged
template <uint32_t OP, int MOD>
__global__ __launch_bounds__(256) void op_kernel(const uint32_t* __restrict__ recs, uint32_t* __restrict__ outs, uint32_t first, uint32_t count) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (OP == OP_G1X29_SHFL_DOWN) {
        // every lane of the wave takes part in the shuffle; a lane past the end holds the identity and stores nothing
        const bool live = t < count;
        const uint32_t* rec = recs + (size_t)(first + (live ? t : 0)) * REC_WORDS;
        G1X29 v = g1x29_load(reinterpret_cast<const G1X29S*>(rec + OPND));
        if (!live) v = g1x29_identity();
        const int off = (int)rec[2];
        const G1X29 r = g1x29_shfl_down(v, off);
        if (live) {
            uint32_t* out = outs + (size_t)(first + t) * OUT_WORDS;
            wr_g1x29(out, r);
            out[OUT_WORDS - 1] = DONE | OP;
        }
    } else {
        if (t >= count) return;
        const uint32_t* rec = recs + (size_t)(first + t) * REC_WORDS;
        uint32_t* out = outs + (size_t)(first + t) * OUT_WORDS;
        if constexpr (OP < OP_G1X_DBL) {
            if constexpr (MOD == 0) run_field<OP, FrParams>(rec + OPND, out);
            else run_field<OP, FqParams>(rec + OPND, out);
        } else {
            run_curve<OP>(rec + OPND, rec[2], out);
        }
        out[OUT_WORDS - 1] = DONE | OP;
    }
}

template <uint32_t OP, int MOD>
static void launch(const uint32_t* recs, uint32_t* outs, uint32_t first, uint32_t count, uint32_t block) {
    hipLaunchKernelGGL((op_kernel<OP, MOD>), dim3((count + block - 1) / block), dim3(block), 0, 0, recs, outs, first, count);
    CHK(hipGetLastError());
}

static bool dispatch(uint32_t op, uint32_t mod, const uint32_t* recs, uint32_t* outs, uint32_t first, uint32_t count, uint32_t block) {
    switch (op * 2 + mod) {
#define X(o)                                                   \
    case o * 2: launch<o, 0>(recs, outs, first, count, block); return true; \
    case o * 2 + 1: launch<o, 1>(recs, outs, first, count, block); return true;
        FIELD_OPS(X)
#undef X
#define X(o) \
    case o * 2 + 1: launch<o, 1>(recs, outs, first, count, block); return true;
        CURVE_OPS(X)
#undef X
    default: return false;
    }
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "field_device_check: cannot open %s\n", argv[1]);
        return 2;
    }
    uint32_t hdr[4];
    if (fread(hdr, 4, 4, f) != 4 || hdr[0] != MAGIC_IN || hdr[2] != REC_WORDS || hdr[1] == 0 || hdr[1] > (1u << 22)) {
        fprintf(stderr, "field_device_check: bad header in %s\n", argv[1]);
        return 2;
    }
    const uint32_t n = hdr[1];
    std::vector<uint32_t> recs((size_t)n * REC_WORDS);
    if (fread(recs.data(), 4, recs.size(), f) != recs.size()) {
        fprintf(stderr, "field_device_check: %s is shorter than its header says\n", argv[1]);
        return 2;
    }
    fclose(f);

    uint32_t *d_recs, *d_out;
    const size_t out_words = (size_t)n * OUT_WORDS;
    CHK(hipMalloc(&d_recs, recs.size() * 4));
    CHK(hipMalloc(&d_out, 2 * out_words * 4));
    CHK(hipMemcpy(d_recs, recs.data(), recs.size() * 4, hipMemcpyHostToDevice));
    CHK(hipMemset(d_out, 0xff, 2 * out_words * 4));

    const uint32_t blocks[2] = {64, 256};
    uint32_t runs = 0;
    for (uint32_t first = 0; first < n;) {
        const uint32_t op = recs[(size_t)first * REC_WORDS], mod = recs[(size_t)first * REC_WORDS + 1];
        uint32_t end = first + 1;
        while (end < n && recs[(size_t)end * REC_WORDS] == op && recs[(size_t)end * REC_WORDS + 1] == mod) end++;
        if (mod > 1) {
            fprintf(stderr, "field_device_check: record %u: modulus %u\n", first, mod);
            return 2;
        }
        if (op == OP_G1X29_CHAIN) {
            for (uint32_t i = first; i < end; i++) {
                if (recs[(size_t)i * REC_WORDS + 2] > 64) {
                    fprintf(stderr, "field_device_check: record %u: chain of %u steps\n", i, recs[(size_t)i * REC_WORDS + 2]);
                    return 2;
                }
            }
        }
        for (int b = 0; b < 2; b++) {
            if (!dispatch(op, mod, d_recs, d_out + b * out_words, first, end - first, blocks[b])) {
                fprintf(stderr, "field_device_check: record %u: unknown op %u for modulus %u\n", first, op, mod);
                return 2;
            }
        }
        runs++;
        first = end;
    }
    CHK(hipDeviceSynchronize());
    std::vector<uint32_t> out(2 * out_words);
    CHK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    CHK(hipFree(d_recs));
    CHK(hipFree(d_out));

    FILE* g = fopen(argv[2], "wb");
    if (!g) {
        fprintf(stderr, "field_device_check: cannot create %s\n", argv[2]);
        return 2;
    }
    const uint32_t ohdr[4] = {MAGIC_OUT, n, OUT_WORDS, 2};
    if (fwrite(ohdr, 4, 4, g) != 4 || fwrite(out.data(), 4, out.size(), g) != out.size() || fclose(g) != 0) {
        fprintf(stderr, "field_device_check: short write to %s\n", argv[2]);
        return 2;
    }
    printf("field_device_check: %u cases in %u runs, ZK_MUL29_ASM=%d ZK_MUL29_MASKRUN=%d ZK_EC29_SQR=%d ZK_EC29_FUSE=%d\n", n, runs,
           ZK_MUL29_ASM, ZK_MUL29_MASKRUN, ZK_EC29_SQR, ZK_EC29_FUSE);
    return 0;
}
