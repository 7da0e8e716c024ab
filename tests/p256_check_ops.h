// p256_check_ops.h — one case of tests/p256_cases.py run through csrc/p256.hip.h: shared by the CPU harness
// (tests/p256_host_check.cpp) and the device harness (tests/p256_device_check.hip).  The record and result layouts are those of
// tests/p256_cases.py.
#pragma once
#include <stdint.h>

#include "p256.hip.h"

namespace p256check {
using namespace zk;

constexpr uint32_t REC_WORDS = 56, OPND = 4, OUT_WORDS = 26, DONE = 0x600d0000u;
constexpr uint32_t MAGIC_IN = 0x43503235u, MAGIC_OUT = 0x52503235u;
enum Op : uint32_t { OP_ADD = 1, OP_SUB, OP_NEG, OP_MUL, OP_SQR, OP_TO_MONT, OP_FROM_MONT, OP_INV, OP_DBL = 20, OP_ADD_MIXED, OP_ADD_FULL, OP_XCMP = 30 };

template <class M>
P256_FN P256Fe<M> rd(const uint32_t* p) {
    P256Fe<M> r;
    for (int i = 0; i < 8; i++) r.v[i] = p[i];
    return r;
}
template <class M>
P256_FN void wr(uint32_t* p, const P256Fe<M>& a) {
    for (int i = 0; i < 8; i++) p[i] = a.v[i];
}
P256_FN P256Jac rd_jac(const uint32_t* p) {
    P256Jac r;
    r.X = rd<P256FpPrm>(p);
    r.Y = rd<P256FpPrm>(p + 8);
    r.Z = rd<P256FpPrm>(p + 16);
    return r;
}
P256_FN void wr_jac(uint32_t* p, const P256Jac& a) {
    wr(p, a.X);
    wr(p + 8, a.Y);
    wr(p + 16, a.Z);
}

template <class M>
P256_FN void run_field(uint32_t op, const uint32_t* in, uint32_t* out) {
    const P256Fe<M> a = rd<M>(in), b = rd<M>(in + 8);
    switch (op) {
        case OP_ADD: wr(out, p256_add(a, b)); break;
        case OP_SUB: wr(out, p256_sub(a, b)); break;
        case OP_NEG: wr(out, p256_neg(a)); break;
        case OP_MUL: wr(out, p256_mul(a, b)); break;
        case OP_SQR: wr(out, p256_sqr(a)); break;
        case OP_TO_MONT: wr(out, p256_to_mont(a)); break;
        case OP_FROM_MONT: wr(out, p256_from_mont(a)); break;
        case OP_INV: wr(out, p256_inv(a)); break;
        default: break;
    }
}

// rec: the REC_WORDS words of the case; out: its OUT_WORDS result words
P256_FN void run_case(const uint32_t* rec, uint32_t* out) {
    const uint32_t op = rec[0], mod = rec[1];
    const uint32_t* in = rec + OPND;
    for (uint32_t i = 0; i < OUT_WORDS; i++) out[i] = 0;
    if (op < OP_DBL) {
        if (mod == 0) run_field<P256FpPrm>(op, in, out);
        else run_field<P256FnPrm>(op, in, out);
    } else if (op == OP_DBL) {
        wr_jac(out, p256_dbl(rd_jac(in)));
    } else if (op == OP_ADD_MIXED) {
        P256Affine q;
        q.x = rd<P256FpPrm>(in + 24);
        q.y = rd<P256FpPrm>(in + 32);
        wr_jac(out, p256_add_mixed(rd_jac(in), q));
    } else if (op == OP_ADD_FULL) {
        wr_jac(out, p256_add_full(rd_jac(in), rd_jac(in + 24)));
    } else if (op == OP_XCMP) {
        uint32_t r[8];
        for (int i = 0; i < 8; i++) r[i] = in[16 + i];
        out[24] = p256_x_matches(rd<P256FpPrm>(in), rd<P256FpPrm>(in + 8), r) ? 1u : 0u;
    }
    out[OUT_WORDS - 1] = DONE | op;
}

}  // namespace p256check
