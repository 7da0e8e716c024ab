// pairing_check_ops.h — one case of tests/pairing_device_cases.py run through csrc/pairing.h: shared by the device kernel and the
// --host mode of tests/pairing_device_check.hip.  The record and result layouts are those of tests/pairing_device_cases.py.
//
// Case record (REC_WORDS 32-bit words): [0] op  [1] aux  [2] table index  [3] 0  [4 ..) a: an Fq12 (96 words; smaller operands
// from its start)  [100 ..) b: the same  [196 ..) p0: a G1 row (16 words)  [212 ..) p1.
// Result record (OUT_WORDS words): [0 .. 96) an Fq12 (smaller results from its start, the rest zero)  [96] a flag  [97] DONE | op.
#pragma once
#include <stdint.h>

#include "pairing.h"

namespace pairingcheck {
using namespace zk;

constexpr uint32_t F12_WORDS = 96, OPND = 4, REC_WORDS = OPND + 2 * F12_WORDS + 32, OUT_WORDS = F12_WORDS + 2, DONE = 0x600d0000u;
constexpr uint32_t OFF_A = OPND, OFF_B = OPND + F12_WORDS, OFF_P0 = OPND + 2 * F12_WORDS, OFF_P1 = OFF_P0 + 16;
constexpr uint32_t MAGIC_IN = 0x43524150u, MAGIC_OUT = 0x52524150u, MAGIC_TAB = 0x54524150u;
constexpr uint32_t MAX_TABLES = 16;
enum Op : uint32_t {
    OP_F2_MUL = 1, OP_F2_MUL_XI, OP_F2_MUL_FQ, OP_F2_INV,
    OP_F6_MUL = 10, OP_F6_MUL_01, OP_F6_MUL_V, OP_F6_INV,
    OP_F12_MUL = 20, OP_F12_SQR, OP_F12_INV, OP_F12_CONJ, OP_F12_FROB, OP_F12_MUL_LINE, OP_F12_POW_U, OP_F12_IS_ONE,
    OP_FQ_CANON = 40, OP_MILLER, OP_FEXP, OP_CHECK
};

ZK_PAIR_FN Fq rd_fq(const uint32_t* p) {
    Fq r;
    for (int i = 0; i < 8; i++) r.v[i] = p[i];
    return r;
}
ZK_PAIR_FN Fq2 rd_f2(const uint32_t* p) { return {rd_fq(p), rd_fq(p + 8)}; }
ZK_PAIR_FN Fq6 rd_f6(const uint32_t* p) { return {rd_f2(p), rd_f2(p + 16), rd_f2(p + 32)}; }
ZK_PAIR_FN Fq12 rd_f12(const uint32_t* p) { return {rd_f6(p), rd_f6(p + 48)}; }
ZK_PAIR_FN G1Affine rd_g1(const uint32_t* p) {
    G1Affine r;
    r.x = rd_fq(p);
    r.y = rd_fq(p + 8);
    return r;
}
ZK_PAIR_FN void wr_fq(uint32_t* p, const Fq& a) {
    for (int i = 0; i < 8; i++) p[i] = a.v[i];
}
ZK_PAIR_FN void wr_f2(uint32_t* p, const Fq2& a) {
    wr_fq(p, a.c0);
    wr_fq(p + 8, a.c1);
}
ZK_PAIR_FN void wr_f6(uint32_t* p, const Fq6& a) {
    wr_f2(p, a.c0);
    wr_f2(p + 16, a.c1);
    wr_f2(p + 32, a.c2);
}
ZK_PAIR_FN void wr_f12(uint32_t* p, const Fq12& a) {
    wr_f6(p, a.c0);
    wr_f6(p + 48, a.c1);
}

// rec: the REC_WORDS words of the case; tables: the PairingTables of the run (rec[2] is below their count: the harness checks
// every record before it runs one); out: the case's OUT_WORDS result words
ZK_PAIR_FN void run_case(const uint32_t* rec, const PairingTable* tables, uint32_t* out) {
    const uint32_t op = rec[0], aux = rec[1];
    const PairingTable& t = tables[rec[2]];
    const uint32_t *a = rec + OFF_A, *b = rec + OFF_B;
    for (uint32_t i = 0; i < OUT_WORDS; i++) out[i] = 0;
    switch (op) {
        case OP_F2_MUL: wr_f2(out, f2_mul(rd_f2(a), rd_f2(b))); break;
        case OP_F2_MUL_XI: wr_f2(out, f2_mul_xi(rd_f2(a))); break;
        case OP_F2_MUL_FQ: wr_f2(out, f2_mul_fq(rd_f2(a), rd_fq(b))); break;
        case OP_F2_INV: wr_f2(out, f2_inv(rd_f2(a))); break;
        case OP_F6_MUL: wr_f6(out, f6_mul(rd_f6(a), rd_f6(b))); break;
        case OP_F6_MUL_01: wr_f6(out, f6_mul_01(rd_f6(a), rd_f2(b), rd_f2(b + 16))); break;
        case OP_F6_MUL_V: wr_f6(out, f6_mul_v(rd_f6(a))); break;
        case OP_F6_INV: wr_f6(out, f6_inv(rd_f6(a))); break;
        case OP_F12_MUL: wr_f12(out, f12_mul(rd_f12(a), rd_f12(b))); break;
        case OP_F12_SQR: wr_f12(out, f12_sqr(rd_f12(a))); break;
        case OP_F12_INV: wr_f12(out, f12_inv(rd_f12(a))); break;
        case OP_F12_CONJ: wr_f12(out, f12_conj(rd_f12(a))); break;
        case OP_F12_FROB: wr_f12(out, f12_frobenius_with(rd_f12(a), t.gamma)); break;
        case OP_F12_MUL_LINE: wr_f12(out, f12_mul_line(rd_f12(a), t.line[(aux >> 8) & 1][aux & 0xff], rd_g1(rec + OFF_P0))); break;  // (the step is below PAIRING_STEPS: checked with the table index)
        case OP_F12_POW_U: wr_f12(out, f12_pow_u(rd_f12(a))); break;
        case OP_F12_IS_ONE: out[F12_WORDS] = f12_is_one(rd_f12(a)) ? 1u : 0u; break;
        case OP_FQ_CANON: out[F12_WORDS] = fq_is_canonical(rd_fq(a)) ? 1u : 0u; break;
        case OP_MILLER: wr_f12(out, miller_loop_lines(rd_g1(rec + OFF_P0), rd_g1(rec + OFF_P1), t)); break;
        case OP_FEXP: wr_f12(out, final_exponentiation_chain(rd_f12(a), t.gamma)); break;
        case OP_CHECK: out[F12_WORDS] = pairing_check_lines(rd_g1(rec + OFF_P0), rd_g1(rec + OFF_P1), t); break;
        default: break;
    }
    out[OUT_WORDS - 1] = DONE | op;
}

// what the harness refuses before it runs anything: a table index or a line step outside what it holds
inline bool record_in_bounds(const uint32_t* rec, uint32_t n_tables) {
    if (rec[2] >= n_tables) return false;
    if (rec[0] == OP_F12_MUL_LINE && ((rec[1] & 0xff) >= (uint32_t)PAIRING_STEPS || (rec[1] >> 9) != 0)) return false;
    return true;
}

}  // namespace pairingcheck
