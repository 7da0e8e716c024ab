// pairing.h — BN254 G2 and the optimal-ate pairing: the KZG check of zk_verify / zk_verify_batch on the host, and the one copy
// of the per-check arithmetic that the device form (pairing.hip: zk_pairing_check_batch, one check per lane) compiles too.
//
// Fq2 = Fq[u] / (u^2 + 1), Fq6 = Fq2[v] / (v^3 - xi), Fq12 = Fq6[w] / (w^2 - v), xi = 9 + u: halo2curves bn256's tower.
// G2 is the D-type twist y^2 = x^3 + 3 / xi over Fq2, untwisted by (x, y) -> (x w^2, y w^3).  The Miller loop runs over
// the bits of 6u + 2 (u = 4965661367192848881) in affine coordinates, followed by the two Frobenius lines of the optimal
// ate pairing; the final exponentiation is the easy part (p^6 - 1)(p^2 + 1) and the hard part (p^4 - p^2 + 1) / r.
// Host and device: the tower, the Frobenius map (its constants are an argument: the device reads them as data), the line
// evaluation, the Miller loop over PREPARED lines (pairing_prepare walks T once per G2 point on the host and keeps every
// step's slope and constant, so the evaluation inverts nothing and does not depend on G2 arithmetic), and a final
// exponentiation without a table (final_exponentiation_chain: three powers by u and the Frobenius maps); and, for a check that
// brings its own G2 point (zk_pairing_check_each, zk_srs_contribution_check_batch), inversion-free G2 arithmetic in Jacobian
// coordinates, the subgroup test on it and a Miller loop that walks that point while it evaluates (miller_loop_walk).  Host
// only: affine G2 arithmetic, the table of constants, multi_miller_loop and final_exponentiation — the latter takes the hard part as
// one multi-exponentiation of f, f^p, f^p^2, f^p^3 by the base-p digits of the exponent through a 16-entry Fq12 table, which a
// lane could only keep in scratch.  The same Fq2 / G2 helpers serve the SRS file's G2 half (serde.hip).
// On the device the Fq2 / Fq6 / Fq12 products are calls, not copies per use (ZK_PAIR_MULFN): inlined, a check is about
// 33 000 field-product sites and many times the instruction cache.
#pragma once
#include <string.h>

#include <vector>

#include "ec.hip.h"
#include "field.hip.h"
#include "g1_codec.hip.h"
#include "hostutil.h"

#ifndef ZK_PAIRING_VALID  // (include/zkmi355.h defines the same four: this header also stands alone)
#define ZK_PAIRING_VALID 0
#define ZK_PAIRING_RANGE 1
#define ZK_PAIRING_OFF_CURVE 2
#define ZK_PAIRING_MISMATCH 3
#endif
#ifndef ZK_PAIRING_G2
#define ZK_PAIRING_G2 4
#endif
#ifndef ZK_SRS_CONTRIB_SAME_SECRET
#define ZK_SRS_CONTRIB_SAME_SECRET 1u
#define ZK_SRS_CONTRIB_LINKS 2u
#define ZK_SRS_CONTRIB_NONTRIVIAL 4u
#endif

#define ZK_PAIR_FN __host__ __device__ inline
#if defined(__HIP_DEVICE_COMPILE__)
#define ZK_PAIR_MULFN __host__ __device__ __noinline__ inline
#else
#define ZK_PAIR_MULFN __host__ __device__ inline
#endif

namespace zk {

ZK_PAIR_FN bool fq_is_canonical(const Fq& a) { return a.below_modulus(); }  // (fq_small, the G1 curve test: g1_codec.hip.h)
// the inverse; one value whichever way it is found (the host's binary Euclid, the device's Fermat power)
ZK_PAIR_FN Fq fq_inv_any(const Fq& a) {
#if defined(__HIP_DEVICE_COMPILE__)
    return fe_inv(a);
#else
    return fe_inv_fast(a);
#endif
}

// ---- Fq2 and the twist y^2 = x^3 + 3 / (9 + u) ---------------------------------------------------------------------
struct Fq2 {
    Fq c0, c1;
};
ZK_PAIR_FN Fq2 f2_add(const Fq2& a, const Fq2& b) { return {fe_add(a.c0, b.c0), fe_add(a.c1, b.c1)}; }
ZK_PAIR_FN Fq2 f2_sub(const Fq2& a, const Fq2& b) { return {fe_sub(a.c0, b.c0), fe_sub(a.c1, b.c1)}; }
ZK_PAIR_FN Fq2 f2_neg(const Fq2& a) { return {fe_neg(a.c0), fe_neg(a.c1)}; }
ZK_PAIR_MULFN Fq2 f2_mul(const Fq2& a, const Fq2& b) {  // Karatsuba over u^2 = -1
    const Fq t0 = fe_mul(a.c0, b.c0), t1 = fe_mul(a.c1, b.c1);
    return {fe_sub(t0, t1), fe_sub(fe_sub(fe_mul(fe_add(a.c0, a.c1), fe_add(b.c0, b.c1)), t0), t1)};
}
ZK_PAIR_FN Fq2 f2_mul_fq(const Fq2& a, const Fq& s) { return {fe_mul(a.c0, s), fe_mul(a.c1, s)}; }
ZK_PAIR_FN Fq2 f2_conj(const Fq2& a) { return {a.c0, fe_neg(a.c1)}; }
ZK_PAIR_FN Fq2 f2_inv(const Fq2& a) {
    const Fq d = fq_inv_any(fe_add(fe_sqr(a.c0), fe_sqr(a.c1)));
    return {fe_mul(a.c0, d), fe_neg(fe_mul(a.c1, d))};
}
ZK_PAIR_FN bool f2_is_zero(const Fq2& a) { return a.c0.is_zero() && a.c1.is_zero(); }
ZK_PAIR_FN bool f2_eq(const Fq2& a, const Fq2& b) { return a.c0 == b.c0 && a.c1 == b.c1; }
ZK_PAIR_FN Fq2 f2_small(uint32_t a, uint32_t b) { return {fq_small(a), fq_small(b)}; }
ZK_PAIR_FN Fq2 f2_one() { return {Fq::one(), Fq::zero()}; }
ZK_PAIR_FN Fq2 f2_zero() { return {Fq::zero(), Fq::zero()}; }
ZK_PAIR_FN Fq2 f2_mul_xi(const Fq2& a) {  // a (9 + u) = (9 a0 - a1) + (a0 + 9 a1) u, 9 x = 8 x + x
    const Fq n0 = fe_add(fe_dbl(fe_dbl(fe_dbl(a.c0))), a.c0), n1 = fe_add(fe_dbl(fe_dbl(fe_dbl(a.c1))), a.c1);
    return {fe_sub(n0, a.c1), fe_add(a.c0, n1)};
}
inline Fq2 f2_twist_b() { return f2_mul(f2_small(3, 0), f2_inv(f2_small(9, 1))); }
// a^e, e as 8 little-endian 32-bit words
inline Fq2 f2_pow(const Fq2& a, const uint32_t e[8]) {
    Fq2 acc = f2_one();
    for (int i = 255; i >= 0; i--) {
        acc = f2_mul(acc, acc);
        if ((e[i >> 5] >> (i & 31)) & 1) acc = f2_mul(acc, a);
    }
    return acc;
}

struct G2A {
    Fq2 x, y;
    bool inf;
};
inline G2A g2_add(const G2A& a, const G2A& b) {
    if (a.inf) return b;
    if (b.inf) return a;
    Fq2 lam;
    if (f2_eq(a.x, b.x)) {
        if (!f2_eq(a.y, b.y)) return G2A{a.x, a.y, true};
        lam = f2_mul(f2_mul(f2_small(3, 0), f2_mul(a.x, a.x)), f2_inv(f2_add(a.y, a.y)));
    } else {
        lam = f2_mul(f2_sub(b.y, a.y), f2_inv(f2_sub(b.x, a.x)));
    }
    G2A r;
    r.inf = false;
    r.x = f2_sub(f2_sub(f2_mul(lam, lam), a.x), b.x);
    r.y = f2_sub(f2_mul(lam, f2_sub(a.x, r.x)), a.y);
    return r;
}
inline G2A g2_mul(G2A p, const Fr& k_mont) {
    const Fr k = fe_from_mont(k_mont);
    G2A acc{p.x, p.y, true};
    for (int i = 0; i < 256; i++) {
        if ((k.v[i >> 5] >> (i & 31)) & 1) acc = g2_add(acc, p);
        p = g2_add(p, p);
    }
    return acc;
}
inline Fq fq_from_hex_words(const uint32_t be[8]) {  // big-endian word order, canonical -> Montgomery
    Fq t;
    for (int i = 0; i < 8; i++) t.v[i] = be[7 - i];
    return fe_to_mont(t);
}
inline G2A g2_generator() {  // the BN254 G2 generator (reference proving-server/P256Verifier.yul:1125-1128 holds it as x.c1, x.c0, y.c1, y.c0)
    static const uint32_t X0[8] = {0x1800DEEF, 0x121F1E76, 0x426A0066, 0x5E5C4479, 0x674322D4, 0xF75EDADD, 0x46DEBD5C, 0xD992F6ED};
    static const uint32_t X1[8] = {0x198E9393, 0x920D483A, 0x7260BFB7, 0x31FB5D25, 0xF1AA4933, 0x35A9E712, 0x97E485B7, 0xAEF312C2};
    static const uint32_t Y0[8] = {0x12C85EA5, 0xDB8C6DEB, 0x4AAB7180, 0x8DCB408F, 0xE3D1E769, 0x0C43D37B, 0x4CE6CC01, 0x66FA7DAA};
    static const uint32_t Y1[8] = {0x090689D0, 0x585FF075, 0xEC9E99AD, 0x690C3395, 0xBC4B3133, 0x70B38EF3, 0x55ACDADC, 0xD122975B};
    return G2A{{fq_from_hex_words(X0), fq_from_hex_words(X1)}, {fq_from_hex_words(Y0), fq_from_hex_words(Y1)}, false};
}
inline bool g2_on_curve(const G2A& p) { return f2_eq(f2_mul(p.y, p.y), f2_add(f2_mul(f2_mul(p.x, p.x), p.x), f2_twist_b())); }
// a point of G2 other than the identity: coordinates reduced, on the twist, and of order r (the twist has a cofactor)
inline bool g2_is_proper(const G2A& q) {
    if (q.inf || !fq_is_canonical(q.x.c0) || !fq_is_canonical(q.x.c1) || !fq_is_canonical(q.y.c0) || !fq_is_canonical(q.y.c1)) return false;
    if (!g2_on_curve(q)) return false;
    G2A acc{q.x, q.y, true};
    for (int i = 255; i >= 0; i--) {  // [r] q
        acc = g2_add(acc, acc);
        if ((FrParams::P[i >> 5] >> (i & 31)) & 1) acc = g2_add(acc, q);
    }
    return acc.inf;
}

// raw image: x.c0 || x.c1 || y.c0 || y.c1 Montgomery; identity = all zero
inline void g2_to_raw(const G2A& p, uint8_t raw[128]) {
    if (p.inf) {
        memset(raw, 0, 128);
        return;
    }
    memcpy(raw, p.x.c0.v, 32);
    memcpy(raw + 32, p.x.c1.v, 32);
    memcpy(raw + 64, p.y.c0.v, 32);
    memcpy(raw + 96, p.y.c1.v, 32);
}
inline G2A g2_from_raw(const uint8_t raw[128]) {
    G2A p;
    memcpy(p.x.c0.v, raw, 32);
    memcpy(p.x.c1.v, raw + 32, 32);
    memcpy(p.y.c0.v, raw + 64, 32);
    memcpy(p.y.c1.v, raw + 96, 32);
    p.inf = f2_is_zero(p.x) && f2_is_zero(p.y);
    return p;
}

// ---- Fq6, Fq12 -----------------------------------------------------------------------------------------------------
struct Fq6 {
    Fq2 c0, c1, c2;
};
ZK_PAIR_FN Fq6 f6_zero() { return {f2_zero(), f2_zero(), f2_zero()}; }
ZK_PAIR_FN Fq6 f6_one() { return {f2_one(), f2_zero(), f2_zero()}; }
ZK_PAIR_FN Fq6 f6_add(const Fq6& a, const Fq6& b) { return {f2_add(a.c0, b.c0), f2_add(a.c1, b.c1), f2_add(a.c2, b.c2)}; }
ZK_PAIR_FN Fq6 f6_sub(const Fq6& a, const Fq6& b) { return {f2_sub(a.c0, b.c0), f2_sub(a.c1, b.c1), f2_sub(a.c2, b.c2)}; }
ZK_PAIR_FN Fq6 f6_neg(const Fq6& a) { return {f2_neg(a.c0), f2_neg(a.c1), f2_neg(a.c2)}; }
ZK_PAIR_MULFN Fq6 f6_mul(const Fq6& a, const Fq6& b) {  // Karatsuba over v^3 = xi
    const Fq2 t0 = f2_mul(a.c0, b.c0), t1 = f2_mul(a.c1, b.c1), t2 = f2_mul(a.c2, b.c2);
    const Fq2 c0 = f2_add(t0, f2_mul_xi(f2_sub(f2_sub(f2_mul(f2_add(a.c1, a.c2), f2_add(b.c1, b.c2)), t1), t2)));
    const Fq2 c1 = f2_add(f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c1), f2_add(b.c0, b.c1)), t0), t1), f2_mul_xi(t2));
    const Fq2 c2 = f2_add(f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c2), f2_add(b.c0, b.c2)), t0), t2), t1);
    return {c0, c1, c2};
}
// a (b0 + b1 v): the shape of a line's w-half
ZK_PAIR_MULFN Fq6 f6_mul_01(const Fq6& a, const Fq2& b0, const Fq2& b1) {
    const Fq2 t0 = f2_mul(a.c0, b0), t1 = f2_mul(a.c1, b1);
    const Fq2 c0 = f2_add(t0, f2_mul_xi(f2_mul(a.c2, b1)));
    const Fq2 c1 = f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c1), f2_add(b0, b1)), t0), t1);
    const Fq2 c2 = f2_add(t1, f2_mul(a.c2, b0));
    return {c0, c1, c2};
}
ZK_PAIR_FN Fq6 f6_mul_v(const Fq6& a) { return {f2_mul_xi(a.c2), a.c0, a.c1}; }
ZK_PAIR_FN Fq6 f6_inv(const Fq6& a) {
    const Fq2 A = f2_sub(f2_mul(a.c0, a.c0), f2_mul_xi(f2_mul(a.c1, a.c2)));
    const Fq2 B = f2_sub(f2_mul_xi(f2_mul(a.c2, a.c2)), f2_mul(a.c0, a.c1));
    const Fq2 C = f2_sub(f2_mul(a.c1, a.c1), f2_mul(a.c0, a.c2));
    const Fq2 F = f2_add(f2_mul(a.c0, A), f2_mul_xi(f2_add(f2_mul(a.c2, B), f2_mul(a.c1, C))));
    const Fq2 fi = f2_inv(F);
    return {f2_mul(A, fi), f2_mul(B, fi), f2_mul(C, fi)};
}

struct Fq12 {
    Fq6 c0, c1;  // c0 + c1 w
};
ZK_PAIR_FN Fq12 f12_one() { return {f6_one(), f6_zero()}; }
ZK_PAIR_FN bool f12_is_one(const Fq12& a) {
    const Fq2 z = f2_zero();
    return f2_eq(a.c0.c0, f2_one()) && f2_eq(a.c0.c1, z) && f2_eq(a.c0.c2, z) && f2_eq(a.c1.c0, z) && f2_eq(a.c1.c1, z) && f2_eq(a.c1.c2, z);
}
ZK_PAIR_MULFN Fq12 f12_mul(const Fq12& a, const Fq12& b) {
    const Fq6 t0 = f6_mul(a.c0, b.c0), t1 = f6_mul(a.c1, b.c1);
    return {f6_add(t0, f6_mul_v(t1)), f6_sub(f6_sub(f6_mul(f6_add(a.c0, a.c1), f6_add(b.c0, b.c1)), t0), t1)};
}
// (c0 + c1 w)^2 = (c0 + c1)(c0 + v c1) - c0 c1 - v c0 c1 + 2 c0 c1 w
ZK_PAIR_MULFN Fq12 f12_sqr(const Fq12& a) {
    const Fq6 m = f6_mul(a.c0, a.c1);
    const Fq6 s = f6_mul(f6_add(a.c0, a.c1), f6_add(a.c0, f6_mul_v(a.c1)));
    return {f6_sub(f6_sub(s, m), f6_mul_v(m)), f6_add(m, m)};
}
ZK_PAIR_FN Fq12 f12_conj(const Fq12& a) { return {a.c0, f6_neg(a.c1)}; }
ZK_PAIR_FN Fq12 f12_inv(const Fq12& a) {  // (c0 - c1 w) / (c0^2 - v c1^2)
    const Fq6 d = f6_inv(f6_sub(f6_mul(a.c0, a.c0), f6_mul_v(f6_mul(a.c1, a.c1))));
    return {f6_mul(a.c0, d), f6_neg(f6_mul(a.c1, d))};
}

// gamma[i] = xi^(i (p - 1) / 6), i = 1 .. 5: (sum c_i w^i)^p = sum conj(c_i) gamma[i] w^i
struct PairingConsts {
    Fq2 gamma[6];
    Fq2 gamma2_x, gamma2_y;  // xi^((p^2 - 1) / 3), xi^((p^2 - 1) / 2)
    PairingConsts() {
        uint32_t pm1[8], e[8];
        for (int i = 0; i < 8; i++) pm1[i] = FqParams::P[i];
        pm1[0] -= 1;
        uint64_t rem = 0;
        for (int i = 7; i >= 0; i--) {
            const uint64_t cur = (rem << 32) | pm1[i];
            e[i] = (uint32_t)(cur / 6);
            rem = cur % 6;
        }
        gamma[0] = f2_one();
        gamma[1] = f2_pow(f2_small(9, 1), e);
        for (int i = 2; i < 6; i++) gamma[i] = f2_mul(gamma[i - 1], gamma[1]);
        gamma2_x = f2_mul(f2_conj(gamma[2]), gamma[2]);  // (x^p)^p: the norm of xi^((p-1)/3)
        gamma2_y = f2_mul(f2_conj(gamma[3]), gamma[3]);
    }
    static const PairingConsts& get() {
        static const PairingConsts k;  // (thread-safe since C++11)
        return k;
    }
};

// a^p with the six gamma[i] given (the device has them in memory)
ZK_PAIR_MULFN Fq12 f12_frobenius_with(const Fq12& a, const Fq2* g) {
    // w-power of each coefficient: c0.c0 w^0, c1.c0 w^1, c0.c1 w^2, c1.c1 w^3, c0.c2 w^4, c1.c2 w^5
    Fq12 r;
    r.c0.c0 = f2_conj(a.c0.c0);
    r.c1.c0 = f2_mul(f2_conj(a.c1.c0), g[1]);
    r.c0.c1 = f2_mul(f2_conj(a.c0.c1), g[2]);
    r.c1.c1 = f2_mul(f2_conj(a.c1.c1), g[3]);
    r.c0.c2 = f2_mul(f2_conj(a.c0.c2), g[4]);
    r.c1.c2 = f2_mul(f2_conj(a.c1.c2), g[5]);
    return r;
}
inline Fq12 f12_frobenius(const Fq12& a) { return f12_frobenius_with(a, PairingConsts::get().gamma); }

// ---- Miller loop ---------------------------------------------------------------------------------------------------
constexpr uint64_t SIX_U_PLUS_2_LO = 0x9d797039be763ba8ULL;  // 6u + 2 is 65 bits: 2^64 + this (the top bit: T starts at Q)
constexpr uint64_t BN_U = 4965661367192848881ULL;            // 63 bits
// the steps of T through one Miller loop: a doubling per low bit of 6u + 2, an addition per set one, the two Frobenius lines
constexpr int PAIRING_STEPS = 64 + __builtin_popcountll(SIX_U_PLUS_2_LO) + 2;

// one step's line through T with slope lam: all of it that does not depend on the G1 point
struct PairingLine {
    Fq2 lam, c;  // c = lam xT - yT
};
// that line untwisted and evaluated at P: yP - lam xP w + c w^3
ZK_PAIR_FN Fq12 pairing_line_at(const PairingLine& s, const G1Affine& P) {
    Fq12 l;
    l.c0 = f6_zero();
    l.c1 = f6_zero();
    l.c0.c0 = Fq2{P.y, Fq::zero()};
    l.c1.c0 = f2_neg(f2_mul_fq(s.lam, P.x));
    l.c1.c1 = s.c;
    return l;
}
// f times that line, with the line's zero coefficients left out of the products
ZK_PAIR_MULFN Fq12 f12_mul_line(const Fq12& f, const PairingLine& s, const G1Affine& P) {
    const Fq2 b = f2_neg(f2_mul_fq(s.lam, P.x));
    const Fq6 t0 = {f2_mul_fq(f.c0.c0, P.y), f2_mul_fq(f.c0.c1, P.y), f2_mul_fq(f.c0.c2, P.y)};
    const Fq6 t1 = f6_mul_01(f.c1, b, s.c);
    const Fq6 m = f6_mul_01(f6_add(f.c0, f.c1), Fq2{fe_add(P.y, b.c0), b.c1}, s.c);
    return {f6_add(t0, f6_mul_v(t1)), f6_sub(f6_sub(m, t0), t1)};
}
// the line through T (twist, affine) with slope lam, untwisted and evaluated at P: yP - lam xP w + (lam xT - yT) w^3
inline Fq12 pairing_line(const Fq2& lam, const Fq2& xT, const Fq2& yT, const G1Affine& P) {
    return pairing_line_at(PairingLine{lam, f2_sub(f2_mul(lam, xT), yT)}, P);
}
// T <- T + Q (Q != -T) or 2T (Q == T), returning the step's line
inline PairingLine pairing_step_line(G2A& T, const G2A& Q) {
    Fq2 lam;
    if (f2_eq(T.x, Q.x)) lam = f2_mul(f2_mul(f2_small(3, 0), f2_mul(T.x, T.x)), f2_inv(f2_add(T.y, T.y)));
    else lam = f2_mul(f2_sub(Q.y, T.y), f2_inv(f2_sub(Q.x, T.x)));
    const PairingLine s{lam, f2_sub(f2_mul(lam, T.x), T.y)};
    G2A r;
    r.inf = false;
    r.x = f2_sub(f2_sub(f2_mul(lam, lam), T.x), Q.x);
    r.y = f2_sub(f2_mul(lam, f2_sub(T.x, r.x)), T.y);
    T = r;
    return s;
}
// the same, returning the line's factor at P
inline Fq12 pairing_step(G2A& T, const G2A& Q, const G1Affine& P) { return pairing_line_at(pairing_step_line(T, Q), P); }

// prod_i ML(P_i, Q_i); pairs with an identity on either side contribute 1
inline Fq12 multi_miller_loop(const G1Affine* P, const G2A* Q, int n) {
    std::vector<int> idx;
    for (int i = 0; i < n; i++)
        if (!affine_is_identity(P[i]) && !Q[i].inf) idx.push_back(i);
    std::vector<G2A> T;
    for (int i : idx) T.push_back(Q[i]);
    Fq12 f = f12_one();
    for (int b = 63; b >= 0; b--) {
        f = f12_sqr(f);
        for (size_t j = 0; j < idx.size(); j++) f = f12_mul(f, pairing_step(T[j], T[j], P[idx[j]]));
        if ((SIX_U_PLUS_2_LO >> b) & 1)
            for (size_t j = 0; j < idx.size(); j++) f = f12_mul(f, pairing_step(T[j], Q[idx[j]], P[idx[j]]));
    }
    const PairingConsts& k = PairingConsts::get();
    for (size_t j = 0; j < idx.size(); j++) {
        const G2A& q = Q[idx[j]];
        const G2A q1{f2_mul(f2_conj(q.x), k.gamma[2]), f2_mul(f2_conj(q.y), k.gamma[3]), false};
        const G2A nq2{f2_mul(q.x, k.gamma2_x), f2_neg(f2_mul(q.y, k.gamma2_y)), false};
        f = f12_mul(f, pairing_step(T[j], q1, P[idx[j]]));
        f = f12_mul(f, pairing_step(T[j], nq2, P[idx[j]]));
    }
    return f;
}

// ---- prepared lines: the Miller loop with its G2 side done once -------------------------------------------------------
// the PAIRING_STEPS lines of q's walk (q not the identity), in the order multi_miller_loop takes them
inline void pairing_prepare(const G2A& q, PairingLine* out) {
    const PairingConsts& k = PairingConsts::get();
    G2A T = q;
    int n = 0;
    for (int b = 63; b >= 0; b--) {
        out[n++] = pairing_step_line(T, T);
        if ((SIX_U_PLUS_2_LO >> b) & 1) out[n++] = pairing_step_line(T, q);
    }
    const G2A q1{f2_mul(f2_conj(q.x), k.gamma[2]), f2_mul(f2_conj(q.y), k.gamma[3]), false};
    const G2A nq2{f2_mul(q.x, k.gamma2_x), f2_neg(f2_mul(q.y, k.gamma2_y)), false};
    out[n++] = pairing_step_line(T, q1);
    out[n++] = pairing_step_line(T, nq2);
}

// everything a check against one (g2, s_g2) pair reads: the Frobenius constants and both walks.  Plain data: the device form
// is this struct's bytes
struct PairingTable {
    Fq2 gamma[6];
    uint32_t inf[8];  // [0]: s_g2 is the identity, [1]: g2 is (pairs with them contribute 1); the rest pads to 16 bytes
    PairingLine line[2][PAIRING_STEPS];  // [0]: s_g2's walk, [1]: g2's
};
inline void pairing_table_make(const G2A& g2, const G2A& s_g2, PairingTable* t) {
    memset((void*)t, 0, sizeof(*t));
    for (int i = 0; i < 6; i++) t->gamma[i] = PairingConsts::get().gamma[i];
    t->inf[0] = s_g2.inf;
    t->inf[1] = g2.inf;
    if (!s_g2.inf) pairing_prepare(s_g2, t->line[0]);
    if (!g2.inf) pairing_prepare(g2, t->line[1]);
}

// ML(P0, Q0) ML(P1, Q1) over the two prepared walks; an identity on either side of a pair leaves the pair out.  Fixed trip
// counts: the bits are those of the constant 6u + 2
ZK_PAIR_FN Fq12 miller_loop_lines(const G1Affine& P0, const G1Affine& P1, const PairingTable& t) {
    const bool use0 = !affine_is_identity(P0) && !t.inf[0], use1 = !affine_is_identity(P1) && !t.inf[1];
    Fq12 f = f12_one();
    int n = 0;
#pragma unroll 1
    for (int b = 63; b >= -2; b--) {
        if (b >= 0) f = f12_sqr(f);
        // a doubling step, then an addition step where the bit is set; b = -1, -2: the Frobenius lines
        const int steps = (b >= 0 && ((SIX_U_PLUS_2_LO >> b) & 1)) ? 2 : 1;
#pragma unroll 1
        for (int s = 0; s < steps; s++, n++) {
            if (use0) f = f12_mul_line(f, t.line[0][n], P0);
            if (use1) f = f12_mul_line(f, t.line[1][n], P1);
        }
    }
    return f;
}

// f^u, u = BN_U, by squarings and products (f anywhere in Fq12)
ZK_PAIR_FN Fq12 f12_pow_u(const Fq12& f) {
    Fq12 acc = f;
#pragma unroll 1
    for (int i = 61; i >= 0; i--) {
        acc = f12_sqr(acc);
        if ((BN_U >> i) & 1) acc = f12_mul(acc, f);
    }
    return acc;
}

// f^((p^12 - 1) / r) without a table: the easy part as below, then the hard part (p^4 - p^2 + 1) / r itself by the chain of
// Devegili, Scott and Dahab: with a = t^u, b = a^u, c = b^u, the product y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36 of
// y0 = t^p t^p^2 t^p^3, y1 = 1/t, y2 = b^p^2, y3 = 1/a^p, y4 = 1/(a b^p), y5 = 1/b, y6 = 1/(c c^p).  After the easy part t lies
// in the cyclotomic subgroup, where 1/x is the conjugate.  (tests/test_pairing_lines.py adds the exponents up as integers.)
ZK_PAIR_FN Fq12 final_exponentiation_chain(const Fq12& f, const Fq2* gamma) {
    Fq12 t = f12_mul(f12_conj(f), f12_inv(f));                                      // ^(p^6 - 1)
    t = f12_mul(f12_frobenius_with(f12_frobenius_with(t, gamma), gamma), t);        // ^(p^2 + 1)
    const Fq12 fp = f12_frobenius_with(t, gamma), fp2 = f12_frobenius_with(fp, gamma);
    const Fq12 y0 = f12_mul(f12_mul(fp, fp2), f12_frobenius_with(fp2, gamma));
    const Fq12 fu = f12_pow_u(t), fu2 = f12_pow_u(fu), fu3 = f12_pow_u(fu2);
    const Fq12 fu2p = f12_frobenius_with(fu2, gamma);
    const Fq12 y2 = f12_frobenius_with(fu2p, gamma);
    const Fq12 y3 = f12_conj(f12_frobenius_with(fu, gamma));
    const Fq12 y4 = f12_conj(f12_mul(fu, fu2p));
    const Fq12 y5 = f12_conj(fu2);
    Fq12 y6 = f12_conj(f12_mul(fu3, f12_frobenius_with(fu3, gamma)));
    y6 = f12_mul(f12_mul(f12_sqr(y6), y4), y5);
    Fq12 t1 = f12_mul(f12_mul(y3, y5), y6);
    y6 = f12_mul(y6, y2);
    t1 = f12_sqr(f12_mul(f12_sqr(t1), y6));
    const Fq12 t0 = f12_sqr(f12_mul(t1, f12_conj(t)));
    return f12_mul(t0, f12_mul(t1, y0));
}

// f^((p^12 - 1) / r)
inline Fq12 final_exponentiation(const Fq12& f) {
    Fq12 t = f12_mul(f12_conj(f), f12_inv(f));           // ^(p^6 - 1)
    t = f12_mul(f12_frobenius(f12_frobenius(t)), t);     // ^(p^2 + 1)
    // hard part (p^4 - p^2 + 1) / r = l0 + l1 p + l2 p^2 + l3 p^3 (l3 = 1)
    static const uint32_t L[3][8] = {
        {0xd0f9fa91u, 0x85989436u, 0xfd736beau, 0x5cea24f6u, 0x3fd84104u, 0x048b6e19u, 0xe131a029u, 0x30644e72u},
        {0x606a30c5u, 0x138f3176u, 0xdae41fe4u, 0x3b852988u, 0x3fd84105u, 0x048b6e19u, 0xe131a029u, 0x30644e72u},
        {0xe87cfd46u, 0xf83e9682u, 0xeeb859fbu, 0x6f4d8248u, 0, 0, 0, 0}};
    Fq12 base[4];
    base[0] = t;
    for (int i = 1; i < 4; i++) base[i] = f12_frobenius(base[i - 1]);
    Fq12 tab[16];
    tab[0] = f12_one();
    for (int m = 1; m < 16; m++) {
        const int low = m & -m, i = __builtin_ctz(low);
        tab[m] = (m == low) ? base[i] : f12_mul(tab[m ^ low], base[i]);
    }
    Fq12 acc = f12_one();
    bool started = false;
    for (int b = 253; b >= 0; b--) {
        if (started) acc = f12_sqr(acc);
        int m = 0;
        for (int i = 0; i < 3; i++) m |= (int)((L[i][b >> 5] >> (b & 31)) & 1) << i;
        if (b == 0) m |= 8;  // l3 = 1
        if (m) {
            acc = started ? f12_mul(acc, tab[m]) : tab[m];
            started = true;
        }
    }
    return acc;
}

inline Fq12 pairing(const G1Affine& P, const G2A& Q) { return final_exponentiation(multi_miller_loop(&P, &Q, 1)); }

// the KZG check: e(a, s_g2) * e(-b, g2) == 1
inline bool pairing_check(const G1Affine& a, const G1Affine& b, const G2A& g2, const G2A& s_g2) {
    G1Affine P[2] = {a, b};
    if (!affine_is_identity(b)) P[1].y = fe_neg(b.y);
    const G2A Q[2] = {s_g2, g2};
    return f12_is_one(final_exponentiation(multi_miller_loop(P, Q, 2)));
}

// the same check of one (a, b) against a prepared pair, as a lane of pairing_check_kernel runs it: the ZK_PAIRING_* reason.
// a and b are validated first (both coordinates below p, then on y^2 = x^3 + 3 or the identity (0, 0))
ZK_PAIR_FN uint8_t pairing_check_lines(const G1Affine& a, const G1Affine& b, const PairingTable& t) {
    if (!fq_is_canonical(a.x) || !fq_is_canonical(a.y) || !fq_is_canonical(b.x) || !fq_is_canonical(b.y)) return ZK_PAIRING_RANGE;
    if (!affine_is_identity(a) && !g1_on_curve(a.x, a.y)) return ZK_PAIRING_OFF_CURVE;
    if (!affine_is_identity(b) && !g1_on_curve(b.x, b.y)) return ZK_PAIRING_OFF_CURVE;
    G1Affine nb = b;
    nb.y = fe_neg(b.y);  // (the identity stays (0, 0))
    const Fq12 f = final_exponentiation_chain(miller_loop_lines(a, nb, t), t.gamma);
    return f12_is_one(f) ? ZK_PAIRING_VALID : ZK_PAIRING_MISMATCH;
}

// a point of G1 other than the identity: both coordinates reduced, y^2 = x^3 + 3 (G1 has cofactor 1)
ZK_PAIR_FN bool g1_is_proper(const G1Affine& p) {
    if (!fq_is_canonical(p.x) || !fq_is_canonical(p.y) || affine_is_identity(p)) return false;
    return g1_on_curve(p.x, p.y);
}

// ---- G2 on a lane: a G2 point per check -------------------------------------------------------------------------------------
// A lane that brings its own G2 point walks it through the Miller loop itself, so the walk may not invert: T is kept in Jacobian
// coordinates (x / z^2, y / z^3; z = 0 the identity) and a step hands out its line times a factor of Fq2 — the final
// exponentiation sends every element of a proper subfield to 1, so what is pinned is the value after final_exponentiation_chain.
struct G2J {
    Fq2 x, y, z;
};
// a step's line before it meets a G1 point P: a yP + b xP w + c w^3, pairing_line_at's line times 2 yT z^3 (a doubling) or z3 (an addition)
struct PairingLineJ {
    Fq2 a, b, c;
};
ZK_PAIR_FN bool g2j_is_identity(const G2J& t) { return f2_is_zero(t.z); }
// T <- 2 T with the tangent's line.  (x, y, z) -> (m^2 - 2 s, m (s - x3) - 8 y^4, 2 y z), m = 3 x^2, s = 4 x y^2; the slope is m / z3.
// The identity stays the identity (z3 = 0); the twist has odd order, so no other point doubles to it
ZK_PAIR_MULFN PairingLineJ g2j_double_line(G2J& T) {
    const Fq2 xx = f2_mul(T.x, T.x), yy = f2_mul(T.y, T.y), zz = f2_mul(T.z, T.z);
    const Fq2 m = f2_add(f2_add(xx, xx), xx);
    Fq2 s = f2_mul(T.x, yy), y4 = f2_mul(yy, yy);
    s = f2_add(s, s);
    s = f2_add(s, s);
    y4 = f2_add(y4, y4);
    y4 = f2_add(y4, y4);
    y4 = f2_add(y4, y4);
    const Fq2 z3 = f2_mul(f2_add(T.y, T.y), T.z);
    PairingLineJ l;
    l.a = f2_mul(z3, zz);
    l.b = f2_neg(f2_mul(m, zz));
    l.c = f2_sub(f2_mul(m, T.x), f2_add(yy, yy));
    const Fq2 x3 = f2_sub(f2_mul(m, m), f2_add(s, s));
    T.y = f2_sub(f2_mul(m, f2_sub(s, x3)), y4);
    T.x = x3;
    T.z = z3;
    return l;
}
// T <- T + Q with the line through both, Q = (qx, qy) affine, T neither the identity nor +-Q.  With h = qx z^2 - x and
// r = qy z^3 - y: (r^2 - h^3 - 2 x h^2, r (x h^2 - x3) - y h^3, z h); the slope is r / z3
ZK_PAIR_MULFN PairingLineJ g2j_add_line(G2J& T, const Fq2& qx, const Fq2& qy) {
    const Fq2 zz = f2_mul(T.z, T.z);
    const Fq2 h = f2_sub(f2_mul(qx, zz), T.x), r = f2_sub(f2_mul(qy, f2_mul(T.z, zz)), T.y);
    const Fq2 hh = f2_mul(h, h);
    const Fq2 hhh = f2_mul(h, hh), v = f2_mul(T.x, hh);
    const Fq2 z3 = f2_mul(T.z, h);
    PairingLineJ l;
    l.a = z3;
    l.b = f2_neg(r);
    l.c = f2_sub(f2_mul(r, qx), f2_mul(z3, qy));
    const Fq2 x3 = f2_sub(f2_sub(f2_mul(r, r), hhh), f2_add(v, v));
    T.y = f2_sub(f2_mul(r, f2_sub(v, x3)), f2_mul(T.y, hhh));
    T.x = x3;
    T.z = z3;
    return l;
}
// T <- T + Q for any T and any affine Q on the twist: the cases the Miller loop of a proper point never meets
ZK_PAIR_FN void g2j_add_any(G2J& T, const Fq2& qx, const Fq2& qy) {
    if (g2j_is_identity(T)) {
        T = G2J{qx, qy, f2_one()};
        return;
    }
    const Fq2 zz = f2_mul(T.z, T.z);
    if (f2_eq(f2_mul(qx, zz), T.x)) {
        if (f2_eq(f2_mul(qy, f2_mul(T.z, zz)), T.y)) (void)g2j_double_line(T);
        else T.z = f2_zero();
        return;
    }
    (void)g2j_add_line(T, qx, qy);
}
// g2_is_proper's verdict for every input, as a lane finds it: coordinates reduced, on the twist, [r] q the identity, q not.
// The twist equation is taken times xi, (y^2 - x^3) xi = 3, and [r] q runs in Jacobian coordinates from the top bit of r (bit 253)
// down: nothing is inverted, and the trip count is that of the constant r
ZK_PAIR_FN bool g2_is_proper_lane(const G2A& q) {
    if (q.inf || !fq_is_canonical(q.x.c0) || !fq_is_canonical(q.x.c1) || !fq_is_canonical(q.y.c0) || !fq_is_canonical(q.y.c1)) return false;
    if (!f2_eq(f2_mul_xi(f2_sub(f2_mul(q.y, q.y), f2_mul(f2_mul(q.x, q.x), q.x))), f2_small(3, 0))) return false;
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = FrParams::P[i];
    G2J acc{q.x, q.y, f2_one()};
#pragma unroll 1
    for (int i = 252; i >= 0; i--) {
        (void)g2j_double_line(acc);
        if ((e[i >> 5] >> (i & 31)) & 1) g2j_add_any(acc, q.x, q.y);
    }
    return g2j_is_identity(acc);
}

// f times the line l0 + l1 w + l3 w^3 with all three coefficients in Fq2 (f12_mul_line's shape, its Fq coefficient widened)
ZK_PAIR_MULFN Fq12 f12_mul_line3(const Fq12& f, const Fq2& l0, const Fq2& l1, const Fq2& l3) {
    const Fq6 t0 = {f2_mul(f.c0.c0, l0), f2_mul(f.c0.c1, l0), f2_mul(f.c0.c2, l0)};
    const Fq6 t1 = f6_mul_01(f.c1, l1, l3);
    const Fq6 m = f6_mul_01(f6_add(f.c0, f.c1), f2_add(l0, l1), l3);
    return {f6_add(t0, f6_mul_v(t1)), f6_sub(f6_sub(m, t0), t1)};
}

// f[k] = ML(Pw[k], q) ML(Pf[k], g2), k < N, over ONE walk of q (a proper point): every line of the walk is evaluated at each
// Pw[k] into its own accumulator, and g2's lines come from the prepared walk t.line[1].  An identity on either side of a pair
// leaves the pair out.  Fixed trip counts, as in miller_loop_lines
template <int N>
ZK_PAIR_FN void miller_loop_walk(const G2A& q, const G1Affine* Pw, const G1Affine* Pf, const PairingTable& t, Fq12* f) {
    bool usew[N], usef[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        usew[k] = !affine_is_identity(Pw[k]);
        usef[k] = !affine_is_identity(Pf[k]) && !t.inf[1];
        f[k] = f12_one();
    }
    // pi(q) and -pi^2(q), the ends of the two Frobenius lines
    const Fq2 q1x = f2_mul(f2_conj(q.x), t.gamma[2]), q1y = f2_mul(f2_conj(q.y), t.gamma[3]);
    const Fq2 nq2x = f2_mul(q.x, f2_mul(f2_conj(t.gamma[2]), t.gamma[2])), nq2y = f2_neg(f2_mul(q.y, f2_mul(f2_conj(t.gamma[3]), t.gamma[3])));
    G2J T{q.x, q.y, f2_one()};
    int n = 0;
#pragma unroll 1
    for (int b = 63; b >= -2; b--) {
        if (b >= 0) {
#pragma unroll
            for (int k = 0; k < N; k++) f[k] = f12_sqr(f[k]);
        }
        const int steps = (b >= 0 && ((SIX_U_PLUS_2_LO >> b) & 1)) ? 2 : 1;
#pragma unroll 1
        for (int s = 0; s < steps; s++, n++) {
            PairingLineJ l;
            if (b >= 0 && s == 0) l = g2j_double_line(T);
            else if (b >= 0) l = g2j_add_line(T, q.x, q.y);
            else if (b == -1) l = g2j_add_line(T, q1x, q1y);
            else l = g2j_add_line(T, nq2x, nq2y);
#pragma unroll
            for (int k = 0; k < N; k++) {
                if (usew[k]) f[k] = f12_mul_line3(f[k], f2_mul_fq(l.a, Pw[k].y), f2_mul_fq(l.b, Pw[k].x), l.c);
                if (usef[k]) f[k] = f12_mul_line(f[k], t.line[1][n], Pf[k]);
            }
        }
    }
}

// e(a, q) = e(b, g2) with the lane's own q, as a lane of pairing_check_each_kernel runs it: pairing_check_lines' reasons in its
// order, then ZK_PAIRING_G2 for a q that is not a proper point (such a lane returns before it walks).  t: a table whose line[1]
// is g2's walk
ZK_PAIR_FN uint8_t pairing_check_walk(const G1Affine& a, const G1Affine& b, const G2A& q, const PairingTable& t) {
    if (!fq_is_canonical(a.x) || !fq_is_canonical(a.y) || !fq_is_canonical(b.x) || !fq_is_canonical(b.y)) return ZK_PAIRING_RANGE;
    if (!affine_is_identity(a) && !g1_is_proper(a)) return ZK_PAIRING_OFF_CURVE;
    if (!affine_is_identity(b) && !g1_is_proper(b)) return ZK_PAIRING_OFF_CURVE;
    if (!g2_is_proper_lane(q)) return ZK_PAIRING_G2;
    G1Affine nb = b;
    nb.y = fe_neg(b.y);
    Fq12 f;
    miller_loop_walk<1>(q, &a, &nb, t, &f);
    return f12_is_one(final_exponentiation_chain(f, t.gamma)) ? ZK_PAIRING_VALID : ZK_PAIRING_MISMATCH;
}

// The receipt rule of a ceremony contribution (srs_update.h srs_contribution_flags) as a lane of contribution_check_kernel runs
// it: ZK_SRS_CONTRIB_SAME_SECRET | LINKS | NONTRIVIAL, and no bit for a receipt with an improper point.  Both equations,
// e(G1, s_g2) = e(s_g1, G2) and e(before, s_g2) = e(after, G2), share s_g2: one walk, two accumulators, two final
// exponentiations.  t: a table whose line[1] is the walk of the G2 generator
ZK_PAIR_FN uint32_t contribution_check_lanes(const G1Affine& before, const G1Affine& after, const G1Affine& s_g1, const G2A& s_g2, const PairingTable& t) {
    if (!g1_is_proper(before) || !g1_is_proper(after) || !g1_is_proper(s_g1) || !g2_is_proper_lane(s_g2)) return 0;
    G1Affine Pw[2], Pf[2] = {s_g1, after};
    Pw[0].x = Fq::one();
    Pw[0].y = fe_add(Fq::one(), Fq::one());
    Pw[1] = before;
    uint32_t flags = (s_g1.x == Pw[0].x && s_g1.y == Pw[0].y) ? 0 : ZK_SRS_CONTRIB_NONTRIVIAL;
    Pf[0].y = fe_neg(Pf[0].y);
    Pf[1].y = fe_neg(Pf[1].y);
    Fq12 f[2];
    miller_loop_walk<2>(s_g2, Pw, Pf, t, f);
#pragma unroll 1
    for (int k = 0; k < 2; k++)
        if (f12_is_one(final_exponentiation_chain(f[k], t.gamma))) flags |= k ? ZK_SRS_CONTRIB_LINKS : ZK_SRS_CONTRIB_SAME_SECRET;
    return flags;
}

}  // namespace zk
