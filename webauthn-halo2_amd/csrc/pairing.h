// pairing.h — BN254 G2 and the optimal-ate pairing on the host (the KZG check of zk_verify / zk_verify_batch).
//
// Fq2 = Fq[u] / (u^2 + 1), Fq6 = Fq2[v] / (v^3 - xi), Fq12 = Fq6[w] / (w^2 - v), xi = 9 + u: halo2curves bn256's tower.
// G2 is the D-type twist y^2 = x^3 + 3 / xi over Fq2, untwisted by (x, y) -> (x w^2, y w^3).  The Miller loop runs over
// the bits of 6u + 2 (u = 4965661367192848881) in affine coordinates, followed by the two Frobenius lines of the optimal
// ate pairing; the final exponentiation is the easy part (p^6 - 1)(p^2 + 1) and the hard part (p^4 - p^2 + 1) / r taken as
// one multi-exponentiation of f, f^p, f^p^2, f^p^3 by the base-p digits of that exponent.  A verifier computes two Miller
// loops per check, so this stays host code (field.hip.h's 64-bit host products): nothing here runs enough pairings to
// pay for a device form.  The same Fq2 / G2 helpers serve the SRS file's G2 half (serde.hip).
#pragma once
#include <string.h>

#include <vector>

#include "ec.hip.h"
#include "field.hip.h"
#include "hostutil.h"

namespace zk {

inline Fq fq_small(uint32_t x) {
    Fq t = Fq::zero();
    t.v[0] = x;
    return fe_to_mont(t);
}

// ---- Fq2 and the twist y^2 = x^3 + 3 / (9 + u) ---------------------------------------------------------------------
struct Fq2 {
    Fq c0, c1;
};
inline Fq2 f2_add(const Fq2& a, const Fq2& b) { return {fe_add(a.c0, b.c0), fe_add(a.c1, b.c1)}; }
inline Fq2 f2_sub(const Fq2& a, const Fq2& b) { return {fe_sub(a.c0, b.c0), fe_sub(a.c1, b.c1)}; }
inline Fq2 f2_neg(const Fq2& a) { return {fe_neg(a.c0), fe_neg(a.c1)}; }
inline Fq2 f2_mul(const Fq2& a, const Fq2& b) {
    return {fe_sub(fe_mul(a.c0, b.c0), fe_mul(a.c1, b.c1)), fe_add(fe_mul(a.c0, b.c1), fe_mul(a.c1, b.c0))};
}
inline Fq2 f2_mul_fq(const Fq2& a, const Fq& s) { return {fe_mul(a.c0, s), fe_mul(a.c1, s)}; }
inline Fq2 f2_conj(const Fq2& a) { return {a.c0, fe_neg(a.c1)}; }
inline Fq2 f2_inv(const Fq2& a) {
    const Fq d = fe_inv_fast(fe_add(fe_sqr(a.c0), fe_sqr(a.c1)));
    return {fe_mul(a.c0, d), fe_neg(fe_mul(a.c1, d))};
}
inline bool f2_is_zero(const Fq2& a) { return a.c0.is_zero() && a.c1.is_zero(); }
inline bool f2_eq(const Fq2& a, const Fq2& b) { return a.c0 == b.c0 && a.c1 == b.c1; }
inline Fq2 f2_small(uint32_t a, uint32_t b) { return {fq_small(a), fq_small(b)}; }
inline Fq2 f2_one() { return {Fq::one(), Fq::zero()}; }
inline Fq2 f2_zero() { return {Fq::zero(), Fq::zero()}; }
inline Fq2 f2_mul_xi(const Fq2& a) {  // a (9 + u)
    const Fq n9 = fq_small(9);
    return {fe_sub(fe_mul(a.c0, n9), a.c1), fe_add(a.c0, fe_mul(a.c1, n9))};
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
inline Fq6 f6_zero() { return {f2_zero(), f2_zero(), f2_zero()}; }
inline Fq6 f6_one() { return {f2_one(), f2_zero(), f2_zero()}; }
inline Fq6 f6_add(const Fq6& a, const Fq6& b) { return {f2_add(a.c0, b.c0), f2_add(a.c1, b.c1), f2_add(a.c2, b.c2)}; }
inline Fq6 f6_sub(const Fq6& a, const Fq6& b) { return {f2_sub(a.c0, b.c0), f2_sub(a.c1, b.c1), f2_sub(a.c2, b.c2)}; }
inline Fq6 f6_neg(const Fq6& a) { return {f2_neg(a.c0), f2_neg(a.c1), f2_neg(a.c2)}; }
inline Fq6 f6_mul(const Fq6& a, const Fq6& b) {  // Karatsuba over v^3 = xi
    const Fq2 t0 = f2_mul(a.c0, b.c0), t1 = f2_mul(a.c1, b.c1), t2 = f2_mul(a.c2, b.c2);
    const Fq2 c0 = f2_add(t0, f2_mul_xi(f2_sub(f2_sub(f2_mul(f2_add(a.c1, a.c2), f2_add(b.c1, b.c2)), t1), t2)));
    const Fq2 c1 = f2_add(f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c1), f2_add(b.c0, b.c1)), t0), t1), f2_mul_xi(t2));
    const Fq2 c2 = f2_add(f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c2), f2_add(b.c0, b.c2)), t0), t2), t1);
    return {c0, c1, c2};
}
inline Fq6 f6_mul_v(const Fq6& a) { return {f2_mul_xi(a.c2), a.c0, a.c1}; }
inline Fq6 f6_inv(const Fq6& a) {
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
inline Fq12 f12_one() { return {f6_one(), f6_zero()}; }
inline bool f12_is_one(const Fq12& a) {
    const Fq12 o = f12_one();
    return memcmp(&a, &o, sizeof(Fq12)) == 0;
}
inline Fq12 f12_mul(const Fq12& a, const Fq12& b) {
    const Fq6 t0 = f6_mul(a.c0, b.c0), t1 = f6_mul(a.c1, b.c1);
    return {f6_add(t0, f6_mul_v(t1)), f6_sub(f6_sub(f6_mul(f6_add(a.c0, a.c1), f6_add(b.c0, b.c1)), t0), t1)};
}
inline Fq12 f12_sqr(const Fq12& a) { return f12_mul(a, a); }
inline Fq12 f12_conj(const Fq12& a) { return {a.c0, f6_neg(a.c1)}; }
inline Fq12 f12_inv(const Fq12& a) {  // (c0 - c1 w) / (c0^2 - v c1^2)
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

inline Fq12 f12_frobenius(const Fq12& a) {
    const Fq2* g = PairingConsts::get().gamma;
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

// ---- Miller loop ---------------------------------------------------------------------------------------------------
// the line through T (twist, affine) with slope lam, untwisted and evaluated at P: yP - lam xP w + (lam xT - yT) w^3
inline Fq12 pairing_line(const Fq2& lam, const Fq2& xT, const Fq2& yT, const G1Affine& P) {
    Fq12 l;
    l.c0 = f6_zero();
    l.c1 = f6_zero();
    l.c0.c0 = Fq2{P.y, Fq::zero()};
    l.c1.c0 = f2_neg(f2_mul_fq(lam, P.x));
    l.c1.c1 = f2_sub(f2_mul(lam, xT), yT);
    return l;
}
// T <- T + Q (Q != -T) or 2T (Q == T), returning the line's factor at P
inline Fq12 pairing_step(G2A& T, const G2A& Q, const G1Affine& P) {
    Fq2 lam;
    if (f2_eq(T.x, Q.x)) lam = f2_mul(f2_mul(f2_small(3, 0), f2_mul(T.x, T.x)), f2_inv(f2_add(T.y, T.y)));
    else lam = f2_mul(f2_sub(Q.y, T.y), f2_inv(f2_sub(Q.x, T.x)));
    const Fq12 l = pairing_line(lam, T.x, T.y, P);
    G2A r;
    r.inf = false;
    r.x = f2_sub(f2_sub(f2_mul(lam, lam), T.x), Q.x);
    r.y = f2_sub(f2_mul(lam, f2_sub(T.x, r.x)), T.y);
    T = r;
    return l;
}

// prod_i ML(P_i, Q_i); pairs with an identity on either side contribute 1
inline Fq12 multi_miller_loop(const G1Affine* P, const G2A* Q, int n) {
    static const uint64_t SIX_U_PLUS_2_HI = 1, SIX_U_PLUS_2_LO = 0x9d797039be763ba8ULL;  // 6u + 2, 65 bits
    std::vector<int> idx;
    for (int i = 0; i < n; i++)
        if (!affine_is_identity(P[i]) && !Q[i].inf) idx.push_back(i);
    std::vector<G2A> T;
    for (int i : idx) T.push_back(Q[i]);
    Fq12 f = f12_one();
    (void)SIX_U_PLUS_2_HI;  // the top bit: T starts at Q
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

}  // namespace zk
