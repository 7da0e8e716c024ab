// p256.hip.h — secp256r1 (NIST P-256): the base field Fp, the scalar field Fn, the curve, and the ES256 verification rule.
//
// Host and device twin of what ecdsa_p256.es256_verify computes on Python integers (and of the values halo2-lib's
// ecdsa_verify_no_pubkey_check assigns: u1 = z / s, u2 = r / s, the trace of u1 G + u2 Q).  Every function here is
// __host__ __device__ in ONE portable form: the kernel (es256.hip) is a loop around p256_verify_one, and a CPU program can run
// the same code (tests/p256_host_check.cpp does, under the sanitizers).  On the device the 32 x 32 + 64 products of the
// portable form compile to v_mad_u64_u32, like field.hip.h's; there are no inline-assembly forms.
//
// Why not field.hip.h: that header relies on p < 2^254 (no carry out of a sum, lazy column bounds, an 8-word reduce_once).
// Both P-256 moduli lie above 2^256 - 2^225, so
//   - a + b of two reduced elements can carry out of 256 bits:            p256_add looks at the carry AND at the comparison;
//   - the Montgomery total (a b + m M) / 2^256 lies in [0, 2 M) and 2 M > 2^256: the running value of the CIOS loop is NINE words
//     plus one bit (a tenth word), and the final subtraction is taken when the ninth word is set OR the low eight are >= M.
// Montgomery form, R = 2^256, 8 x 32-bit limbs, one templated routine for both moduli (no special-form reduction for p).
//
// NOT constant time, on purpose: signatures, keys and hashes are public request data and the exponents of the Fermat inversions
// are the public constants M - 2.  Nothing here may be used with a secret.
//
// Points: Jacobian (X, Y, Z) over y^2 = x^3 - 3 x + b, Z = 0 the identity; affine (x, y) with (0, 0) standing for the identity
// ((0, 0) is not on the curve).  Doubling, mixed and full addition handle every exceptional case: either operand the identity,
// equal points (the doubling), opposite points (the identity).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef ZK_ES256_VALID  // (include/zkmi355.h defines the same four: this header also stands alone)
#define ZK_ES256_VALID 0
#define ZK_ES256_RANGE 1
#define ZK_ES256_OFF_CURVE 2
#define ZK_ES256_MISMATCH 3
#endif

// The field product is ONE function per modulus on the device (a call, not a copy per use: a verification has about 60 product
// sites, and inlined they are several times the instruction cache); P256_MUL_INLINE=1 inlines it everywhere instead.
#ifndef P256_MUL_INLINE
#define P256_MUL_INLINE 0
#endif
#if defined(__HIP_DEVICE_COMPILE__) && !P256_MUL_INLINE
#define P256_MULFN __host__ __device__ __noinline__
#else
#define P256_MULFN __host__ __device__ inline
#endif
#define P256_FN __host__ __device__ __forceinline__

namespace zk {

struct P256FpPrm {  // p = 2^256 - 2^224 + 2^192 + 2^96 - 1
    static constexpr uint32_t P[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000001u, 0xffffffffu};
    static constexpr uint32_t INV = 0x00000001u;  // -p^-1 mod 2^32
    static constexpr uint32_t ONE[8] = {0x00000001u, 0x00000000u, 0x00000000u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xfffffffeu, 0x00000000u};
    static constexpr uint32_t R2[8] = {0x00000003u, 0x00000000u, 0xffffffffu, 0xfffffffbu, 0xfffffffeu, 0xffffffffu, 0xfffffffdu, 0x00000004u};
};
struct P256FnPrm {  // n, the group order
    static constexpr uint32_t P[8] = {0xfc632551u, 0xf3b9cac2u, 0xa7179e84u, 0xbce6faadu, 0xffffffffu, 0xffffffffu, 0x00000000u, 0xffffffffu};
    static constexpr uint32_t INV = 0xee00bc4fu;
    static constexpr uint32_t ONE[8] = {0x039cdaafu, 0x0c46353du, 0x58e8617bu, 0x43190552u, 0x00000000u, 0x00000000u, 0xffffffffu, 0x00000000u};
    static constexpr uint32_t R2[8] = {0xbe79eea2u, 0x83244c95u, 0x49bd6fa6u, 0x4699799cu, 0x2b6bec59u, 0x2845b239u, 0xf3d95620u, 0x66e12d94u};
};

// an element of Z / M, fully reduced; as an operand of the products in Montgomery form
template <class M>
struct P256Fe {
    uint32_t v[8];
};
typedef P256Fe<P256FpPrm> P256Fp;
typedef P256Fe<P256FnPrm> P256Fn;

struct P256Affine {  // Montgomery coordinates; (0, 0): the identity
    P256Fp x, y;
};
struct P256Jac {  // Montgomery coordinates; Z = 0: the identity
    P256Fp X, Y, Z;
};

// curve constants in Montgomery form: b, the generator
struct P256Curve {
    static constexpr uint32_t B[8] = {0x29c4bddfu, 0xd89cdf62u, 0x78843090u, 0xacf005cdu, 0xf7212ed6u, 0xe5a220abu, 0x04874834u, 0xdc30061du};
    static constexpr uint32_t GX[8] = {0x18a9143cu, 0x79e730d4u, 0x5fedb601u, 0x75ba95fcu, 0x77622510u, 0x79fb732bu, 0xa53755c6u, 0x18905f76u};
    static constexpr uint32_t GY[8] = {0xce95560au, 0xddf25357u, 0xba19e45cu, 0x8b4ab8e4u, 0xdd21f325u, 0xd2e88688u, 0x25885d85u, 0x8571ff18u};
    static constexpr uint32_t P_MINUS_N[8] = {0x039cdaaeu, 0x0c46353du, 0x58e8617bu, 0x43190553u, 0, 0, 0, 0};  // 127 bits
};

template <class M>
P256_FN P256Fe<M> p256_zero() {
    P256Fe<M> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = 0;
    return r;
}
template <class M>
P256_FN P256Fe<M> p256_one() {
    P256Fe<M> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = M::ONE[i];
    return r;
}
template <class M>
P256_FN bool p256_is_zero(const P256Fe<M>& a) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) o |= a.v[i];
    return o == 0;
}
template <class M>
P256_FN bool p256_eq(const P256Fe<M>& a, const P256Fe<M>& b) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) o |= a.v[i] ^ b.v[i];
    return o == 0;
}
// a < b as 256-bit integers (eight little-endian words each)
P256_FN bool p256_words_lt(const uint32_t* a, const uint32_t* b) {
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) c = ((int64_t)a[i] - (int64_t)b[i] + c) >> 32;
    return c != 0;
}

// t (eight words) with `top` above them, top * 2^256 + t < 2 M: the value mod M.  The subtraction is taken when top is set
// (the value is then >= 2^256 > M, and value - M < M < 2^256 is what the low eight words of the difference hold) or t >= M
template <class M>
P256_FN P256Fe<M> p256_final_sub(const uint32_t (&t)[8], uint32_t top) {
    uint32_t d[8];
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (int64_t)t[i] - (int64_t)M::P[i];
        d[i] = (uint32_t)c;
        c >>= 32;
    }
    const bool take = top != 0 || c == 0;  // c == 0: no borrow, t >= M
    P256Fe<M> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = take ? d[i] : t[i];
    return r;
}

template <class M>
P256_FN P256Fe<M> p256_add(const P256Fe<M>& a, const P256Fe<M>& b) {
    uint32_t t[8];
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)a.v[i] + b.v[i];
        t[i] = (uint32_t)c;
        c >>= 32;
    }
    return p256_final_sub<M>(t, (uint32_t)c);  // the carry out of 256 bits is the ninth word
}

template <class M>
P256_FN P256Fe<M> p256_sub(const P256Fe<M>& a, const P256Fe<M>& b) {
    P256Fe<M> r;
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (int64_t)a.v[i] - (int64_t)b.v[i];
        r.v[i] = (uint32_t)c;
        c >>= 32;
    }
    const uint32_t mask = c != 0 ? 0xffffffffu : 0u;  // borrow: add M back (the carry out of that sum cancels the borrow)
    uint64_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        d += (uint64_t)r.v[i] + (M::P[i] & mask);
        r.v[i] = (uint32_t)d;
        d >>= 32;
    }
    return r;
}

template <class M>
P256_FN P256Fe<M> p256_neg(const P256Fe<M>& a) {
    return p256_sub(p256_zero<M>(), a);
}

// CIOS Montgomery product a b / 2^256 mod M.  The running value t stays below 2 M at the end of every round, so it needs a
// ninth word (t[8] <= 1); inside a round, t + a b_i < M (2^32 + 1) can pass 2^288 by one bit: the tenth word t9.
template <class M>
P256_MULFN P256Fe<M> p256_mul(const P256Fe<M> a, const P256Fe<M> b) {  // (by value: sixteen words in registers across the call)
    uint32_t t[9];
#pragma unroll
    for (int i = 0; i < 9; i++) t[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t c = 0;
        const uint32_t bi = b.v[i];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            c += (uint64_t)a.v[j] * bi + t[j];
            t[j] = (uint32_t)c;
            c >>= 32;
        }
        c += t[8];
        const uint32_t t8 = (uint32_t)c, t9 = (uint32_t)(c >> 32);
        const uint32_t m = t[0] * M::INV;
        c = ((uint64_t)m * M::P[0] + t[0]) >> 32;
#pragma unroll
        for (int j = 1; j < 8; j++) {
            c += (uint64_t)m * M::P[j] + t[j];
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        c += t8;
        t[7] = (uint32_t)c;
        t[8] = (uint32_t)(c >> 32) + t9;
    }
    uint32_t lo[8];
#pragma unroll
    for (int i = 0; i < 8; i++) lo[i] = t[i];
    return p256_final_sub<M>(lo, t[8]);
}

template <class M>
P256_FN P256Fe<M> p256_sqr(const P256Fe<M>& a) {
    return p256_mul(a, a);
}

template <class M>
P256_FN P256Fe<M> p256_to_mont(const P256Fe<M>& a) {
    P256Fe<M> r2;
#pragma unroll
    for (int i = 0; i < 8; i++) r2.v[i] = M::R2[i];
    return p256_mul(a, r2);
}
template <class M>
P256_FN P256Fe<M> p256_from_mont(const P256Fe<M>& a) {
    P256Fe<M> one = p256_zero<M>();
    one.v[0] = 1;
    return p256_mul(a, one);
}

// a^(M - 2) (Montgomery in, Montgomery out), by square and multiply over the PUBLIC exponent; 0 -> 0
template <class M>
P256_FN P256Fe<M> p256_inv(const P256Fe<M>& a) {
    P256Fe<M> r = p256_one<M>();
#pragma unroll
    for (int w = 7; w >= 0; w--) {
        const uint32_t e = M::P[w] - (w == 0 ? 2u : 0u);  // (both moduli end in a word >= 2: no borrow)
        for (int bit = 31; bit >= 0; bit--) {
            r = p256_sqr(r);
            if ((e >> bit) & 1) r = p256_mul(r, a);
        }
    }
    return r;
}

// ---- the curve ---------------------------------------------------------------------------------------------------------------
P256_FN P256Fp p256_fp_const(const uint32_t (&w)[8]) {
    P256Fp r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = w[i];
    return r;
}
P256_FN P256Jac p256_identity() {
    P256Jac r;
    r.X = p256_one<P256FpPrm>();
    r.Y = p256_one<P256FpPrm>();
    r.Z = p256_zero<P256FpPrm>();
    return r;
}
P256_FN bool p256_is_identity(const P256Jac& p) { return p256_is_zero(p.Z); }
P256_FN bool p256_is_identity(const P256Affine& p) { return p256_is_zero(p.x) && p256_is_zero(p.y); }
P256_FN P256Jac p256_from_affine(const P256Affine& p) {
    if (p256_is_identity(p)) return p256_identity();
    P256Jac r;
    r.X = p.x;
    r.Y = p.y;
    r.Z = p256_one<P256FpPrm>();
    return r;
}
P256_FN P256Affine p256_generator() {
    P256Affine g;
    g.x = p256_fp_const(P256Curve::GX);
    g.y = p256_fp_const(P256Curve::GY);
    return g;
}

// y^2 = x^3 - 3 x + b (Montgomery coordinates); (0, 0) is not on the curve (b != 0)
P256_FN bool p256_on_curve(const P256Fp& x, const P256Fp& y) {
    const P256Fp x2 = p256_sqr(x);
    P256Fp rhs = p256_mul(x2, x);
    const P256Fp x3 = p256_add(p256_add(x, x), x);
    rhs = p256_add(p256_sub(rhs, x3), p256_fp_const(P256Curve::B));
    return p256_eq(p256_sqr(y), rhs);
}

// 2 P (dbl-2001-b, a = -3).  Z = 0 gives Z3 = (Y + 0)^2 - Y^2 - 0 = 0: the identity stays the identity.  The group has odd
// order, so no point has Y = 0
P256_FN P256Jac p256_dbl(const P256Jac& p) {
    const P256Fp delta = p256_sqr(p.Z), gamma = p256_sqr(p.Y), beta = p256_mul(p.X, gamma);
    const P256Fp t = p256_mul(p256_sub(p.X, delta), p256_add(p.X, delta));
    const P256Fp alpha = p256_add(p256_add(t, t), t);
    const P256Fp beta2 = p256_add(beta, beta), beta4 = p256_add(beta2, beta2), beta8 = p256_add(beta4, beta4);
    P256Jac r;
    r.X = p256_sub(p256_sqr(alpha), beta8);
    r.Z = p256_sub(p256_sub(p256_sqr(p256_add(p.Y, p.Z)), gamma), delta);
    P256Fp g2 = p256_sqr(gamma);
    g2 = p256_add(g2, g2);
    g2 = p256_add(g2, g2);
    g2 = p256_add(g2, g2);
    r.Y = p256_sub(p256_mul(alpha, p256_sub(beta4, r.X)), g2);
    return r;
}

// the shared tail of both additions: P1 = (U1 : S1 : .) and P2 = (U2 : S2 : .) brought to the common denominator, H = U2 - U1
// and Rr = S2 - S1 not both zero, Z3 the product of the denominators times H
P256_FN P256Jac p256_add_tail(const P256Fp& U1, const P256Fp& S1, const P256Fp& H, const P256Fp& Rr, const P256Fp& Z3) {
    const P256Fp H2 = p256_sqr(H), H3 = p256_mul(H2, H), V = p256_mul(U1, H2);
    P256Jac r;
    r.X = p256_sub(p256_sub(p256_sqr(Rr), H3), p256_add(V, V));
    r.Y = p256_sub(p256_mul(Rr, p256_sub(V, r.X)), p256_mul(S1, H3));
    r.Z = Z3;
    return r;
}

// P + Q, Q affine.  The four exceptional cases: P the identity, Q the identity, P = Q (the doubling), P = -Q (the identity)
P256_FN P256Jac p256_add_mixed(const P256Jac& p, const P256Affine& q) {
    if (p256_is_identity(q)) return p;
    if (p256_is_identity(p)) return p256_from_affine(q);
    const P256Fp z2 = p256_sqr(p.Z), U2 = p256_mul(q.x, z2), S2 = p256_mul(q.y, p256_mul(p.Z, z2));
    const P256Fp H = p256_sub(U2, p.X), Rr = p256_sub(S2, p.Y);
    if (p256_is_zero(H)) return p256_is_zero(Rr) ? p256_dbl(p) : p256_identity();
    return p256_add_tail(p.X, p.Y, H, Rr, p256_mul(p.Z, H));
}

// P + Q, both Jacobian; the same four exceptional cases
P256_FN P256Jac p256_add_full(const P256Jac& p, const P256Jac& q) {
    if (p256_is_identity(q)) return p;
    if (p256_is_identity(p)) return q;
    const P256Fp z1 = p256_sqr(p.Z), z2 = p256_sqr(q.Z);
    const P256Fp U1 = p256_mul(p.X, z2), U2 = p256_mul(q.X, z1);
    const P256Fp S1 = p256_mul(p.Y, p256_mul(q.Z, z2)), S2 = p256_mul(q.Y, p256_mul(p.Z, z1));
    const P256Fp H = p256_sub(U2, U1), Rr = p256_sub(S2, S1);
    if (p256_is_zero(H)) return p256_is_zero(Rr) ? p256_dbl(p) : p256_identity();
    return p256_add_tail(U1, S1, H, Rr, p256_mul(p256_mul(p.Z, q.Z), H));
}

// "the affine x of (X : . : Z), reduced mod n, equals r" without an inversion.  r: the signature's r as an integer in [1, n)
// (plain words).  x mod n = r means x = r, or x = r + n where that is still below p, i.e. r < p - n (p - n has 127 bits: no
// signature that can be constructed gets there); x = X / Z^2, so the test is X = r Z^2 resp. X = (r + n) Z^2 in Fp.  Z = 0
// (the identity) is never a match
P256_FN bool p256_x_matches(const P256Fp& X, const P256Fp& Z, const uint32_t (&r)[8]) {
    if (p256_is_zero(Z)) return false;
    const P256Fp z2 = p256_sqr(Z);
    P256Fp rf;
#pragma unroll
    for (int i = 0; i < 8; i++) rf.v[i] = r[i];
    if (p256_eq(X, p256_mul(p256_to_mont(rf), z2))) return true;  // (r < n < p: a reduced element of Fp)
    if (!p256_words_lt(r, P256Curve::P_MINUS_N)) return false;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {  // r + n < p: no carry, reduced
        c += (uint64_t)r[i] + P256FnPrm::P[i];
        rf.v[i] = (uint32_t)c;
        c >>= 32;
    }
    return p256_eq(X, p256_mul(p256_to_mont(rf), z2));
}

// ---- tables --------------------------------------------------------------------------------------------------------------------
// A table of 15 Jacobian points indexed by a per-lane RUNTIME digit must not be a register array (the compiler would send it to
// scratch memory).  The routines below take a store instead: an object with  P256Jac get(int i) const  and  void put(int i, const
// P256Jac&)  for i in [0, 15).  P256LocalStore is a plain array (host; one point set per call); es256.hip's store lives in LDS.
struct P256LocalStore {
    P256Jac t[15];
    __host__ __device__ P256Jac get(int i) const { return t[i]; }
    __host__ __device__ void put(int i, const P256Jac& p) { t[i] = p; }
};

constexpr int P256_COMB_WINDOWS = 64, P256_COMB_ENTRIES = 15;  // the comb of G: entry [w][j] = (j + 1) 16^w G, affine
constexpr int P256_COMB_POINTS = P256_COMB_WINDOWS * P256_COMB_ENTRIES;

// st[j] = (j + 1) B, j = 0 .. 14
template <class Store>
P256_FN void p256_multiples(Store& st, const P256Jac& B) {
    st.put(0, B);
    P256Jac acc = p256_dbl(B);
    st.put(1, acc);
    for (int j = 2; j < 15; j++) {
        acc = p256_add_full(acc, B);
        st.put(j, acc);
    }
}

// Window w of the comb: out[0 .. 15) = (j + 1) 16^w G in affine form, through `st` as working space.  The 15 points are
// normalised with ONE inversion (Montgomery's trick over their Z; none of them is the identity: (j + 1) 16^w < n).  The windows are
// independent: the device builds all 64 side by side, one per lane (es256.hip), the host one after another.  out[j].x holds the
// running products in between
template <class Store>
P256_FN void p256_comb_window(int w, Store& st, P256Affine* out) {
    P256Jac B = p256_from_affine(p256_generator());
    for (int i = 0; i < 4 * w; i++) B = p256_dbl(B);
    p256_multiples(st, B);
    P256Fp run = p256_one<P256FpPrm>();
    for (int j = 0; j < 15; j++) {
        out[j].x = run;  // the product of Z_0 .. Z_{j-1}
        run = p256_mul(run, st.get(j).Z);
    }
    P256Fp inv = p256_inv(run);
    for (int j = 14; j >= 0; j--) {
        const P256Jac pj = st.get(j);
        const P256Fp zi = p256_mul(inv, out[j].x), zi2 = p256_sqr(zi);
        inv = p256_mul(inv, pj.Z);
        out[j].x = p256_mul(pj.X, zi2);
        out[j].y = p256_mul(pj.Y, p256_mul(zi2, zi));
    }
}

// the top base-16 digit of k, and k moved up by one digit: the windows are walked from the top without ever indexing the
// scalar's words by a runtime value (k[w >> 3] would move the scalar from registers into scratch memory)
P256_FN uint32_t p256_take_digit(uint32_t (&k)[8]) {
    const uint32_t d = k[7] >> 28;
#pragma unroll
    for (int j = 7; j > 0; j--) k[j] = (k[j] << 4) | (k[j - 1] >> 28);
    k[0] <<= 4;
    return d;
}

// ---- the rule --------------------------------------------------------------------------------------------------------------------
// The key's part of the rule alone, for a caller that has a key and no signature yet (webauthn_register.hip.h): x, y as eight
// little-endian words each.  ZK_ES256_RANGE unless both are below p, ZK_ES256_OFF_CURVE unless (x, y) is on the curve: the two
// tests p256_verify_with applies to a record's key, from the same primitives
P256_FN uint8_t p256_key_check(const uint32_t (&x)[8], const uint32_t (&y)[8]) {
    if (!p256_words_lt(x, P256FpPrm::P) || !p256_words_lt(y, P256FpPrm::P)) return ZK_ES256_RANGE;
    P256Affine Q;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        Q.x.v[i] = x[i];
        Q.y.v[i] = y[i];
    }
    return p256_on_curve(p256_to_mont(Q.x), p256_to_mont(Q.y)) ? ZK_ES256_VALID : ZK_ES256_OFF_CURVE;
}

// One request: sig = pubkey_x || pubkey_y || r || s || msghash, each 32 little-endian bytes.  Returns the FIRST failing test
// (ZK_ES256_RANGE, ZK_ES256_OFF_CURVE, ZK_ES256_MISMATCH) or ZK_ES256_VALID.  g_table: the comb of G (P256_COMB_POINTS entries).
// `st`: working space for the multiples of Q.  u2 Q: 4-bit windows over st, 4 doublings per window; u1 G: mixed additions from
// the comb into a second accumulator, no doublings; the two meet in one full addition, which is where u1 G = +- u2 Q lands
template <class Store>
P256_FN uint8_t p256_verify_with(const uint8_t* sig, const P256Affine* g_table, Store& st) {
    uint32_t f[5][8];
#pragma unroll
    for (int k = 0; k < 5; k++)
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint8_t* b = sig + 32 * k + 4 * i;
            f[k][i] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        }
    const uint32_t(&x)[8] = f[0], (&y)[8] = f[1], (&r)[8] = f[2], (&s)[8] = f[3], (&z)[8] = f[4];
    uint32_t rs = 0, ss = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        rs |= r[i];
        ss |= s[i];
    }
    if (!p256_words_lt(x, P256FpPrm::P) || !p256_words_lt(y, P256FpPrm::P) || !p256_words_lt(z, P256FnPrm::P) || rs == 0 ||
        !p256_words_lt(r, P256FnPrm::P) || ss == 0 || !p256_words_lt(s, P256FnPrm::P))
        return ZK_ES256_RANGE;
    P256Affine Q;
    P256Fn sn, rn, zn;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        Q.x.v[i] = x[i];
        Q.y.v[i] = y[i];
        sn.v[i] = s[i];
        rn.v[i] = r[i];
        zn.v[i] = z[i];
    }
    Q.x = p256_to_mont(Q.x);
    Q.y = p256_to_mont(Q.y);
    if (!p256_on_curve(Q.x, Q.y)) return ZK_ES256_OFF_CURVE;
    // u1 = z / s, u2 = r / s as integers: (z R)(s R)^-1 ... the Montgomery factors cancel through one product with the plain z, r
    const P256Fn w = p256_inv(p256_to_mont(sn));  // s^-1 R
    P256Fn u1 = p256_mul(zn, w), u2 = p256_mul(rn, w);
    p256_multiples(st, p256_from_affine(Q));
    P256Jac aq = p256_identity(), ag = p256_identity();
    for (int i = P256_COMB_WINDOWS - 1; i >= 0; i--) {
        for (int d = 0; d < 4; d++) aq = p256_dbl(aq);
        const uint32_t d2 = p256_take_digit(u2.v), d1 = p256_take_digit(u1.v);  // digit i of each
        if (d2) aq = p256_add_full(aq, st.get((int)d2 - 1));
        if (d1) ag = p256_add_mixed(ag, g_table[i * P256_COMB_ENTRIES + (int)d1 - 1]);
    }
    const P256Jac sum = p256_add_full(ag, aq);
    return p256_x_matches(sum.X, sum.Z, r) ? ZK_ES256_VALID : ZK_ES256_MISMATCH;
}

// The same with the working space of the caller's side: a local array on the host; on the device the wave's LDS block (one
// signature per lane, a workgroup of ONE wave of 64 lanes: 15 x 24 words per lane, word-interleaved across the lanes so that a
// wave's accesses fall into 64 different banks whatever digit each lane holds)
#if defined(__HIPCC__)
struct P256LdsStore {
    uint32_t* base;  // [15][24][64] words
    __device__ __forceinline__ P256Jac get(int i) const {
        P256Jac p;
        const uint32_t* q = base + (size_t)i * 24 * 64;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            p.X.v[k] = q[k * 64];
            p.Y.v[k] = q[(8 + k) * 64];
            p.Z.v[k] = q[(16 + k) * 64];
        }
        return p;
    }
    __device__ __forceinline__ void put(int i, const P256Jac& p) {
        uint32_t* q = base + (size_t)i * 24 * 64;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            q[k * 64] = p.X.v[k];
            q[(8 + k) * 64] = p.Y.v[k];
            q[(16 + k) * 64] = p.Z.v[k];
        }
    }
};
constexpr int P256_LDS_WORDS = 15 * 24 * 64;  // 90 KiB of the CU's 160
__device__ __forceinline__ P256LdsStore p256_lds_store() {
    __shared__ uint32_t p256_lds[P256_LDS_WORDS];
    P256LdsStore st;
    st.base = p256_lds + (threadIdx.x & 63u);
    return st;
}
#endif

P256_FN uint8_t p256_verify_one(const uint8_t sig[160], const P256Affine* g_table) {
#if defined(__HIP_DEVICE_COMPILE__)
    P256LdsStore st = p256_lds_store();
#else
    P256LocalStore st;
#endif
    return p256_verify_with(sig, g_table, st);
}

}  // namespace zk
