// srs_update.h — the host half of one ceremony contribution (zk_srs_update, g1_ntt.hip): the G2 step, the receipt and its check.
//
// A contribution multiplies a secret s into the SRS: g[i] -> [s^i] g[i], s_g2 -> [s] s_g2, so tau -> s tau.  Its receipt holds
// g[1] before and after, [s] G1 and [s] G2.  The check is a knowledge-of-exponent style argument, not a Schnorr proof: the
// pair ([s] G1, [s] G2) can only be made by somebody who knows s (the knowledge-of-exponent assumption over a pairing), and
// the two pairing equations tie that one s to the step from before_g1 to after_g1.  Nothing here needs a device, so the
// rule is compiled and tested on its own (tests/srs_update_host_check.cpp).
#pragma once
#include <string.h>

#include "../../include/zkmi355.h"
#include "pairing.h"

namespace zk {

// overwrite secret bytes in a way the optimiser may not drop
inline void secure_zero(void* p, size_t n) {
    volatile uint8_t* v = (volatile uint8_t*)p;
    while (n--) *v++ = 0;
}

inline G1Affine g1_from_words(const uint64_t w[8]) {
    G1Affine p;
    memcpy(p.x.v, w, 32);
    memcpy(p.y.v, w + 4, 32);
    return p;
}
inline void g1_to_words(const G1Affine& p, uint64_t w[8]) {
    memcpy(w, p.x.v, 32);
    memcpy(w + 4, p.y.v, 32);
}
// (g1_is_proper, and g2_is_proper, the same for G2 with the subgroup test, are pairing.h's: the device form of the receipt rule,
// contribution_check_lanes, and zk_pairing_check_batch apply them too)

inline G1Affine g1_generator_host() {
    G1Affine g;
    g.x = Fq::one();
    g.y = fe_add(Fq::one(), Fq::one());
    return g;
}
inline G1Affine g1x_to_affine_host(const G1X& p) {
    G1Affine r;
    if (p.is_identity()) {
        r.x = Fq::zero();
        r.y = Fq::zero();
        return r;
    }
    const Fq t = fe_inv_fast(p.zzz);  // 1/ZZZ
    const Fq u = fe_mul(p.zz, t);     // 1/Z
    r.x = fe_mul(p.x, fe_sqr(u));
    r.y = fe_mul(p.y, t);
    return r;
}
// [s] p on the host; every bit takes a doubling and an addition (the unused sum is dropped), so the sequence of point
// operations does not depend on s
inline G1Affine g1_mul_host(const G1Affine& p, const Fr& s_mont) {
    Fr s = fe_from_mont(s_mont);
    G1X acc = G1X::identity();
    if (!affine_is_identity(p)) {
        for (int i = 255; i >= 0; i--) {
            acc = g1x_dbl(acc);
            G1X t = acc;
            g1x_add_affine(t, p.x, p.y);
            if ((s.v[i >> 5] >> (i & 31)) & 1) acc = t;
        }
    }
    secure_zero(&s, sizeof(s));
    return g1x_to_affine_host(acc);
}

// s_g2' = [s] s_g2 on raw images (zk_srs_set_g2's layout); pairing.h's g2_mul with its canonical copy of s cleared
inline void srs_update_s_g2(const uint8_t s_g2_raw[128], const Fr& s_mont, uint8_t out[128]) {
    G2A p = g2_from_raw(s_g2_raw);
    Fr s = fe_from_mont(s_mont);
    G2A acc{p.x, p.y, true};
    for (int i = 0; i < 256; i++) {
        if ((s.v[i >> 5] >> (i & 31)) & 1) acc = g2_add(acc, p);
        p = g2_add(p, p);
    }
    secure_zero(&s, sizeof(s));
    g2_to_raw(acc, out);
}

// the first Fr draw of ChaCha20Rng::from_seed(seed) (zk_srs_setup's rule for its tau), leaving nothing of the keystream behind
inline Fr srs_update_secret(const uint8_t seed[32]) {
    ChaCha20Rng rng(seed);
    uint8_t b[64];
    rng.fill(b, 64);
    const Fr s = fr_from_u512_le(b);
    secure_zero(b, sizeof(b));
    secure_zero(&rng, sizeof(rng));
    return s;
}

// the receipt of a step by s from an SRS whose g[1] is before_g1 (after_g1 is read back from the device by the caller)
inline void srs_contribution_make(const G1Affine& before_g1, const G1Affine& after_g1, const Fr& s_mont, zk_srs_contribution* out) {
    g1_to_words(before_g1, out->before_g1);
    g1_to_words(after_g1, out->after_g1);
    g1_to_words(g1_mul_host(g1_generator_host(), s_mont), out->s_g1);
    uint8_t gen[128], sg[128];
    g2_to_raw(g2_generator(), gen);
    srs_update_s_g2(gen, s_mont, sg);
    memcpy(out->s_g2, sg, 128);
}

// ZK_SRS_CONTRIB_SAME_SECRET | LINKS | NONTRIVIAL of a receipt: three pairing equations' worth of host work.  A receipt
// whose points are not proper group elements gets no pairing bit either: the equations mean nothing for such input.
inline uint32_t srs_contribution_flags(const zk_srs_contribution& c) {
    const G1Affine before = g1_from_words(c.before_g1), after = g1_from_words(c.after_g1), s_g1 = g1_from_words(c.s_g1);
    uint8_t raw[128];
    memcpy(raw, c.s_g2, 128);
    const G2A s_g2 = g2_from_raw(raw);
    const G1Affine gen = g1_generator_host();
    if (!g1_is_proper(before) || !g1_is_proper(after) || !g1_is_proper(s_g1) || !g2_is_proper(s_g2)) return 0;
    uint32_t f = 0;
    if (!(s_g1.x == gen.x && s_g1.y == gen.y)) f |= ZK_SRS_CONTRIB_NONTRIVIAL;
    const G2A g2 = g2_generator();
    // pairing_check(a, b, g2, s_g2): e(a, s_g2) == e(b, g2)
    if (pairing_check(gen, s_g1, g2, s_g2)) f |= ZK_SRS_CONTRIB_SAME_SECRET;  // e(G1, s_g2) == e(s_g1, G2)
    if (pairing_check(before, after, g2, s_g2)) f |= ZK_SRS_CONTRIB_LINKS;    // e(before_g1, s_g2) == e(after_g1, G2)
    return f;
}

}  // namespace zk
