// serde_host.h — the host half of the file codecs (serde.hip): one G1 / G2 point <-> bytes in a SerdeFormat, the square root
// in Fq2 that the compressed G2 encoding needs, and the bounded reader / writer over a caller's buffer.  Nothing here needs a
// device, so the admission rules are compiled and tested on their own (tests/serde_host_check.cpp).
#pragma once
#include <string.h>

#include "../../include/zkmi355.h"
#include "pairing.h"

namespace zk {

// one G1 point <-> bytes in `format` (the rules themselves: g1_codec.hip.h); false on a malformed point
inline size_t g1_size(int format) { return format == ZK_SERDE_PROCESSED ? 32 : 64; }

inline bool host_g1_read(const uint8_t* b, int format, G1Affine* out) {
    if (format == ZK_SERDE_PROCESSED) return g1_decompress(b, out) != G1_REFUSED;  // a file may hold the identity
    memcpy(out, b, 64);
    return format != ZK_SERDE_RAW_BYTES || g1_raw_is_valid(*out);  // RawBytesUnchecked: the bytes as they are
}

inline void host_g1_write(const G1Affine& p, int format, uint8_t* b) {
    if (format == ZK_SERDE_PROCESSED) g1_compress(p, b);
    else memcpy(b, &p, 64);
}

// sqrt in Fq2 (complex method); false if `a` is not a square
inline bool f2_sqrt(const Fq2& a, Fq2* out) {
    if (f2_is_zero(a)) {
        *out = a;
        return true;
    }
    if (a.c1.is_zero()) {  // an element of Fq is always a square here: its root lies in Fq, or is sqrt(-c0) u for a non-residue c0
        Fq r;             // (the complex method below meets delta = 0 on a non-residue c0 and would refuse it)
        if (fq_sqrt(a.c0, &r)) {
            *out = Fq2{r, Fq::zero()};
            return true;
        }
        if (!fq_sqrt(fe_neg(a.c0), &r)) return false;
        *out = Fq2{Fq::zero(), r};
        return true;
    }
    Fq alpha;
    if (!fq_sqrt(fe_add(fe_sqr(a.c0), fe_sqr(a.c1)), &alpha)) return false;
    const Fq half = fe_inv(fq_small(2));
    Fq delta = fe_mul(fe_add(a.c0, alpha), half), x0;
    if (!fq_sqrt(delta, &x0)) {
        delta = fe_mul(fe_sub(a.c0, alpha), half);
        if (!fq_sqrt(delta, &x0)) return false;
    }
    if (x0.is_zero()) return false;
    const Fq x1 = fe_mul(a.c1, fe_inv(fe_add(x0, x0)));
    *out = Fq2{x0, x1};
    return f2_eq(f2_mul(*out, *out), a);
}

inline size_t g2_size(int format) { return format == ZK_SERDE_PROCESSED ? 64 : 128; }
inline void host_g2_write(const uint8_t raw[128], int format, uint8_t* b) {
    if (format != ZK_SERDE_PROCESSED) {
        memcpy(b, raw, 128);
        return;
    }
    const G2A p = g2_from_raw(raw);
    if (p.inf) {
        memset(b, 0, 64);
        return;
    }
    const Fq x0 = fe_from_mont(p.x.c0), x1 = fe_from_mont(p.x.c1);
    memcpy(b, x0.v, 32);
    memcpy(b + 32, x1.v, 32);
    b[63] |= (uint8_t)((fe_from_mont(p.y.c0).v[0] & 1u) << 7);
}
inline bool host_g2_read(const uint8_t* b, int format, uint8_t raw[128]) {
    if (format != ZK_SERDE_PROCESSED) {
        memcpy(raw, b, 128);
        if (format == ZK_SERDE_RAW_BYTES) {
            const G2A p = g2_from_raw(raw);
            if (!p.x.c0.below_modulus() || !p.x.c1.below_modulus() || !p.y.c0.below_modulus() || !p.y.c1.below_modulus()) return false;
            if (!p.inf && !g2_on_curve(p)) return false;
        }
        return true;
    }
    Fq x0 = fe_from_bytes<FqParams>(b, false), x1 = fe_from_bytes<FqParams>(b + 32, false);
    const uint32_t sign = x1.v[7] >> 31;
    x1.v[7] &= 0x7fffffffu;
    if (!x0.below_modulus() || !x1.below_modulus()) return false;
    G2A p;
    p.inf = false;
    if (x0.is_zero() && x1.is_zero() && !sign) {
        memset(raw, 0, 128);
        return true;
    }
    p.x = Fq2{fe_to_mont(x0), fe_to_mont(x1)};
    if (!f2_sqrt(f2_add(f2_mul(f2_mul(p.x, p.x), p.x), f2_twist_b()), &p.y)) return false;
    if ((fe_from_mont(p.y.c0).v[0] & 1u) != sign) p.y = Fq2{fe_neg(p.y.c0), fe_neg(p.y.c1)};
    g2_to_raw(p, raw);
    return true;
}

inline void put_be32(uint8_t* b, uint32_t v) {
    b[0] = (uint8_t)(v >> 24);
    b[1] = (uint8_t)(v >> 16);
    b[2] = (uint8_t)(v >> 8);
    b[3] = (uint8_t)v;
}
inline uint32_t get_be32(const uint8_t* b) { return ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3]; }

// a bounded reader / writer over the caller's buffer
struct Out {
    uint8_t* p;
    size_t cap, pos = 0;
    bool real;  // false: size computation only
    Out(uint8_t* buf, size_t c) : p(buf), cap(c), real(buf != nullptr) {}
    uint8_t* take(size_t n) {
        uint8_t* r = (real && pos + n <= cap) ? p + pos : nullptr;
        if (real && pos + n > cap) real = false;  // overflow: keep counting, report ZK_EINVAL at the end
        pos += n;
        return r;
    }
};
struct In {
    const uint8_t* p;
    size_t len, pos = 0;
    const uint8_t* take(size_t n) {
        if (n > len - pos) return nullptr;
        const uint8_t* r = p + pos;
        pos += n;
        return r;
    }
};

}  // namespace zk
