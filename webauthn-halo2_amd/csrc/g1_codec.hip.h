// g1_codec.hip.h — which bytes are a BN254 field element or a G1 point: the one statement of every encoding rule the engine has.
//
// Every function here is __host__ __device__ in ONE portable form (the pattern of p256.hip.h): the codec kernels (serde.hip,
// verify.hip) are index arithmetic around a call, the host readers and writers (serde_host.h, transcript.h, verifier.h) call
// the same functions, and a CPU program runs them under the sanitizers (tests/serde_host_check.cpp).  A rule that differs between
// two users — the identity is a point of a file and no point of a proof; RawBytesUnchecked validates nothing — is not in here:
// it is stated at the call site that owns it.
//
//   field element   32 bytes, the integer little-endian (halo2's `to_repr`, the Blake2b transcript) or big-endian (the EVM
//                   transcript); canonical = the integer is below the modulus (Fe::below_modulus, field.hip.h)
//   compressed G1   x little-endian with the parity of y in bit 255; all zero = the identity (SerdeFormat::Processed, the
//                   Blake2b transcript)
//   EVM G1          x || y big-endian, 64 bytes; there is no identity
//   RawBytes G1     the Montgomery image x || y as it lies in memory; (0, 0) = the identity
#pragma once
#include <stdint.h>

#include "ec.hip.h"
#include "field.hip.h"

#define ZK_CODEC_FN __host__ __device__ inline

namespace zk {

ZK_CODEC_FN Fq fq_small(uint32_t x) {
    Fq t = Fq::zero();
    t.v[0] = x;
    return fe_to_mont(t);
}
// the curve y^2 = x^3 + 3 (Montgomery)
ZK_CODEC_FN Fq g1_curve_rhs(const Fq& x) { return fe_add(fe_mul(fe_sqr(x), x), fq_small(3)); }
ZK_CODEC_FN bool g1_on_curve(const Fq& x, const Fq& y) { return fe_sqr(y) == g1_curve_rhs(x); }

// (p + 1) / 4, the exponent of the square root (p = 3 mod 4), worked out of FqParams::P by the compiler
constexpr uint32_t fq_sqrt_exp_word(int i) {
    uint32_t t[9] = {};  // p + 1; p < 2^254, so t[8] = 0
    uint64_t c = 1;
    for (int k = 0; k < 8; k++) {
        c += FqParams::P[k];
        t[k] = (uint32_t)c;
        c >>= 32;
    }
    return (t[i] >> 2) | (t[i + 1] << 30);
}
struct FqSqrt {
    static constexpr uint32_t EXP[8] = {fq_sqrt_exp_word(0), fq_sqrt_exp_word(1), fq_sqrt_exp_word(2), fq_sqrt_exp_word(3),
                                        fq_sqrt_exp_word(4), fq_sqrt_exp_word(5), fq_sqrt_exp_word(6), fq_sqrt_exp_word(7)};
};
// 4 EXP = p + 1 over all eight words, multiplied back out word by word
constexpr bool fq_sqrt_exp_is_exact() {
    uint64_t c4 = 0, c1 = 1;
    for (int k = 0; k < 8; k++) {
        c4 += 4 * (uint64_t)FqSqrt::EXP[k];
        c1 += FqParams::P[k];
        if ((uint32_t)c4 != (uint32_t)c1) return false;
        c4 >>= 32;
        c1 >>= 32;
    }
    return c4 == 0 && c1 == 0;
}
static_assert((FqParams::P[0] & 3u) == 3u && fq_sqrt_exp_is_exact(), "a^((p + 1) / 4) is a root only for p = 3 (mod 4), and EXP must be that exponent");
// *r = a root of a (Montgomery); false if a is not a square
ZK_CODEC_FN bool fq_sqrt(const Fq& a, Fq* r) {
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = FqSqrt::EXP[i];
    *r = fe_pow(a, e);
    return fe_sqr(*r) == a;
}

// 32 bytes <-> the 256-bit integer they spell (no reduction, no Montgomery conversion)
template <class PRM>
ZK_CODEC_FN Fe<PRM> fe_from_bytes(const uint8_t* b, bool big_endian) {
    Fe<PRM> r;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        uint32_t w = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) w |= (uint32_t)(big_endian ? b[31 - (4 * k + t)] : b[4 * k + t]) << (8 * t);
        r.v[k] = w;
    }
    return r;
}
template <class PRM>
ZK_CODEC_FN void fe_to_bytes(const Fe<PRM>& a, bool big_endian, uint8_t* b) {
#pragma unroll
    for (int i = 0; i < 32; i++) b[big_endian ? 31 - i : i] = (uint8_t)(a.v[i >> 2] >> (8 * (i & 3)));
}

// compressed G1 -> affine Montgomery.  Refused: x >= p, or x^3 + 3 not a square (x = 0 with the sign bit among them: 3 is not a
// square).  *out is (0, 0) unless the answer is G1_POINT
enum G1Decoded { G1_REFUSED = 0, G1_IDENTITY = 1, G1_POINT = 2 };
ZK_CODEC_FN G1Decoded g1_decompress(const uint8_t* b, G1Affine* out) {
    Fq x = fe_from_bytes<FqParams>(b, false);
    const uint32_t sign = x.v[7] >> 31;
    x.v[7] &= 0x7fffffffu;
    out->x = Fq::zero();
    out->y = Fq::zero();
    if (!x.below_modulus()) return G1_REFUSED;
    if (x.is_zero() && !sign) return G1_IDENTITY;
    const Fq xm = fe_to_mont(x);
    Fq y;
    if (!fq_sqrt(g1_curve_rhs(xm), &y)) return G1_REFUSED;
    if ((fe_from_mont(y).v[0] & 1u) != sign) y = fe_neg(y);
    out->x = xm;
    out->y = y;
    return G1_POINT;
}
ZK_CODEC_FN void g1_compress(const G1Affine& p, uint8_t* b) {
    Fq x = Fq::zero();
    if (!affine_is_identity(p)) {
        x = fe_from_mont(p.x);
        x.v[7] |= (fe_from_mont(p.y).v[0] & 1u) << 31;
    }
    fe_to_bytes(x, false, b);
}

// the EVM transcript's point: both coordinates canonical, on the curve, not (0, 0).  *out is (0, 0) when refused
ZK_CODEC_FN bool g1_read_evm(const uint8_t* b, G1Affine* out) {
    const Fq x = fe_from_bytes<FqParams>(b, true), y = fe_from_bytes<FqParams>(b + 32, true);
    out->x = Fq::zero();
    out->y = Fq::zero();
    if (!x.below_modulus() || !y.below_modulus() || (x.is_zero() && y.is_zero())) return false;
    const Fq xm = fe_to_mont(x), ym = fe_to_mont(y);
    if (!g1_on_curve(xm, ym)) return false;
    out->x = xm;
    out->y = ym;
    return true;
}
ZK_CODEC_FN void g1_write_evm(const G1Affine& p, uint8_t* b) {
    fe_to_bytes(fe_from_mont(p.x), true, b);
    fe_to_bytes(fe_from_mont(p.y), true, b + 32);
}

// the checked RawBytes rule for a Montgomery image: both coordinates below p, and on the curve or the identity (0, 0)
ZK_CODEC_FN bool g1_raw_is_valid(const G1Affine& p) {
    return p.x.below_modulus() && p.y.below_modulus() && (affine_is_identity(p) || g1_on_curve(p.x, p.y));
}

}  // namespace zk
