// webauthn.hip.h — the relying party's check of a WebAuthn assertion (navigator.credentials.get, ES256): SHA-256, strict DER of
// the signature, the rules for clientDataJSON and authenticatorData, and the assembly of the 160-byte record p256_verify_one takes.
//
// Like p256.hip.h, every function is __host__ __device__ in ONE portable form, no inline assembly: the kernel (webauthn.hip) is a
// wrapper around webauthn_digest_one, and a CPU program runs the same code (tests/webauthn_host_check.cpp does, under the
// sanitizers).  NOT constant time, on purpose: everything an assertion carries is public request data; nothing here may be used
// with a secret.  At the end stands the host-only packing of a batch into its upload image ("the upload image of a batch"),
// which that program calls too.
//
// The rule.  An assertion is (authenticatorData, clientDataJSON, a DER signature, the credential's public key) and the relying
// party's expectations (the challenge it issued, its origin, SHA-256 of its RP ID, the flags it requires, whether it accepts a
// cross-origin call).  webauthn_check_one applies these tests in this order and returns the FIRST that fails:
//   SIZE           authenticatorData longer than 1024 bytes, clientDataJSON longer than 4096, a signature outside 8 .. 72 bytes, a
//                  challenge outside 1 .. 64 bytes, an origin longer than 255
//   AUTHDATA       authenticatorData shorter than 37 bytes
//   RPID           bytes 0 .. 31 of authenticatorData differ from the expected rpIdHash
//   FLAGS          (flags & required) != required; flags is byte 32, UP = 0x01, UV = 0x04.  Bytes 33 .. 36, big-endian, are the
//                  signature counter: returned, not judged
//   CLIENTDATA     the "limited verification algorithm" of WebAuthn Level 2 (5.8.1.2; 5.8.1.1 fixes the serialisation it relies on).
//                  With  E = {"type":"webauthn.get","challenge":"  +  base64url-without-padding(challenge)  +  ","origin":"  +
//                  origin  +  ","crossOrigin":   clientDataJSON passes iff it starts with E, the bytes after E start with `true`
//                  or `false`, the byte after that word is `,` or `}`, and the last byte of the whole string is `}`; `true` passes
//                  only where the policy allows cross-origin.  The caller builds E (webauthn_expected_prefix: base64url and
//                  concatenation); the check compares bytes.  There is NO JSON parser here: a clientDataJSON with the same members
//                  in any other order, or with insignificant white space, is a CLIENTDATA verdict, although a full parse would
//                  accept it.  Conforming clients serialise exactly this way.
//   SIGNATURE_DER  the signature is not the strict DER of ECDSA-Sig-Value,  30 len 02 lr r 02 ls s : short-form lengths only, len
//                  equal to the remaining length exactly, each INTEGER of 1 .. 33 content bytes with the top bit of the first clear
//                  (non-negative), a leading 00 only where the next byte has its top bit set (minimal), a 33-byte INTEGER starting
//                  with 00, nothing after s
//   then p256_verify_one's RANGE, OFF_CURVE, MISMATCH over the assembled record: pubkey_x || pubkey_y || r || s || msghash, each
//   32 LITTLE-endian bytes (zk_es256_verify's order), msghash = SHA-256(authenticatorData || SHA-256(clientDataJSON)) read as a
//   big-endian integer, so its bytes are reversed.
//
// SHA-256 (FIPS 180-4) on the device: the eight state words and a rolling 16-word schedule sit in registers — every index is a
// compile-time constant after the rounds are unrolled; a runtime-indexed W[] would go to scratch memory.  Message words are
// assembled from byte loads: the records of a batch are packed back to back, so no alignment is assumed.  The message is a
// concatenation of two pieces (the second hash is authenticatorData, then the first digest).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "p256.hip.h"

#ifndef ZK_WEBAUTHN_SIZE  // (include/zkmi355.h defines the same: this header also stands alone)
#define ZK_WEBAUTHN_VALID 0
#define ZK_WEBAUTHN_RANGE 1
#define ZK_WEBAUTHN_OFF_CURVE 2
#define ZK_WEBAUTHN_MISMATCH 3
#define ZK_WEBAUTHN_SIZE 4
#define ZK_WEBAUTHN_AUTHDATA 5
#define ZK_WEBAUTHN_RPID 6
#define ZK_WEBAUTHN_FLAGS 7
#define ZK_WEBAUTHN_CLIENTDATA 8
#define ZK_WEBAUTHN_SIGNATURE_DER 9
#define ZK_WEBAUTHN_AUTHDATA_MAX 1024
#define ZK_WEBAUTHN_CLIENTDATA_MAX 4096
#define ZK_WEBAUTHN_CHALLENGE_MAX 64
#define ZK_WEBAUTHN_ORIGIN_MAX 255
#endif

namespace zk {

constexpr uint32_t WEBAUTHN_AUTHDATA_MIN = 37, WEBAUTHN_SIG_MIN = 8, WEBAUTHN_SIG_MAX = 72;
// the longest E: the three literal parts (36 + 12 + 16 bytes), 86 base64url characters of a 64-byte challenge, the origin
constexpr uint32_t WEBAUTHN_PREFIX_MAX = 36 + 86 + 12 + ZK_WEBAUTHN_ORIGIN_MAX + 16;

// ---- SHA-256 -------------------------------------------------------------------------------------------------------------------
struct Sha256Consts {
    static constexpr uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
        0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
        0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
        0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
        0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
        0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
};

P256_FN uint32_t sha256_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// byte `pos` of the padded message  p0[0 .. len0) || p1[0 .. len1) || 80 || 00 ...  (the length words are put in by the caller)
P256_FN uint32_t sha256_byte(const uint8_t* p0, uint32_t len0, const uint8_t* p1, uint32_t len, uint32_t pos) {
    if (pos < len0) return p0[pos];
    if (pos < len) return p1[pos - len0];
    return pos == len ? 0x80u : 0u;
}

// big-endian word at `pos` (a multiple of 4) of the padded message: four byte loads from one piece where the word lies inside
// it, the byte rule above at the seams and in the padding
P256_FN uint32_t sha256_word(const uint8_t* p0, uint32_t len0, const uint8_t* p1, uint32_t len, uint32_t pos) {
    const uint8_t* b = nullptr;
    if (pos + 4 <= len0)
        b = p0 + pos;
    else if (pos >= len0 && pos + 4 <= len)
        b = p1 + (pos - len0);
    if (b) return ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | (uint32_t)b[3];
    return (sha256_byte(p0, len0, p1, len, pos) << 24) | (sha256_byte(p0, len0, p1, len, pos + 1) << 16) |
           (sha256_byte(p0, len0, p1, len, pos + 2) << 8) | sha256_byte(p0, len0, p1, len, pos + 3);
}

// h[0 .. 8) = SHA-256(p0[0 .. len0) || p1[0 .. len1)); len0 + len1 < 2^29.  p1 may be null where len1 is 0
P256_FN void sha256_two(const uint8_t* p0, uint32_t len0, const uint8_t* p1, uint32_t len1, uint32_t (&h)[8]) {
    const uint32_t len = len0 + len1, blocks = (len + 9 + 63) / 64;
    h[0] = 0x6a09e667u, h[1] = 0xbb67ae85u, h[2] = 0x3c6ef372u, h[3] = 0xa54ff53au;
    h[4] = 0x510e527fu, h[5] = 0x9b05688cu, h[6] = 0x1f83d9abu, h[7] = 0x5be0cd19u;
    for (uint32_t blk = 0; blk < blocks; blk++) {
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = sha256_word(p0, len0, p1, len, blk * 64 + 4 * (uint32_t)j);
        if (blk == blocks - 1) w[15] |= len << 3;  // the bit length: below 2^32, so the high word stays 0
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
        for (int t = 0; t < 64; t++) {
            if (t >= 16) {
                const uint32_t w15 = w[(t - 15) & 15], w2 = w[(t - 2) & 15];
                const uint32_t s0 = sha256_rotr(w15, 7) ^ sha256_rotr(w15, 18) ^ (w15 >> 3);
                const uint32_t s1 = sha256_rotr(w2, 17) ^ sha256_rotr(w2, 19) ^ (w2 >> 10);
                w[t & 15] += s0 + w[(t - 7) & 15] + s1;
            }
            const uint32_t S1 = sha256_rotr(e, 6) ^ sha256_rotr(e, 11) ^ sha256_rotr(e, 25);
            const uint32_t t1 = hh + S1 + ((e & f) ^ (~e & g)) + Sha256Consts::K[t] + w[t & 15];
            const uint32_t S0 = sha256_rotr(a, 2) ^ sha256_rotr(a, 13) ^ sha256_rotr(a, 22);
            const uint32_t t2 = S0 + ((a & b) ^ (a & c) ^ (b & c));
            hh = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
        }
        h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += hh;
    }
}

// the digest as its 32 bytes (big-endian words)
P256_FN void sha256_put(const uint32_t (&h)[8], uint8_t* out) {
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) out[4 * i + j] = (uint8_t)(h[i] >> (24 - 8 * j));
}

// ---- strict DER of ECDSA-Sig-Value ----------------------------------------------------------------------------------------------
// One INTEGER at sig[pos ..): tag, short-form length 1 .. 33, non-negative, minimal, below 2^256.  On success `off` / `n` name its
// value bytes without the leading 00 (n in 0 .. 32: `02 01 00` has none) and pos moves past it
P256_FN bool webauthn_der_int(const uint8_t* sig, uint32_t len, uint32_t& pos, uint32_t& off, uint32_t& n) {
    if (pos + 2 > len || sig[pos] != 0x02) return false;
    const uint32_t l = sig[pos + 1];
    if (l < 1 || l > 33 || pos + 2 + l > len) return false;  // (a long-form length byte, 0x80 and above, is > 33)
    const uint32_t first = sig[pos + 2];
    if (first & 0x80) return false;
    if (l > 1 && first == 0 && !(sig[pos + 3] & 0x80)) return false;
    if (l == 33 && first != 0) return false;
    const uint32_t skip = first == 0 ? 1 : 0;
    off = pos + 2 + skip;
    n = l - skip;
    pos += 2 + l;
    return true;
}

P256_FN bool webauthn_der_parse(const uint8_t* sig, uint32_t len, uint32_t& r_off, uint32_t& r_n, uint32_t& s_off, uint32_t& s_n) {
    if (len < WEBAUTHN_SIG_MIN || len > WEBAUTHN_SIG_MAX) return false;
    if (sig[0] != 0x30 || sig[1] != len - 2) return false;  // (len - 2 <= 70: a long-form length byte never equals it)
    uint32_t pos = 2;
    return webauthn_der_int(sig, len, pos, r_off, r_n) && webauthn_der_int(sig, len, pos, s_off, s_n) && pos == len;
}

// ---- the rules ------------------------------------------------------------------------------------------------------------------
P256_FN bool webauthn_size_ok(size_t ad_len, size_t cd_len, size_t sig_len, size_t challenge_len, size_t origin_len) {
    return ad_len <= ZK_WEBAUTHN_AUTHDATA_MAX && cd_len <= ZK_WEBAUTHN_CLIENTDATA_MAX && sig_len >= WEBAUTHN_SIG_MIN && sig_len <= WEBAUTHN_SIG_MAX &&
           challenge_len >= 1 && challenge_len <= ZK_WEBAUTHN_CHALLENGE_MAX && origin_len <= ZK_WEBAUTHN_ORIGIN_MAX;
}

P256_FN bool webauthn_client_data_ok(const uint8_t* cd, uint32_t cd_len, const uint8_t* e, uint32_t e_len, bool allow_cross_origin) {
    if (cd_len < e_len) return false;
    for (uint32_t i = 0; i < e_len; i++)
        if (cd[i] != e[i]) return false;
    const uint8_t* t = cd + e_len;
    const uint32_t rest = cd_len - e_len;
    uint32_t word = 0;
    if (rest >= 4 && t[0] == 't' && t[1] == 'r' && t[2] == 'u' && t[3] == 'e')
        word = 4;
    else if (rest >= 5 && t[0] == 'f' && t[1] == 'a' && t[2] == 'l' && t[3] == 's' && t[4] == 'e')
        word = 5;
    if (!word || rest < word + 1) return false;
    if (t[word] != ',' && t[word] != '}') return false;
    if (cd[cd_len - 1] != '}') return false;
    return word == 5 || allow_cross_origin;
}

// E of the rule above into out (WEBAUTHN_PREFIX_MAX bytes at least); returns its length.  Host side: the library and the tests
// build it per request.  challenge_len in 1 .. 64, origin_len <= 255 (webauthn_size_ok).  create: the type is webauthn.create
// (a registration, webauthn_register.hip.h), E is three bytes longer and out has WEBAUTHN_CREATE_PREFIX_MAX bytes at least
constexpr uint32_t WEBAUTHN_CREATE_PREFIX_MAX = WEBAUTHN_PREFIX_MAX + 3;
inline uint32_t webauthn_expected_prefix(const uint8_t* challenge, size_t challenge_len, const char* origin, size_t origin_len, uint8_t* out,
                                         bool create = false) {
    static const char B64[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_";
    static const char GET[] = "{\"type\":\"webauthn.get\",\"challenge\":\"", CREATE[] = "{\"type\":\"webauthn.create\",\"challenge\":\"";
    static const char P1[] = "\",\"origin\":\"", P2[] = "\",\"crossOrigin\":";
    uint32_t n = 0;
    for (const char* p = create ? CREATE : GET; *p; p++) out[n++] = (uint8_t)*p;
    for (size_t i = 0; i < challenge_len; i += 3) {
        const size_t left = challenge_len - i;
        const uint32_t v = ((uint32_t)challenge[i] << 16) | (left > 1 ? (uint32_t)challenge[i + 1] << 8 : 0) | (left > 2 ? (uint32_t)challenge[i + 2] : 0);
        out[n++] = (uint8_t)B64[v >> 18];
        out[n++] = (uint8_t)B64[(v >> 12) & 63];
        if (left > 1) out[n++] = (uint8_t)B64[(v >> 6) & 63];
        if (left > 2) out[n++] = (uint8_t)B64[v & 63];
    }
    for (const char* p = P1; *p; p++) out[n++] = (uint8_t)*p;
    for (size_t i = 0; i < origin_len; i++) out[n++] = (uint8_t)origin[i];
    for (const char* p = P2; *p; p++) out[n++] = (uint8_t)*p;
    return n;
}

// The 160-byte record of (key, r, s, SHA-256(ad || SHA-256(cd))) for p256_verify_one, from a signature webauthn_der_parse took
// apart.  Bytes 128 .. 159 hold the first digest in between: the second hash reads it from there, so that no lane keeps a byte
// array of its own.  x_be, y_be: the key, big-endian (COSE's -2 / -3)
P256_FN void webauthn_record(const uint8_t* ad, uint32_t ad_len, const uint8_t* cd, uint32_t cd_len, const uint8_t* sig, uint32_t r_off, uint32_t r_n,
                             uint32_t s_off, uint32_t s_n, const uint8_t* x_be, const uint8_t* y_be, uint8_t* record) {
    uint32_t h[8];
    sha256_two(cd, cd_len, nullptr, 0, h);
    sha256_put(h, record + 128);
    sha256_two(ad, ad_len, record + 128, 32, h);
    for (uint32_t k = 0; k < 32; k++) {
        record[k] = x_be[31 - k];
        record[32 + k] = y_be[31 - k];
        record[64 + k] = k < r_n ? sig[r_off + r_n - 1 - k] : 0;
        record[96 + k] = k < s_n ? sig[s_off + s_n - 1 - k] : 0;
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) record[128 + 4 * i + j] = (uint8_t)(h[7 - i] >> (8 * j));
}

// Everything before the curve: AUTHDATA .. SIGNATURE_DER over lengths that passed webauthn_size_ok, both hashes, and the record.
// Returns the first failing test, or ZK_WEBAUTHN_VALID where the record is ready for p256_verify_one.  record: 160 bytes, all
// zero on a failure, else webauthn_record's.  sign_count: 0 on AUTHDATA, else the counter.  x_be, y_be: the key, big-endian
P256_FN uint8_t webauthn_digest_one(const uint8_t* ad, uint32_t ad_len, const uint8_t* cd, uint32_t cd_len, const uint8_t* sig, uint32_t sig_len,
                                    const uint8_t* e, uint32_t e_len, const uint8_t* x_be, const uint8_t* y_be, const uint8_t* rp_id_hash,
                                    uint8_t flags_required, bool allow_cross_origin, uint8_t* record, uint32_t* sign_count) {
    uint8_t reason = ZK_WEBAUTHN_VALID;
    uint32_t r_off = 0, r_n = 0, s_off = 0, s_n = 0;
    *sign_count = 0;
    if (ad_len < WEBAUTHN_AUTHDATA_MIN) {
        reason = ZK_WEBAUTHN_AUTHDATA;
    } else {
        *sign_count = ((uint32_t)ad[33] << 24) | ((uint32_t)ad[34] << 16) | ((uint32_t)ad[35] << 8) | (uint32_t)ad[36];
        uint32_t diff = 0;
        for (int i = 0; i < 32; i++) diff |= (uint32_t)(ad[i] ^ rp_id_hash[i]);
        if (diff)
            reason = ZK_WEBAUTHN_RPID;
        else if ((ad[32] & flags_required) != flags_required)
            reason = ZK_WEBAUTHN_FLAGS;
        else if (!webauthn_client_data_ok(cd, cd_len, e, e_len, allow_cross_origin))
            reason = ZK_WEBAUTHN_CLIENTDATA;
        else if (!webauthn_der_parse(sig, sig_len, r_off, r_n, s_off, s_n))
            reason = ZK_WEBAUTHN_SIGNATURE_DER;
    }
    if (reason != ZK_WEBAUTHN_VALID) {
        for (int i = 0; i < 160; i++) record[i] = 0;
        return reason;
    }
    webauthn_record(ad, ad_len, cd, cd_len, sig, r_off, r_n, s_off, s_n, x_be, y_be, record);
    return ZK_WEBAUTHN_VALID;
}

// The whole rule for one assertion, E already built; g_table: the comb of G (p256.hip.h).  The device runs it as two launches
// (webauthn.hip): webauthn_digest_one, then p256_verify_one over the records of the lanes that came through
P256_FN uint8_t webauthn_check_one(const uint8_t* ad, size_t ad_len, const uint8_t* cd, size_t cd_len, const uint8_t* sig, size_t sig_len,
                                   size_t challenge_len, size_t origin_len, const uint8_t* e, uint32_t e_len, const uint8_t* x_be, const uint8_t* y_be,
                                   const uint8_t* rp_id_hash, uint8_t flags_required, bool allow_cross_origin, const P256Affine* g_table, uint8_t* record,
                                   uint32_t* sign_count) {
    if (!webauthn_size_ok(ad_len, cd_len, sig_len, challenge_len, origin_len)) {
        for (int i = 0; i < 160; i++) record[i] = 0;
        *sign_count = 0;
        return ZK_WEBAUTHN_SIZE;
    }
    const uint8_t reason = webauthn_digest_one(ad, (uint32_t)ad_len, cd, (uint32_t)cd_len, sig, (uint32_t)sig_len, e, e_len, x_be, y_be, rp_id_hash,
                                               flags_required, allow_cross_origin, record, sign_count);
    return reason != ZK_WEBAUTHN_VALID ? reason : p256_verify_one(record, g_table);
}

// ---- the upload image of a batch -------------------------------------------------------------------------------------------------
// Host only, and nothing of HIP is called: the library packs with these (webauthn.hip, webauthn_register.hip), and the CPU programs
// of the tests call the same functions under the sanitizers.  An image is one fixed-size descriptor per LIVE request (one inside
// the caps; the others are never uploaded and get no lane), then ONE blob with every live request's strings and its E back to
// back; a descriptor's offsets count from the start of the blob.

// one assertion as the lane sees it
struct WebauthnDesc {
    uint32_t ad_off, ad_len, cd_off, cd_len, sig_off, sig_len, e_off, e_len;
    uint8_t x[32], y[32], rp_id_hash[32];
    uint8_t flags_required, allow_cross_origin, pad[2];
};
static_assert(sizeof(WebauthnDesc) == 132, "the descriptor is packed words and bytes");

struct WebauthnImage {
    std::vector<uint32_t> live;  // the indices of the live requests in the caller's array, ascending: descriptor j is request live[j]
    std::vector<uint8_t> bytes;  // live.size() descriptors, then the blob; its size is the upload's length
};

// the end of a blob being filled: appends a string and says where it lies
struct WebauthnCursor {
    uint8_t* blob;
    uint32_t pos = 0;  // (16 384 requests of 8192 + 4096 + 362 bytes stay below 2^28)
    uint32_t put(const uint8_t* p, size_t len) {
        const uint32_t at = pos;
        if (len) memcpy(blob + pos, p, len);
        pos += (uint32_t)len;
        return at;
    }
};

// The image of r[0 .. count).  room(q): 0 for a request outside the caps (not live), else an upper bound of its bytes in the blob;
// fill(q, cur, d): puts a live request's strings through the cursor and fills what is the ceremony's own in its descriptor d,
// which comes zeroed.  What both ceremonies have is done here: E (built in place behind the strings; create: its type) and the
// relying party's expectations
template <class Desc, class Req, class Room, class Fill>
WebauthnImage webauthn_pack_image(const Req* r, size_t count, bool create, Room room, Fill fill) {
    WebauthnImage im;
    im.live.reserve(count);
    size_t blob_room = 0;
    for (size_t i = 0; i < count; i++)
        if (const size_t bytes = room(r[i])) {
            im.live.push_back((uint32_t)i);
            blob_room += bytes;
        }
    const size_t n = im.live.size(), desc_bytes = n * sizeof(Desc);
    im.bytes.resize(desc_bytes + blob_room);
    WebauthnCursor cur{im.bytes.data() + desc_bytes};
    for (size_t j = 0; j < n; j++) {
        const Req& q = r[im.live[j]];
        Desc d;
        memset(&d, 0, sizeof d);
        fill(q, cur, d);
        d.e_off = cur.pos;
        d.e_len = webauthn_expected_prefix(q.challenge, q.challenge_len, q.origin, q.origin_len, cur.blob + cur.pos, create);
        cur.pos += d.e_len;
        memcpy(d.rp_id_hash, q.rp_id_hash, 32);
        d.flags_required = q.flags_required;
        d.allow_cross_origin = q.allow_cross_origin;
        memcpy(im.bytes.data() + j * sizeof(Desc), &d, sizeof d);
    }
    im.bytes.resize(desc_bytes + cur.pos);
    return im;
}

// n reason bytes padded to whole words: what follows them in a download (counters, credentials) stays aligned
inline size_t webauthn_padded(size_t n) { return (n + 3) & ~(size_t)3; }

// the image of `count` assertions; Req: zk_webauthn_assertion (include/zkmi355.h), which this header does not need otherwise
template <class Req>
WebauthnImage webauthn_pack(const Req* a, size_t count) {
    return webauthn_pack_image<WebauthnDesc>(
        a, count, false,
        [](const Req& q) -> size_t {
            if (!webauthn_size_ok(q.authenticator_data_len, q.client_data_json_len, q.signature_len, q.challenge_len, q.origin_len)) return 0;
            return q.authenticator_data_len + q.client_data_json_len + q.signature_len + WEBAUTHN_PREFIX_MAX;
        },
        [](const Req& q, WebauthnCursor& cur, WebauthnDesc& d) {
            d.ad_len = (uint32_t)q.authenticator_data_len, d.ad_off = cur.put(q.authenticator_data, q.authenticator_data_len);
            d.cd_len = (uint32_t)q.client_data_json_len, d.cd_off = cur.put(q.client_data_json, q.client_data_json_len);
            d.sig_len = (uint32_t)q.signature_len, d.sig_off = cur.put(q.signature, q.signature_len);
            memcpy(d.x, q.pubkey_x, 32);
            memcpy(d.y, q.pubkey_y, 32);
        });
}

}  // namespace zk
