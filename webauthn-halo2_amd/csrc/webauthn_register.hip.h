// webauthn_register.hip.h — the relying party's check of a WebAuthn registration (navigator.credentials.create, ES256): a CBOR
// walker over the attestationObject, the attested-credential-data rules, the COSE key template, and - for packed self attestation -
// the record p256_verify_one takes.  It is one more stage in front of webauthn.hip.h, whose SHA-256, strict DER parse, client-data
// rule and record assembly it uses as they are.
//
// Like webauthn.hip.h, every function is __host__ __device__ in ONE portable form, no inline assembly: the kernel
// (webauthn_register.hip) is a wrapper around webauthn_register_one, and a CPU program runs the same code
// (tests/webauthn_register_host_check.cpp does, under the sanitizers).  NOT constant time, on purpose: everything a registration
// carries is public request data; nothing here may be used with a secret.
//
// The rule.  A registration is (attestationObject, clientDataJSON), the relying party's expectations (the challenge it issued, its
// origin, SHA-256 of its RP ID, the flags it requires, whether it accepts a cross-origin call) and an attestation policy.
// webauthn_register_check_one applies these tests in this order and returns the FIRST that fails (0 .. 9 are webauthn.hip.h's):
//   SIZE           the attestationObject outside 1 .. 8192 bytes, clientDataJSON longer than 4096, a challenge outside 1 .. 64 bytes,
//                  an origin longer than 255
//   CBOR           the attestationObject is not the accepted encoding: a definite-length map of exactly three entries in CTAP2's
//                  canonical order - text "fmt" -> a text string, text "attStmt" -> a map, text "authData" -> a byte string - with
//                  nothing after it, and every data item in it well-formed under these rules:
//                    - definite lengths only: additional information 31 is refused everywhere, the `break` byte ff included;
//                      additional information 28 .. 30 is refused;
//                    - every head in its shortest form: a value below 24 in the head byte, below 2^8 in one byte, below 2^16 in
//                      two, below 2^32 in four.  Floats (major type 7, additional information 25 .. 27) are taken as they are; a
//                      simple value in one extra byte must be 32 or more;
//                    - a declared count of bytes, items or pairs larger than the number of bytes left behind the head is refused at
//                      the head, before anything is skipped: the walk is bounded by the object's length, and no sum can overflow.
//                  Text is not checked for UTF-8; map keys are not compared with each other.  Another member order, a fourth
//                  member or an indefinite-length map is this reason, although a general CBOR decoder would read it
//   AUTHDATA, RPID, FLAGS   webauthn.hip.h's rules over the authData bytes: at least 37, bytes 0 .. 31, (flags & required)
//   CREDENTIAL     attested credential data: the flag AT (0x40) is set; behind byte 37 stand 16 bytes of aaguid, a big-endian
//                  16-bit credentialIdLength in 1 .. 1023, that many bytes, and the key: ONE well-formed data item under the rules
//                  above (its end is where the walker stops).  Any of these running past the end of authData is this reason.
//                  Behind the key, with ED (0x80) clear authData ends; with ED set exactly one well-formed map follows and ends
//                  where authData ends
//   COSE_KEY       the key is not the 77 bytes of the canonical COSE EC2 / ES256 / P-256 key,
//                    a5  01 02  03 26  20 01  21 58 20 <x: 32 bytes>  22 58 20 <y: 32 bytes>
//                  compared byte for byte with that template, like the client-data rule.  Refused: other algorithms (-8 EdDSA, -257
//                  RS256), other key types (OKP) and curves, the members in another order, extra members, coordinates not of 32
//                  bytes.  (A key whose altered byte moves the item's end - the map's count, a coordinate's length - fails
//                  CREDENTIAL already, where ED is clear.)
//   CLIENTDATA     webauthn.hip.h's limited verification algorithm with "type":"webauthn.create" in E
//   RANGE, OFF_CURVE   the credential key itself: x, y below p and on the curve (p256_key_check), whatever the statement
//   ATTESTATION    only under policy NONE_OR_SELF: the statement is neither fmt "none" with an empty map nor fmt "packed" with
//                  exactly {"alg": -7, "sig": <byte string>} in that order (self attestation: no x5c).  Another fmt, x5c present,
//                  another alg, "none" with members: refused.  Under policy IGNORE the statement only has to be well-formed (CBOR)
//                  and is not judged: what a relying party that asked for conveyance "none" does
//   SIGNATURE_DER, then p256_verify_one's RANGE / MISMATCH   for a packed self statement under NONE_OR_SELF: sig through the strict
//                  DER parse, the record  x || y || r || s || SHA-256(authData || SHA-256(clientDataJSON))  assembled exactly as
//                  for an assertion (webauthn_record), the key the credential's own.  Only these registrations hash anything.
//
// The walker.  A CBOR item is skipped with ONE counter of items still owed: a head takes one off, a map of n pairs adds 2 n, an
// array n, a tag 1, and a string moves the position by its length.  The walk ends when nothing is owed.  No recursion, no stack, no
// depth limit: nesting 200 deep costs 200 heads.  Each head is refused unless what it declares fits into the bytes left, so the
// counter stays below 2 x 8192 per head and the position never passes the end.  The lane reads the object by byte loads at a moving
// position and keeps a handful of scalars (position, owed, the current head): no per-lane byte array, nothing indexed at run time.
// Templates (the member names, the COSE key) are compared as big-endian integers of up to eight bytes read the same way.
#pragma once
#include "webauthn.hip.h"

#ifndef ZK_WEBAUTHN_CBOR  // (include/zkmi355.h defines the same: this header also stands alone)
#define ZK_WEBAUTHN_CBOR 10
#define ZK_WEBAUTHN_CREDENTIAL 11
#define ZK_WEBAUTHN_COSE_KEY 12
#define ZK_WEBAUTHN_ATTESTATION 13
#define ZK_WEBAUTHN_ATTOBJ_MAX 8192
#define ZK_WEBAUTHN_ATT_IGNORE 0
#define ZK_WEBAUTHN_ATT_NONE_OR_SELF 1
#define ZK_WEBAUTHN_ATTESTED_NONE 0
#define ZK_WEBAUTHN_ATTESTED_SELF 1
#define ZK_WEBAUTHN_ATTESTED_NOT_JUDGED 2
#endif

namespace zk {

// zk_webauthn_credential (include/zkmi355.h), field for field: the library's kernel writes this and the call hands it out
struct WebauthnCredential {
    uint8_t pubkey_x[32], pubkey_y[32];
    uint8_t aaguid[16];
    uint32_t auth_data_off, auth_data_len;
    uint32_t credential_id_off, credential_id_len;
    uint32_t sign_count;
    uint8_t flags;
    uint8_t attestation;
};
static_assert(sizeof(WebauthnCredential) == 104, "64 key bytes, 16 of aaguid, five words, two bytes and two of padding");

constexpr uint32_t WEBAUTHN_COSE_KEY_BYTES = 77, WEBAUTHN_CREDENTIAL_ID_MAX = 1023;
constexpr uint8_t WEBAUTHN_FLAG_AT = 0x40, WEBAUTHN_FLAG_ED = 0x80;

// ---- CBOR (RFC 8949), the strict subset ------------------------------------------------------------------------------------------
// p[pos .. pos + n) as a big-endian integer, n <= 8; the caller has checked pos + n <= len
P256_FN uint64_t webauthn_be(const uint8_t* p, uint32_t pos, uint32_t n) {
    uint64_t v = 0;
    for (uint32_t k = 0; k < n; k++) v = (v << 8) | p[pos + k];
    return v;
}

// p[pos ..) starts with the n <= 8 bytes of `want`; false where fewer than n are left
P256_FN bool webauthn_starts(const uint8_t* p, uint32_t len, uint32_t pos, uint32_t n, uint64_t want) {
    return len - pos >= n && webauthn_be(p, pos, n) == want;
}

// The head at p[pos ..): major type and argument, pos moved behind the head.  false: no byte left, additional information 28 ..
// 31, argument bytes past the end, a head longer than its value needs, a one-byte simple value below 32
P256_FN bool cbor_head(const uint8_t* p, uint32_t len, uint32_t& pos, uint32_t& major, uint64_t& val) {
    if (pos >= len) return false;
    const uint32_t b = p[pos++], ai = b & 31u;
    major = b >> 5;
    val = ai;
    if (ai < 24) return true;
    if (ai > 27) return false;
    const uint32_t nb = 1u << (ai - 24);
    if (len - pos < nb) return false;
    val = webauthn_be(p, pos, nb);
    pos += nb;
    if (major == 7) return ai != 24 || val >= 32;  // (25 .. 27: a float, any bits)
    return val >= (ai == 24 ? 24u : ai == 25 ? 0x100ull : ai == 26 ? 0x10000ull : 0x100000000ull);
}

// One whole data item at p[pos ..): pos moved behind it.  false: not well-formed under the rule above (pos is then meaningless)
P256_FN bool cbor_skip(const uint8_t* p, uint32_t len, uint32_t& pos) {
    uint32_t owed = 1;  // stays below 2^28: at most 8192 heads of an accepted object, each adding 2 x 8192 at the most
    while (owed) {
        uint32_t major;
        uint64_t val;
        if (!cbor_head(p, len, pos, major, val)) return false;
        owed--;
        if (major >= 2 && major <= 5 && val > (uint64_t)(len - pos)) return false;  // bytes, items or pairs: more than bytes left
        if (major == 2 || major == 3)
            pos += (uint32_t)val;
        else if (major == 4)
            owed += (uint32_t)val;
        else if (major == 5)
            owed += 2 * (uint32_t)val;
        else if (major == 6)
            owed += 1;
    }
    return true;
}

// The attestationObject's three members.  On success fmt / stmt / ad name the bytes of the fmt text, of the whole attStmt item and
// of the authData byte string's content
P256_FN bool webauthn_attobj_parse(const uint8_t* o, uint32_t len, uint32_t& fmt_off, uint32_t& fmt_len, uint32_t& stmt_off, uint32_t& stmt_len,
                                   uint32_t& ad_off, uint32_t& ad_len) {
    uint32_t pos = 0, major;
    uint64_t val;
    if (!cbor_head(o, len, pos, major, val) || major != 5 || val != 3) return false;
    if (!webauthn_starts(o, len, pos, 4, 0x63666d74ull)) return false;  // 63 "fmt"
    pos += 4;
    if (!cbor_head(o, len, pos, major, val) || major != 3 || val > (uint64_t)(len - pos)) return false;
    fmt_off = pos, fmt_len = (uint32_t)val;
    pos += fmt_len;
    if (!webauthn_starts(o, len, pos, 8, 0x6761747453746d74ull)) return false;  // 67 "attStmt"
    pos += 8;
    stmt_off = pos;
    if (pos >= len || (o[pos] >> 5) != 5 || !cbor_skip(o, len, pos)) return false;
    stmt_len = pos - stmt_off;
    if (!webauthn_starts(o, len, pos, 8, 0x6861757468446174ull) || !webauthn_starts(o, len, pos + 8, 1, 0x61ull)) return false;  // 68 "authData"
    pos += 9;
    if (!cbor_head(o, len, pos, major, val) || major != 2 || val > (uint64_t)(len - pos)) return false;
    ad_off = pos, ad_len = (uint32_t)val;
    return pos + ad_len == len;
}

// ---- the rules -------------------------------------------------------------------------------------------------------------------
P256_FN bool webauthn_register_size_ok(size_t obj_len, size_t cd_len, size_t challenge_len, size_t origin_len) {
    return obj_len >= 1 && obj_len <= ZK_WEBAUTHN_ATTOBJ_MAX && cd_len <= ZK_WEBAUTHN_CLIENTDATA_MAX && challenge_len >= 1 &&
           challenge_len <= ZK_WEBAUTHN_CHALLENGE_MAX && origin_len <= ZK_WEBAUTHN_ORIGIN_MAX;
}

// Attested credential data in ad[0 .. ad_len), ad_len >= 37 with AT set: the offsets of the credential id and of the key.  false:
// the CREDENTIAL verdict
P256_FN bool webauthn_credential_parse(const uint8_t* ad, uint32_t ad_len, uint32_t& id_off, uint32_t& id_len, uint32_t& key_off, uint32_t& key_len) {
    if (ad_len < WEBAUTHN_AUTHDATA_MIN + 16 + 2) return false;
    id_off = WEBAUTHN_AUTHDATA_MIN + 16 + 2;
    id_len = (uint32_t)webauthn_be(ad, id_off - 2, 2);
    if (id_len < 1 || id_len > WEBAUTHN_CREDENTIAL_ID_MAX || ad_len - id_off < id_len) return false;
    uint32_t pos = key_off = id_off + id_len;
    if (!cbor_skip(ad, ad_len, pos)) return false;
    key_len = pos - key_off;
    if (!(ad[32] & WEBAUTHN_FLAG_ED)) return pos == ad_len;
    return pos < ad_len && (ad[pos] >> 5) == 5 && cbor_skip(ad, ad_len, pos) && pos == ad_len;
}

// key[0 .. key_len) is the template with any x, y
P256_FN bool webauthn_cose_key_ok(const uint8_t* key, uint32_t key_len) {
    return key_len == WEBAUTHN_COSE_KEY_BYTES && webauthn_be(key, 0, 8) == 0xa501020326200121ull && webauthn_be(key, 8, 2) == 0x5820u &&
           webauthn_be(key, 42, 3) == 0x225820u;
}

// a big-endian coordinate as p256.hip.h's eight little-endian words
P256_FN void webauthn_words_of_be(const uint8_t* be, uint32_t (&w)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++)
        w[i] = (uint32_t)be[31 - 4 * i] | ((uint32_t)be[30 - 4 * i] << 8) | ((uint32_t)be[29 - 4 * i] << 16) | ((uint32_t)be[28 - 4 * i] << 24);
}

// The statement under policy NONE_OR_SELF: 0 refused, 1 fmt "none" with an empty map, 2 packed self attestation with sig naming
// the signature's bytes within the object
P256_FN int webauthn_statement(const uint8_t* o, uint32_t fmt_off, uint32_t fmt_len, uint32_t stmt_off, uint32_t stmt_len, uint32_t& sig_off,
                               uint32_t& sig_len) {
    if (fmt_len == 4 && webauthn_be(o, fmt_off, 4) == 0x6e6f6e65u) return stmt_len == 1 ? 1 : 0;  // "none", a0 (a map of one byte is empty)
    if (fmt_len != 6 || webauthn_be(o, fmt_off, 6) != 0x7061636b6564ull) return 0;              // "packed"
    // a2  63 "alg"  26  63 "sig"  <the head of a byte string>: the item is well-formed, so the string ends where the map ends
    const uint32_t end = stmt_off + stmt_len;
    if (!webauthn_starts(o, end, stmt_off, 8, 0xa263616c67266373ull) || !webauthn_starts(o, end, stmt_off + 8, 2, 0x6967u)) return 0;
    uint32_t pos = stmt_off + 10, major;
    uint64_t val;
    if (!cbor_head(o, end, pos, major, val) || major != 2 || val != (uint64_t)(end - pos)) return 0;
    sig_off = pos, sig_len = (uint32_t)val;
    return 2;
}

P256_FN void webauthn_zero(uint8_t* p, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) p[i] = 0;
}

// Everything before the curve verification: CBOR .. SIGNATURE_DER over lengths that passed webauthn_register_size_ok, and for a
// packed self statement both hashes and the record.  e: E with webauthn.create (webauthn_expected_prefix(.., true)).  Returns the
// first failing test, or ZK_WEBAUTHN_VALID.  On VALID `cred` is filled (offsets within o) and *to_verify says whether the
// registration is accepted only if p256_verify_one accepts `record`; record is all zero where *to_verify is false.  On a failure
// cred and record are all zero
P256_FN uint8_t webauthn_register_one(const uint8_t* o, uint32_t o_len, const uint8_t* cd, uint32_t cd_len, const uint8_t* e, uint32_t e_len,
                                      const uint8_t* rp_id_hash, uint8_t flags_required, bool allow_cross_origin, uint8_t policy, uint8_t* record,
                                      WebauthnCredential* cred, bool* to_verify) {
    uint8_t reason = ZK_WEBAUTHN_VALID;
    uint32_t fmt_off = 0, fmt_len = 0, stmt_off = 0, stmt_len = 0, ad_off = 0, ad_len = 0, id_off = 0, id_len = 0, key_off = 0, key_len = 0;
    uint32_t sig_off = 0, sig_len = 0, r_off = 0, r_n = 0, s_off = 0, s_n = 0;
    int statement = 0;
    const uint8_t* ad = o;
    *to_verify = false;
    if (!webauthn_attobj_parse(o, o_len, fmt_off, fmt_len, stmt_off, stmt_len, ad_off, ad_len)) {
        reason = ZK_WEBAUTHN_CBOR;
    } else if (ad_len < WEBAUTHN_AUTHDATA_MIN) {
        reason = ZK_WEBAUTHN_AUTHDATA;
    } else {
        ad = o + ad_off;
        uint32_t diff = 0;
        for (int i = 0; i < 32; i++) diff |= (uint32_t)(ad[i] ^ rp_id_hash[i]);
        if (diff)
            reason = ZK_WEBAUTHN_RPID;
        else if ((ad[32] & flags_required) != flags_required)
            reason = ZK_WEBAUTHN_FLAGS;
        else if (!(ad[32] & WEBAUTHN_FLAG_AT) || !webauthn_credential_parse(ad, ad_len, id_off, id_len, key_off, key_len))
            reason = ZK_WEBAUTHN_CREDENTIAL;
        else if (!webauthn_cose_key_ok(ad + key_off, key_len))
            reason = ZK_WEBAUTHN_COSE_KEY;
        else if (!webauthn_client_data_ok(cd, cd_len, e, e_len, allow_cross_origin))
            reason = ZK_WEBAUTHN_CLIENTDATA;
        else {
            uint32_t x[8], y[8];
            webauthn_words_of_be(ad + key_off + 10, x);
            webauthn_words_of_be(ad + key_off + 45, y);
            reason = p256_key_check(x, y);  // (ZK_ES256_RANGE / _OFF_CURVE are ZK_WEBAUTHN_'s values)
            if (reason == ZK_WEBAUTHN_VALID && policy == ZK_WEBAUTHN_ATT_NONE_OR_SELF) {
                statement = webauthn_statement(o, fmt_off, fmt_len, stmt_off, stmt_len, sig_off, sig_len);
                if (!statement)
                    reason = ZK_WEBAUTHN_ATTESTATION;
                else if (statement == 2 && !webauthn_der_parse(o + sig_off, sig_len, r_off, r_n, s_off, s_n))
                    reason = ZK_WEBAUTHN_SIGNATURE_DER;
            }
        }
    }
    if (reason != ZK_WEBAUTHN_VALID) {
        webauthn_zero(record, 160);
        webauthn_zero((uint8_t*)cred, sizeof(WebauthnCredential));
        return reason;
    }
    for (int i = 0; i < 32; i++) {
        cred->pubkey_x[i] = ad[key_off + 10 + i];
        cred->pubkey_y[i] = ad[key_off + 45 + i];
    }
    for (int i = 0; i < 16; i++) cred->aaguid[i] = ad[WEBAUTHN_AUTHDATA_MIN + i];
    cred->auth_data_off = ad_off, cred->auth_data_len = ad_len;
    cred->credential_id_off = ad_off + id_off, cred->credential_id_len = id_len;
    cred->sign_count = (uint32_t)webauthn_be(ad, 33, 4);
    cred->flags = ad[32];
    cred->attestation = policy != ZK_WEBAUTHN_ATT_NONE_OR_SELF ? ZK_WEBAUTHN_ATTESTED_NOT_JUDGED
                        : statement == 2                        ? ZK_WEBAUTHN_ATTESTED_SELF
                                                                : ZK_WEBAUTHN_ATTESTED_NONE;
    ((uint8_t*)cred)[sizeof(WebauthnCredential) - 2] = 0, ((uint8_t*)cred)[sizeof(WebauthnCredential) - 1] = 0;  // the padding
    if (statement == 2) {
        webauthn_record(ad, ad_len, cd, cd_len, o + sig_off, r_off, r_n, s_off, s_n, ad + key_off + 10, ad + key_off + 45, record);
        *to_verify = true;
    } else {
        webauthn_zero(record, 160);
    }
    return ZK_WEBAUTHN_VALID;
}

// The whole rule for one registration, E already built; g_table: the comb of G (p256.hip.h).  The device runs it as two launches
// (webauthn_register.hip): webauthn_register_one, then p256_verify_one over the records of the lanes with a signature.  A refused
// registration never hands out a key: cred is all zero unless the return value is ZK_WEBAUTHN_VALID
P256_FN uint8_t webauthn_register_check_one(const uint8_t* o, size_t o_len, const uint8_t* cd, size_t cd_len, size_t challenge_len, size_t origin_len,
                                            const uint8_t* e, uint32_t e_len, const uint8_t* rp_id_hash, uint8_t flags_required, bool allow_cross_origin,
                                            uint8_t policy, const P256Affine* g_table, WebauthnCredential* cred) {
    if (!webauthn_register_size_ok(o_len, cd_len, challenge_len, origin_len)) {
        webauthn_zero((uint8_t*)cred, sizeof(WebauthnCredential));
        return ZK_WEBAUTHN_SIZE;
    }
    uint8_t record[160];
    bool to_verify;
    uint8_t reason = webauthn_register_one(o, (uint32_t)o_len, cd, (uint32_t)cd_len, e, e_len, rp_id_hash, flags_required, allow_cross_origin, policy,
                                           record, cred, &to_verify);
    if (reason == ZK_WEBAUTHN_VALID && to_verify && (reason = p256_verify_one(record, g_table)) != ZK_WEBAUTHN_VALID)
        webauthn_zero((uint8_t*)cred, sizeof(WebauthnCredential));
    return reason;
}

// ---- the upload image of a batch (webauthn.hip.h: host only) ----------------------------------------------------------------------
// one registration as the lane sees it; the offsets count from the start of the blob
struct WebauthnRegisterDesc {
    uint32_t obj_off, obj_len, cd_off, cd_len, e_off, e_len;
    uint8_t rp_id_hash[32];
    uint8_t flags_required, allow_cross_origin, policy, pad;
};
static_assert(sizeof(WebauthnRegisterDesc) == 60, "the descriptor is packed words and bytes");

// the image of `count` registrations; Req: zk_webauthn_registration (include/zkmi355.h)
template <class Req>
WebauthnImage webauthn_register_pack(const Req* r, size_t count) {
    return webauthn_pack_image<WebauthnRegisterDesc>(
        r, count, true,
        [](const Req& q) -> size_t {
            if (!webauthn_register_size_ok(q.attestation_object_len, q.client_data_json_len, q.challenge_len, q.origin_len)) return 0;
            return q.attestation_object_len + q.client_data_json_len + WEBAUTHN_CREATE_PREFIX_MAX;
        },
        [](const Req& q, WebauthnCursor& cur, WebauthnRegisterDesc& d) {
            d.obj_len = (uint32_t)q.attestation_object_len, d.obj_off = cur.put(q.attestation_object, q.attestation_object_len);
            d.cd_len = (uint32_t)q.client_data_json_len, d.cd_off = cur.put(q.client_data_json, q.client_data_json_len);
            d.policy = q.attestation_policy;
        });
}

}  // namespace zk
