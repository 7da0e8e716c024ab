"""The relying party's check of a WebAuthn registration over Python bytes and integers: the reference of zk_webauthn_register and
of csrc/webauthn_register.hip.h, written from the rule as include/zkmi355.h states it and independent of the package: a CBOR reader
of its own that DECODES (recursively, to Python values) where the package only skips, hashlib, tests/webauthn_ref.py for the shared
rules (authData's first 37 bytes, the client-data rule, strict DER, msghash) and tests/es256_ref.py for the curve.  The COSE key
and the statement are judged on the decoded values: under the strict rule (definite lengths, shortest heads) a value has exactly
one encoding, so "decodes to the canonical key" and "is the 77 template bytes" are one statement said two ways.

check() returns (reason, credential): the FIRST failing test in the order SIZE, CBOR, AUTHDATA, RPID, FLAGS, CREDENTIAL, COSE_KEY,
CLIENTDATA, RANGE, OFF_CURVE, ATTESTATION, SIGNATURE_DER, then es256_ref's verdict over the self attestation; credential is None
unless the reason is VALID.
"""
import struct

import es256_ref as R
import webauthn_ref as W

VALID, RANGE, OFF_CURVE, MISMATCH, SIZE, AUTHDATA, RPID, FLAGS, CLIENTDATA, SIGNATURE_DER, CBOR, CREDENTIAL, COSE_KEY, ATTESTATION = range(14)
REASON_NAMES = dict(W.REASON_NAMES)
REASON_NAMES.update({CBOR: "CBOR", CREDENTIAL: "CREDENTIAL", COSE_KEY: "COSE_KEY", ATTESTATION: "ATTESTATION"})
ATTOBJ_MAX = 8192
ATT_IGNORE, ATT_NONE_OR_SELF = 0, 1
ATTESTED_NONE, ATTESTED_SELF, ATTESTED_NOT_JUDGED = 0, 1, 2
UP, UV, AT, ED = 0x01, 0x04, 0x40, 0x80


# ---- CBOR, the strict subset --------------------------------------------------------------------------------------------------------
class Malformed(Exception):
    pass


class Text:
    """A text string, kept as its bytes (no UTF-8 check)."""

    def __init__(self, raw):
        self.raw = bytes(raw)

    def __eq__(self, other):
        return isinstance(other, Text) and other.raw == self.raw

    def __hash__(self):
        return hash(("text", self.raw))

    def __repr__(self):
        return "Text(%r)" % self.raw


class Map:
    """A map as the list of its (key, value) pairs in the order they stand (keys may repeat: nobody compares them)."""

    def __init__(self, pairs):
        self.pairs = list(pairs)

    def __eq__(self, other):
        return isinstance(other, Map) and other.pairs == self.pairs

    def __repr__(self):
        return "Map(%r)" % self.pairs


class Tag:
    def __init__(self, number, item):
        self.number, self.item = number, item

    def __eq__(self, other):
        return isinstance(other, Tag) and (other.number, other.item) == (self.number, self.item)

    def __repr__(self):
        return "Tag(%d, %r)" % (self.number, self.item)


class Simple:
    def __init__(self, value):
        self.value = value

    def __eq__(self, other):
        return isinstance(other, Simple) and other.value == self.value

    def __repr__(self):
        return "Simple(%d)" % self.value


FALSE, TRUE, NULL, UNDEFINED = Simple(20), Simple(21), Simple(22), Simple(23)
_SHORTEST = {24: 24, 25: 1 << 8, 26: 1 << 16, 27: 1 << 32}  # the least argument each longer head may carry


def read_item(b, pos=0):
    """The data item at b[pos:] under the strict rule -> (value, the position behind it); Malformed otherwise."""
    if pos >= len(b):
        raise Malformed("no byte left")
    major, ai = b[pos] >> 5, b[pos] & 31
    pos += 1
    if ai < 24:
        arg = ai
    elif ai <= 27:
        width = 1 << (ai - 24)
        raw = b[pos:pos + width]
        if len(raw) != width:
            raise Malformed("the head runs past the end")
        pos += width
        arg = int.from_bytes(raw, "big")
        if major == 7:
            if ai == 24:
                if arg < 32:
                    raise Malformed("a simple value below 32 in two bytes")
                return Simple(arg), pos
            return struct.unpack({25: ">e", 26: ">f", 27: ">d"}[ai], raw)[0], pos
        if arg < _SHORTEST[ai]:
            raise Malformed("a head longer than its value needs")
    else:
        raise Malformed("additional information %d" % ai)  # 28 .. 30 reserved, 31 indefinite / break
    left = len(b) - pos
    if major == 0:
        return arg, pos
    if major == 1:
        return -1 - arg, pos
    if major == 7:
        return Simple(arg), pos
    if major == 6:
        item, pos = read_item(b, pos)
        return Tag(arg, item), pos
    if arg > left:
        raise Malformed("%d bytes, items or pairs declared with %d bytes left" % (arg, left))
    if major == 2:
        return bytes(b[pos:pos + arg]), pos + arg
    if major == 3:
        return Text(b[pos:pos + arg]), pos + arg
    items = []
    for _ in range(arg * (2 if major == 5 else 1)):
        item, pos = read_item(b, pos)
        items.append(item)
    if major == 4:
        return items, pos
    return Map(zip(items[0::2], items[1::2])), pos


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
class Registration:
    """One request: what the client sent (attestation_object, client_data_json: bytes) and what the relying party expects
    (challenge: bytes, origin: str, rp_id_hash: 32 bytes, flags_required, allow_cross_origin, policy)."""

    def __init__(self, attestation_object, client_data_json, challenge, origin, rp_id_hash, flags_required=UP, allow_cross_origin=False,
                 policy=ATT_IGNORE):
        self.attestation_object, self.client_data_json = bytes(attestation_object), bytes(client_data_json)
        self.challenge, self.origin, self.rp_id_hash = bytes(challenge), origin, bytes(rp_id_hash)
        self.flags_required, self.allow_cross_origin, self.policy = flags_required, bool(allow_cross_origin), policy

    def replace(self, **kw):
        d = dict(self.__dict__)
        d.update(kw)
        return Registration(**d)


def expected_prefix(challenge, origin):
    return b'{"type":"webauthn.create","challenge":"' + W.b64url(challenge) + b'","origin":"' + origin.encode() + b'","crossOrigin":'


def client_data_ok(cd, challenge, origin, allow_cross_origin):
    """webauthn_ref.client_data_ok with the other type: the same words after E."""
    e = expected_prefix(challenge, origin)
    if not cd.startswith(e):
        return False
    get = W.expected_prefix(challenge, origin)
    return W.client_data_ok(get + cd[len(e):], challenge, origin, allow_cross_origin)


def cose_es256_p256(x, y):
    """The canonical COSE EC2 / ES256 / P-256 key as a decoded value."""
    return Map([(1, 2), (3, -7), (-1, 1), (-2, x), (-3, y)])


def check(g):
    """(reason, credential dict or None) of one Registration."""
    o, cd = g.attestation_object, g.client_data_json
    if (not 1 <= len(o) <= ATTOBJ_MAX or len(cd) > W.CLIENTDATA_MAX or not 1 <= len(g.challenge) <= W.CHALLENGE_MAX
            or len(g.origin.encode()) > W.ORIGIN_MAX):
        return SIZE, None
    try:
        top, end = read_item(o)
    except Malformed:
        return CBOR, None
    if end != len(o) or not isinstance(top, Map) or len(top.pairs) != 3:
        return CBOR, None
    (k0, fmt), (k1, stmt), (k2, ad) = top.pairs
    if ((k0, k1, k2) != (Text(b"fmt"), Text(b"attStmt"), Text(b"authData")) or not isinstance(fmt, Text) or not isinstance(stmt, Map)
            or not isinstance(ad, bytes)):
        return CBOR, None
    ad_off = len(o) - len(ad)  # the last member's content ends the object
    assert o[ad_off:] == ad
    if len(ad) < 37:
        return AUTHDATA, None
    if ad[:32] != g.rp_id_hash:
        return RPID, None
    flags = ad[32]
    if flags & g.flags_required != g.flags_required:
        return FLAGS, None
    # attested credential data
    if not flags & AT or len(ad) < 55:
        return CREDENTIAL, None
    id_len = int.from_bytes(ad[53:55], "big")
    if not 1 <= id_len <= 1023 or 55 + id_len > len(ad):
        return CREDENTIAL, None
    try:
        key, pos = read_item(ad, 55 + id_len)
        if flags & ED:
            ext, pos = read_item(ad, pos)
            if not isinstance(ext, Map):
                return CREDENTIAL, None
    except Malformed:
        return CREDENTIAL, None
    if pos != len(ad):
        return CREDENTIAL, None
    if (not isinstance(key, Map) or len(key.pairs) != 5 or not isinstance(key.pairs[3][1], bytes) or not isinstance(key.pairs[4][1], bytes)
            or len(key.pairs[3][1]) != 32 or len(key.pairs[4][1]) != 32 or key != cose_es256_p256(key.pairs[3][1], key.pairs[4][1])):
        return COSE_KEY, None
    if not client_data_ok(cd, g.challenge, g.origin, g.allow_cross_origin):
        return CLIENTDATA, None
    xb, yb = key.pairs[3][1], key.pairs[4][1]
    x, y = int.from_bytes(xb, "big"), int.from_bytes(yb, "big")
    if x >= R.P or y >= R.P:
        return RANGE, None
    if not R.on_curve(x, y):
        return OFF_CURVE, None
    attestation = ATTESTED_NOT_JUDGED
    if g.policy == ATT_NONE_OR_SELF:
        if fmt == Text(b"none") and stmt == Map([]):
            attestation = ATTESTED_NONE
        elif (fmt == Text(b"packed") and len(stmt.pairs) == 2 and stmt.pairs[0] == (Text(b"alg"), -7) and stmt.pairs[1][0] == Text(b"sig")
              and isinstance(stmt.pairs[1][1], bytes)):
            attestation = ATTESTED_SELF
            rs = W.der_parse(stmt.pairs[1][1])
            if rs is None:
                return SIGNATURE_DER, None
            verdict = R.verify_ints(x, y, rs[0], rs[1], W.msghash(ad, cd))
            if verdict != R.VALID:
                return verdict, None
        else:
            return ATTESTATION, None
    return VALID, {"pubkey_x": xb, "pubkey_y": yb, "aaguid": ad[37:53], "auth_data_off": ad_off, "auth_data_len": len(ad),
                   "credential_id_off": ad_off + 55, "credential_id_len": id_len, "sign_count": int.from_bytes(ad[33:37], "big"), "flags": flags,
                   "attestation": attestation}
