"""The relying party's check of a WebAuthn assertion over Python bytes and integers: the reference of zk_webauthn_verify and of
csrc/webauthn.hip.h, written from the rule as include/zkmi355.h states it and independent of the package: hashlib.sha256, base64,
and tests/es256_ref.py for the curve.  check() returns (reason, record, sign_count): the FIRST failing test in the order SIZE,
AUTHDATA, RPID, FLAGS, CLIENTDATA, SIGNATURE_DER, then es256_ref's RANGE, OFF_CURVE, MISMATCH over the assembled record.
"""
import base64
import hashlib

import es256_ref as R

VALID, RANGE, OFF_CURVE, MISMATCH, SIZE, AUTHDATA, RPID, FLAGS, CLIENTDATA, SIGNATURE_DER = range(10)
REASON_NAMES = dict(R.REASON_NAMES)
REASON_NAMES.update({SIZE: "SIZE", AUTHDATA: "AUTHDATA", RPID: "RPID", FLAGS: "FLAGS", CLIENTDATA: "CLIENTDATA", SIGNATURE_DER: "SIGNATURE_DER"})
AUTHDATA_MAX, CLIENTDATA_MAX, CHALLENGE_MAX, ORIGIN_MAX = 1024, 4096, 64, 255
UP, UV = 0x01, 0x04


class Assertion:
    """One request: what the client sent (authenticator_data, client_data_json, signature: bytes), the credential's key (x, y:
    integers) and what the relying party expects (challenge: bytes, origin: str, rp_id_hash: 32 bytes, flags_required,
    allow_cross_origin)."""

    def __init__(self, authenticator_data, client_data_json, signature, x, y, challenge, origin, rp_id_hash, flags_required=UP,
                 allow_cross_origin=False):
        self.authenticator_data, self.client_data_json, self.signature = bytes(authenticator_data), bytes(client_data_json), bytes(signature)
        self.x, self.y, self.challenge, self.origin, self.rp_id_hash = x, y, bytes(challenge), origin, bytes(rp_id_hash)
        self.flags_required, self.allow_cross_origin = flags_required, bool(allow_cross_origin)

    def replace(self, **kw):
        d = dict(self.__dict__)
        d.update(kw)
        return Assertion(**d)


def b64url(b):
    return base64.urlsafe_b64encode(b).rstrip(b"=")


def expected_prefix(challenge, origin):
    return b'{"type":"webauthn.get","challenge":"' + b64url(challenge) + b'","origin":"' + origin.encode() + b'","crossOrigin":'


def client_data_ok(cd, challenge, origin, allow_cross_origin):
    e = expected_prefix(challenge, origin)
    if not cd.startswith(e):
        return False
    rest = cd[len(e):]
    for word in (b"true", b"false"):
        if rest.startswith(word):
            break
    else:
        return False
    if rest[len(word):len(word) + 1] not in (b",", b"}") or not cd.endswith(b"}"):
        return False
    return word == b"false" or allow_cross_origin


def der_integer(sig, pos):
    """The INTEGER at sig[pos:] under the strict rule -> (value, position behind it), or None."""
    if pos + 2 > len(sig) or sig[pos] != 0x02:
        return None
    n = sig[pos + 1]
    body = sig[pos + 2:pos + 2 + n]
    if n & 0x80 or not 1 <= n <= 33 or len(body) != n:
        return None
    if body[0] & 0x80:
        return None  # negative
    if n > 1 and body[0] == 0 and not body[1] & 0x80:
        return None  # not minimal
    if n == 33 and body[0] != 0:
        return None
    return int.from_bytes(body, "big"), pos + 2 + n


def der_parse(sig):
    """(r, s) of the strict DER of ECDSA-Sig-Value, or None."""
    if not 8 <= len(sig) <= 72 or sig[0] != 0x30 or sig[1] & 0x80 or sig[1] != len(sig) - 2:
        return None
    a = der_integer(sig, 2)
    if a is None:
        return None
    b = der_integer(sig, a[1])
    if b is None or b[1] != len(sig):
        return None
    return a[0], b[0]


def der_encode(r, s):
    """The DER a conforming authenticator emits for (r, s)."""
    def integer(v):
        b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
        if b[0] & 0x80:
            b = b"\x00" + b
        return bytes([0x02, len(b)]) + b
    body = integer(r) + integer(s)
    return bytes([0x30, len(body)]) + body


def msghash(authenticator_data, client_data_json):
    return int.from_bytes(hashlib.sha256(authenticator_data + hashlib.sha256(client_data_json).digest()).digest(), "big")


def check(a):
    """(reason, the 160-byte record, the signature counter) of one Assertion."""
    zero = bytes(160)
    ad, cd, sig = a.authenticator_data, a.client_data_json, a.signature
    if (len(ad) > AUTHDATA_MAX or len(cd) > CLIENTDATA_MAX or not 8 <= len(sig) <= 72 or not 1 <= len(a.challenge) <= CHALLENGE_MAX
            or len(a.origin.encode()) > ORIGIN_MAX):
        return SIZE, zero, 0
    if len(ad) < 37:
        return AUTHDATA, zero, 0
    count = int.from_bytes(ad[33:37], "big")
    if ad[:32] != a.rp_id_hash:
        return RPID, zero, count
    if ad[32] & a.flags_required != a.flags_required:
        return FLAGS, zero, count
    if not client_data_ok(cd, a.challenge, a.origin, a.allow_cross_origin):
        return CLIENTDATA, zero, count
    rs = der_parse(sig)
    if rs is None:
        return SIGNATURE_DER, zero, count
    z = msghash(ad, cd)
    return R.verify_ints(a.x, a.y, rs[0], rs[1], z), R.record(a.x, a.y, rs[0], rs[1], z), count
