"""The assertion set of the WebAuthn tests: a few hundred named assertions, deterministic, with the (reason, record, counter)
tests/webauthn_ref.py gives each.  Signatures come from es256_ref.sign's formula with the fixed key D and the fixed nonces KS
(r = x(k G) is computed once per nonce).  build() costs a few seconds of CPU and is cached for the session.

What is in it, by name prefix:
  valid/        plain assertions: varying counters, extension bytes, nonces, with and without a trailing member
  cdlen/        clientDataJSON of length L, lengthened by a trailing member after crossOrigin: L mod 64 in {0, 1, 55, 56, 63} around
                the ends of the second, third and fourth block (119 .. 257) and below and at the cap of 4096.  A clientDataJSON that
                passes the client-data rule has at least 72 bytes (the literal parts of E are 64, a challenge of one byte gives two
                characters, then `false}`), and one that fails it is never hashed: so no hashed message ends in the first block or
                has 64 or 65 bytes (the second message has 37 + 32 bytes at least).  cdlen/72 is that minimum; cdlen/64 and
                cdlen/65 are in the set as the CLIENTDATA verdicts they are; tests/webauthn_host_check.cpp hashes the lengths of the
                first block, 64 and 65 directly (hash_messages below)
  adlen/        authenticatorData of 37, 87, 88, 95, 96 and 1024 bytes (length + 32 = 5, 55, 56, 63, 0 and 32 mod 64), the extension
                part filled with bytes 0x80 .. 0xff
  cap/          each length at its cap (passes) and one above (SIZE); authenticatorData of 36 bytes (AUTHDATA); an empty challenge
  rpid/ flags/  rpIdHash wrong in byte 0 / byte 31; UP clear; UV required and clear / set
  cd/           the client-data rule: webauthn.create, the challenge wrong in its first / last character, challenges of 1, 2, 3, 32
                and 64 bytes, another origin, the closing quote of the origin, shorter than E, equal to E, `tru}`, `true` with and
                without the policy, `false` followed by another byte, a last byte that is not `}`
  der/          33-, 32-, 31- and 1-byte integers, a non-minimal 00, a negative integer, a byte after s, long-form lengths, wrong
                tags, the sequence length off by one either way, a zero-length integer, r = 0, 7- and 73-byte signatures
  ecdsa/        s altered, another key, a key off the curve, x >= p
  order/        two defects each: the earlier test's reason wins
  pad/          fillers of chosen lengths, so that in the order of the set the two messages of some request start at every
                residue mod 4 of the packed blob (packing below; assert_alignment_coverage)

msghash >= n would need a SHA-256 preimage (n is 2^256 - 2^224 + ...: a digest with 32 leading one bits and more): it cannot be
constructed and is not in the set; zk_es256_verify's own set holds that RANGE case.
"""
import functools
import hashlib
import struct

import es256_ref as R
import webauthn_ref as W

D = 0x1F2E3D4C5B6A79880796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF1
KS = [0x5A5A0000 + 0x01010101 * i + (0x77 << 200) for i in range(1, 9)]
RP_ID = "a.example"
RP_HASH = hashlib.sha256(RP_ID.encode()).digest()
ORIGIN = "https://a.example"
CHALLENGE = bytes(range(0xE0, 0x100))  # 32 bytes


@functools.lru_cache(maxsize=None)
def _key(d):
    return R.affine_mul(d, R.G)


@functools.lru_cache(maxsize=None)
def _r_of(k):
    return R.affine_mul(k, R.G)[0] % R.N


def sign(z, k, d=D):
    r = _r_of(k)
    s = pow(k, -1, R.N) * (z + r * d) % R.N
    assert r and s
    return r, s


def auth_data(length=37, flags=W.UP, counter=7, rp_hash=RP_HASH):
    ext = bytes(0x80 + (5 * i + 3) % 0x80 for i in range(max(0, length - 37)))
    full = rp_hash + bytes([flags]) + counter.to_bytes(4, "big") + ext
    return full[:length] if length < 37 else full


def client_data(challenge=CHALLENGE, origin=ORIGIN, length=None, cross=b"false", typ=b"webauthn.get"):
    """What a conforming client serialises; length: lengthened to exactly that by a trailing member (None: no extra member)."""
    head = b'{"type":"' + typ + b'","challenge":"' + W.b64url(challenge) + b'","origin":"' + origin.encode() + b'","crossOrigin":' + cross
    if length is None:
        return head + b"}"
    if length == len(head) + 1:
        return head + b"}"
    fill = length - len(head) - len(b',"x":""}')
    assert fill >= 0, "a clientDataJSON of %d bytes cannot carry a trailing member" % length
    return head + b',"x":"' + bytes(0x61 + i % 26 for i in range(fill)) + b'"}'


def make(ad=None, cd=None, k=KS[0], d=D, challenge=CHALLENGE, origin=ORIGIN, flags_required=W.UP, allow_cross_origin=False, rp_hash=RP_HASH):
    """A correctly signed assertion over (ad, cd) and the expectations given."""
    ad = auth_data() if ad is None else ad
    cd = client_data(challenge, origin) if cd is None else cd
    r, s = sign(W.msghash(ad, cd), k, d)
    q = _key(d)
    return W.Assertion(ad, cd, W.der_encode(r, s), q[0], q[1], challenge, origin, rp_hash, flags_required, allow_cross_origin)


def _find(pred, what):
    """The first (counter, nonce) whose plain assertion satisfies pred(r, s)."""
    for counter in range(1, 4000):
        for k in KS:
            a = make(ad=auth_data(counter=counter), k=k)
            r, s = W.der_parse(a.signature)
            if pred(r, s):
                return a
    raise AssertionError("no signature with " + what)


class CaseSet:
    def __init__(self, names, assertions, built_for):
        self.names, self.assertions = names, assertions
        res = [W.check(a) for a in assertions]
        self.reasons, self.records, self.counts = [r[0] for r in res], [r[1] for r in res], [r[2] for r in res]
        for name, want, got in zip(names, built_for, self.reasons):
            assert want is None or want == got, "%s: built for %s, the reference says %s" % (name, W.REASON_NAMES[want], W.REASON_NAMES[got])

    def __len__(self):
        return len(self.names)

    def index(self, name):
        return self.names.index(name)

    def valid_indices(self):
        return [i for i, v in enumerate(self.reasons) if v == W.VALID]

    def invalid_indices(self):
        return [i for i, v in enumerate(self.reasons) if v != W.VALID]


CD_MIN = 72  # the shortest clientDataJSON that passes the rule
CD_RESIDUES = (0, 1, 55, 56, 63)
CD_LENGTHS = [CD_MIN] + [64 * q + m for q in (1, 2, 3, 4) for m in CD_RESIDUES if CD_MIN <= 64 * q + m <= 257] + [4096 - 64 + m for m in CD_RESIDUES[1:]] + [4096]
AD_LENGTHS = [37, 87, 88, 95, 96, 1024]
CHALLENGE_LENGTHS = [1, 2, 3, 32, 64]


def _cd_of_length(length):
    """(challenge, origin, clientDataJSON) with len(clientDataJSON) = length: the usual expectations where they fit, the shortest
    ones for the lengths below."""
    for challenge, origin in ((CHALLENGE, ORIGIN), (b"\xfb", "o"), (b"\xfb", "")):
        shortest = len(client_data(challenge, origin))
        if length == shortest or length >= shortest + len(b',"x":""'):
            return challenge, origin, client_data(challenge, origin, length)
    raise AssertionError("no passing clientDataJSON has %d bytes" % length)


@functools.lru_cache(maxsize=None)
def build():
    cases = []  # (name, Assertion, the reason the construction is built for or None)

    def add(name, a, want=None):
        cases.append((name, a, want))

    for i in range(64):
        ad = auth_data(37 + (i % 4) * 11, flags=W.UP | (W.UV if i & 1 else 0) | (0x40 if i & 2 else 0), counter=0x01020300 + i)
        cd = client_data(length=None if i % 3 else 140 + 7 * i)
        add("valid/%d" % i, make(ad, cd, k=KS[i % len(KS)]), W.VALID)
    add("valid/counter=ffffffff", make(auth_data(counter=0xFFFFFFFF)), W.VALID)
    add("valid/counter=80000000", make(auth_data(counter=0x80000000)), W.VALID)

    for n in CD_LENGTHS:
        ch, org, cd = _cd_of_length(n)
        assert len(cd) == n
        add("cdlen/%d" % n, make(cd=cd, challenge=ch, origin=org, k=KS[n % len(KS)]), W.VALID)
    for n in (64, 65):  # (too short to pass: see the module's text)
        add("cdlen/%d" % n, make(cd=client_data(b"\xfb", "")[:n - 1] + b"}", challenge=b"\xfb", origin=""), W.CLIENTDATA)
    for n in AD_LENGTHS:
        add("adlen/%d" % n, make(ad=auth_data(n, counter=n), k=KS[n % len(KS)]), W.VALID)
    add("adlen/1024+cdlen/4096", make(ad=auth_data(1024), cd=client_data(length=4096)), W.VALID)

    # caps
    add("cap/authdata=1025", make(ad=auth_data(1025)), W.SIZE)
    add("cap/clientdata=4097", make(cd=client_data(length=4097)), W.SIZE)
    add("cap/authdata=36", make().replace(authenticator_data=auth_data(37)[:36]), W.AUTHDATA)
    add("cap/authdata=0", make().replace(authenticator_data=b""), W.AUTHDATA)
    add("cap/clientdata=0", make().replace(client_data_json=b""), W.CLIENTDATA)
    ch64, ch65 = bytes(range(100, 164)), bytes(range(100, 165))
    add("cap/challenge=64", make(challenge=ch64), W.VALID)
    add("cap/challenge=65", make(challenge=ch65), W.SIZE)
    add("cap/challenge=0", make(challenge=b""), W.SIZE)
    o255 = "https://" + "b" * (255 - 8 - 8) + ".example"
    assert len(o255) == 255
    add("cap/origin=255", make(origin=o255), W.VALID)
    add("cap/origin=256", make(origin="c" + o255), W.SIZE)
    add("cap/origin=0", make(origin=""), W.VALID)
    both33 = _find(lambda r, s: r >> 255 and s >> 255, "r and s of 33 bytes")
    assert len(both33.signature) == 72
    add("cap/signature=72", both33, W.VALID)
    add("cap/signature=73", both33.replace(signature=both33.signature + b"\x00"), W.SIZE)
    add("cap/signature=7", make().replace(signature=bytes.fromhex("30050201010201")), W.SIZE)
    add("cap/signature=0", make().replace(signature=b""), W.SIZE)

    # rpIdHash and flags
    base = make()
    for byte in (0, 31):
        h = bytearray(RP_HASH)
        h[byte] ^= 0x01
        add("rpid/expected-wrong-in-byte-%d" % byte, base.replace(rp_id_hash=bytes(h)), W.RPID)
        add("rpid/sent-wrong-in-byte-%d" % byte, make(ad=auth_data(rp_hash=bytes(h))), W.RPID)
    add("flags/up-clear", make(ad=auth_data(flags=0)), W.FLAGS)
    add("flags/up-clear-uv-set", make(ad=auth_data(flags=W.UV)), W.FLAGS)
    add("flags/uv-required-and-clear", make(ad=auth_data(flags=W.UP), flags_required=W.UP | W.UV), W.FLAGS)
    add("flags/uv-required-and-set", make(ad=auth_data(flags=W.UP | W.UV), flags_required=W.UP | W.UV), W.VALID)
    add("flags/nothing-required", make(ad=auth_data(flags=0), flags_required=0), W.VALID)
    add("flags/all-set", make(ad=auth_data(flags=0xFF), flags_required=W.UP | W.UV), W.VALID)

    # the client-data rule
    add("cd/type=webauthn.create", make(cd=client_data(typ=b"webauthn.create")), W.CLIENTDATA)
    good = client_data()
    at = good.index(b'"challenge":"') + len(b'"challenge":"')
    n64 = len(W.b64url(CHALLENGE))
    for name, pos in (("first", at), ("last", at + n64 - 1)):
        cd = bytearray(good)
        cd[pos] = ord("A") if cd[pos] != ord("A") else ord("B")
        add("cd/challenge-wrong-in-its-%s-character" % name, make(cd=bytes(cd)), W.CLIENTDATA)
    for n in CHALLENGE_LENGTHS:
        ch = bytes((0xF9 + 3 * i) & 0xFF for i in range(n))
        add("cd/challenge=%d" % n, make(challenge=ch), W.VALID)
        other = bytes([ch[-1] ^ 0x01])
        add("cd/challenge=%d-last-byte-differs" % n, make(cd=client_data(ch[:-1] + other), challenge=ch), W.CLIENTDATA)
    add("cd/challenge-one-byte-short", make(cd=client_data(CHALLENGE[:-1])), W.CLIENTDATA)
    add("cd/origin-differs", make(cd=client_data(origin="https://b.example")), W.CLIENTDATA)
    add("cd/origin-closing-quote", make(cd=client_data(origin="https://a.example.evil")), W.CLIENTDATA)
    add("cd/origin-expected-longer", make(cd=client_data(origin="https://a.exampl")), W.CLIENTDATA)
    e = W.expected_prefix(CHALLENGE, ORIGIN)
    add("cd/shorter-than-E", make(cd=e[:-1]), W.CLIENTDATA)
    add("cd/one-byte", make(cd=b"{"), W.CLIENTDATA)
    add("cd/equal-to-E", make(cd=e), W.CLIENTDATA)
    add("cd/tru}", make(cd=e + b"tru}"), W.CLIENTDATA)
    add("cd/true", make(cd=e + b"true"), W.CLIENTDATA)
    add("cd/false", make(cd=e + b"false"), W.CLIENTDATA)
    add("cd/fals}", make(cd=e + b"fals}"), W.CLIENTDATA)
    add("cd/true-without-the-policy", make(cd=client_data(cross=b"true")), W.CLIENTDATA)
    add("cd/true-with-the-policy", make(cd=client_data(cross=b"true"), allow_cross_origin=True), W.VALID)
    add("cd/true-with-the-policy-and-a-member", make(cd=client_data(cross=b"true", length=200), allow_cross_origin=True), W.VALID)
    add("cd/false-with-the-policy", make(allow_cross_origin=True), W.VALID)
    add("cd/false-then-another-byte", make(cd=e + b"false }"), W.CLIENTDATA)
    add("cd/falsey", make(cd=e + b"falsey}"), W.CLIENTDATA)
    add("cd/null", make(cd=e + b"null}"), W.CLIENTDATA)
    add("cd/last-byte-not-a-brace", make(cd=e + b'false,"x":"y"} '), W.CLIENTDATA)
    add("cd/last-byte-missing", make(cd=e + b'false,"x":"y"'), W.CLIENTDATA)
    add("cd/leading-space", make(cd=b" " + good), W.CLIENTDATA)
    add("cd/other-member-order", make(cd=b'{"challenge":"' + W.b64url(CHALLENGE) + b'","type":"webauthn.get","origin":"' + ORIGIN.encode()
                                      + b'","crossOrigin":false}'), W.CLIENTDATA)

    # DER
    r33 = _find(lambda r, s: r >> 255 and not s >> 255 and s >> 248, "r of 33 bytes and s of 32")
    s33 = _find(lambda r, s: not r >> 255 and r >> 248 and s >> 255, "r of 32 bytes and s of 33")
    both32 = _find(lambda r, s: not r >> 255 and r >> 248 and not s >> 255 and s >> 248, "r and s of 32 bytes")
    s31 = _find(lambda r, s: 0 < s >> 240 < 0x80, "s of 31 bytes")
    add("der/r=33-bytes", r33, W.VALID)
    add("der/s=33-bytes", s33, W.VALID)
    add("der/r=s=32-bytes", both32, W.VALID)
    add("der/s=31-bytes", s31, W.VALID)
    assert len(s31.signature) in (69, 70)
    r, s = W.der_parse(base.signature)
    add("der/r=31-bytes", base.replace(signature=W.der_encode(r >> 9, s)), W.MISMATCH)
    add("der/r=1-byte", base.replace(signature=W.der_encode(5, s)), W.MISMATCH)
    add("der/s=1-byte", base.replace(signature=W.der_encode(r, 0x7F)), W.MISMATCH)
    add("der/r=s=1-byte", base.replace(signature=W.der_encode(1, 1)), W.MISMATCH)
    add("der/r=0", base.replace(signature=W.der_encode(0, s)), W.RANGE)
    add("der/s=0", base.replace(signature=W.der_encode(r, 0)), W.RANGE)
    add("der/r=n", base.replace(signature=W.der_encode(R.N, s)), W.RANGE)
    add("der/s=2^256-1", base.replace(signature=W.der_encode(r, 2**256 - 1)), W.RANGE)

    def raw(rb, sb, seq_len=None, tags=(0x30, 0x02, 0x02), tail=b""):
        body = bytes([tags[1], len(rb)]) + rb + bytes([tags[2], len(sb)]) + sb
        return bytes([tags[0], len(body) if seq_len is None else seq_len]) + body + tail

    rb, sb = r.to_bytes(32, "big"), s.to_bytes(32, "big")
    rb = rb if rb[0] < 0x80 else b"\x00" + rb
    sb = sb if sb[0] < 0x80 else b"\x00" + sb
    assert raw(rb, sb) == base.signature
    small = bytes([0x12]) + bytes(range(30))  # a 31-byte positive value
    bad = W.SIGNATURE_DER
    add("der/non-minimal-00-on-r", base.replace(signature=raw(b"\x00" + small, sb)), bad)
    add("der/non-minimal-00-on-s", base.replace(signature=raw(rb, b"\x00" + small)), bad)
    add("der/00-00", base.replace(signature=raw(b"\x00\x00", sb)), bad)
    add("der/negative-r", base.replace(signature=raw(b"\x80" + small, sb)), bad)
    add("der/negative-s", base.replace(signature=raw(rb, b"\xff" + small)), bad)
    add("der/negative-one-byte", base.replace(signature=raw(b"\x80", sb)), bad)
    add("der/33-bytes-without-00", base.replace(signature=raw(b"\x01" + bytes([0x80]) + bytes(31), small)), bad)
    add("der/34-bytes", base.replace(signature=raw(b"\x00" + bytes([0x80]) + bytes(32), small)), bad)
    add("der/byte-after-s-counted", base.replace(signature=bytes([0x30, len(raw(rb, sb)) - 1]) + raw(rb, sb)[2:] + b"\x00"), bad)
    add("der/byte-after-s-uncounted", base.replace(signature=raw(rb, sb, tail=b"\x00")), bad)
    add("der/long-form-sequence", base.replace(signature=bytes([0x30, 0x81, len(raw(small, small)) - 2]) + raw(small, small)[2:]), bad)
    add("der/long-form-integer", base.replace(signature=bytes([0x30, 3 + 31 + 2 + 31, 0x02, 0x81, 31]) + small + bytes([0x02, 31]) + small), bad)
    add("der/indefinite-length", base.replace(signature=bytes([0x30, 0x80]) + raw(small, small)[2:]), bad)
    add("der/tag-31", base.replace(signature=raw(rb, sb, tags=(0x31, 0x02, 0x02))), bad)
    add("der/r-tag-03", base.replace(signature=raw(rb, sb, tags=(0x30, 0x03, 0x02))), bad)
    add("der/s-tag-30", base.replace(signature=raw(rb, sb, tags=(0x30, 0x02, 0x30))), bad)
    add("der/sequence-length+1", base.replace(signature=raw(rb, sb, seq_len=len(raw(rb, sb)) - 1)), bad)
    add("der/sequence-length-1", base.replace(signature=raw(rb, sb, seq_len=len(raw(rb, sb)) - 3)), bad)
    add("der/zero-length-r", base.replace(signature=raw(b"", sb)), bad)
    add("der/zero-length-s", base.replace(signature=raw(rb, b"")), bad)
    add("der/s-runs-past-the-end", base.replace(signature=raw(rb, sb)[:-1]), bad)
    add("der/s-length-past-the-end", base.replace(signature=raw(rb, sb)[:-len(sb) - 1] + bytes([len(sb) + 1]) + sb), bad)
    add("der/only-r", base.replace(signature=bytes([0x30, 2 + len(rb), 0x02, len(rb)]) + rb), bad)
    add("der/8-bytes", base.replace(signature=bytes.fromhex("3006020101020101")), W.MISMATCH)
    add("der/8-bytes-of-ff", base.replace(signature=b"\xff" * 8), bad)
    add("der/72-bytes-of-00", base.replace(signature=bytes(72)), bad)

    # ECDSA over the assembled record
    add("ecdsa/s+1", base.replace(signature=W.der_encode(r, s + 1)), W.MISMATCH)
    add("ecdsa/r-and-s-swapped", base.replace(signature=W.der_encode(s, r)), W.MISMATCH)
    other = _key(D + 1)
    add("ecdsa/another-key", base.replace(x=other[0], y=other[1]), W.MISMATCH)
    add("ecdsa/y-negated", base.replace(y=R.P - base.y), W.MISMATCH)
    add("ecdsa/signed-by-another-key", make(d=D + 1).replace(x=base.x, y=base.y), W.MISMATCH)
    add("ecdsa/key-off-the-curve", base.replace(y=(base.y + 1) % R.P), W.OFF_CURVE)
    add("ecdsa/key=(0,0)", base.replace(x=0, y=0), W.OFF_CURVE)
    add("ecdsa/x=p", base.replace(x=R.P), W.RANGE)
    add("ecdsa/x=2^256-1", base.replace(x=2**256 - 1), W.RANGE)
    add("ecdsa/y=p", base.replace(y=R.P), W.RANGE)
    add("ecdsa/counter-changed-after-signing", base.replace(authenticator_data=auth_data(counter=8)), W.MISMATCH)
    add("ecdsa/extension-byte-changed-after-signing", make(ad=auth_data(96)).replace(authenticator_data=auth_data(96)[:-1] + b"\x00"), W.MISMATCH)
    add("ecdsa/member-changed-after-signing", make(cd=client_data(length=150)).replace(client_data_json=client_data(length=150)[:-3] + b'!"}'),
        W.MISMATCH)

    # two defects: the earlier test wins
    wrong_rp = bytes([RP_HASH[0] ^ 1]) + RP_HASH[1:]
    add("order/size-before-authdata", make(cd=client_data(length=4097)).replace(authenticator_data=auth_data(37)[:36]), W.SIZE)
    add("order/size-before-der", base.replace(signature=b"\xff" * 73), W.SIZE)
    add("order/authdata-before-clientdata", base.replace(authenticator_data=auth_data(37)[:20], client_data_json=b"{}"), W.AUTHDATA)
    add("order/rpid-before-flags", base.replace(authenticator_data=auth_data(flags=0), rp_id_hash=wrong_rp), W.RPID)
    add("order/flags-before-clientdata", base.replace(authenticator_data=auth_data(flags=0), client_data_json=b"{}"), W.FLAGS)
    add("order/clientdata-before-der", base.replace(client_data_json=good[:-1], signature=bytes(72)), W.CLIENTDATA)
    add("order/der-before-range", base.replace(signature=raw(b"\x80", sb), x=R.P), bad)
    add("order/range-before-off-curve", base.replace(signature=W.der_encode(0, s), y=(base.y + 1) % R.P), W.RANGE)
    add("order/off-curve-before-mismatch", base.replace(signature=W.der_encode(r, s + 1), y=(base.y + 1) % R.P), W.OFF_CURVE)

    # fillers: the start of a request's messages in the packed blob moves by the lengths before it; these make every residue occur
    for i in range(8):
        add("pad/%d" % i, make(ad=auth_data(37 + i, counter=i), cd=client_data(length=140 + (3 * i) % 4), k=KS[i]), W.VALID)

    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    cs = CaseSet(names, [c[1] for c in cases], [c[2] for c in cases])
    assert_alignment_coverage(cs)
    return cs


def packing(assertions):
    """Where zk_webauthn_verify puts the messages of the requests it uploads (csrc/webauthn.hip): the requests inside the caps, in
    order, each as authenticatorData, clientDataJSON, signature, E back to back in one blob that starts on a word boundary.
    -> [(index, offset of authenticatorData, offset of clientDataJSON)]"""
    out, pos = [], 0
    for i, a in enumerate(assertions):
        if W.check(a)[0] == W.SIZE:
            continue
        out.append((i, pos, pos + len(a.authenticator_data)))
        pos += len(a.authenticator_data) + len(a.client_data_json) + len(a.signature) + len(W.expected_prefix(a.challenge, a.origin))
    return out


def alignment_coverage(cs):
    """(residues mod 4 at which the authenticatorData of a VALID request starts, the same for its clientDataJSON)."""
    ad, cd = set(), set()
    for i, a_off, c_off in packing(cs.assertions):
        if cs.reasons[i] == W.VALID:
            ad.add(a_off % 4)
            cd.add(c_off % 4)
    return ad, cd


def assert_alignment_coverage(cs):
    ad, cd = alignment_coverage(cs)
    assert ad == {0, 1, 2, 3} and cd == {0, 1, 2, 3}, (ad, cd)


def hash_messages():
    """(first piece, second piece) pairs for the hash alone: every length around the first three block edges, split at every kind
    of seam; with the FIPS 180-4 vectors."""
    out = [(b"", b""), (b"abc", b""), (b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", b""), (b"ab", b"c"), (b"", b"abc")]
    body = bytes((151 * i + 0x7B) & 0xFF for i in range(200))
    for n in (1, 3, 4, 5, 54, 55, 56, 57, 62, 63, 64, 65, 66, 118, 119, 120, 121, 127, 128, 129, 183, 184, 191, 192, 193):
        for cut in sorted({0, 1, 2, 3, n // 2, max(0, n - 32), n - 1, n}):
            if 0 <= cut <= n:
                out.append((body[:cut], body[cut:n]))
    return out


MAGIC_IN, MAGIC_OUT = 0x57414331, 0x5741434F  # "WAC1", "WACO"
OUT_BYTES = 1 + 4 + 160


def write_case_file(path, cs):
    """The set and hash_messages() as tests/webauthn_host_check.cpp reads them, everything back to back (so nothing is aligned):
    MAGIC_IN, the two counts; per assertion five u32 lengths (authenticatorData, clientDataJSON, signature, challenge, origin), the
    key big-endian (x, y), rpIdHash, flags_required, allow_cross_origin, then the five byte strings; per message two u32 lengths and
    the two pieces.  All integers little-endian."""
    msgs = hash_messages()
    out = [struct.pack("<III", MAGIC_IN, len(cs), len(msgs))]
    for a in cs.assertions:
        origin = a.origin.encode()
        out.append(struct.pack("<IIIII", len(a.authenticator_data), len(a.client_data_json), len(a.signature), len(a.challenge), len(origin)))
        out.append(a.x.to_bytes(32, "big") + a.y.to_bytes(32, "big") + a.rp_id_hash + bytes([a.flags_required, int(a.allow_cross_origin)]))
        out.append(a.authenticator_data + a.client_data_json + a.signature + a.challenge + origin)
    for p0, p1 in msgs:
        out.append(struct.pack("<II", len(p0), len(p1)) + p0 + p1)
    with open(path, "wb") as f:
        f.write(b"".join(out))
    return len(msgs)
