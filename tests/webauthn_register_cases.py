"""The registration set of the WebAuthn registration tests: a few hundred named registrations, deterministic, with the (reason,
credential) tests/webauthn_register_ref.py gives each.  Self attestations are signed with webauthn_cases.sign's formula, its fixed
key D and its fixed nonces KS.  build() asserts for each case the reason it was built for against the reference; it costs a few
seconds of CPU and is cached for the session.

What is in it, by name prefix (the smallest inputs at which each part of the rule can go wrong):
  valid/   fmt none and packed self under both policies; an x5c statement and the fmts tpm, apple, fido-u2f under policy 0
           (accepted, NOT_JUDGED) and policy 1 (ATTESTATION); UV required and set; counters 0, 0x80000000, 0xffffffff
  ad/      the three authData rules shared with the assertion check: 36 bytes, rpIdHash wrong in byte 0 / 31, UP clear, UV required
  head/    authData byte strings of 255 and 256 bytes (the one- and two-byte length heads; credential ids of 123 / 124 bytes);
           credential ids of 1, 23, 24, 255, 256, 1023 bytes; each head once in a longer form than needed (58 17, 59 00 xx, 5a,
           5b, and the same on a text, an array, a map, an integer and a tag); additional information 28, 29, 30; 5f, 7f, 9f, bf and
           a lone ff; an 8-byte length of 2^64 - 1 and of "bytes left + 1", the latter in its shortest head too; a map count of
           "bytes left + 1"; the object cut after each of its first 12 bytes and one byte before its end; one byte after the end
  shape/   two and four entries; authData before attStmt; "fmt" as a byte string; a key repeated; fmt not text; attStmt an array;
           authData a text string
  stmt/    each well-formed one under both policies: every major type and a tag; half, single and double floats; false / true /
           null / undefined; a one-byte simple value >= 32 and < 32 (the latter CBOR); arrays nested 1, 2 and 200 deep, maps 200
           deep; an x5c array of three byte strings of 700 bytes; "none" with a member; packed with sig before alg, alg -257 and
           -8, a third member, sig a text string
  cred/    AT clear; authData of exactly 37 bytes with AT set; authData cut inside aaguid, the length, the id, the key; id length 0
           and 1024; ED set with nothing after the key; ED clear with one byte after; ED set with {"credProtect": 2}, with an array,
           with a malformed map, with a byte after the map; an extension string of exactly the bytes left, and of one more
  cose/    every one of the 13 template bytes changed once (the three changes that move the key's end - the map count and the two
           coordinate lengths - are CREDENTIAL verdicts: the key no longer ends where authData does); the members in another
           order; six members; x of 31 and 33 bytes; an OKP key; a key off the curve (OFF_CURVE); x = p (RANGE)
  cd/      type webauthn.get; wrong challenge, wrong origin; crossOrigin true with and without the policy
  self/    s + 1 and a signature by another key (MISMATCH); three DER defects; signatures of 7 and 73 bytes; hashed messages whose
           length mod 64 is 55, 56, 63, 0, 1 - both of them: authData || digest has 164 + idLength bytes, so id lengths 19, 20, 27,
           28, 29, with clientDataJSON of 183, 184, 191, 192, 193 bytes
  cap/     each size at its cap (accepted) and one above (SIZE); empty object, empty challenge
  order/   one case per adjacent pair of tests with both defects present: the earlier reason wins
  pad/     fillers, so that in the set's packing (packing below) the object and the clientDataJSON of some accepted request start
           at every residue mod 4 of the blob (assert_alignment_coverage)
"""
import functools
import struct

import es256_ref as R
import webauthn_cases as A
import webauthn_ref as W
import webauthn_register_ref as G

D, KS, RP_ID, RP_HASH, ORIGIN, CHALLENGE = A.D, A.KS, A.RP_ID, A.RP_HASH, A.ORIGIN, A.CHALLENGE
AAGUID = bytes(range(0xA0, 0xB0))
T = G.Text


class Raw(bytes):
    """Bytes that stand in an encoding as they are (a malformed item, a float, a head in another form)."""


def head(major, n, width=None):
    """The head of `major` with argument n: in shortest form, or with `width` argument bytes (0, 1, 2, 4, 8)."""
    if width is None:
        width = 0 if n < 24 else 1 if n < 1 << 8 else 2 if n < 1 << 16 else 4 if n < 1 << 32 else 8
    if width == 0:
        return bytes([major << 5 | n])
    return bytes([major << 5 | {1: 24, 2: 25, 4: 26, 8: 27}[width]]) + n.to_bytes(width, "big")


def enc(v):
    """The canonical (shortest-head, definite-length) encoding of a value made of int, bytes, Text, list, Map, Tag, Simple, Raw."""
    if isinstance(v, Raw):
        return bytes(v)
    if isinstance(v, bool):
        raise TypeError("use G.TRUE / G.FALSE")
    if isinstance(v, int):
        return head(0, v) if v >= 0 else head(1, -1 - v)
    if isinstance(v, bytes):
        return head(2, len(v)) + v
    if isinstance(v, T):
        return head(3, len(v.raw)) + v.raw
    if isinstance(v, list):
        return head(4, len(v)) + b"".join(enc(x) for x in v)
    if isinstance(v, G.Map):
        return head(5, len(v.pairs)) + b"".join(enc(k) + enc(x) for k, x in v.pairs)
    if isinstance(v, G.Tag):
        return head(6, v.number) + enc(v.item)
    if isinstance(v, G.Simple):
        return head(7, v.value)
    raise TypeError(type(v))


def cose_key(q, pairs=None):
    x, y = (c if isinstance(c, bytes) else c.to_bytes(32, "big") for c in q)
    return enc(G.Map(pairs if pairs is not None else [(1, 2), (3, -7), (-1, 1), (-2, x), (-3, y)]))


def cred_id(n):
    return bytes((7 * i + 0x31) & 0xFF for i in range(n))


def auth_data(flags=G.UP | G.AT, counter=7, rp_hash=RP_HASH, id_len=16, key=None, ext=b"", id_len_field=None):
    key = cose_key(A._key(D)) if key is None else key
    return (rp_hash + bytes([flags]) + counter.to_bytes(4, "big") + AAGUID + (id_len if id_len_field is None else id_len_field).to_bytes(2, "big")
            + cred_id(id_len) + key + ext)


def att_obj(ad=None, fmt=T(b"none"), stmt=G.Map([])):
    return enc(G.Map([(T(b"fmt"), fmt), (T(b"attStmt"), stmt), (T(b"authData"), auth_data() if ad is None else ad)]))


def client_data(challenge=CHALLENGE, origin=ORIGIN, length=None, cross=b"false", typ=b"webauthn.create"):
    return A.client_data(challenge, origin, length, cross, typ)


def reg(obj=None, cd=None, challenge=CHALLENGE, origin=ORIGIN, flags_required=G.UP, allow_cross_origin=False, policy=G.ATT_IGNORE, rp_hash=RP_HASH):
    return G.Registration(att_obj() if obj is None else obj, client_data(challenge, origin) if cd is None else cd, challenge, origin, rp_hash,
                          flags_required, allow_cross_origin, policy)


def self_stmt(ad, cd, k=KS[0], d=D, extra=()):
    r, s = A.sign(W.msghash(ad, cd), k, d)
    return G.Map([(T(b"alg"), -7), (T(b"sig"), W.der_encode(r, s))] + list(extra))


def packed_self(ad=None, cd=None, k=KS[0], d=D, **kw):
    """A registration with a correct packed self attestation over (ad, cd)."""
    ad = auth_data() if ad is None else ad
    cd = client_data(kw.get("challenge", CHALLENGE), kw.get("origin", ORIGIN)) if cd is None else cd
    return reg(att_obj(ad, T(b"packed"), self_stmt(ad, cd, k, d)), cd, **kw)


def cred_bytes(c):
    """A credential dict (None: refused) as the 104 bytes of zk_webauthn_credential."""
    if c is None:
        return bytes(104)
    return struct.pack("<32s32s16sIIIIIBBxx", c["pubkey_x"], c["pubkey_y"], c["aaguid"], c["auth_data_off"], c["auth_data_len"], c["credential_id_off"],
                       c["credential_id_len"], c["sign_count"], c["flags"], c["attestation"])


class CaseSet:
    def __init__(self, names, regs, built_for):
        self.names, self.regs = names, regs
        res = [G.check(g) for g in regs]
        self.reasons, self.creds = [r[0] for r in res], [r[1] for r in res]
        for name, want, got, c in zip(names, built_for, self.reasons, self.creds):
            reason, att = want if isinstance(want, tuple) else (want, None)
            assert reason == got, "%s: built for %s, the reference says %s" % (name, G.REASON_NAMES[reason], G.REASON_NAMES[got])
            assert att is None or c["attestation"] == att, "%s: built for attestation %d, the reference says %d" % (name, att, c["attestation"])
            assert (c is None) == (got != G.VALID), name

    def __len__(self):
        return len(self.names)

    def index(self, name):
        return self.names.index(name)

    def valid_indices(self):
        return [i for i, v in enumerate(self.reasons) if v == G.VALID]

    def invalid_indices(self):
        return [i for i, v in enumerate(self.reasons) if v != G.VALID]


ID_LENGTHS = (1, 23, 24, 255, 256, 1023)
HASH_RESIDUES = (55, 56, 63, 0, 1)
HASH_ID_LENGTHS = (19, 20, 27, 28, 29)      # 164 + idLength = 55, 56, 63, 0, 1 mod 64
HASH_CD_LENGTHS = (183, 184, 191, 192, 193)  # the same residues
# cose/: (index in the 77 bytes, the byte put there, the verdict)
COSE_CHANGES = ((0, 0xA4, G.CREDENTIAL), (1, 0x04, G.COSE_KEY), (2, 0x01, G.COSE_KEY), (3, 0x04, G.COSE_KEY), (4, 0x27, G.COSE_KEY),
                (5, 0x21, G.COSE_KEY), (6, 0x02, G.COSE_KEY), (7, 0x23, G.COSE_KEY), (8, 0x78, G.COSE_KEY), (9, 0x21, G.CREDENTIAL),
                (42, 0x23, G.COSE_KEY), (43, 0x78, G.COSE_KEY), (44, 0x21, G.CREDENTIAL))
BOTH = ((G.ATT_IGNORE, "policy=0"), (G.ATT_NONE_OR_SELF, "policy=1"))


@functools.lru_cache(maxsize=None)
def build():
    cases = []  # (name, Registration, the reason - or (reason, attestation) - the construction is built for)

    def add(name, g, want):
        cases.append((name, g, want))

    Q = A._key(D)
    key = cose_key(Q)
    assert key == bytes.fromhex("a5010203262001215820") + Q[0].to_bytes(32, "big") + bytes.fromhex("225820") + Q[1].to_bytes(32, "big") and len(key) == 77
    good_ad, good_cd = auth_data(), client_data()
    assert len(good_ad) == 132 + 16

    # ---- valid/
    add("valid/none/policy=0", reg(), (G.VALID, G.ATTESTED_NOT_JUDGED))
    add("valid/none/policy=1", reg(policy=G.ATT_NONE_OR_SELF), (G.VALID, G.ATTESTED_NONE))
    add("valid/packed-self/policy=0", packed_self(), (G.VALID, G.ATTESTED_NOT_JUDGED))
    add("valid/packed-self/policy=1", packed_self(policy=G.ATT_NONE_OR_SELF), (G.VALID, G.ATTESTED_SELF))
    for i in range(1, len(KS)):
        ad = auth_data(flags=G.UP | G.AT | (G.UV if i & 1 else 0), counter=0x01020300 + i, id_len=16 + 5 * i)
        add("valid/packed-self/%d" % i, packed_self(ad, client_data(length=None if i % 3 else 150 + 7 * i), k=KS[i], policy=G.ATT_NONE_OR_SELF),
            (G.VALID, G.ATTESTED_SELF))
    x5c = [bytes((i + 3 * j) & 0xFF for i in range(300)) for j in range(2)]
    full = G.Map(self_stmt(good_ad, good_cd).pairs + [(T(b"x5c"), x5c)])
    others = [("x5c", T(b"packed"), full), ("tpm", T(b"tpm"), G.Map([(T(b"ver"), T(b"2.0")), (T(b"alg"), -65535), (T(b"sig"), bytes(64))])),
              ("apple", T(b"apple"), G.Map([(T(b"x5c"), x5c)])), ("fido-u2f", T(b"fido-u2f"), G.Map([(T(b"sig"), bytes(70)), (T(b"x5c"), x5c[:1])]))]
    for name, fmt, stmt in others:
        add("valid/%s/policy=0" % name, reg(att_obj(fmt=fmt, stmt=stmt)), (G.VALID, G.ATTESTED_NOT_JUDGED))
        add("valid/%s/policy=1" % name, reg(att_obj(fmt=fmt, stmt=stmt), policy=G.ATT_NONE_OR_SELF), G.ATTESTATION)
    uv = auth_data(flags=G.UP | G.UV | G.AT)
    add("valid/uv-required-and-set", packed_self(uv, flags_required=G.UP | G.UV, policy=G.ATT_NONE_OR_SELF), G.VALID)
    for c in (0, 0x80000000, 0xFFFFFFFF):
        add("valid/counter=%x" % c, reg(att_obj(auth_data(counter=c)), policy=G.ATT_NONE_OR_SELF), G.VALID)

    # ---- ad/
    add("ad/36-bytes", reg(att_obj(good_ad[:36])), G.AUTHDATA)
    add("ad/empty", reg(att_obj(b"")), G.AUTHDATA)
    for byte in (0, 31):
        h = bytearray(RP_HASH)
        h[byte] ^= 0x01
        add("ad/rpid-expected-wrong-in-byte-%d" % byte, reg(rp_hash=bytes(h)), G.RPID)
        add("ad/rpid-sent-wrong-in-byte-%d" % byte, reg(att_obj(auth_data(rp_hash=bytes(h)))), G.RPID)
    add("ad/up-clear", reg(att_obj(auth_data(flags=G.AT))), G.FLAGS)
    add("ad/uv-required-and-clear", reg(flags_required=G.UP | G.UV), G.FLAGS)
    add("ad/nothing-required", reg(att_obj(auth_data(flags=G.AT)), flags_required=0), G.VALID)

    # ---- head/
    for n, id_len in ((255, 123), (256, 124)):
        ad = auth_data(id_len=id_len)
        obj = att_obj(ad)
        assert len(ad) == n and obj[-n - (2 if n < 256 else 3):-n] == (b"\x58\xff" if n < 256 else b"\x59\x01\x00")
        add("head/authdata=%d" % n, packed_self(ad, policy=G.ATT_NONE_OR_SELF), G.VALID)
    for n in ID_LENGTHS:
        add("head/id=%d" % n, packed_self(auth_data(id_len=n), k=KS[n % len(KS)], policy=G.ATT_NONE_OR_SELF), G.VALID)

    def with_stmt_value(raw, policy=G.ATT_IGNORE):
        """fmt "packed" with the statement {"v": <raw>}."""
        return reg(att_obj(fmt=T(b"packed"), stmt=G.Map([(T(b"v"), Raw(raw))])), policy=policy)

    def with_ad_head(h):
        return reg(enc(G.Map([(T(b"fmt"), T(b"none")), (T(b"attStmt"), G.Map([])), (T(b"authData"), Raw(h + good_ad))])))

    add("head/shortest/58-18", with_stmt_value(head(2, 24) + bytes(24)), G.VALID)
    add("head/longer-form/58-17", with_stmt_value(head(2, 23, 1) + bytes(23)), G.CBOR)
    add("head/shortest/authdata-58", with_ad_head(head(2, len(good_ad))), G.VALID)
    add("head/longer-form/authdata-59-00-xx", with_ad_head(head(2, len(good_ad), 2)), G.CBOR)
    add("head/longer-form/authdata-5a", with_ad_head(head(2, len(good_ad), 4)), G.CBOR)
    add("head/longer-form/authdata-5b", with_ad_head(head(2, len(good_ad), 8)), G.CBOR)
    add("head/longer-form/59-00-ff", with_stmt_value(head(2, 255, 2) + bytes(255)), G.CBOR)
    add("head/shortest/59-01-00", with_stmt_value(head(2, 256) + bytes(256)), G.VALID)
    add("head/longer-form/5a-00-00-ff-ff", with_stmt_value(head(2, 300, 4) + bytes(300)), G.CBOR)
    add("head/longer-form/text-78-04", reg(enc(G.Map([(T(b"fmt"), Raw(head(3, 4, 1) + b"none")), (T(b"attStmt"), G.Map([])), (T(b"authData"), good_ad)]))),
        G.CBOR)
    add("head/longer-form/key-text-78-03", reg(enc(G.Map([(Raw(head(3, 3, 1) + b"fmt"), T(b"none")), (T(b"attStmt"), G.Map([])), (T(b"authData"), good_ad)]))),
        G.CBOR)
    add("head/longer-form/top-map-b8-03", reg(head(5, 3, 1) + att_obj()[1:]), G.CBOR)
    add("head/longer-form/statement-map-b8-00", reg(att_obj(stmt=Raw(head(5, 0, 1)))), G.CBOR)
    add("head/longer-form/array-98-01", with_stmt_value(head(4, 1, 1) + b"\x00"), G.CBOR)
    add("head/longer-form/integer-18-17", with_stmt_value(head(0, 23, 1)), G.CBOR)
    add("head/longer-form/integer-19-00-ff", with_stmt_value(head(0, 255, 2)), G.CBOR)
    add("head/longer-form/negative-3a-00-00-ff-ff", with_stmt_value(head(1, 0xFFFF, 4)), G.CBOR)
    add("head/longer-form/integer-1b-00-00-00-00-ff-ff-ff-ff", with_stmt_value(head(0, 0xFFFFFFFF, 8)), G.CBOR)
    add("head/longer-form/tag-d8-01", with_stmt_value(head(6, 1, 1) + b"\x00"), G.CBOR)
    add("head/shortest/integers", reg(att_obj(fmt=T(b"packed"), stmt=G.Map([(24, 255), (256, 65535), (65536, 2**32 - 1), (2**32, 2**64 - 1), (-25, -2**64)]))),
        G.VALID)
    for ai in (28, 29, 30):
        for major in (0, 2, 7):
            add("head/ai=%d/major=%d" % (ai, major), with_stmt_value(bytes([major << 5 | ai]) + bytes(8)), G.CBOR)
    add("head/indefinite/5f", with_stmt_value(bytes.fromhex("5f4100ff")), G.CBOR)
    add("head/indefinite/7f", with_stmt_value(bytes.fromhex("7f6161ff")), G.CBOR)
    add("head/indefinite/9f", with_stmt_value(bytes.fromhex("9f00ff")), G.CBOR)
    add("head/indefinite/bf", with_stmt_value(bytes.fromhex("bf0000ff")), G.CBOR)
    add("head/indefinite/statement-bf", reg(att_obj(stmt=Raw(bytes.fromhex("bfff")))), G.CBOR)
    add("head/indefinite/top-bf", reg(b"\xbf" + att_obj()[1:] + b"\xff"), G.CBOR)
    add("head/lone-ff", with_stmt_value(b"\xff"), G.CBOR)
    add("head/length=2^64-1", with_stmt_value(head(2, 2**64 - 1)), G.CBOR)
    add("head/array-count=2^64-1", with_stmt_value(head(4, 2**64 - 1)), G.CBOR)
    add("head/map-count=2^63", with_stmt_value(head(5, 2**63)), G.CBOR)
    tail = enc(T(b"authData")) + enc(good_ad)  # what stands behind the statement
    front = head(5, 3) + enc(T(b"fmt")) + enc(T(b"packed")) + enc(T(b"attStmt")) + head(5, 1) + enc(T(b"v"))
    add("head/8-byte-length=bytes-left+1", reg(front + head(2, len(tail) + 1, 8) + tail), G.CBOR)
    add("head/length=bytes-left+1", reg(front + head(2, len(tail) + 1) + tail), G.CBOR)
    add("head/length=bytes-left", reg(front + head(2, len(tail)) + tail), G.CBOR)  # (the string takes authData with it)
    add("head/array-count=bytes-left+1", reg(front + head(4, len(tail) + 1) + tail), G.CBOR)
    add("head/map-count=bytes-left+1", reg(front + head(5, len(tail) + 1) + tail), G.CBOR)
    add("head/statement-map-count=bytes-left+1", reg(front[:-3] + head(5, len(tail) + 1) + tail), G.CBOR)
    whole = att_obj()
    for n in list(range(1, 13)) + [len(whole) - 1]:
        add("head/cut-after-%d" % n, reg(whole[:n]), G.CBOR)
    add("head/one-byte-after-the-end", reg(whole + b"\x00"), G.CBOR)

    # ---- shape/
    fmt_, stmt_, ad_ = (T(b"fmt"), T(b"none")), (T(b"attStmt"), G.Map([])), (T(b"authData"), good_ad)
    add("shape/two-entries", reg(enc(G.Map([fmt_, stmt_]))), G.CBOR)
    add("shape/two-entries-without-the-statement", reg(enc(G.Map([fmt_, ad_]))), G.CBOR)
    add("shape/four-entries", reg(enc(G.Map([fmt_, stmt_, ad_, (T(b"x"), 0)]))), G.CBOR)
    add("shape/four-entries-counted-as-three", reg(enc(G.Map([fmt_, stmt_, ad_]))  + enc(T(b"x")) + enc(0)), G.CBOR)
    add("shape/authdata-before-the-statement", reg(enc(G.Map([fmt_, ad_, stmt_]))), G.CBOR)
    add("shape/fmt-last", reg(enc(G.Map([stmt_, ad_, fmt_]))), G.CBOR)
    add("shape/fmt-key-a-byte-string", reg(enc(G.Map([(b"fmt", T(b"none")), stmt_, ad_]))), G.CBOR)
    add("shape/key-repeated", reg(enc(G.Map([fmt_, fmt_, ad_]))), G.CBOR)
    add("shape/statement-key-repeated", reg(enc(G.Map([fmt_, stmt_, stmt_]))), G.CBOR)
    add("shape/fmt-a-byte-string", reg(enc(G.Map([(T(b"fmt"), b"none"), stmt_, ad_]))), G.CBOR)
    add("shape/fmt-an-integer", reg(enc(G.Map([(T(b"fmt"), 0), stmt_, ad_]))), G.CBOR)
    add("shape/statement-an-array", reg(enc(G.Map([fmt_, (T(b"attStmt"), []), ad_]))), G.CBOR)
    add("shape/authdata-a-text-string", reg(enc(G.Map([fmt_, stmt_, (T(b"authData"), T(good_ad))]))), G.CBOR)
    add("shape/top-an-array", reg(enc([T(b"fmt"), T(b"none"), T(b"attStmt"), G.Map([]), T(b"authData"), good_ad])), G.CBOR)
    add("shape/key-in-another-case", reg(enc(G.Map([fmt_, (T(b"attstmt"), G.Map([])), ad_]))), G.CBOR)

    # ---- stmt/
    def both(name, stmt, at_policy_1=G.ATTESTATION, fmt=T(b"packed"), at_policy_0=G.VALID):
        for policy, tag in BOTH:
            add("stmt/%s/%s" % (name, tag), reg(att_obj(fmt=fmt, stmt=stmt), policy=policy), at_policy_0 if policy == G.ATT_IGNORE else at_policy_1)

    both("every-major-type-and-a-tag", G.Map([(T(b"a"), 1), (T(b"b"), -1), (T(b"c"), b"xy"), (T(b"d"), T(b"z")), (T(b"e"), [1, [2]]),
                                              (T(b"f"), G.Map([(1, 2)])), (T(b"g"), G.Tag(1, 1363896240)), (T(b"h"), G.TRUE), (-1, G.Tag(2**32, [b""]))]))
    both("floats", G.Map([(T(b"half"), Raw(bytes.fromhex("f93c00"))), (T(b"single"), Raw(bytes.fromhex("fa47c35000"))),
                          (T(b"double"), Raw(bytes.fromhex("fb3ff199999999999a"))), (T(b"nan"), Raw(bytes.fromhex("f97e00"))),
                          (T(b"zero"), Raw(bytes.fromhex("fb0000000000000000")))]))
    both("false-true-null-undefined", G.Map([(1, G.FALSE), (2, G.TRUE), (3, G.NULL), (4, G.UNDEFINED), (5, G.Simple(0)), (6, G.Simple(19))]))
    both("simple-in-one-byte=32", G.Map([(1, Raw(b"\xf8\x20")), (2, G.Simple(255))]))
    both("simple-in-one-byte=31", G.Map([(1, Raw(b"\xf8\x1f"))]), G.CBOR, at_policy_0=G.CBOR)
    both("simple-in-one-byte=0", G.Map([(1, Raw(b"\xf8\x00"))]), G.CBOR, at_policy_0=G.CBOR)
    for depth in (1, 2, 200):
        both("arrays-nested-%d-deep" % depth, G.Map([(T(b"v"), Raw(b"\x81" * depth + b"\x00"))]))
    both("maps-nested-200-deep", G.Map([(T(b"v"), Raw(b"\xa1\x00" * 200 + b"\x00"))]))
    both("tags-nested-200-deep", G.Map([(T(b"v"), Raw(b"\xc1" * 200 + b"\x00"))]))
    big = [bytes((i * (j + 2) + j) & 0xFF for i in range(700)) for j in range(3)]
    both("x5c-of-three-700-byte-strings", G.Map(self_stmt(good_ad, good_cd).pairs + [(T(b"x5c"), big)]))
    both("none-with-a-member", G.Map([(T(b"x"), 0)]), fmt=T(b"none"))
    sp = self_stmt(good_ad, good_cd).pairs
    both("packed-sig-before-alg", G.Map([sp[1], sp[0]]))
    both("packed-alg=-257", G.Map([(T(b"alg"), -257), sp[1]]))
    both("packed-alg=-8", G.Map([(T(b"alg"), -8), sp[1]]))
    both("packed-third-member", G.Map(sp + [(T(b"x"), 0)]))
    both("packed-sig-a-text-string", G.Map([sp[0], (T(b"sig"), T(sp[1][1]))]))
    both("packed-empty", G.Map([]))
    both("packed-only-alg", G.Map([sp[0]]))
    both("fmt-Packed", G.Map(sp), fmt=T(b"Packed"))
    both("fmt-empty", G.Map([]), fmt=T(b""))
    both("fmt-none-then-a-byte", G.Map([]), fmt=T(b"none "))

    # ---- cred/
    add("cred/at-clear", reg(att_obj(auth_data(flags=G.UP))), G.CREDENTIAL)
    add("cred/at-clear-and-37-bytes", reg(att_obj(auth_data(flags=G.UP)[:37])), G.CREDENTIAL)
    add("cred/37-bytes-with-at-set", reg(att_obj(good_ad[:37])), G.CREDENTIAL)
    add("cred/cut-inside-aaguid", reg(att_obj(good_ad[:45])), G.CREDENTIAL)
    add("cred/cut-before-the-length", reg(att_obj(good_ad[:53])), G.CREDENTIAL)
    add("cred/cut-inside-the-length", reg(att_obj(good_ad[:54])), G.CREDENTIAL)
    add("cred/cut-before-the-id", reg(att_obj(good_ad[:55])), G.CREDENTIAL)
    add("cred/cut-inside-the-id", reg(att_obj(good_ad[:60])), G.CREDENTIAL)
    add("cred/cut-before-the-key", reg(att_obj(good_ad[:71])), G.CREDENTIAL)
    add("cred/cut-inside-the-key-head", reg(att_obj(good_ad[:71 + 9])), G.CREDENTIAL)
    add("cred/cut-inside-x", reg(att_obj(good_ad[:71 + 20])), G.CREDENTIAL)
    add("cred/cut-one-byte-before-the-end", reg(att_obj(good_ad[:-1])), G.CREDENTIAL)
    add("cred/id-length=0", reg(att_obj(auth_data(id_len=0))), G.CREDENTIAL)
    add("cred/id-length=1024", reg(att_obj(auth_data(id_len=1024))), G.CREDENTIAL)
    add("cred/id-length=ffff", reg(att_obj(auth_data(id_len=16, id_len_field=0xFFFF))), G.CREDENTIAL)
    add("cred/id-length-one-more-than-there-is", reg(att_obj(auth_data(id_len=16, id_len_field=16 + 77 + 1))), G.CREDENTIAL)
    ed = G.UP | G.AT | G.ED
    add("cred/ed-set-nothing-after-the-key", reg(att_obj(auth_data(flags=ed))), G.CREDENTIAL)
    add("cred/ed-clear-one-byte-after", reg(att_obj(auth_data(ext=b"\x00"))), G.CREDENTIAL)
    add("cred/ed-clear-a-map-after", reg(att_obj(auth_data(ext=b"\xa0"))), G.CREDENTIAL)
    prot = enc(G.Map([(T(b"credProtect"), 2)]))
    add("cred/ed-set-credProtect", reg(att_obj(auth_data(flags=ed, ext=prot)), policy=G.ATT_NONE_OR_SELF), G.VALID)
    add("cred/ed-set-credProtect-self-attested", packed_self(auth_data(flags=ed, ext=prot), policy=G.ATT_NONE_OR_SELF), (G.VALID, G.ATTESTED_SELF))
    add("cred/ed-set-empty-map", reg(att_obj(auth_data(flags=ed, ext=b"\xa0"))), G.VALID)
    add("cred/ed-set-an-array", reg(att_obj(auth_data(flags=ed, ext=enc([T(b"credProtect"), 2])))), G.CREDENTIAL)
    add("cred/ed-set-an-integer", reg(att_obj(auth_data(flags=ed, ext=b"\x00"))), G.CREDENTIAL)
    add("cred/ed-set-malformed-map", reg(att_obj(auth_data(flags=ed, ext=prot[:-1]))), G.CREDENTIAL)
    add("cred/ed-set-indefinite-map", reg(att_obj(auth_data(flags=ed, ext=b"\xbf" + prot[1:] + b"\xff"))), G.CREDENTIAL)
    add("cred/ed-set-longer-form-map", reg(att_obj(auth_data(flags=ed, ext=head(5, 1, 1) + prot[1:]))), G.CREDENTIAL)
    add("cred/ed-set-a-byte-after-the-map", reg(att_obj(auth_data(flags=ed, ext=prot + b"\x00"))), G.CREDENTIAL)
    add("cred/ed-set-two-maps", reg(att_obj(auth_data(flags=ed, ext=prot + prot))), G.CREDENTIAL)
    blob = bytes(range(40))
    add("cred/ed-set-string-of-the-bytes-left", reg(att_obj(auth_data(flags=ed, ext=head(5, 1) + enc(0) + head(2, 40) + blob))), G.VALID)
    add("cred/ed-set-string-of-the-bytes-left+1", reg(att_obj(auth_data(flags=ed, ext=head(5, 1) + enc(0) + head(2, 41) + blob))), G.CREDENTIAL)
    add("cred/ed-set-pairs=bytes-left+1", reg(att_obj(auth_data(flags=ed, ext=head(5, 5) + bytes(4)))), G.CREDENTIAL)
    add("cred/key-an-integer", reg(att_obj(auth_data(key=b"\x00"))), G.COSE_KEY)  # (one well-formed item that ends authData: not the key)

    # ---- cose/
    for at, byte, want in COSE_CHANGES:
        assert key[at] != byte
        add("cose/template-byte-%d=%02x" % (at, byte), reg(att_obj(auth_data(key=key[:at] + bytes([byte]) + key[at + 1:]))), want)
    xb, yb = Q[0].to_bytes(32, "big"), Q[1].to_bytes(32, "big")
    add("cose/another-member-order", reg(att_obj(auth_data(key=cose_key(Q, [(3, -7), (1, 2), (-1, 1), (-2, xb), (-3, yb)])))), G.COSE_KEY)
    add("cose/y-before-x", reg(att_obj(auth_data(key=cose_key(Q, [(1, 2), (3, -7), (-1, 1), (-3, yb), (-2, xb)])))), G.COSE_KEY)
    add("cose/six-members", reg(att_obj(auth_data(key=cose_key(Q, [(1, 2), (3, -7), (-1, 1), (-2, xb), (-3, yb), (-4, b"")])))), G.COSE_KEY)
    add("cose/six-members-key-ops-first", reg(att_obj(auth_data(key=cose_key(Q, [(1, 2), (3, -7), (4, [2]), (-1, 1), (-2, xb), (-3, yb)])))), G.COSE_KEY)
    add("cose/four-members", reg(att_obj(auth_data(key=cose_key(Q, [(1, 2), (3, -7), (-1, 1), (-2, xb)])))), G.COSE_KEY)
    add("cose/x-of-31-bytes", reg(att_obj(auth_data(key=cose_key(Q, [(1, 2), (3, -7), (-1, 1), (-2, xb[1:]), (-3, yb)])))), G.COSE_KEY)
    add("cose/x-of-33-bytes", reg(att_obj(auth_data(key=cose_key(Q, [(1, 2), (3, -7), (-1, 1), (-2, b"\x00" + xb), (-3, yb)])))), G.COSE_KEY)
    add("cose/y-of-31-bytes-x-of-33", reg(att_obj(auth_data(key=cose_key(Q, [(1, 2), (3, -7), (-1, 1), (-2, b"\x00" + xb), (-3, yb[1:])])))), G.COSE_KEY)
    add("cose/okp", reg(att_obj(auth_data(key=cose_key(Q, [(1, 1), (3, -8), (-1, 6), (-2, xb)])))), G.COSE_KEY)
    add("cose/rs256", reg(att_obj(auth_data(key=cose_key(Q, [(1, 3), (3, -257), (-1, bytes(256)), (-2, b"\x01\x00\x01")])))), G.COSE_KEY)
    add("cose/an-array", reg(att_obj(auth_data(key=enc([1, 2, 3, -7, -1, 1, -2, xb, -3, yb])))), G.COSE_KEY)
    add("cose/key-off-the-curve", reg(att_obj(auth_data(key=cose_key((Q[0], (Q[1] + 1) % R.P))))), G.OFF_CURVE)
    add("cose/key=(0,0)", reg(att_obj(auth_data(key=cose_key((0, 0))))), G.OFF_CURVE)
    add("cose/x=p", reg(att_obj(auth_data(key=cose_key((R.P, Q[1]))))), G.RANGE)
    add("cose/y=p", reg(att_obj(auth_data(key=cose_key((Q[0], R.P))))), G.RANGE)
    add("cose/x=2^256-1", reg(att_obj(auth_data(key=cose_key((2**256 - 1, Q[1]))))), G.RANGE)
    add("cose/y-negated", reg(att_obj(auth_data(key=cose_key((Q[0], R.P - Q[1]))))), G.VALID)

    # ---- cd/
    add("cd/type=webauthn.get", reg(cd=client_data(typ=b"webauthn.get")), G.CLIENTDATA)
    add("cd/wrong-challenge", reg(cd=client_data(challenge=CHALLENGE[::-1])), G.CLIENTDATA)
    add("cd/challenge-one-byte-short", reg(cd=client_data(challenge=CHALLENGE[:-1])), G.CLIENTDATA)
    add("cd/wrong-origin", reg(cd=client_data(origin="https://b.example")), G.CLIENTDATA)
    add("cd/origin-closing-quote", reg(cd=client_data(origin="https://a.example.evil")), G.CLIENTDATA)
    add("cd/true-without-the-policy", reg(cd=client_data(cross=b"true")), G.CLIENTDATA)
    add("cd/true-with-the-policy", reg(cd=client_data(cross=b"true"), allow_cross_origin=True), G.VALID)
    add("cd/false-with-the-policy", reg(allow_cross_origin=True), G.VALID)
    add("cd/empty", reg(cd=b""), G.CLIENTDATA)
    add("cd/equal-to-E", reg(cd=G.expected_prefix(CHALLENGE, ORIGIN)), G.CLIENTDATA)
    add("cd/last-byte-not-a-brace", reg(cd=good_cd + b" "), G.CLIENTDATA)
    add("cd/with-a-member", reg(cd=client_data(length=200)), G.VALID)

    # ---- self/
    one = G.ATT_NONE_OR_SELF
    r, s = A.sign(W.msghash(good_ad, good_cd), KS[0], D)
    assert W.der_encode(r, s) == sp[1][1]

    def with_sig(sig, ad=good_ad, policy=one):
        return reg(att_obj(ad, T(b"packed"), G.Map([(T(b"alg"), -7), (T(b"sig"), sig)])), policy=policy)

    add("self/s+1", with_sig(W.der_encode(r, s + 1)), G.MISMATCH)
    add("self/s+1/policy=0", with_sig(W.der_encode(r, s + 1), policy=G.ATT_IGNORE), (G.VALID, G.ATTESTED_NOT_JUDGED))
    add("self/signed-by-another-key", reg(att_obj(good_ad, T(b"packed"), self_stmt(good_ad, good_cd, d=D + 1)), policy=one), G.MISMATCH)
    add("self/counter-changed-after-signing", with_sig(sp[1][1], ad=auth_data(counter=8)), G.MISMATCH)
    add("self/client-data-changed-after-signing", reg(att_obj(good_ad, T(b"packed"), G.Map(sp)), cd=client_data(length=150), policy=one), G.MISMATCH)
    add("self/r=0", with_sig(W.der_encode(0, s)), G.RANGE)
    add("self/s=n", with_sig(W.der_encode(r, R.N)), G.RANGE)
    rb, sb = (v.to_bytes(32, "big") if v >> 255 == 0 else b"\x00" + v.to_bytes(32, "big") for v in (r, s))
    small = bytes([0x12]) + bytes(range(30))

    def raw(rb, sb, tail=b""):
        body = bytes([0x02, len(rb)]) + rb + bytes([0x02, len(sb)]) + sb
        return bytes([0x30, len(body)]) + body + tail

    assert raw(rb, sb) == sp[1][1]
    add("self/der-non-minimal-00-on-r", with_sig(raw(b"\x00" + small, sb)), G.SIGNATURE_DER)
    add("self/der-negative-s", with_sig(raw(rb, b"\xff" + small)), G.SIGNATURE_DER)
    add("self/der-byte-after-s", with_sig(raw(rb, sb, tail=b"\x00")), G.SIGNATURE_DER)
    add("self/der-long-form-sequence", with_sig(bytes([0x30, 0x81, len(raw(small, small)) - 2]) + raw(small, small)[2:]), G.SIGNATURE_DER)
    add("self/sig-of-7-bytes", with_sig(bytes.fromhex("30050201010201")), G.SIGNATURE_DER)
    add("self/sig-of-73-bytes", with_sig(raw(b"\x00" + bytes([0x80]) + bytes(31), b"\x00" + bytes([0x80]) + bytes(31)) + b"\x00"), G.SIGNATURE_DER)
    add("self/sig-empty", with_sig(b""), G.SIGNATURE_DER)
    add("self/der-defect/policy=0", with_sig(raw(rb, sb, tail=b"\x00"), policy=G.ATT_IGNORE), G.VALID)
    for m, id_len, cd_len, k in zip(HASH_RESIDUES, HASH_ID_LENGTHS, HASH_CD_LENGTHS, KS):
        ad = auth_data(id_len=id_len, counter=m)
        assert (len(ad) + 32) % 64 == m and cd_len % 64 == m
        add("self/hashed-lengths-mod-64=%d" % m, packed_self(ad, client_data(length=cd_len), k=k, policy=one), (G.VALID, G.ATTESTED_SELF))

    # ---- cap/
    def obj_of_length(n):
        """fmt "packed" with {"x5c": [<filler>]} sized so that the object has n bytes."""
        for fill in range(n - 400, n):
            obj = att_obj(fmt=T(b"packed"), stmt=G.Map([(T(b"x5c"), [bytes(0x5A for _ in range(fill))])]))
            if len(obj) == n:
                return obj
        raise AssertionError(n)

    add("cap/object=8192", reg(obj_of_length(8192)), G.VALID)
    add("cap/object=8193", reg(obj_of_length(8193)), G.SIZE)
    add("cap/object=0", reg(b""), G.SIZE)
    add("cap/object=1", reg(b"\xa3"), G.CBOR)
    def self_attested_of_length(n):
        """A self-attested registration whose object has n bytes: an extension string sized for it (a DER signature has 70 .. 72
        bytes, so the filler is searched, and signed again at every step)."""
        for k in KS:
            for fill in range(n - 330, n - 200):
                ad = auth_data(flags=ed, ext=head(5, 1) + enc(0) + enc(bytes((3 * i) & 0xFF for i in range(fill))))
                g = packed_self(ad, client_data(length=4096), k=k, policy=one)
                if len(g.attestation_object) == n:
                    return g
        raise AssertionError(n)

    add("cap/object=8192-self-attested", self_attested_of_length(8192), (G.VALID, G.ATTESTED_SELF))
    add("cap/object=8193-self-attested", self_attested_of_length(8193), G.SIZE)
    add("cap/clientdata=4096", packed_self(cd=client_data(length=4096), policy=one), G.VALID)
    add("cap/clientdata=4097", packed_self(cd=client_data(length=4097), policy=one), G.SIZE)
    ch64, ch65 = bytes(range(100, 164)), bytes(range(100, 165))
    add("cap/challenge=64", reg(challenge=ch64), G.VALID)
    add("cap/challenge=65", reg(challenge=ch65), G.SIZE)
    add("cap/challenge=0", reg(challenge=b""), G.SIZE)
    add("cap/challenge=1", reg(challenge=b"\xfb"), G.VALID)
    o255 = "https://" + "b" * (255 - 8 - 8) + ".example"
    add("cap/origin=255", reg(origin=o255), G.VALID)
    add("cap/origin=256", reg(origin="c" + o255), G.SIZE)
    add("cap/origin=0", reg(origin=""), G.VALID)
    add("cap/everything-at-its-cap", reg(obj_of_length(8192), client_data(ch64, o255, 4096), challenge=ch64, origin=o255), G.VALID)

    # ---- order/: two defects each, the earlier test's reason wins
    wrong_rp = bytes([RP_HASH[0] ^ 1]) + RP_HASH[1:]
    bad_key = key[:4] + b"\x27" + key[5:]
    off_key = cose_key((Q[0], (Q[1] + 1) % R.P))
    add("order/size-before-cbor", reg(whole[:5], cd=client_data(length=4097)), G.SIZE)
    add("order/cbor-before-authdata", reg(att_obj(good_ad[:36], stmt=Raw(b"\xa1\x00\xff"))), G.CBOR)
    add("order/authdata-before-rpid", reg(att_obj(good_ad[:36]), rp_hash=wrong_rp), G.AUTHDATA)
    add("order/rpid-before-flags", reg(att_obj(auth_data(flags=G.AT)), rp_hash=wrong_rp), G.RPID)
    add("order/flags-before-credential", reg(att_obj(auth_data(flags=0))), G.FLAGS)
    add("order/credential-before-cose", reg(att_obj(auth_data(key=bad_key, ext=b"\x00"))), G.CREDENTIAL)
    add("order/cose-before-clientdata", reg(att_obj(auth_data(key=bad_key)), cd=b"{}"), G.COSE_KEY)
    add("order/clientdata-before-range", reg(att_obj(auth_data(key=cose_key((R.P, Q[1])))), cd=b"{}"), G.CLIENTDATA)
    add("order/range-before-off-curve", reg(att_obj(auth_data(key=cose_key((R.P, 5))))), G.RANGE)
    add("order/off-curve-before-attestation", reg(att_obj(auth_data(key=off_key), T(b"tpm")), policy=one), G.OFF_CURVE)
    add("order/attestation-before-der", reg(att_obj(good_ad, T(b"packed"), G.Map([(T(b"sig"), b"\xff" * 8), (T(b"alg"), -7)])), policy=one), G.ATTESTATION)
    other_sig = self_stmt(good_ad, good_cd, d=D + 1).pairs[1][1]
    add("order/der-before-mismatch", with_sig(other_sig + b"\x00"), G.SIGNATURE_DER)

    # ---- pad/: fillers; the start of a request's messages in the packed blob moves by the lengths before it
    for i in range(8):
        add("pad/%d" % i, packed_self(auth_data(id_len=30 + i, counter=i), client_data(length=140 + (3 * i) % 4), k=KS[i], policy=one), G.VALID)

    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    cs = CaseSet(names, [c[1] for c in cases], [c[2] for c in cases])
    assert_alignment_coverage(cs)
    return cs


def packing(regs):
    """Where zk_webauthn_register puts the messages of the requests it uploads (csrc/webauthn_register.hip): the requests inside the
    caps, in order, each as attestationObject, clientDataJSON, E back to back in one blob that starts on a word boundary.
    -> [(index, offset of the object, offset of clientDataJSON)]"""
    out, pos = [], 0
    for i, g in enumerate(regs):
        if G.check(g)[0] == G.SIZE:
            continue
        out.append((i, pos, pos + len(g.attestation_object)))
        pos += len(g.attestation_object) + len(g.client_data_json) + len(G.expected_prefix(g.challenge, g.origin))
    return out


def alignment_coverage(cs):
    """(residues mod 4 at which the object of a self-attested accepted request starts - the ones that hash -, the same for its
    clientDataJSON, the same for its authData)."""
    obj, cd, ad = set(), set(), set()
    for i, o_off, c_off in packing(cs.regs):
        if cs.reasons[i] == G.VALID and cs.creds[i]["attestation"] == G.ATTESTED_SELF:
            obj.add(o_off % 4)
            cd.add(c_off % 4)
            ad.add((o_off + cs.creds[i]["auth_data_off"]) % 4)
    return obj, cd, ad


def assert_alignment_coverage(cs):
    obj, cd, ad = alignment_coverage(cs)
    assert obj == {0, 1, 2, 3} and cd == {0, 1, 2, 3} and ad == {0, 1, 2, 3}, (obj, cd, ad)


MAGIC_IN, MAGIC_OUT = 0x57415231, 0x5741524F  # "WAR1", "WARO"
OUT_BYTES = 1 + 104


def write_case_file(path, cs):
    """The set as tests/webauthn_register_host_check.cpp reads it, everything back to back (so nothing is aligned): MAGIC_IN, the
    count; per registration four u32 lengths (attestationObject, clientDataJSON, challenge, origin), rpIdHash, flags_required,
    allow_cross_origin, policy, then the four byte strings.  All integers little-endian."""
    out = [struct.pack("<II", MAGIC_IN, len(cs))]
    for g in cs.regs:
        origin = g.origin.encode()
        out.append(struct.pack("<IIII", len(g.attestation_object), len(g.client_data_json), len(g.challenge), len(origin)))
        out.append(g.rp_id_hash + bytes([g.flags_required, int(g.allow_cross_origin), g.policy]))
        out.append(g.attestation_object + g.client_data_json + g.challenge + origin)
    with open(path, "wb") as f:
        f.write(b"".join(out))
