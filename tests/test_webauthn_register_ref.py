"""The WebAuthn registration check without a GPU: the reference's CBOR reader (tests/webauthn_register_ref.py) anchored by the
examples of RFC 8949 Appendix A, typed in by value; the coverage the registration set (tests/webauthn_register_cases.py) must
have, by name and by reason; the package's own host route (ecdsa_p256.webauthn_register) against the reference on every case; the
public names of the feature; webauthn_expected_prefix for webauthn.get unchanged; and csrc/webauthn_register.hip.h's portable form
on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer.

The last part builds tests/webauthn_register_host_check.cpp - a stand-alone program with its own main, nothing of the library in
it, no GPU touched, nothing loaded into Python - with hipcc and runs it as a child process: webauthn_register_check_one over the
whole set, reason and every field of the credential equal to the reference, and every case a second time with each byte string in
an allocation of exactly its length.  The sanitizers report nothing (either would end the program with a non-zero status).
Skipped without hipcc.
"""
import math
import os
import re
import shutil
import struct
import subprocess

import pytest

import webauthn_ref as W
import webauthn_register_cases as C
import webauthn_register_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = G.Text


@pytest.fixture(scope="module")
def cs():
    return C.build()


def test_cbor_reader_anchors():
    """RFC 8949 Appendix A: (value, encoding in hex)."""
    examples = [
        (0, "00"), (1, "01"), (10, "0a"), (23, "17"), (24, "1818"), (25, "1819"), (100, "1864"), (1000, "1903e8"), (1000000, "1a000f4240"),
        (1000000000000, "1b000000e8d4a51000"), (18446744073709551615, "1bffffffffffffffff"), (-18446744073709551616, "3bffffffffffffffff"),
        (-1, "20"), (-10, "29"), (-100, "3863"), (-1000, "3903e7"),
        (0.0, "f90000"), (1.0, "f93c00"), (1.5, "f93e00"), (65504.0, "f97bff"), (100000.0, "fa47c35000"), (3.4028234663852886e+38, "fa7f7fffff"),
        (1.1, "fb3ff199999999999a"), (1.0e+300, "fb7e37e43c8800759c"), (5.960464477539063e-8, "f90001"), (0.00006103515625, "f90400"),
        (-4.0, "f9c400"), (-4.1, "fbc010666666666666"), (math.inf, "f97c00"), (-math.inf, "f9fc00"), (math.inf, "fa7f800000"),
        (-math.inf, "fbfff0000000000000"),
        (G.FALSE, "f4"), (G.TRUE, "f5"), (G.NULL, "f6"), (G.UNDEFINED, "f7"), (G.Simple(16), "f0"), (G.Simple(255), "f8ff"),
        (G.Tag(0, T(b"2013-03-21T20:04:00Z")), "c074323031332d30332d32315432303a30343a30305a"), (G.Tag(1, 1363896240), "c11a514b67b0"),
        (G.Tag(1, 1363896240.5), "c1fb41d452d9ec200000"), (G.Tag(23, bytes.fromhex("01020304")), "d74401020304"),
        (G.Tag(24, bytes.fromhex("6449455446")), "d818456449455446"), (G.Tag(32, T(b"http://www.example.com")), "d82076687474703a2f2f7777772e6578616d706c652e636f6d"),
        (b"", "40"), (bytes.fromhex("01020304"), "4401020304"), (T(b""), "60"), (T(b"a"), "6161"), (T(b"IETF"), "6449455446"), (T(b"\"\\"), "62225c"),
        (T("ü".encode()), "62c3bc"), (T("水".encode()), "63e6b0b4"),
        ([], "80"), ([1, 2, 3], "83010203"), ([1, [2, 3], [4, 5]], "8301820203820405"),
        (list(range(1, 26)), "98190102030405060708090a0b0c0d0e0f101112131415161718181819"),
        (G.Map([]), "a0"), (G.Map([(1, 2), (3, 4)]), "a201020304"), (G.Map([(T(b"a"), 1), (T(b"b"), [2, 3])]), "a26161016162820203"),
        ([T(b"a"), G.Map([(T(b"b"), T(b"c"))])], "826161a161626163"),
        (G.Map([(T(c.encode()), T(c.upper().encode())) for c in "abcde"]), "a56161614161626142616361436164614461656145"),
    ]
    for value, hexed in examples:
        raw = bytes.fromhex(hexed)
        got, end = G.read_item(raw)
        assert end == len(raw) and got == value and type(got) is type(value), hexed
        assert G.read_item(b"\x00" + raw + b"\xff", 1) == (value, 1 + len(raw))  # at a position, with neighbours
        if not isinstance(value, float) and not (isinstance(value, G.Tag) and isinstance(value.item, float)):
            assert C.enc(value) == raw, hexed  # the set's encoder is canonical (it has no floats)
    nan = G.read_item(bytes.fromhex("f97e00"))[0]
    assert nan != nan and math.isnan(G.read_item(bytes.fromhex("fa7fc00000"))[0]) and math.isnan(G.read_item(bytes.fromhex("fb7ff8000000000000"))[0])
    # Appendix A's indefinite-length examples are well-formed CBOR and refused here, like the `break` alone
    for hexed in ("5f42010243030405ff", "7f657374726561646d696e67ff", "9fff", "9f018202039f0405ffff", "83018202039f0405ff", "bf61610161629f0203ffff",
                  "826161bf61626163ff", "bf6346756ef563416d7421ff", "ff"):
        with pytest.raises(G.Malformed):
            G.read_item(bytes.fromhex(hexed))
    # the strict rule's own refusals: longer heads, reserved additional information, a small simple value in two bytes, a cut, a count
    # above the bytes left
    for hexed in ("1817", "1900ff", "1a0000ffff", "1b00000000ffffffff", "5817" + "00" * 23, "7803616263", "9801" "00", "b80000", "d80100", "f818",
                  "f81f", "1c", "1d", "1e", "5c", "fc", "fd", "fe", "18", "19ff", "4161"[:2], "6261", "8201", "a10102"[:4], "c1", "",
                  "5b" + "ff" * 8, "9b" + "ff" * 8, "bb" + "80" + "00" * 7, "4400010203"[:8], "8500000000"[:8], "a3" + "00" * 5):
        with pytest.raises(G.Malformed):
            G.read_item(bytes.fromhex(hexed))
    assert G.read_item(bytes.fromhex("f820")) == (G.Simple(32), 2) and G.read_item(bytes.fromhex("1818")) == (24, 2)
    assert G.read_item(bytes.fromhex("190100")) == (256, 3) and G.read_item(bytes.fromhex("1a00010000")) == (65536, 5)
    assert G.read_item(bytes.fromhex("1b0000000100000000")) == (2**32, 9)
    assert G.read_item(b"\x81" * 200 + b"\x00")[1] == 201  # nesting costs heads, nothing else
    # a repeated key is two pairs
    assert G.read_item(bytes.fromhex("a2" "0102" "0103"))[0].pairs == [(1, 2), (1, 3)]


def test_reference_shares_the_assertion_rules():
    assert list(range(10)) == [G.VALID, G.RANGE, G.OFF_CURVE, G.MISMATCH, G.SIZE, G.AUTHDATA, G.RPID, G.FLAGS, G.CLIENTDATA, G.SIGNATURE_DER]
    assert (G.CBOR, G.CREDENTIAL, G.COSE_KEY, G.ATTESTATION) == (10, 11, 12, 13)
    assert G.expected_prefix(b"foob", "https://a.example") == b'{"type":"webauthn.create","challenge":"Zm9vYg","origin":"https://a.example","crossOrigin":'
    assert W.expected_prefix(b"foob", "https://a.example") == b'{"type":"webauthn.get","challenge":"Zm9vYg","origin":"https://a.example","crossOrigin":'
    e = G.expected_prefix(b"foob", "o")
    assert G.client_data_ok(e + b"false}", b"foob", "o", False) and not G.client_data_ok(e + b"true}", b"foob", "o", False)
    assert G.client_data_ok(e + b'true,"x":1}', b"foob", "o", True) and not G.client_data_ok(W.expected_prefix(b"foob", "o") + b"false}", b"foob", "o", False)


def test_the_set_covers_what_it_must(cs):
    assert len(cs) >= 250 and len(set(cs.names)) == len(cs)
    assert set(cs.reasons) == set(range(14))
    C.assert_alignment_coverage(cs)
    att = lambda name: cs.creds[cs.index(name)]["attestation"]
    want = {
        "valid/none/policy=0": G.VALID, "valid/none/policy=1": G.VALID, "valid/packed-self/policy=0": G.VALID, "valid/packed-self/policy=1": G.VALID,
        "valid/x5c/policy=0": G.VALID, "valid/tpm/policy=0": G.VALID, "valid/apple/policy=0": G.VALID, "valid/fido-u2f/policy=0": G.VALID,
        "valid/x5c/policy=1": G.ATTESTATION, "valid/tpm/policy=1": G.ATTESTATION, "valid/apple/policy=1": G.ATTESTATION,
        "valid/fido-u2f/policy=1": G.ATTESTATION, "valid/uv-required-and-set": G.VALID, "valid/counter=0": G.VALID, "valid/counter=80000000": G.VALID,
        "valid/counter=ffffffff": G.VALID,
        "ad/36-bytes": G.AUTHDATA, "ad/rpid-sent-wrong-in-byte-0": G.RPID, "ad/rpid-sent-wrong-in-byte-31": G.RPID, "ad/up-clear": G.FLAGS,
        "ad/uv-required-and-clear": G.FLAGS,
        "head/authdata=255": G.VALID, "head/authdata=256": G.VALID, "head/longer-form/58-17": G.CBOR, "head/longer-form/authdata-59-00-xx": G.CBOR,
        "head/longer-form/authdata-5a": G.CBOR, "head/longer-form/authdata-5b": G.CBOR, "head/shortest/58-18": G.VALID,
        "head/shortest/authdata-58": G.VALID, "head/ai=28/major=0": G.CBOR, "head/ai=29/major=2": G.CBOR, "head/ai=30/major=7": G.CBOR,
        "head/indefinite/5f": G.CBOR, "head/indefinite/7f": G.CBOR, "head/indefinite/9f": G.CBOR, "head/indefinite/bf": G.CBOR, "head/lone-ff": G.CBOR,
        "head/length=2^64-1": G.CBOR, "head/8-byte-length=bytes-left+1": G.CBOR, "head/length=bytes-left+1": G.CBOR,
        "head/map-count=bytes-left+1": G.CBOR, "head/one-byte-after-the-end": G.CBOR,
        "shape/two-entries": G.CBOR, "shape/four-entries": G.CBOR, "shape/authdata-before-the-statement": G.CBOR, "shape/fmt-key-a-byte-string": G.CBOR,
        "shape/key-repeated": G.CBOR, "shape/fmt-a-byte-string": G.CBOR, "shape/statement-an-array": G.CBOR, "shape/authdata-a-text-string": G.CBOR,
        "cred/at-clear": G.CREDENTIAL, "cred/37-bytes-with-at-set": G.CREDENTIAL, "cred/cut-inside-aaguid": G.CREDENTIAL,
        "cred/cut-inside-the-length": G.CREDENTIAL, "cred/cut-inside-the-id": G.CREDENTIAL, "cred/cut-inside-x": G.CREDENTIAL,
        "cred/id-length=0": G.CREDENTIAL, "cred/id-length=1024": G.CREDENTIAL, "cred/ed-set-nothing-after-the-key": G.CREDENTIAL,
        "cred/ed-clear-one-byte-after": G.CREDENTIAL, "cred/ed-set-credProtect": G.VALID, "cred/ed-set-an-array": G.CREDENTIAL,
        "cred/ed-set-malformed-map": G.CREDENTIAL, "cred/ed-set-a-byte-after-the-map": G.CREDENTIAL, "cred/ed-set-string-of-the-bytes-left": G.VALID,
        "cred/ed-set-string-of-the-bytes-left+1": G.CREDENTIAL,
        "cose/another-member-order": G.COSE_KEY, "cose/six-members": G.COSE_KEY, "cose/x-of-31-bytes": G.COSE_KEY, "cose/x-of-33-bytes": G.COSE_KEY,
        "cose/okp": G.COSE_KEY, "cose/key-off-the-curve": G.OFF_CURVE, "cose/x=p": G.RANGE,
        "cd/type=webauthn.get": G.CLIENTDATA, "cd/wrong-challenge": G.CLIENTDATA, "cd/wrong-origin": G.CLIENTDATA,
        "cd/true-without-the-policy": G.CLIENTDATA, "cd/true-with-the-policy": G.VALID,
        "self/s+1": G.MISMATCH, "self/signed-by-another-key": G.MISMATCH, "self/der-non-minimal-00-on-r": G.SIGNATURE_DER,
        "self/der-negative-s": G.SIGNATURE_DER, "self/der-byte-after-s": G.SIGNATURE_DER,
        "cap/object=8192": G.VALID, "cap/object=8193": G.SIZE, "cap/object=8192-self-attested": G.VALID, "cap/object=0": G.SIZE,
        "cap/clientdata=4096": G.VALID, "cap/clientdata=4097": G.SIZE, "cap/challenge=64": G.VALID, "cap/challenge=65": G.SIZE, "cap/challenge=0": G.SIZE,
        "cap/origin=255": G.VALID, "cap/origin=256": G.SIZE,
        "order/size-before-cbor": G.SIZE, "order/cbor-before-authdata": G.CBOR, "order/authdata-before-rpid": G.AUTHDATA,
        "order/rpid-before-flags": G.RPID, "order/flags-before-credential": G.FLAGS, "order/credential-before-cose": G.CREDENTIAL,
        "order/cose-before-clientdata": G.COSE_KEY, "order/clientdata-before-range": G.CLIENTDATA, "order/range-before-off-curve": G.RANGE,
        "order/off-curve-before-attestation": G.OFF_CURVE, "order/attestation-before-der": G.ATTESTATION, "order/der-before-mismatch": G.SIGNATURE_DER,
    }
    for n in list(range(1, 13)):
        want["head/cut-after-%d" % n] = G.CBOR
    for n in C.ID_LENGTHS:
        want["head/id=%d" % n] = G.VALID
    for at, byte, reason in C.COSE_CHANGES:
        want["cose/template-byte-%d=%02x" % (at, byte)] = reason
    assert sorted(c[0] for c in C.COSE_CHANGES) == list(range(10)) + [42, 43, 44]
    # each well-formed statement under both policies: accepted unjudged under 0, refused under 1; the malformed one CBOR under both
    for name in ("every-major-type-and-a-tag", "floats", "false-true-null-undefined", "simple-in-one-byte=32", "arrays-nested-1-deep",
                 "arrays-nested-2-deep", "arrays-nested-200-deep", "maps-nested-200-deep", "x5c-of-three-700-byte-strings", "none-with-a-member",
                 "packed-sig-before-alg", "packed-alg=-257", "packed-alg=-8", "packed-third-member", "packed-sig-a-text-string"):
        want["stmt/%s/policy=0" % name], want["stmt/%s/policy=1" % name] = G.VALID, G.ATTESTATION
    want["stmt/simple-in-one-byte=31/policy=0"] = want["stmt/simple-in-one-byte=31/policy=1"] = G.CBOR
    for m in C.HASH_RESIDUES:
        want["self/hashed-lengths-mod-64=%d" % m] = G.VALID
    for name, reason in want.items():
        assert cs.reasons[cs.index(name)] == reason, name
    # what an accepted registration says about its statement
    assert att("valid/none/policy=0") == att("valid/packed-self/policy=0") == att("valid/tpm/policy=0") == G.ATTESTED_NOT_JUDGED
    assert att("valid/none/policy=1") == G.ATTESTED_NONE and att("valid/packed-self/policy=1") == G.ATTESTED_SELF
    # the lengths the cases are named for
    for n, id_len in ((255, 123), (256, 124)):
        c = cs.creds[cs.index("head/authdata=%d" % n)]
        assert (c["auth_data_len"], c["credential_id_len"]) == (n, id_len)
    for n in C.ID_LENGTHS:
        assert cs.creds[cs.index("head/id=%d" % n)]["credential_id_len"] == n
    for m in C.HASH_RESIDUES:
        i = cs.index("self/hashed-lengths-mod-64=%d" % m)
        assert (cs.creds[i]["auth_data_len"] + 32) % 64 == m and len(cs.regs[i].client_data_json) % 64 == m
        assert cs.creds[i]["attestation"] == G.ATTESTED_SELF
    assert len(cs.regs[cs.index("cap/object=8192")].attestation_object) == 8192 == len(cs.regs[cs.index("cap/object=8192-self-attested")].attestation_object)
    assert len(cs.regs[cs.index("cap/object=8193")].attestation_object) == 8193
    for c, name in ((0, "valid/counter=0"), (0x80000000, "valid/counter=80000000"), (0xFFFFFFFF, "valid/counter=ffffffff")):
        assert cs.creds[cs.index(name)]["sign_count"] == c
    # the credential names bytes of the caller's object; a refused registration hands out nothing
    for g, reason, c in zip(cs.regs, cs.reasons, cs.creds):
        assert (c is None) == (reason != G.VALID)
        if c:
            o = g.attestation_object
            ad = o[c["auth_data_off"]:c["auth_data_off"] + c["auth_data_len"]]
            assert c["auth_data_off"] + c["auth_data_len"] == len(o) and ad[32] == c["flags"] and ad[37:53] == c["aaguid"]
            assert o[c["credential_id_off"]:c["credential_id_off"] + c["credential_id_len"]] == C.cred_id(c["credential_id_len"])


def test_the_host_route_agrees_with_the_reference(cs):
    from webauthn_halo2_amd import ecdsa_p256 as api

    for name, g, reason, want in zip(cs.names, cs.regs, cs.reasons, cs.creds):
        ok, got_reason, got = api.webauthn_register(g.attestation_object, g.client_data_json, g.challenge, g.origin, g.rp_id_hash, g.flags_required,
                                                    g.allow_cross_origin, g.policy)
        assert (ok, got_reason) == (reason == G.VALID, reason), name
        assert (got is None) == (want is None), name
        if want:
            assert {k: got[k] for k in want} == want, name
            o = g.attestation_object
            assert got["credential_id"] == o[want["credential_id_off"]:][:want["credential_id_len"]] and got["auth_data"] == o[want["auth_data_off"]:], name
    q = dict(attestation_object=cs.regs[0].attestation_object, client_data_json=cs.regs[0].client_data_json, challenge=C.CHALLENGE, origin=C.ORIGIN,
             rp_id_hash=C.RP_HASH)
    assert api.signature_check() == "host" and api.webauthn_register_check([q])[0][:2] == (True, G.VALID)
    with pytest.raises(ValueError):
        api.webauthn_register(q["attestation_object"], q["client_data_json"], C.CHALLENGE, C.ORIGIN, C.RP_HASH, attestation_policy=2)


def test_header_declares_the_entry_point_and_constants():
    txt = open(os.path.join(ROOT, "include", "zkmi355.h")).read()
    for name, value in (("CBOR", 10), ("CREDENTIAL", 11), ("COSE_KEY", 12), ("ATTESTATION", 13), ("ATTOBJ_MAX", 8192), ("ATT_IGNORE", 0),
                        ("ATT_NONE_OR_SELF", 1), ("ATTESTED_NONE", 0), ("ATTESTED_SELF", 1), ("ATTESTED_NOT_JUDGED", 2)):
        assert re.search(r"#define\s+ZK_WEBAUTHN_%s\s+%d\b" % (name, value), txt), name
    for i, name in enumerate(("VALID", "RANGE", "OFF_CURVE", "MISMATCH", "SIZE", "AUTHDATA", "RPID", "FLAGS", "CLIENTDATA", "SIGNATURE_DER")):
        assert re.search(r"#define\s+ZK_WEBAUTHN_%s\s+%d\b" % (name, i), txt), name  # 0 .. 9 keep their values
    assert re.search(r"int\s+zk_webauthn_register\s*\(\s*zk_ctx\s*\*\s*ctx\s*,\s*size_t\s+count\s*,\s*const\s+zk_webauthn_registration\s*\*\s*r", txt)
    assert "} zk_webauthn_registration;" in txt and "} zk_webauthn_credential;" in txt
    src = open(os.path.join(ROOT, "webauthn-halo2_amd", "csrc", "webauthn_register.hip")).read()
    assert "ZK_API(zk_webauthn_register" in src and "webauthn_register_kernel" in src
    assert "csrc/webauthn_register.hip" in open(os.path.join(ROOT, "build.sh")).read()


def test_python_names():
    import ctypes

    from webauthn_halo2_amd import ecdsa_p256 as api, engine as E, proving_server as srv

    assert (E.ZK_WEBAUTHN_CBOR, E.ZK_WEBAUTHN_CREDENTIAL, E.ZK_WEBAUTHN_COSE_KEY, E.ZK_WEBAUTHN_ATTESTATION) == (10, 11, 12, 13)
    assert (E.ZK_WEBAUTHN_ATTOBJ_MAX, E.ZK_WEBAUTHN_ATT_IGNORE, E.ZK_WEBAUTHN_ATT_NONE_OR_SELF) == (8192, 0, 1)
    assert (E.ZK_WEBAUTHN_ATTESTED_NONE, E.ZK_WEBAUTHN_ATTESTED_SELF, E.ZK_WEBAUTHN_ATTESTED_NOT_JUDGED) == (0, 1, 2)
    assert [api.WEBAUTHN_REASON_NAMES[i] for i in range(14)] == [G.REASON_NAMES[i] for i in range(14)]
    assert ctypes.sizeof(E.WebauthnCredentialC) == 104 and E.WebauthnCredentialC.attestation.offset == 101
    assert E.WebauthnRegistrationC.attestation_policy.offset == E.WebauthnRegistrationC.rp_id_hash.offset + 34
    assert callable(E.Engine.webauthn_register) and callable(api.webauthn_register) and callable(api.webauthn_register_many)
    assert callable(api.webauthn_register_check)
    assert callable(srv.parse_registration) and callable(srv.register_credential) and callable(srv.register_credentials_batch)
    assert api.signature_check() == "host"  # the default route stays the host


def test_expected_prefix_for_an_assertion_is_unchanged():
    from webauthn_halo2_amd import ecdsa_p256 as api

    for challenge, origin in ((b"foob", "https://a.example"), (bytes(range(64)), ""), (b"\xfb\xff", "o")):
        assert api.webauthn_expected_prefix(challenge, origin) == W.expected_prefix(challenge, origin)
        assert api.webauthn_expected_prefix(challenge, origin, b"webauthn.create") == G.expected_prefix(challenge, origin)
    assert api.webauthn_expected_prefix(b"foob", b"https://a.example") == b'{"type":"webauthn.get","challenge":"Zm9vYg","origin":"https://a.example","crossOrigin":'


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_portable_form_on_the_cpu_under_the_sanitizers(cs, tmp_path):
    exe = str(tmp_path / "webauthn_register_host_check")
    # the host side only (nothing runs on a device); -O1: the sanitizers' checks at every access, in seconds
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-x", "hip", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "webauthn-halo2_amd", "csrc"), os.path.join(ROOT, "tests", "webauthn_register_host_check.cpp"), "-o", exe])
    cases, results = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    C.write_case_file(cases, cs)
    r = subprocess.run([exe, cases, results], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), "webauthn_register_host_check failed (%d): %s%s" % (r.returncode, r.stdout, r.stderr)
    raw = open(results, "rb").read()
    assert struct.unpack_from("<II", raw) == (C.MAGIC_OUT, len(cs)) and len(raw) == 8 + len(cs) * C.OUT_BYTES
    bad = []
    for i in range(len(cs)):
        rec = raw[8 + i * C.OUT_BYTES:8 + (i + 1) * C.OUT_BYTES]
        if (rec[0], rec[1:]) != (cs.reasons[i], C.cred_bytes(cs.creds[i])):
            bad.append((cs.names[i], G.REASON_NAMES.get(rec[0], rec[0]), G.REASON_NAMES[cs.reasons[i]], rec[1:] == C.cred_bytes(cs.creds[i])))
    assert not bad, "webauthn_register_check_one differs from the reference on %d cases, first (name, reason got / want, credential equal): %s" % (
        len(bad), bad[:5])
