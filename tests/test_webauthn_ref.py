"""The WebAuthn assertion check without a GPU: the reference (tests/webauthn_ref.py) anchored by the FIPS 180-4 and RFC 4648
vectors and by es256_ref on the assembled records; the coverage the assertion set (tests/webauthn_cases.py) must have; the
package's own host route (ecdsa_p256.webauthn_verify) against the reference on every case; the public names of the feature; and
csrc/webauthn.hip.h's portable forms on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer.

The last part builds tests/webauthn_host_check.cpp - a stand-alone program with its own main, nothing of the library in it, no GPU
touched - with hipcc and runs it as a child process: webauthn_check_one over the whole set (reason, record and counter equal the
reference for every case) and sha256_two over messages of every length around the block edges, split at every kind of seam.  The
sanitizers report nothing (either would end the program with a non-zero status).  Skipped without hipcc.
"""
import hashlib
import os
import re
import shutil
import struct
import subprocess

import pytest

import es256_ref as R
import webauthn_cases as C
import webauthn_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cs():
    return C.build()


def test_reference_anchors():
    # FIPS 180-4 / NIST example vectors, through the one place the reference hashes two pieces
    empty = hashlib.sha256(b"").digest()
    assert empty.hex() == "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"
    assert hashlib.sha256(b"abc").hexdigest() == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"
    assert (hashlib.sha256(b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq").hexdigest()
            == "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1")
    assert W.msghash(b"abc", b"") == int.from_bytes(hashlib.sha256(b"abc" + empty).digest(), "big")
    assert [m[0] + m[1] for m in C.hash_messages()[:3]] == [b"", b"abc", b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq"]
    # RFC 4648 section 10, in url form without padding; and the two characters that differ from plain base64
    for plain, enc in ((b"", b""), (b"f", b"Zg"), (b"fo", b"Zm8"), (b"foo", b"Zm9v"), (b"foob", b"Zm9vYg"), (b"fooba", b"Zm9vYmE"),
                       (b"foobar", b"Zm9vYmFy"), (b"\xfb\xff", b"-_8"), (b"\xff\xef", b"_-8")):
        assert W.b64url(plain) == enc
    assert W.expected_prefix(b"foob", "https://a.example") == b'{"type":"webauthn.get","challenge":"Zm9vYg","origin":"https://a.example","crossOrigin":'
    # DER: the encoder and the strict parser agree, on every integer length
    for r, s in ((1, 1), (0x7F, 0x80), (0, 2**255), (2**256 - 1, 2**248 - 1), (R.N - 1, R.N)):
        assert W.der_parse(W.der_encode(r, s)) == (r, s)
    assert W.der_encode(0x80, 1) == bytes.fromhex("3007020200800201" "01") and len(W.der_encode(2**255, 2**255)) == 72


def test_records_are_es256_records(cs):
    """The record of every case that reaches the curve is es256_ref's record of (key, r, s, msghash), and the verdict over it
    es256_ref's; every other record is all zero."""
    for name, a, reason, rec in zip(cs.names, cs.assertions, cs.reasons, cs.records):
        if reason in (W.VALID, W.RANGE, W.OFF_CURVE, W.MISMATCH):
            assert R.verify_record(rec) == reason, name
            z = hashlib.sha256(a.authenticator_data + hashlib.sha256(a.client_data_json).digest()).digest()
            assert rec[128:] == z[::-1] and rec[:32] == a.x.to_bytes(32, "little") and rec[32:64] == a.y.to_bytes(32, "little"), name
        else:
            assert rec == bytes(160), name
    assert (W.VALID, W.RANGE, W.OFF_CURVE, W.MISMATCH) == (R.VALID, R.RANGE, R.OFF_CURVE, R.MISMATCH)


def test_the_set_covers_what_it_must(cs):
    assert len(cs) >= 200 and len(set(cs.names)) == len(cs)
    assert set(cs.reasons) == set(range(10))
    valid = [a for a, r in zip(cs.assertions, cs.reasons) if r == W.VALID]
    # hash padding edges, on assertions that are hashed and accepted
    cd_lens = {len(a.client_data_json) for a in valid}
    for block in (1, 2, 3):
        for m in (0, 1, 55, 56, 63):
            n = 64 * block + m
            assert n in cd_lens or n < C.CD_MIN, n
    assert {4033, 4087, 4088, 4095, 4096} <= cd_lens and C.CD_MIN in cd_lens
    shortest = min(len(C.client_data(bytes(1), "")), C.CD_MIN)
    assert shortest == C.CD_MIN == 72  # no passing clientDataJSON is shorter: 64 and 65 cannot be hashed messages
    assert {cs.reasons[cs.index("cdlen/64")], cs.reasons[cs.index("cdlen/65")]} == {W.CLIENTDATA}
    ad_lens = {len(a.authenticator_data) for a in valid}
    assert {37, 87, 88, 95, 96, 1024} <= ad_lens
    assert {(n + 32) % 64 for n in ad_lens} >= {55, 56, 63, 0}
    # bytes 0x80 .. 0xff in the extension part
    assert any(max(a.authenticator_data[37:], default=0) >= 0xF0 and min(a.authenticator_data[37:]) >= 0x80
               for a in valid if len(a.authenticator_data) > 37)
    C.assert_alignment_coverage(cs)
    # caps, rules, DER, ECDSA, order: by name, with the reason each is built for (build() asserted them against the reference)
    want = {
        "cap/authdata=1025": W.SIZE, "cap/clientdata=4097": W.SIZE, "cap/challenge=65": W.SIZE, "cap/origin=256": W.SIZE, "cap/challenge=0": W.SIZE,
        "cap/signature=73": W.SIZE, "cap/signature=7": W.SIZE, "cap/authdata=36": W.AUTHDATA, "adlen/1024": W.VALID, "cdlen/4096": W.VALID,
        "cap/challenge=64": W.VALID, "cap/origin=255": W.VALID, "cap/signature=72": W.VALID,
        "rpid/sent-wrong-in-byte-0": W.RPID, "rpid/sent-wrong-in-byte-31": W.RPID, "rpid/expected-wrong-in-byte-0": W.RPID,
        "rpid/expected-wrong-in-byte-31": W.RPID, "flags/up-clear": W.FLAGS, "flags/uv-required-and-clear": W.FLAGS,
        "flags/uv-required-and-set": W.VALID,
        "cd/type=webauthn.create": W.CLIENTDATA, "cd/challenge-wrong-in-its-first-character": W.CLIENTDATA,
        "cd/challenge-wrong-in-its-last-character": W.CLIENTDATA, "cd/challenge=1": W.VALID, "cd/challenge=2": W.VALID, "cd/challenge=3": W.VALID,
        "cd/challenge=32": W.VALID, "cd/challenge=64": W.VALID, "cd/origin-differs": W.CLIENTDATA, "cd/origin-closing-quote": W.CLIENTDATA,
        "cd/shorter-than-E": W.CLIENTDATA, "cd/equal-to-E": W.CLIENTDATA, "cd/tru}": W.CLIENTDATA, "cd/true-without-the-policy": W.CLIENTDATA,
        "cd/true-with-the-policy": W.VALID, "cd/false-then-another-byte": W.CLIENTDATA, "cd/last-byte-not-a-brace": W.CLIENTDATA,
        "der/r=33-bytes": W.VALID, "der/s=33-bytes": W.VALID, "der/r=s=32-bytes": W.VALID, "der/s=31-bytes": W.VALID, "der/r=31-bytes": W.MISMATCH,
        "der/r=1-byte": W.MISMATCH, "der/non-minimal-00-on-r": W.SIGNATURE_DER, "der/negative-r": W.SIGNATURE_DER,
        "der/byte-after-s-counted": W.SIGNATURE_DER, "der/byte-after-s-uncounted": W.SIGNATURE_DER, "der/long-form-sequence": W.SIGNATURE_DER,
        "der/long-form-integer": W.SIGNATURE_DER, "der/tag-31": W.SIGNATURE_DER, "der/r-tag-03": W.SIGNATURE_DER, "der/s-tag-30": W.SIGNATURE_DER,
        "der/sequence-length+1": W.SIGNATURE_DER, "der/sequence-length-1": W.SIGNATURE_DER, "der/zero-length-r": W.SIGNATURE_DER,
        "der/zero-length-s": W.SIGNATURE_DER, "der/r=0": W.RANGE,
        "ecdsa/s+1": W.MISMATCH, "ecdsa/another-key": W.MISMATCH, "ecdsa/key-off-the-curve": W.OFF_CURVE, "ecdsa/x=p": W.RANGE,
        "order/size-before-authdata": W.SIZE, "order/authdata-before-clientdata": W.AUTHDATA, "order/rpid-before-flags": W.RPID,
        "order/flags-before-clientdata": W.FLAGS, "order/clientdata-before-der": W.CLIENTDATA, "order/der-before-range": W.SIGNATURE_DER,
        "order/range-before-off-curve": W.RANGE, "order/off-curve-before-mismatch": W.OFF_CURVE,
    }
    for name, reason in want.items():
        assert cs.reasons[cs.index(name)] == reason, name
    # the integer lengths the DER cases are named for
    for name, lens in (("der/r=33-bytes", (33, 32)), ("der/s=33-bytes", (32, 33)), ("der/r=s=32-bytes", (32, 32)), ("cap/signature=72", (33, 33))):
        sig = cs.assertions[cs.index(name)].signature
        assert (sig[3], sig[5 + sig[3]]) == lens, name
    sig = cs.assertions[cs.index("der/s=31-bytes")].signature
    assert sig[5 + sig[3]] == 31
    assert cs.assertions[cs.index("der/r=31-bytes")].signature[3] == 31
    # the counter comes back wherever authenticatorData has one, whatever fails later
    assert cs.counts[cs.index("valid/counter=ffffffff")] == 0xFFFFFFFF and cs.counts[cs.index("valid/counter=80000000")] == 0x80000000
    assert cs.counts[cs.index("flags/up-clear")] == 7 and cs.counts[cs.index("cap/authdata=36")] == 0 and cs.counts[cs.index("cap/authdata=1025")] == 0


def test_the_host_route_agrees_with_the_reference(cs):
    from webauthn_halo2_amd import ecdsa_p256 as api

    for name, a, reason, rec, count in zip(cs.names, cs.assertions, cs.reasons, cs.records, cs.counts):
        got = api.webauthn_verify(a.authenticator_data, a.client_data_json, a.signature, a.x.to_bytes(32, "big"), a.y.to_bytes(32, "big"),
                                  a.challenge, a.origin, a.rp_id_hash, a.flags_required, a.allow_cross_origin)
        assert got == (reason == W.VALID, reason, rec, count), name


def test_header_declares_the_entry_point_and_constants():
    txt = open(os.path.join(ROOT, "include", "zkmi355.h")).read()
    for i, name in enumerate(("VALID", "RANGE", "OFF_CURVE", "MISMATCH", "SIZE", "AUTHDATA", "RPID", "FLAGS", "CLIENTDATA", "SIGNATURE_DER")):
        assert re.search(r"#define\s+ZK_WEBAUTHN_%s\s+%d\b" % (name, i), txt), name
    for name, value in (("AUTHDATA_MAX", 1024), ("CLIENTDATA_MAX", 4096), ("CHALLENGE_MAX", 64), ("ORIGIN_MAX", 255)):
        assert re.search(r"#define\s+ZK_WEBAUTHN_%s\s+%d\b" % (name, value), txt), name
    assert re.search(r"#define\s+ZK_WEBAUTHN_BATCH_MAX\s+ZK_ES256_BATCH_MAX\b", txt)
    assert re.search(r"int\s+zk_webauthn_verify\s*\(\s*zk_ctx\s*\*\s*ctx\s*,\s*size_t\s+count\s*,\s*const\s+zk_webauthn_assertion\s*\*\s*a", txt)
    src = open(os.path.join(ROOT, "webauthn-halo2_amd", "csrc", "webauthn.hip")).read()
    assert "ZK_API(zk_webauthn_verify" in src
    assert "csrc/webauthn.hip" in open(os.path.join(ROOT, "build.sh")).read()


def test_python_names():
    from webauthn_halo2_amd import ecdsa_p256 as api, engine as E, proving_server as srv

    assert [getattr(E, "ZK_WEBAUTHN_" + n) for n in ("VALID", "RANGE", "OFF_CURVE", "MISMATCH", "SIZE", "AUTHDATA", "RPID", "FLAGS", "CLIENTDATA",
                                                     "SIGNATURE_DER")] == list(range(10))
    assert (E.ZK_WEBAUTHN_BATCH_MAX, E.ZK_WEBAUTHN_AUTHDATA_MAX, E.ZK_WEBAUTHN_CLIENTDATA_MAX, E.ZK_WEBAUTHN_CHALLENGE_MAX,
            E.ZK_WEBAUTHN_ORIGIN_MAX) == (16384, 1024, 4096, 64, 255)
    assert callable(E.Engine.webauthn_verify) and callable(api.webauthn_verify) and callable(api.webauthn_verify_many)
    assert callable(srv.parse_assertion) and callable(srv.prove_assertion) and callable(srv.prove_assertion_evm) and callable(srv.prove_assertions_batch)
    assert api.signature_check() == "host"  # the default route stays the host


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_portable_forms_on_the_cpu_under_the_sanitizers(cs, tmp_path):
    exe = str(tmp_path / "webauthn_host_check")
    # the host side only (nothing runs on a device); -O1: the sanitizers' checks at every access, in seconds
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-x", "hip", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "webauthn-halo2_amd", "csrc"), os.path.join(ROOT, "tests", "webauthn_host_check.cpp"), "-o", exe])
    cases, results = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    n_msgs = C.write_case_file(cases, cs)
    r = subprocess.run([exe, cases, results], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), "webauthn_host_check failed (%d): %s%s" % (r.returncode, r.stdout, r.stderr)
    raw = open(results, "rb").read()
    assert struct.unpack_from("<III", raw) == (C.MAGIC_OUT, len(cs), n_msgs)
    assert len(raw) == 12 + len(cs) * C.OUT_BYTES + 32 * n_msgs
    bad = []
    for i in range(len(cs)):
        rec = raw[12 + i * C.OUT_BYTES:12 + (i + 1) * C.OUT_BYTES]
        got = (rec[0], rec[5:], struct.unpack_from("<I", rec, 1)[0])
        if got != (cs.reasons[i], cs.records[i], cs.counts[i]):
            bad.append((cs.names[i], got[0], cs.reasons[i], got[2], cs.counts[i], got[1] == cs.records[i]))
    assert not bad, "webauthn_check_one differs from the reference on %d cases, first (name, reason got / want, counter got / want, record equal): %s" % (
        len(bad), bad[:5])
    at = 12 + len(cs) * C.OUT_BYTES
    for j, (p0, p1) in enumerate(C.hash_messages()):
        assert raw[at + 32 * j:at + 32 * j + 32] == hashlib.sha256(p0 + p1).digest(), "sha256_two of %d + %d bytes" % (len(p0), len(p1))
