"""ES256 without a GPU: the reference (tests/es256_ref.py) against the server's own host check on every record of the signature
set (tests/es256_cases.py) and on the RFC 6979 vector; the public names of the feature; and csrc/p256.hip.h's portable forms on
the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer.

The last part builds tests/p256_host_check.cpp - a stand-alone program with its own main, nothing of the library in it, no GPU
touched - with hipcc and runs it as a child process: the field, point and x-compare cases of tests/p256_cases.py through the
header's routines, and p256_verify_one over the whole signature set with a comb table of G the program builds itself.  Every
result equals the Python model, every verdict and reason the reference, and the sanitizers report nothing (either would end the
program with a non-zero status).  Skipped without hipcc.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import es256_cases
import es256_ref as R
import p256_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cs():
    return es256_cases.build()


def test_reference_matches_the_host_check_on_every_record(cs):
    from webauthn_halo2_amd import ecdsa_p256 as api

    assert len(cs) >= 400
    assert sum(1 for n in cs.names if n.startswith("valid/")) >= 300
    for name, rec, reason in zip(cs.names, cs.records, cs.reasons):
        got = api.es256_verify(*(rec[32 * i:32 * i + 32] for i in range(5)))
        assert got == (reason == R.VALID), name
    # every reason occurs, valid and invalid records both
    assert set(cs.reasons) == {R.VALID, R.RANGE, R.OFF_CURVE, R.MISMATCH}


def test_rfc6979_vector(cs):
    i = cs.index("kat/rfc6979-a.2.5-sample-sha256")
    assert cs.reasons[i] == R.VALID
    assert R.affine_mul(es256_cases.KAT_D, R.G) == (es256_cases.KAT_UX, es256_cases.KAT_UY)
    x, y, r, s, z = cs.fields[i]
    assert R.verify_ints(x, y, r, s, z ^ 1) == R.MISMATCH and R.verify_ints(x, y, s, r, z) == R.MISMATCH


def test_constructed_cases_do_what_they_are_built_for(cs):
    want = {"range/z=n-1": R.MISMATCH, "range/x=p": R.RANGE, "range/r=n": R.RANGE, "range/s=0": R.RANGE, "curve/(0,0)": R.OFF_CURVE,
            "key/d=1/0": R.VALID, "key/d=n-1/0": R.VALID, "key/d=2/0": R.VALID, "z0/0": R.VALID, "meet/equal/0": R.VALID,
            "meet/opposite/0": R.MISMATCH}
    for name, reason in want.items():
        assert cs.reasons[cs.index(name)] == reason, name
    assert cs.fields[cs.index("key/d=1/0")][:2] == R.G and cs.fields[cs.index("key/d=n-1/0")][:2] == (R.GX, R.P - R.GY)
    es256_cases.assert_digit_coverage(cs)


def test_header_declares_the_entry_point_and_constants():
    txt = open(os.path.join(ROOT, "include", "zkmi355.h")).read()
    for name, value in (("ZK_ES256_VALID", 0), ("ZK_ES256_RANGE", 1), ("ZK_ES256_OFF_CURVE", 2), ("ZK_ES256_MISMATCH", 3),
                        ("ZK_ES256_BATCH_MAX", 16384)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), txt), name
    assert re.search(r"int\s+zk_es256_verify\s*\(\s*zk_ctx\s*\*\s*ctx\s*,\s*size_t\s+count\s*,\s*const\s+uint8_t\s*\*\s*sigs", txt)
    src = open(os.path.join(ROOT, "webauthn-halo2_amd", "csrc", "es256.hip")).read()
    assert "ZK_API(zk_es256_verify" in src
    assert "csrc/es256.hip" in open(os.path.join(ROOT, "build.sh")).read()


def test_python_names():
    from webauthn_halo2_amd import ecdsa_p256 as api, engine as E

    assert (E.ZK_ES256_VALID, E.ZK_ES256_RANGE, E.ZK_ES256_OFF_CURVE, E.ZK_ES256_MISMATCH, E.ZK_ES256_BATCH_MAX) == (0, 1, 2, 3, 16384)
    assert (R.VALID, R.RANGE, R.OFF_CURVE, R.MISMATCH) == (0, 1, 2, 3)
    assert callable(E.Engine.es256_verify) and callable(api.es256_verify_many) and callable(api.set_signature_check)
    assert api.signature_check() == "host"  # the default: today's path
    for bad in ("", "gpu", "Device", "auto", None, 1):
        with pytest.raises(ValueError):
            api.set_signature_check(bad)
    assert api.signature_check() == "host"
    try:
        api.set_signature_check("device")
        assert api.signature_check() == "device"
    finally:
        api.set_signature_check("host")
    assert api.signature_check() == "host"


def test_field_and_point_case_classes():
    """The branch classes of tests/p256_cases.py, counted by the model alone."""
    recs, expect, classes = p256_cases.build()
    assert recs.shape[1] == p256_cases.REC_WORDS and len(expect) == recs.shape[0]
    p256_cases.assert_classes(classes)
    keys = [(int(o), int(m)) for o, m in zip(recs[:, 0], recs[:, 1])]
    assert keys == sorted(keys)
    assert {o for o, _ in keys} == set(p256_cases.OP_NAMES)
    assert {(o, m) for o, m in keys if o in p256_cases.FIELD_OPS} == {(o, m) for o in p256_cases.FIELD_OPS for m in (0, 1)}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_portable_forms_on_the_cpu_under_the_sanitizers(cs, tmp_path):
    exe = str(tmp_path / "p256_host_check")
    # the host side only (nothing runs on a device); -O1: the sanitizers' checks at every access, in seconds
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-x", "hip", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "webauthn-halo2_amd", "csrc"), "-I", os.path.join(ROOT, "tests"),
                           os.path.join(ROOT, "tests", "p256_host_check.cpp"), "-o", exe])
    cases, results, sigs, reasons = (str(tmp_path / n) for n in ("cases.bin", "results.bin", "sigs.bin", "reasons.bin"))
    n = p256_cases.write_case_file(cases)
    with open(sigs, "wb") as f:
        f.write(cs.blob)
    r = subprocess.run([exe, cases, results, sigs, reasons], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), "p256_host_check failed (%d): %s%s" % (r.returncode, r.stdout, r.stderr)
    raw = np.fromfile(results, dtype="<u4")
    assert raw[:4].tolist() == [p256_cases.MAGIC_OUT, n, p256_cases.OUT_WORDS, 1]
    p256_cases.check_results(raw[4:].reshape(n, p256_cases.OUT_WORDS), "CPU")
    got = list(open(reasons, "rb").read())
    assert len(got) == len(cs)
    bad = [(cs.names[i], got[i], cs.reasons[i]) for i in range(len(cs)) if got[i] != cs.reasons[i]]
    assert not bad, "p256_verify_one differs from the reference on %d records, first (name, got, want): %s" % (len(bad), bad[:5])
