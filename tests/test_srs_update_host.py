"""One ceremony contribution without a GPU: the tests' own rule (tests/srs_update_ref.py) against the oracle's tau-built SRS, the
engine's host half (csrc/srs_update.h through tests/srs_update_host_check.cpp, built here with hipcc) against that rule, the two new
entry points in the public header, and the refusals contribute_params makes before it opens a device."""
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import srs_update_ref as ref
from zkoracle import curve, field as F, srs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


def G(s):
    return srs.g1_of_scalar(s)


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6])
def test_reference_update_of_the_srs_is_the_srs_of_the_product(k):
    n = 1 << k
    s = ref.secret_of_seed(bytes([k]) * 32)
    t = srs.TAU * s % F.R
    g, gl = ref.update_both(srs.srs_points(k), s, k)
    assert g == [G(pow(t, i, F.R)) for i in range(n)]
    assert gl == [G(x) for x in srs.lagrange_at(k, t)]


def test_reference_keeps_degenerate_points_exact():
    k, n, s = 3, 8, 0x1234567
    P = G(99)
    assert ref.update([None] * n, s) == [None] * n
    assert ref.update_both([None] * n, s, k)[1] == [None] * n
    got = ref.update([P] * n, s)
    assert got == [G(99 * pow(s, i, F.R)) for i in range(n)] and got[0] == P
    one = [None] * n
    one[5] = P
    g, gl = ref.update_both(one, s, k)
    assert g == [None] * 5 + [G(99 * pow(s, 5, F.R))] + [None] * 2
    assert gl == ref.g_to_lagrange(g, k) and None not in gl
    # opposite points: g'[0] + g'[1] is [1 - s] P, no longer the identity; with s = r - 1 ([s] = negation) it is [2] P
    opp = [P, curve.neg(P)] * 4
    assert ref.update(opp, F.R - 1)[:2] == [P, P]
    assert ref.secret_of_seed(bytes(32)) == srs.TAU


def test_expected_flags_of_the_rule():
    assert ref.expected_flags(5, 35, 7, 7) == 7
    assert ref.expected_flags(5, 35, 8, 7) == ref.LINKS | ref.NONTRIVIAL  # s_g1 of another scalar
    assert ref.expected_flags(5, 35, 7, 9) == ref.NONTRIVIAL  # s_g2 of another scalar: it is in both equations
    assert ref.expected_flags(5, 36, 7, 7) == ref.SAME_SECRET | ref.NONTRIVIAL
    assert ref.expected_flags(6, 35, 7, 7) == ref.SAME_SECRET | ref.NONTRIVIAL
    assert ref.expected_flags(5, 5, 1, 1) == ref.SAME_SECRET | ref.LINKS  # s = 1
    assert ref.expected_flags(5, 0, 7, 7) == 0


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("suh") / "srs_update_host_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-x", "hip", "-I", os.path.join(ROOT, "webauthn-halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "srs_update_host_check.cpp"), "-o", out])
    return out


def receipt_bytes(c):
    lim = ref.contribution_to_limbs(c)
    return b"".join(lim[f].astype("<u8").tobytes() for f in ref.FIELDS)


def ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    res = [ln.split() for ln in out.stdout.splitlines()]
    assert len(res) == len(lines)
    return res


def flags_of(exe, blobs):
    res = ask(exe, ["receipt " + b.hex() for b in blobs])
    assert all(r[0] == "flags" for r in res)
    return [int(r[1]) for r in res]


@needs_hipcc
def test_header_rule_equals_the_python_rule(exe):
    rnd = random.Random(20260)
    cases = []  # (b, a, u, v)
    for tau, s in [(srs.TAU, ref.secret_of_seed(b"\x01" * 32)), (rnd.randrange(2, F.R), rnd.randrange(2, F.R)), (3, F.R - 1), (1, 2)]:
        honest = (tau, tau * s % F.R, s, s)
        assert ref.expected_flags(*honest) == 7
        cases.append(honest)
        for field in range(4):  # each field replaced by a point of another scalar
            t = list(honest)
            t[field] = rnd.randrange(2, F.R)
            cases.append(tuple(t))
    cases.append((5, 5, 1, 1))  # s_g1 = G: the step by s = 1
    cases.append((7, 7 * 9, 9, F.R + 9))
    # a consistent step by another secret under the same before_g1, and a receipt of s whose link is to the step by s^2
    cases.append((11, 11 * 5, 5, 5))
    cases.append((11, 11 * 25, 5, 5))
    got = flags_of(exe, [receipt_bytes(ref.contribution_of_scalars(*c)) for c in cases])
    want = [ref.expected_flags(*c) for c in cases]
    assert got == want, [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert got[0] == 7 and got[1] == ref.SAME_SECRET | ref.NONTRIVIAL and got[3] == ref.LINKS | ref.NONTRIVIAL
    assert got[20] == ref.SAME_SECRET | ref.LINKS


@needs_hipcc
def test_header_refuses_improper_points(exe):
    good = ref.contribution_of_scalars(5, 35, 7, 7)
    blob = receipt_bytes(good)
    bad = []
    for off in (0, 64, 128, 192):  # one bit of each field's first coordinate: off its curve
        b = bytearray(blob)
        b[off] ^= 1
        bad.append(bytes(b))
    for f in ref.FIELDS:  # the identity in each place
        bad.append(receipt_bytes(dict(good, **{f: None})))
    # a coordinate image not below p (x + p): the same point to a careless reader, not a canonical image
    lim = ref.contribution_to_limbs(good)
    x = sum(int(lim["s_g1"][q]) << (64 * q) for q in range(4)) + F.P
    assert x < 1 << 256
    lim["s_g1"][:4] = [(x >> (64 * q)) & 0xFFFFFFFFFFFFFFFF for q in range(4)]
    bad.append(b"".join(lim[f].astype("<u8").tobytes() for f in ref.FIELDS))
    got = flags_of(exe, [blob] + bad)
    assert got[0] == 7
    assert all(not g & ref.NONTRIVIAL for g in got[1:]), got
    assert got[1:] == [0] * len(bad)


@needs_hipcc
def test_g2_step_and_receipt_equal_the_oracle(exe):
    rnd = random.Random(7)
    lines, want = [], []
    for t, s in [(srs.TAU, ref.secret_of_seed(b"\x02" * 32)), (rnd.randrange(1, F.R), rnd.randrange(1, F.R)), (1, F.R - 1)]:
        pt = curve.g2_mul(curve.G2_GEN, t)
        lines.append("g2mul %s %x" % (ref.g2_to_words(pt).astype("<u8").tobytes().hex(), s))
        want.append(["g2", ref.g2_to_words(curve.g2_mul(pt, s)).astype("<u8").tobytes().hex()])
        before = G(t)
        c = ref.contribution(before, s)
        pts = ref.to_mont_limbs([before, c["after_g1"]]).astype("<u8")
        lines.append("make %s %s %x" % (pts[0].tobytes().hex(), pts[1].tobytes().hex(), s))
        want.append(["receipt", receipt_bytes(c).hex()])
    assert ask(exe, lines) == want


def test_header_declares_the_contribution_entry_points():
    txt = open(os.path.join(ROOT, "include", "zkmi355.h")).read()
    for decl in (r"int zk_srs_update\(zk_ctx\* ctx, const uint8_t seed\[32\], zk_srs_contribution\* out\)",
                 r"int zk_srs_contribution_check\(zk_ctx\* ctx, const zk_srs_contribution\* c, uint32_t\* flags\)",
                 r"typedef struct \{\s*uint64_t before_g1\[8\];[^}]*uint64_t after_g1\[8\];[^}]*uint64_t s_g1\[8\];[^}]*uint64_t s_g2\[16\];[^}]*\} zk_srs_contribution;",
                 r"#define ZK_SRS_CONTRIB_SAME_SECRET +1u", r"#define ZK_SRS_CONTRIB_LINKS +2u", r"#define ZK_SRS_CONTRIB_NONTRIVIAL +4u",
                 r"#define ZK_SRS_CONTRIB_RESIDENT +8u"):
        assert re.search(decl, txt), decl
    assert "knowledge-of-exponent" in txt and "not a Schnorr proof" in txt


def test_engine_and_api_expose_the_contribution():
    import webauthn_halo2_amd as zk
    from webauthn_halo2_amd import ecdsa_p256, engine as E

    for m in ("srs_update", "srs_contribution_check"):
        assert callable(getattr(zk.Engine, m))
    assert (E.ZK_SRS_CONTRIB_SAME_SECRET, E.ZK_SRS_CONTRIB_LINKS, E.ZK_SRS_CONTRIB_NONTRIVIAL, E.ZK_SRS_CONTRIB_RESIDENT) == (1, 2, 4, 8)
    assert callable(ecdsa_p256.contribute_params) and callable(ecdsa_p256.check_contributions)
    L = zk.load_library()
    for s in ("zk_srs_update", "zk_srs_contribution_check"):
        assert hasattr(L, s)
    import ctypes
    assert ctypes.sizeof(E.SrsContributionC) == 320


def test_contribute_params_refuses_before_a_device_is_opened(tmp_path, monkeypatch):
    from webauthn_halo2_amd import ecdsa_p256 as api

    def no_engine(*a, **kw):
        raise AssertionError("a device was opened")

    monkeypatch.setattr(api, "Engine", no_engine)
    src, dst = tmp_path / "kzg_bn254_4.srs", tmp_path / "out.srs"
    src.write_bytes((4).to_bytes(4, "little") + bytes(16))
    with pytest.raises(FileNotFoundError):
        api.contribute_params(str(tmp_path / "missing.srs"), str(dst), bytes(32))
    with pytest.raises(ValueError):
        api.contribute_params(str(src), str(src), bytes(32))
    with pytest.raises(ValueError):
        api.contribute_params(str(src), str(tmp_path / "." / "kzg_bn254_4.srs"), bytes(32))
    with pytest.raises(ValueError):
        api.contribute_params(str(src), str(dst), bytes(31))
    with pytest.raises(ValueError):
        api.contribute_params(None, str(dst), bytes(32))  # neither a source nor a degree
    assert not dst.exists() and src.read_bytes() == (4).to_bytes(4, "little") + bytes(16)
    assert api.check_contributions(str(src), []) is False  # (an empty chain proves nothing; no device either)
    assert api.check_contributions(str(tmp_path / "missing.srs"), [{}]) is False
