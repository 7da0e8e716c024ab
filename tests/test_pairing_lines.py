"""The device pairing's arithmetic without a GPU: the shared host / device half of csrc/pairing.h (prepared lines, the Miller loop
over them, the table-free final exponentiation, the G1 reasons) compiled for the host in tests/pairing_lines_check.cpp and held
against the host pairing it must agree with.  Expected verdicts come from scalars (tests/pairing_cases.py), never from a pairing."""
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import pairing_cases as pc
from zkoracle import curve, field as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

U = 4965661367192848881


def test_the_chain_of_the_final_exponentiation_adds_up_to_the_hard_part():
    """final_exponentiation_chain's products and squarings, replayed on exponents: the result is t^((p^4 - p^2 + 1) / r) exactly
    (in the cyclotomic subgroup a conjugate is an inverse, and exponents live mod p^4 - p^2 + 1)."""
    p, r = F.P, F.R
    assert p == 36 * U**4 + 36 * U**3 + 24 * U**2 + 6 * U + 1 and r == 36 * U**4 + 36 * U**3 + 18 * U**2 + 6 * U + 1
    phi = p**4 - p**2 + 1
    assert phi % r == 0
    fp, fp2 = p, p * p
    y0 = fp + fp2 + fp2 * p
    fu, fu2, fu3 = U, U * U, U**3
    fu2p = fu2 * p
    y2 = fu2p * p
    y3 = -(fu * p)
    y4 = -(fu + fu2p)
    y5 = -fu2
    y6 = -(fu3 + fu3 * p)
    y6 = 2 * y6 + y4 + y5
    t1 = y3 + y5 + y6
    y6 = y6 + y2
    t1 = 2 * (2 * t1 + y6)
    t0 = 2 * (t1 - 1)
    e = t0 + t1 + y0
    assert e % phi == (phi // r) % phi
    assert (1 << 64) + 0x9D797039BE763BA8 == 6 * U + 2 and U.bit_length() == 63


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plc") / "pairing_lines_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-x", "hip", "-I", os.path.join(ROOT, "webauthn-halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "pairing_lines_check.cpp"), "-o", out])
    return out


def ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    res = [ln.split() for ln in out.stdout.splitlines()]
    assert len(res) == len(lines)
    return res


def hx(words):
    return np.asarray(words, dtype=np.uint64).astype("<u8").tobytes().hex()


def check_line(a, b, g2, s_g2):
    """points (G1 tuples or None, G2 tuples) -> one `check` line"""
    return "check %s %s %s %s" % (hx(pc.g1_words([a])[0]), hx(pc.g1_words([b])[0]), hx(pc.g2_to_words(g2)), hx(pc.g2_to_words(s_g2)))


@needs_hipcc
def test_prepared_lines_equal_the_host_pairing(exe):
    rnd = random.Random(2026)
    xs = [1, 2, F.R - 1, rnd.randrange(3, F.R)]
    ts = [1, 2, rnd.randrange(3, F.R)]
    lines, want = [], []
    for t in ts:
        s_g2 = pc.g2(t)
        for x in xs:
            for y in xs:  # every (a, b) of the grid: most do not hold
                lines.append(check_line(pc.g1(x), pc.g1(y), curve.G2_GEN, s_g2))
                want.append(pc.holds(x, y, t))
            lines.append(check_line(pc.g1(x), pc.g1(x * t), curve.G2_GEN, s_g2))  # the holding partner of every x
            want.append(True)
            lines.append(check_line(pc.g1(x), curve.neg(pc.g1(x * t)), curve.G2_GEN, s_g2))  # b = -(correct b)
            want.append(False)
    # a pair whose g2 is not the generator: e([x] G, [t v] G2) = e([x t] G, [v] G2)
    v, t, x = rnd.randrange(2, F.R), rnd.randrange(2, F.R), rnd.randrange(2, F.R)
    lines.append(check_line(pc.g1(x), pc.g1(x * t), pc.g2(v), pc.g2(t * v)))
    want.append(True)
    lines.append(check_line(pc.g1(x), pc.g1(x * t + 1), pc.g2(v), pc.g2(t * v)))
    want.append(False)
    # the identity cases: (O, O) holds, (O, b) and (a, O) do not
    for a, b, w in [(None, None, True), (None, pc.g1(5), False), (pc.g1(5), None, False)]:
        lines.append(check_line(a, b, curve.G2_GEN, pc.g2(7)))
        want.append(w)
    assert any(want) and not all(want)
    res = ask(exe, lines)
    for ln, r, w in zip(lines, res, want):
        assert r[0] == "check"
        assert r[1] == "1", "miller_loop_lines != multi_miller_loop: " + ln
        assert r[2] == "1", "final_exponentiation_chain != final_exponentiation: " + ln
        assert int(r[3]) == int(w), "pairing_check: " + ln
        assert int(r[4]) == (pc.VALID if w else pc.MISMATCH), "pairing_check_lines: " + ln


@needs_hipcc
def test_reasons_of_improper_g1_points(exe):
    good_a, good_b = pc.g1_words([pc.g1(3)])[0], pc.g1_words([pc.g1(21)])[0]
    g2, s_g2 = hx(pc.g2_to_words(curve.G2_GEN)), hx(pc.g2_to_words(pc.g2(7)))
    p_x = good_a.copy()
    p_x[:4] = pc.p_words()  # a coordinate EQUAL to p
    one_one = pc.g1_words([(1, 1)])[0]
    cases = [(good_a, good_b, pc.VALID), (p_x, good_b, pc.RANGE), (good_a, pc.with_p_added(good_b, 4), pc.RANGE), (one_one, good_b, pc.OFF_CURVE),
             (good_a, one_one, pc.OFF_CURVE), (one_one, pc.with_p_added(good_b, 0), pc.RANGE)]  # RANGE before OFF_CURVE
    res = ask(exe, ["check %s %s %s %s" % (hx(a), hx(b), g2, s_g2) for a, b, _ in cases])
    assert [int(r[4]) for r in res] == [w for _, _, w in cases]


@needs_hipcc
def test_step_count_of_the_table(exe):
    res = ask(exe, ["steps " + hx(pc.g2_to_words(pc.g2(t))) for t in (1, 12345)])
    pop = bin(0x9D797039BE763BA8).count("1")
    for r in res:
        assert [int(v) for v in r[1:]] == [64 + pop + 2, 64 + pop + 2, pop]
    assert 64 + pop + 2 == 102


@needs_hipcc
def test_g2_refusals(exe):
    good = pc.g2_to_words(pc.g2(9))
    over = good.copy()
    v = sum(int(over[q]) << (64 * q) for q in range(4)) + F.P
    over[:4] = [(v >> (64 * q)) & 0xFFFFFFFFFFFFFFFF for q in range(4)]
    off = good.copy()
    off[0] ^= np.uint64(1)
    outside = pc.twist_point_outside_g2()
    assert pc.g2_on_twist(outside)
    cases = [(good, 1), (pc.g2_to_words(curve.G2_GEN), 1), (over, 0), (off, 0), (pc.g2_to_words(outside), 0), (pc.g2_to_words(None), 0)]
    res = ask(exe, ["g2proper " + hx(w) for w, _ in cases])
    assert [int(r[1]) for r in res] == [w for _, w in cases]


def test_header_declares_the_pairing_entry_points():
    txt = open(os.path.join(ROOT, "include", "zkmi355.h")).read()
    for decl in (r"int zk_pairing_check_batch\(zk_ctx\* ctx, size_t count, const uint64_t\* a[^;]*const uint64_t\* b[^;]*const uint64_t g2\[16\], const uint64_t s_g2\[16\][^;]*uint8_t\* verdicts[^;]*uint8_t\* reasons[^;]*\);",
                 r"int zk_verify_pairing_mode\(zk_ctx\* ctx, int mode\);", r"int zk_verify_pairing_stats\(zk_ctx\* ctx, uint64_t out\[2\]\);",
                 r"#define ZK_PAIRING_VALID 0", r"#define ZK_PAIRING_RANGE 1", r"#define ZK_PAIRING_OFF_CURVE 2", r"#define ZK_PAIRING_MISMATCH 3",
                 r"#define ZK_PAIRING_BATCH_MAX 4096", r"#define ZK_VERIFY_PAIRING_AUTO 0", r"#define ZK_VERIFY_PAIRING_HOST 1",
                 r"#define ZK_VERIFY_PAIRING_DEVICE 2"):
        assert re.search(decl, txt), decl


def test_engine_and_api_expose_the_pairing_check():
    import webauthn_halo2_amd as zk
    from webauthn_halo2_amd import ecdsa_p256, engine as E

    for m in ("pairing_check_batch", "verify_pairing_mode", "verify_pairing_stats"):
        assert callable(getattr(zk.Engine, m))
    assert (E.ZK_PAIRING_VALID, E.ZK_PAIRING_RANGE, E.ZK_PAIRING_OFF_CURVE, E.ZK_PAIRING_MISMATCH, E.ZK_PAIRING_BATCH_MAX) == (0, 1, 2, 3, 4096)
    assert (E.ZK_VERIFY_PAIRING_AUTO, E.ZK_VERIFY_PAIRING_HOST, E.ZK_VERIFY_PAIRING_DEVICE) == (0, 1, 2)
    L = zk.load_library()
    for s in ("zk_pairing_check_batch", "zk_verify_pairing_mode", "zk_verify_pairing_stats"):
        assert hasattr(L, s)
    assert ecdsa_p256.verify_pairing() == "auto"
    try:
        for mode in ("host", "device", "auto"):
            ecdsa_p256.set_verify_pairing(mode)
            assert ecdsa_p256.verify_pairing() == mode
        with pytest.raises(ValueError):
            ecdsa_p256.set_verify_pairing("gpu")
    finally:
        ecdsa_p256.set_verify_pairing("auto")
