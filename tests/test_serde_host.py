"""csrc/serde_host.h on the host (tests/serde_host_check.cpp, built here with hipcc; no GPU): host_g1_read / host_g2_read admit and
refuse exactly what the oracle's plain-integer codec does, on every malformed class of tests/serde_cases.py, and decode to the
oracle's point; the writers produce the oracle's bytes; In / Out hold their bounds at the edges.  The readers are format switches
over csrc/g1_codec.hip.h, whose functions the codec kernels of serde.hip and verify.hip call too: the second half holds that header's
proof-point forms, its compile-time square-root exponent and verifier.h's fr_read against plain integers and the oracle, and runs the
whole job list once more under AddressSanitizer and UndefinedBehaviorSanitizer."""
import functools
import os
import shutil
import subprocess

import pytest

import serde_cases as sc
from zkoracle import curve as C, plonk, serde
from zkoracle.field import P, R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = (sc.PROCESSED, sc.RAW_BYTES, sc.RAW_BYTES_UNCHECKED)

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


def build_check(out, flags):
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", *flags, "-std=c++17", "-x", "hip", "-I", os.path.join(ROOT, "webauthn-halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "serde_host_check.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_check(str(tmp_path_factory.mktemp("shc") / "serde_host_check"), ["-O2"])


def ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    res = out.stdout.splitlines()
    assert len(res) == len(lines)
    return res


def want_read(parse, to_raw, enc, fmt):
    ok, dec = sc.oracle_verdict(parse, enc, fmt)
    return "admit " + to_raw(dec, serde.RAW_BYTES).hex() if ok else "refuse"


def g2_neg(p):
    return (p[0], ((-p[1][0]) % P, (-p[1][1]) % P))


@functools.lru_cache(maxsize=None)
def g1_read_jobs():
    """((label, fmt, element), ..), (the oracle's answer per job, ..)"""
    pts = sc.section_points(7)
    jobs = []
    for fmt in sc.CHECKED:
        for c in sc.point_cases(7, fmt):
            if c.index == 0:  # the element depends on the section's donor only
                jobs.append(((c.cls, c.section), fmt, c.element))
    # every valid point of a section, identities included, in every format
    for fmt in FMTS:
        jobs += [(("valid", i), fmt, serde.g1_bytes(pt, fmt)) for i, pt in enumerate(pts[0][:72])]
    return tuple(jobs), tuple(want_read(serde.g1_parse, serde.g1_bytes, enc, fmt) for _, fmt, enc in jobs)


def test_g1_classes_same_verdicts_and_points(exe):
    jobs, want = g1_read_jobs()
    got = ask(exe, ["g1r %d %s" % (fmt, enc.hex()) for _, fmt, enc in jobs])
    assert got == list(want), [j[0] for j, g, w in zip(jobs, got, want) if g != w]
    assert sum(w == "refuse" for w in want) == 2 * (7 + 5)
    # RawBytesUnchecked takes the refused RawBytes elements as they are
    raw_bad = [c.element for c in sc.point_cases(7, sc.RAW_BYTES) if c.index == 0 and not c.admit]
    assert ask(exe, ["g1r 2 " + e.hex() for e in raw_bad]) == ["admit " + e.hex() for e in raw_bad]


def test_g1_writer_equals_the_oracle(exe):
    pts = sc.section_points(7)[1][:72]
    jobs = [(fmt, pt) for fmt in FMTS for pt in pts]
    got = ask(exe, ["g1w %d %s" % (fmt, serde.g1_bytes(pt, serde.RAW_BYTES).hex()) for fmt, pt in jobs])
    assert got == ["bytes " + serde.g1_bytes(pt, fmt).hex() for fmt, pt in jobs]


def test_g2_classes_same_verdicts_and_points(exe):
    jobs = []
    for fmt in sc.CHECKED:
        jobs += [((c.cls, c.which), fmt, c.element) for c in sc.g2_cases(7, fmt)]
    valid = list(sc.g2_points()) + [g2_neg(p) for p in sc.g2_points()] + [C.g2_mul(C.G2_GEN, m) for m in (2, 3, 5, 7, 0x1234567)] + [None]
    for fmt in FMTS:
        jobs += [(("valid", i), fmt, serde.g2_bytes(pt, fmt)) for i, pt in enumerate(valid)]
    got = ask(exe, ["g2r %d %s" % (fmt, enc.hex()) for _, fmt, enc in jobs])
    want = [want_read(serde.g2_parse, serde.g2_bytes, enc, fmt) for _, fmt, enc in jobs]
    assert got == want, [j[0] for j, g, w in zip(jobs, got, want) if g != w]
    assert sum(w == "refuse" for w in want) == 2 * (6 + 5)
    raw_bad = [c.element for c in sc.g2_cases(7, sc.RAW_BYTES) if not c.admit]
    assert ask(exe, ["g2r 2 " + e.hex() for e in raw_bad]) == ["admit " + e.hex() for e in raw_bad]
    # the writer
    jobs = [(fmt, pt) for fmt in FMTS for pt in valid]
    got = ask(exe, ["g2w %d %s" % (fmt, serde.g2_bytes(pt, serde.RAW_BYTES).hex()) for fmt, pt in jobs])
    assert got == ["bytes " + serde.g2_bytes(pt, fmt).hex() for fmt, pt in jobs]


def model_in(length, takes):
    pos, out = 0, []
    for n in takes:
        if n > length - pos:
            out.append(-1)
        else:
            out.append(pos)
            pos += n
    return " ".join(map(str, out)) + " pos %d" % pos


def model_out(cap, takes):
    """cap None: the size-only writer.  An overflowing take hands out nothing, and neither does any take after it; the count goes on."""
    pos, real, out = 0, cap is not None, []
    for n in takes:
        fits = real and pos + n <= cap
        out.append(pos if fits else -1)
        if real and not fits:
            real = False
        pos += n
    return " ".join(map(str, out)) + " pos %d real %d" % (pos, 1 if real else 0)


def test_bounded_reader_and_writer_edges(exe):
    SIZE_MAX = (1 << 64) - 1
    word = lambda n: "max" if n == SIZE_MAX else str(n)
    ins = [(10, [10]), (10, [10, 0, 1]), (10, [11]), (10, [4, 6]), (10, [4, 7, 6]), (10, [4, SIZE_MAX, 6, 1]), (10, [SIZE_MAX]),
           (0, [0, 1]), (1, [0, 1, 1]), (64, [32, 32, 32])]
    outs = [(10, [10]), (10, [11]), (10, [4, 6]), (10, [4, 7, 1]), (10, [10, 1, 0]), (1, [0, 1, 1]), (None, [5, 7]), (None, [0]), (None, [1 << 40, 3])]
    got = ask(exe, ["in %d %s" % (ln, " ".join(word(n) for n in t)) for ln, t in ins] +
              ["out %s %s" % ("null" if cap is None else cap, " ".join(word(n) for n in t)) for cap, t in outs] + ["be32 0", "be32 258", "be32 4294967295"])
    want = [model_in(ln, t) for ln, t in ins] + [model_out(cap, t) for cap, t in outs] + \
           ["bytes %s back %d" % (v.to_bytes(4, "big").hex(), v) for v in (0, 258, 4294967295)]
    assert got == want
    # spelled out: exactly len; one past len leaves the position; SIZE_MAX after a partial read is refused and the rest still reads
    assert want[0] == "0 pos 10" and want[2] == "-1 pos 0" and want[5] == "0 -1 4 -1 pos 10"
    assert want[len(ins) + 6] == "-1 -1 pos 12 real 0"  # size only: nothing handed out, the length counted


# ------------------------------------------------------------------------------- the codec under the readers ---
# csrc/g1_codec.hip.h is the one statement of the encodings: the kernels of serde.hip and verify.hip call the functions this program
# calls.  The rules are restated below on plain integers; where the oracle has the rule (zkoracle.plonk's two read_point, its two
# read_scalar) it must agree with that statement too.

def test_sqrt_exponent_is_a_quarter_of_p_plus_1(exe):
    assert P % 4 == 3
    assert ask(exe, ["sqrtexp"]) == ["%064x" % ((P + 1) // 4)]


def model_blake2b_point(b):
    """A proof point of the Blake2b transcript: x little-endian below p, the parity of y in bit 255; never the identity"""
    v = int.from_bytes(b, "little")
    sign, x = v >> 255, v & (sc.TOP - 1)
    if x >= P or (x == 0 and not sign):  # all zero spells the identity: a point of a file, no point of a proof
        return None
    rhs = (x * x * x + 3) % P
    y = pow(rhs, (P + 1) // 4, P)
    if y * y % P != rhs:
        return None
    return (x, y if (y & 1) == sign else (P - y) % P)


def model_evm_point(b):
    """A proof point of the EVM transcript: x || y big-endian, both below p, on the curve, not (0, 0)"""
    x, y = int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")
    if x >= P or y >= P or (x, y) == (0, 0) or (y * y - x * x * x - 3) % P:
        return None
    return (x, y)


def oracle_point(op, b):
    tr = (plonk.Blake2bTranscript if op == "ptb" else plonk.EvmTranscript)(bytes(b))
    try:
        return tr.read_point()
    except ValueError:
        return None


@functools.lru_cache(maxsize=None)
def proof_point_jobs():
    """((class, op, bytes), ..), (the expected answer per job, ..) — expected by the plain-integer rule, which the oracle shares"""
    be = lambda v: int(v).to_bytes(32, "big")
    pts = sc.section_points(7)[0]
    donors = [pts[sc.GEN_AT], pts[sc.NEG_GEN_AT], pts[sc.XPM1_AT], pts[sc.DONOR_AT], pts[6]]
    assert {y & 1 for _, y in donors} == {0, 1} and donors[2][0] == P - 1
    jobs = []
    for x, y in donors:
        assert x + P < sc.TOP  # x + p fits the 255 bits of the compressed form (and the 256 of the EVM form)
        jobs += [("valid", "ptb", sc._proc(x, y & 1)), ("valid_other_sign", "ptb", sc._proc(x, 1 - (y & 1))),
                 ("x_plus_p", "ptb", sc._proc(x + P, y & 1)),
                 ("valid", "pte", be(x) + be(y)), ("valid_other_sign", "pte", be(x) + be(P - y)),
                 ("x_plus_p", "pte", be(x + P) + be(y)), ("y_plus_p", "pte", be(x) + be(y + P)),
                 ("y_off_by_one", "pte", be(x) + be((y + 1) % P)), ("y_off_by_one", "pte", be(x) + be((y - 1) % P))]
    y2 = sc.Y_OF_XPM1
    jobs += [("x_0", "ptb", sc._proc(0, 0)), ("x_0_signed", "ptb", sc._proc(0, 1)),
             ("x_p_minus_1", "ptb", sc._proc(P - 1, 0)), ("x_p_minus_1", "ptb", sc._proc(P - 1, 1)),
             ("x_p", "ptb", sc._proc(P, 0)), ("x_p", "ptb", sc._proc(P, 1)), ("x_all_ones", "ptb", sc._proc(sc.TOP - 1, 1)),
             ("nonresidue", "ptb", sc.NONRESIDUE_X), ("nonresidue", "ptb", sc._proc(10, 1)),
             ("zero_zero", "pte", be(0) + be(0)), ("x_0", "pte", be(0) + be(2)), ("x_p", "pte", be(P) + be(0)), ("x_p", "pte", be(P) + be(2)),
             ("x_p_minus_1", "pte", be(P - 1) + be(y2)), ("y_eq_p", "pte", be(P - 1) + be(P)), ("all_ones", "pte", b"\xff" * 64),
             ("nonresidue", "pte", be(4) + be(1)), ("nonresidue", "pte", be(4) + be(0))]
    want = []
    for cls, op, b in jobs:
        pt = (model_blake2b_point if op == "ptb" else model_evm_point)(b)
        assert pt == oracle_point(op, b), (cls, op)
        assert (pt is not None) == cls.startswith(("valid", "x_p_minus_1")), (cls, op)
        want.append("refuse" if pt is None else "point " + (be(pt[0]) + be(pt[1])).hex())
    return tuple(jobs), tuple(want)


def test_proof_points_of_both_transcripts(exe):
    jobs, want = proof_point_jobs()
    got = ask(exe, ["%s %s" % (op, b.hex()) for _, op, b in jobs])
    assert got == list(want), [j[:2] for j, g, w in zip(jobs, got, want) if g != w]
    # the one difference between a file and a proof: all zero is the file's identity
    assert ask(exe, ["g1r %d %s" % (sc.PROCESSED, sc._proc(0, 0).hex())]) == ["admit " + bytes(64).hex()]


def oracle_scalar(big_endian, b):
    tr = (plonk.EvmTranscript if big_endian else plonk.Blake2bTranscript)(bytes(b))
    try:
        return tr.read_scalar()
    except ValueError:
        return None


@functools.lru_cache(maxsize=None)
def scalar_jobs():
    jobs, want = [], []
    for v in (0, 1, R - 1, R, R + 1, (1 << 256) - 1):
        for big_endian in (0, 1):
            b = v.to_bytes(32, "big" if big_endian else "little")
            assert oracle_scalar(big_endian, b) == (v if v < R else None)
            jobs.append("frr %d %s" % (big_endian, b.hex()))
            want.append("value %064x" % v if v < R else "refuse")
    return tuple(jobs), tuple(want)


def test_fr_read_refuses_r_and_above_in_both_byte_orders(exe):
    jobs, want = scalar_jobs()
    assert ask(exe, list(jobs)) == list(want)
    assert want.count("refuse") == 6


def test_codec_on_the_cpu_under_the_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UndefinedBehaviorSanitizer, over every G1 and proof-point job above: the answers are
    the same, and neither sanitizer reports (either would end the program with a non-zero status).  Host code, stand-alone."""
    san = build_check(str(tmp_path / "serde_host_check_san"), ["--cuda-host-only", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                                                              "-Xarch_host", "-fno-sanitize-recover=undefined"])
    g1, g1_want = g1_read_jobs()
    pp, pp_want = proof_point_jobs()
    fr, fr_want = scalar_jobs()
    writes = [(fmt, pt) for fmt in FMTS for pt in sc.section_points(7)[1][:72]]
    lines = (["g1r %d %s" % (fmt, enc.hex()) for _, fmt, enc in g1] + ["%s %s" % (op, b.hex()) for _, op, b in pp] + list(fr) + ["sqrtexp"] +
             ["g1w %d %s" % (fmt, serde.g1_bytes(pt, serde.RAW_BYTES).hex()) for fmt, pt in writes])
    want = list(g1_want) + list(pp_want) + list(fr_want) + ["%064x" % ((P + 1) // 4)] + ["bytes " + serde.g1_bytes(pt, fmt).hex() for fmt, pt in writes]
    assert ask(san, lines) == want
