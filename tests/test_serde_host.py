"""csrc/serde_host.h on the host (tests/serde_host_check.cpp, built here with hipcc; no GPU): host_g1_read / host_g2_read admit and
refuse exactly what the oracle's plain-integer codec does, on every malformed class of tests/serde_cases.py, and decode to the
oracle's point; the writers produce the oracle's bytes; In / Out hold their bounds at the edges."""
import os
import shutil
import subprocess

import pytest

import serde_cases as sc
from zkoracle import curve as C, serde
from zkoracle.field import P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = (sc.PROCESSED, sc.RAW_BYTES, sc.RAW_BYTES_UNCHECKED)

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shc") / "serde_host_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-x", "hip", "-I", os.path.join(ROOT, "webauthn-halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "serde_host_check.cpp"), "-o", out])
    return out


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


def test_g1_classes_same_verdicts_and_points(exe):
    pts = sc.section_points(7)
    jobs = []  # (label, fmt, element)
    for fmt in sc.CHECKED:
        for c in sc.point_cases(7, fmt):
            if c.index == 0:  # the element depends on the section's donor only
                jobs.append(((c.cls, c.section), fmt, c.element))
    # every valid point of a section, identities included, in every format
    for fmt in FMTS:
        jobs += [(("valid", i), fmt, serde.g1_bytes(pt, fmt)) for i, pt in enumerate(pts[0][:72])]
    got = ask(exe, ["g1r %d %s" % (fmt, enc.hex()) for _, fmt, enc in jobs])
    want = [want_read(serde.g1_parse, serde.g1_bytes, enc, fmt) for _, fmt, enc in jobs]
    assert got == want, [j[0] for j, g, w in zip(jobs, got, want) if g != w]
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
