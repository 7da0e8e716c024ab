"""The device forms of csrc/field.hip.h, field29.hip.h, ec.hip.h and ec29.hip.h, run directly (tests/field_device_check.hip)
at their edge operands and lazy bounds, in every instruction form the headers compile to.

Per build the harness runs once, as a child process under its own time limit, over the cases of tests/field_device_cases.py
(one case per lane, each (op, modulus) run launched in blocks of 64 and of 256 lanes).  Groups A and C are compared with big
integers / zkoracle.curve, groups B and D limb for limb with tests/field29_model.py — so every build, both SER forms and both
block sizes also agree with each other to the bit.  The coverage counts asserted below come from the model alone
(test_case_set_covers_every_branch_class runs without a GPU).

Builds: (ZK_MUL29_ASM, ZK_MUL29_MASKRUN) = (0, 0), (1, 0), (2, 0), (2, 1), and (2, 0) with ZK_EC29_SQR=0 ZK_EC29_FUSE=0.

Measured: generating the 204 k cases and their expected results takes about 36 s of Python on the CPU, once per session and
shared by the five builds.  One build's harness run (process start to exit, both block sizes) takes 0.3 to 0.45 s of wall
time on an MI355X: MEASURED_WALL_SECONDS below.

Found by this test: fe_mul_gfx950 opened every column with a[i] * b[j] and no carry instruction; with words of all ones
(0xffffffff^2 + the shifted-in accumulator >= 2^64) the carry was lost — fe_sqr(2^96 - 1) was wrong for both moduli.
"""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import field_device_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]
BUILDS = {  # name -> (defines, which expectation: 1 = the curve's squarings and fused product switched off)
    "a0": (["-DZK_MUL29_ASM=0"], 0),
    "a1": (["-DZK_MUL29_ASM=1"], 0),
    "a2": (["-DZK_MUL29_ASM=2"], 0),
    "a2m": (["-DZK_MUL29_ASM=2", "-DZK_MUL29_MASKRUN=1"], 0),
    "a2p": (["-DZK_MUL29_ASM=2", "-DZK_EC29_SQR=0", "-DZK_EC29_FUSE=0"], 1),
}
# wall time of one harness run (process start to exit, 204 k cases, both block sizes) on an MI355X, per build
MEASURED_WALL_SECONDS = {"a0": 0.39, "a1": 0.30, "a2": 0.45, "a2m": 0.34, "a2p": 0.38}
RUN_TIMEOUT = 120


def _binary(name):
    """The build's harness binary: build.sh makes it; a missing one is built here when hipcc is on the path.  Neither: fail."""
    exe = os.path.join(HERE, "field_device_check_" + name)
    if os.path.isfile(exe):
        return exe
    hipcc = shutil.which("hipcc")
    assert hipcc, "%s is missing (build.sh makes it) and there is no hipcc on the path to build it" % exe
    subprocess.check_call([hipcc] + FLAGS + BUILDS[name][0] + ["-I", os.path.join(ROOT, "webauthn-halo2_amd", "csrc"),
                                                             os.path.join(HERE, "field_device_check.hip"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def cases():
    return D.build()


@pytest.fixture(scope="module")
def case_file(cases, tmp_path_factory):
    recs = cases[0]
    path = str(tmp_path_factory.mktemp("field_device") / "cases.bin")
    with open(path, "wb") as f:
        np.array([D.MAGIC_IN, recs.shape[0], D.REC_WORDS, 0], dtype="<u4").tofile(f)
        recs.astype("<u4").tofile(f)
    return path


def test_case_set_covers_every_branch_class(cases):
    recs, exp, mask, classes = cases
    per_op = {}
    for op, mod in zip(recs[:, 0].tolist(), recs[:, 1].tolist()):
        per_op[(op, mod)] = per_op.get((op, mod), 0) + 1
    field_ops = [o for o in D.OP_NAMES if o < 60]
    assert set(per_op) == {(o, m) for o in field_ops for m in (0, 1)} | {(o, 1) for o in D.OP_NAMES if o >= 60}, "an op has no case"
    for (op, mod), n in per_op.items():
        name = D.OP_NAMES[op]
        if op < 60 and name not in ("FE_INV", "IS_ZERO29"):
            assert n >= 2048, (name, mod, n)
        else:
            assert n >= 512, (name, mod, n)
    assert per_op[(D.G1X29_SHFL_DOWN, 1)] % 64 == 0
    c = lambda *k: classes[k]
    for mod in (0, 1):
        # at least 200 cases on each side of every final conditional subtraction
        for name in ("FE_MUL", "FE_SQR"):
            assert c(name, mod, "total<p") >= 200 and c(name, mod, "total>=p") >= 200, name
        for name in ("REDUCE_ONCE", "REDUCE_ONCE_ASM"):
            assert c(name, mod, "a<p") >= 200 and c(name, mod, "a>=p") >= 200
        assert c("INTERNAL_TO_STD", mod, "raw<p") >= 200 and c("INTERNAL_TO_STD", mod, "raw>=p") >= 200
        for name in ("MUL29", "SQR29", "MUL2ADD29", "MUL1ADD29", "MUL4ADD29", "MUL5ADD29"):
            for ser in ("_S", "_C"):
                assert c(name + ser, mod, "total<p") >= 200 and c(name + ser, mod, "total>=p") >= 200, name
                assert c(name + ser, mod, "total=p") >= 1, name  # zero in a non-zero representative: the total is exactly p
        assert c("FE_ADD", mod, "sum<p") >= 200 and c("FE_ADD", mod, "sum=p") >= 50 and c("FE_ADD", mod, "sum>p") >= 200
        assert c("FE_SUB", mod, "borrow") >= 200 and c("FE_SUB", mod, "equal") >= 50 and c("FE_SUB", mod, "plain") >= 200
        assert c("FE_NEG", mod, "zero") >= 1 and c("FE_DBL", mod, "2a<p") >= 200 and c("FE_DBL", mod, "2a>=p") >= 200
        assert c("IS_ZERO29", mod, "zero") >= 4 and c("IS_ZERO29", mod, "nonzero") >= 100
        assert c("TO29_X32", mod, "largest") == 1 and c("STD_TO_INTERNAL", mod, "largest") == 1
    assert c("MUL29_CALL", 1, "total>=p") >= 200 and c("MUL29_CALL", 1, "total=p") >= 1
    assert c("INTERNAL_TO_STD_CALL", 1, "raw>=p") >= 200 and c("INTERNAL_TO_STD_CALL", 1, "raw<p") >= 200
    for name in ("G1X_ADD", "G1X_ADD_AFFINE"):
        assert c(name, 1, "add") >= 500 and c(name, 1, "dbl") >= 20 and c(name, 1, "cancel") >= 20 and c(name, 1, "acc_inf") >= 1
    assert c("G1X_ADD", 1, "b_inf") >= 2  # identity as addend, and as both
    assert c("G1X_DBL", 1, "inf") >= 1 and c("G1X_TO_JAC", 1, "inf") >= 1
    for v in ("CS", "CI", "NS", "NI"):
        name = "G1X29_ADD_AFFINE_" + v
        assert c(name, 1, "generic") == 4 * len(D.LIFTS) and c(name, 1, "same") == c(name, 1, "negated") == 2 * len(D.LIFTS)
        assert c(name, 1, "acc_inf") >= 20
        if v[0] == "C":
            assert c(name, 1, "refused") == 4 * len(D.LIFTS)  # CHECK = true: false, accumulator unchanged, on every same-x step
        else:
            assert c(name, 1, "zz=0") == 4 * len(D.LIFTS)     # CHECK = false: ZZ = 0 (mod p) afterwards
    for lift in D.LIFTS:
        assert classes[("lift", 1, lift)] == 4
    for name in ("G1X29_ADD_S", "G1X29_ADD_C"):
        assert c(name, 1, "add") == 3 * len(D.LIFTS)
        assert c(name, 1, "dbl") == c(name, 1, "cancel") == c(name, 1, "acc_inf") == len(D.LIFTS) and c(name, 1, "b_inf") == len(D.LIFTS) + 1
    assert c("G1X29_DBL_RARE", 1, "point") == 3 * len(D.LIFTS) and c("G1X29_DBL_RARE", 1, "inf") == 1
    assert c("G1X29_CHAIN", 1, "n=1") >= 100 and c("G1X29_CHAIN", 1, "n=2") >= 100 and c("G1X29_CHAIN", 1, "n=40") >= 100
    for off in D.SHFL_OFFSETS:
        assert c("G1X29_SHFL_DOWN", 1, "off=%d" % off) == 320
    assert c("G1X29_SHFL_DOWN", 1, "inf") >= 100 and c("G1X29_SHFL_DOWN", 1, "point") >= 1000
    # every masked expected word is set, the two expectations differ only where the curve's switches matter
    differs = np.unique(recs[(exp[0] != exp[1]).any(axis=1), 0]).tolist()
    assert set(differs) <= {D.G1X29_ADD_AFFINE_CS, D.G1X29_ADD_AFFINE_CI, D.G1X29_ADD_AFFINE_NS, D.G1X29_ADD_AFFINE_NI, D.G1X29_CHAIN}
    assert mask[:, D.OUT_WORDS - 1].all()


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_device_forms_against_the_model(build, cases, case_file, tmp_path):
    recs, exp, mask, _ = cases
    n = recs.shape[0]
    exe = _binary(build)
    out = str(tmp_path / "results.bin")
    t0 = time.perf_counter()
    r = subprocess.run([exe, case_file, out], capture_output=True, text=True, timeout=RUN_TIMEOUT)
    wall = time.perf_counter() - t0
    print("build %s: harness wall time %.2f s; %s" % (build, wall, r.stdout.strip()))
    assert r.returncode == 0, "harness %s failed (%d): %s%s" % (build, r.returncode, r.stdout, r.stderr)
    raw = np.fromfile(out, dtype="<u4")
    assert raw[:4].tolist() == [D.MAGIC_OUT, n, D.OUT_WORDS, 2] and raw.size == 4 + 2 * n * D.OUT_WORDS, "result file malformed"
    got = raw[4:].reshape(2, n, D.OUT_WORDS)
    want = exp[BUILDS[build][1]]
    for b, block in enumerate((64, 256)):
        # one result per case: every lane wrote its marker
        done = got[b, :, D.OUT_WORDS - 1]
        assert int((done == (D.DONE | recs[:, 0])).sum()) == n, "block %d: %d of %d cases have no result" % (
            block, n - int((done == (D.DONE | recs[:, 0])).sum()), n)
        bad = ((got[b] != want) & mask).any(axis=1)
        if bad.any():
            k = int(np.argmax(bad))
            words = np.nonzero((got[b, k] != want[k]) & mask[k])[0].tolist()
            per_op = {}
            for o, m in zip(recs[bad, 0].tolist(), recs[bad, 1].tolist()):
                key = "%s/%s" % (D.OP_NAMES[o], "Fq" if m else "Fr")
                per_op[key] = per_op.get(key, 0) + 1
            used = np.nonzero(recs[k, D.OPND:])[0]
            opnd = recs[k, D.OPND:D.OPND + (int(used[-1]) + 1 if used.size else 1)]
            first = int(np.argmax((recs[:, 0] == recs[k, 0]) & (recs[:, 1] == recs[k, 1])))
            pytest.fail("build %s, block %d: %d mismatches, by op %s.  First: case %d (number %d of its run) op %s modulus %s aux %d\n"
                        "  operands %s\n  differing result words %s\n  got  %s\n  want %s" % (
                            build, block, int(bad.sum()), per_op, k, k - first, D.OP_NAMES[int(recs[k, 0])],
                            "Fq" if recs[k, 1] else "Fr", int(recs[k, 2]), [hex(int(w)) for w in opnd], words,
                            [hex(int(w)) for w in got[b, k][mask[k]]], [hex(int(w)) for w in want[k][mask[k]]]))
    assert np.array_equal(got[0][mask], got[1][mask])
