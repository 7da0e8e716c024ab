"""csrc/pairing.h on the device (tests/pairing_device_check.hip, built by build.sh), value for value: the Fq2 / Fq6 / Fq12 tower at
zero and p - 1 coefficients, single positions, the subfields and the sums that cancel inside each Karatsuba level; the Frobenius
map with its constants read from the table in device memory; the sparse line product at the first, last, Frobenius and
doubling / addition steps of both walks; f^u; the Miller loop over prepared lines against five tables (two of them with an
identity G2 point, which no public entry point can make) with identity G1 points on either side; the table-free final
exponentiation; and whole checks with all four reasons.  Expected words come from the Python integers of tests/pairing_ref.py
(tests/pairing_device_cases.py, whose class counts tests/test_pairing_device_cases.py asserts without a GPU); every comparison
is exact.  One case per lane in one-wave workgroups, the product kernel's shape.  The set runs twice: grouped by op (uniform
waves), and interleaved, where consecutive lanes carry different ops — the __noinline__ products run under partial exec masks —
and every wave has a CHECK lane that returns early beside one that runs a whole VALID check.  The harness runs ONCE as a child
process under its own time limit.

Limit: the harness compiles the device forms of pairing.h in its own translation unit, with the library's flags.  The shipped
pairing_check_kernel itself (pairing.hip) stays covered by the verdict tests of tests/test_gpu_pairing.py and
tests/test_gpu_verify_pairing.py.

Found: nothing.  Both passes equalled the reference at all 4585 cases on an MI355X, as did the --host run.  Measured wall time of
the harness run (both passes, tables, files): 0.48 s; the fixture prints it on every run.
"""
import subprocess
import time

import numpy as np
import pytest

import pairing_device_cases as C

RUN_TIMEOUT = 120
PASSES = ("grouped by op", "interleaved ops")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("pairing_device")
    cases, out, tables = str(d / "cases.bin"), str(d / "results.bin"), str(d / "tables.bin")
    C.write_case_file(cases)
    t0 = time.perf_counter()
    r = subprocess.run([C.binary(), cases, out, tables], capture_output=True, text=True, timeout=RUN_TIMEOUT)
    print("pairing_device_check: wall time %.2f s; %s" % (time.perf_counter() - t0, r.stdout.strip()))
    assert r.returncode == 0, "the harness failed (%d): %s%s" % (r.returncode, r.stdout, r.stderr)
    return C.read_results(out, 2), tables


@pytest.mark.gpu
@pytest.mark.parametrize("pass_", [0, 1], ids=["grouped", "interleaved"])
def test_device_forms_against_python_integers(run, pass_):
    C.assert_classes()
    C.check_results(run[0][pass_], PASSES[pass_])


@pytest.mark.gpu
def test_both_passes_agree_to_the_bit(run):
    assert np.array_equal(run[0][0], run[0][1])


@pytest.mark.gpu
def test_every_case_has_its_marker_in_both_passes(run):
    want = C.build()["expect"][:, C.OUT_WORDS - 1]
    for p in (0, 1):
        missing = np.nonzero(run[0][p][:, C.OUT_WORDS - 1] != want)[0]
        assert missing.size == 0, "%s: %d cases without a DONE marker, first %d" % (PASSES[p], missing.size, int(missing[0]))


@pytest.mark.gpu
def test_uploaded_tables_equal_the_references_walks(run):
    C.check_tables(run[1])
