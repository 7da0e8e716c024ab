"""csrc/p256.hip.h on the device (tests/p256_device_check.hip, built by build.sh): the field operations of both moduli at the
2^256 carry - sums that carry out of 256 bits, Montgomery totals in [m, 2^256) and above 2^256 -, the point operations at
every exceptional case, and the x-compare's two clauses.  One case per lane, the whole set launched in blocks of 64 and of 256
lanes, run ONCE as a child process under its own time limit; results are compared with Python integers (tests/p256_cases.py,
whose class counts tests/test_es256_ref.py asserts without a GPU).
"""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import p256_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]
RUN_TIMEOUT = 120


def _binary():
    """build.sh makes it; a missing one is built here when hipcc is on the path.  Neither: fail."""
    exe = os.path.join(HERE, "p256_device_check")
    if os.path.isfile(exe):
        return exe
    hipcc = shutil.which("hipcc")
    assert hipcc, "%s is missing (build.sh makes it) and there is no hipcc on the path to build it" % exe
    subprocess.check_call([hipcc] + FLAGS + ["-I", os.path.join(ROOT, "webauthn-halo2_amd", "csrc"), os.path.join(HERE, "p256_device_check.hip"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("p256_device")
    cases, out = str(d / "cases.bin"), str(d / "results.bin")
    n = C.write_case_file(cases)
    t0 = time.perf_counter()
    r = subprocess.run([_binary(), cases, out], capture_output=True, text=True, timeout=RUN_TIMEOUT)
    print("p256_device_check: wall time %.2f s; %s" % (time.perf_counter() - t0, r.stdout.strip()))
    assert r.returncode == 0, "the harness failed (%d): %s%s" % (r.returncode, r.stdout, r.stderr)
    raw = np.fromfile(out, dtype="<u4")
    assert raw[:4].tolist() == [C.MAGIC_OUT, n, C.OUT_WORDS, 2] and raw.size == 4 + 2 * n * C.OUT_WORDS, "result file malformed"
    return raw[4:].reshape(2, n, C.OUT_WORDS)


@pytest.mark.gpu
@pytest.mark.parametrize("pass_", [0, 1], ids=["blocks-of-64", "blocks-of-256"])
def test_device_forms_against_python_integers(results, pass_):
    C.assert_classes(C.build()[2])
    C.check_results(results[pass_], "blocks of %d" % (64, 256)[pass_])


@pytest.mark.gpu
def test_both_block_sizes_agree_to_the_bit(results):
    assert np.array_equal(results[0], results[1])
