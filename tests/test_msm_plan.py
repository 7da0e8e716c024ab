"""The MSM plan rules (csrc/msm_plan.h) on the host: tests/msm_plan_check.cpp, built with the host compiler under ASan + UBSan,
walks both modes over every log n, ZK_OPT_MSM_WINDOW value and pass width, asserts the kernels' invariants and the documented
defaults, and prints one line per combination; the lines equal the Python restatement of tests/msm_cases.py.  No GPU."""
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_cases as MC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "webauthn-halo2_amd", "csrc")


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    exe = str(tmp_path_factory.mktemp("msm_plan") / "msm_plan_check")
    # host code only: plain C++ through hipcc's clang; the address and undefined-behaviour sanitizers go to the host side alone
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["hipcc", "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + san +
                          ["-I", CSRC, os.path.join(ROOT, "tests", "msm_plan_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def plan_output(plan_check):
    out = subprocess.run([plan_check], capture_output=True, text=True, timeout=120)
    return out


def test_msm_plan_invariants_and_documented_defaults(plan_output):
    """nwin c >= 255; sort2 only with 24-bit table indexes and <= CBINS_MAX coarse bins; 16 / 17 bits only on the wide path; widest
    pass 1 wherever msm_run refuses a wider one; 16 bits at 2^16 .. 2^21, 15 from 2^22, lg - 5 (at least 9) below, 14 instead of
    15 .. 17 under the 1024 floor — and a clean run under the sanitizers."""
    assert plan_output.returncode == 0 and "msm plan: 0 failures" in plan_output.stdout, plan_output.stdout[-4000:] + plan_output.stderr[-4000:]
    assert "runtime error" not in plan_output.stderr and "AddressSanitizer" not in plan_output.stderr


def test_msm_plan_header_agrees_with_the_python_restatement(plan_output):
    got = [ln for ln in plan_output.stdout.splitlines() if ln.startswith(("fixed ", "generic "))]
    want = MC.plan_lines()
    assert len(got) == len(want) == len(MC.PLAN_LOG_N) * (len(MC.PLAN_OVERRIDES) * len(MC.PLAN_WIDTHS) + 1)
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, diff[:5]


def test_widest_pass_is_one_where_msm_run_refuses_more(plan_output):
    """The k >= 22 refusal: every fixed-base plan that is neither wide nor fused answers 1 whatever width is asked for, and
    only those do."""
    seen = 0
    for ln in plan_output.stdout.splitlines():
        if not ln.startswith("fixed "):
            continue
        f = dict(t.split("=") for t in ln.split()[1:])
        if f["wide"] == "0" and f["fused"] == "0":
            seen += 1
            assert f["pass"] == "1" and int(f["lg"]) >= 22 and f["c"] == "15", ln
        elif f["req"] != "0":
            assert f["pass"] == f["req"], ln
    assert seen == 5 * len(MC.PLAN_WIDTHS) * 4  # lg 22 .. 26 x overrides {0, 15, 16, 17}
