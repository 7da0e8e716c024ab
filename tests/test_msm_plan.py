"""The MSM plan rules (csrc/msm_plan.h) on the host: tests/msm_plan_check.cpp, built with the host compiler under ASan + UBSan,
walks both modes over every log n, ZK_OPT_MSM_WINDOW value and pass width, asserts the kernels' invariants and the documented
defaults, and prints one line per combination; the lines equal the Python restatement of tests/msm_cases.py.  It then walks
every workspace get_msm_ws can make and asserts that no launcher of msm.hip reaches beyond a buffer of its plan's layout (`ws `
lines).  No GPU."""
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


def test_every_workspace_holds_its_own_plan_only_and_prints_its_size(plan_output):
    """One `ws ` line per (mode, log n, ZK_OPT_MSM_WINDOW, pass width in {default, 1, 3, 8, 256}); the bounds themselves are the
    program's assertions (test_msm_plan_invariants_and_documented_defaults).  Here: wide exactly where the fixed-base plan line says
    so, never for arbitrary bases — 15 bits over 2^21 points included — and a k = 19 workspace of two columns well under the 1.1 GiB
    it took when it carried both plans' buffers."""
    ws = [dict(t.split("=") for t in ln.split()[2:]) | {"mode": ln.split()[1]} for ln in plan_output.stdout.splitlines() if ln.startswith("ws ")]
    assert len(ws) == len(MC.PLAN_LOG_N) * (len(MC.PLAN_OVERRIDES) * 5 + 1)
    for w in ws:
        if w["mode"] == "generic":
            assert w["plan"] == "generic" and w["cols"] == "1", w
        else:
            assert (w["plan"] == "wide") == MC.plan("fixed", 1 << int(w["lg"]), int(w["ov"]))["wide"], w
        assert int(w["largest"].split(":")[1]) <= int(w["bytes"]) and w["largest"].split(":")[0] in ("slot_pt", "w_part", "entries", "digits", "inter", "part", "counts"), w
    assert [w["c"] for w in ws if w["mode"] == "generic" and w["lg"] == "21"] == ["15"]
    k19 = [w for w in ws if w["mode"] == "fixed" and (w["lg"], w["ov"], w["req"]) == ("19", "0", "0")]
    assert len(k19) == 1 and k19[0]["cols"] == "2" and int(k19[0]["bytes"]) < 512 << 20
