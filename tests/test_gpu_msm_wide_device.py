"""The wide MSM path (csrc/msm_wide.hip.h) stage by stage at every entry layout, on the device: tests/msm_wide_device_check.hip
(built by build.sh with -DZK_MSM_POISON) runs the passes of tests/msm_wide_cases.py on workspaces and tables of stride 2^12,
2^20 and 2^21 — over columns of a few hundred scalars — ONCE, as a child process under its own time limit, and writes out
every buffer of every pass; tests/msm_wide_model.py states what each must hold.  One test per geometry and stage.

Which case reaches which branch of msm_wide.hip.h (the conditions are asserted without a GPU by tests/test_msm_wide_cases.py):
  wide_binscan, top = min(63, keys - 1)        keys = 128: (15|16|17, 2^12); keys = 64: (15, 2^20), (16, 2^21); keys = 32:
                                               (15, 2^21) — every column of those geometries
  wide_binscan, the wave == 1 seam (128 keys)  "ladder": buckets 62 / 63 / 64 / 65 of one bin, and a bin whose only bucket is 127
  the escape test d < esc                      "ladder": gaps esc - 1, esc, esc + 1 and 0 inside one bin, a bin's first bucket in
                                               bin 0, a middle bin and the last bin; "sparse" (msm_cases): whole bins empty
  hist[128] / kid / keys in the part regions   "one bucket" (4096 entries and one scalar more: one full sort chunk, and a second;
                                               640 scalars: more than 64 parts, a second head), "halves" (bucket nb - 1), "bool"
  the spare block of msm_wscatter2             "zero", "ladder", "edges": bins without entries
  msm_wbucket_kernel, len <= lmax              "seam": buckets of 23, 24, 25 and 26 slots under T1 mode 1 and mode 0
  msm_wrowcol / msm_wbits weights              "edges": buckets 0, 255, 256, 257, nb - 256, nb - 1, column 255 of every row
  msm_wacc_fast -> msm_wacc_redo               "equal points", "opposite points", "identity sum" over the degenerate basis, unchecked
  msm_wacc (SAFE)                              the same checked, and the basis with identity points
  the two counter sets, used_cols              pass widths 3 1 3, 1 2 1 1 3, 2 empty 2; a 1100-scalar pass followed by n = 17

Measured on an MI355X (two runs): the harness 1.1 - 1.2 s of wall time for all six geometries, the module 19 - 26 s (the rest
is the reference: every expected point is an oracle scalar multiplication).  Per geometry — passes, bytes allocated (workspace,
table, columns), harness time, reference time:
  (15, 2^12)   29   0.033 GB    76 -  95 ms   2.9 s        (15, 2^20)   27   2.455 GB    86 - 110 ms   2.3 s
  (15, 2^21)   27   4.886 GB   119 - 219 ms   2.1 s        (16, 2^12)   29   0.055 GB   124 - 136 ms   3.1 s
  (16, 2^21)   27   4.635 GB   100 - 180 ms   2.4 s        (17, 2^12)   29   0.101 GB   182 - 222 ms   3.9 s
Every stage of every geometry agreed with the model at its first run; no escape is taken where the distance field would do
(the head check asserts the field itself).
"""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import msm_wide_cases as C
import msm_wide_model as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result", "-DZK_MSM_POISON"]
RUN_TIMEOUT = 120
GEO_IDS = ["c%d-2^%d" % (c, S.bit_length() - 1) for c, S in C.GEOMETRIES]


def _binary():
    """build.sh makes it; a missing one is built here when hipcc is on the path.  Neither: fail."""
    exe = os.path.join(HERE, "msm_wide_device_check")
    if os.path.isfile(exe):
        return exe
    hipcc = shutil.which("hipcc")
    assert hipcc, "%s is missing (build.sh makes it) and there is no hipcc on the path to build it" % exe
    subprocess.check_call([hipcc] + FLAGS + ["-I", os.path.join(ROOT, "webauthn-halo2_amd", "csrc"), os.path.join(HERE, "msm_wide_device_check.hip"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp("msm_wide_device")
    cases, out = str(d / "cases.bin"), str(d / "results.bin")
    C.write_case_file(cases)
    t0 = time.perf_counter()
    r = subprocess.run([_binary(), cases, out], capture_output=True, text=True, timeout=RUN_TIMEOUT)
    print("msm_wide_device_check: wall time %.2f s\n%s" % (time.perf_counter() - t0, r.stdout.strip()))
    assert r.returncode == 0, "the harness failed (%d): %s%s" % (r.returncode, r.stdout, r.stderr)
    geos = W.parse_results(np.fromfile(out, dtype="<u4"))
    os.remove(out)  # (a few hundred megabytes)
    assert sorted(geos) == list(range(len(C.GEOMETRIES))), "result file malformed"
    return geos


@pytest.fixture(scope="module")
def verdicts(dumps):
    """geometry -> {stage: [errors]}, every pass of a geometry checked once, on first use"""
    done = {}

    def of(gi):
        if gi not in done:
            c, S = C.GEOMETRIES[gi]
            g, G, t0 = W.Geo(c, S), dumps[gi], time.perf_counter()
            out = {s: [] for s in W.STAGES}
            got = (G.info.ib, G.info.fb, G.info.bins, G.info.rows, G.info.row_bits, G.info.lane_stride, G.info.slot_stride, G.info.part_stride, G.info.wl)
            want = (g.ib, g.fb, g.bins, g.rows, g.row_bits, g.lane_stride, g.slot_stride, g.part_stride, W.WL)
            if got != want:
                out["head"].append("the workspace's layout is %s, the model's %s" % (got, want))
            ps = C.passes(c, S)
            assert sorted(G.passes) == list(range(len(ps))), "result file malformed"
            pts = W.Points()  # the expected points of the whole geometry: one oracle call
            par = 0
            for pi, p in enumerate(ps):
                par ^= 1 if p.n else 0
                for stage, errs in W.check_pass(g, C.bases()[p.basis], p, G.passes[pi], pts, "pass %d %s: " % (pi, p.kinds), par).items():
                    out[stage] += ["pass %d %s: %s" % (pi, p.kinds, e) for e in errs]
            for label in pts.failures():
                out[W.stage_of(label)].append(label)
            print("(%d, 2^%d): harness %d ms, %.3f GB allocated; reference %.2f s" % (c, S.bit_length() - 1, G.info.ms, G.info.bytes / 1e9, time.perf_counter() - t0))
            done[gi] = out
        return done[gi]

    return of


@pytest.mark.gpu
@pytest.mark.parametrize("stage", W.STAGES)
@pytest.mark.parametrize("gi", range(len(C.GEOMETRIES)), ids=GEO_IDS)
def test_stage_matches_the_model(verdicts, gi, stage):
    errs = verdicts(gi)[stage]
    assert not errs, "%d disagreements with the model, the first: %s" % (len(errs), errs[:6])
