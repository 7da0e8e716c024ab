"""The device pairing harness without a GPU: the class counts of tests/pairing_device_cases.py, and the harness's --host mode (the
same per-case code as the device kernel, tests/pairing_check_ops.h, compiled for the CPU in the same binary; no device is opened)
against the Python integers of tests/pairing_ref.py — every word of every result, every DONE marker, and the bytes of the tables
pairing_table_make prepared against the reference's own walk of the G2 points.  This ties the reference to the host compile of
csrc/pairing.h's shared half, and with it to the host pairing tests/test_pairing_lines.py holds equal to it (the one zk_verify,
zk_srs_update and the SRS check use).  What it cannot see is the device compile: tests/test_gpu_pairing_device.py runs that.
"""
import os
import subprocess

import pytest

import pairing_device_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
RUN_TIMEOUT = 120


def test_case_set_covers_every_class():
    per_op = C.assert_classes()
    assert sum(per_op.values()) == C.build()["recs"].shape[0]


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("pairing_host")
    cases, out, tables = str(d / "cases.bin"), str(d / "results.bin"), str(d / "tables.bin")
    C.write_case_file(cases)
    r = subprocess.run([C.binary(), "--host", cases, out, tables], capture_output=True, text=True, timeout=RUN_TIMEOUT)
    assert r.returncode == 0, "the harness failed (%d): %s%s" % (r.returncode, r.stdout, r.stderr)
    return C.read_results(out, 1), tables


def test_host_mode_equals_the_reference(host_run):
    C.check_results(host_run[0][0], "host mode")


def test_every_case_wrote_its_marker(host_run):
    got, want = host_run[0][0], C.build()["expect"]
    assert (got[:, C.OUT_WORDS - 1] == want[:, C.OUT_WORDS - 1]).all()


def test_prepared_tables_equal_the_references_walks(host_run):
    C.check_tables(host_run[1])


def test_layouts_match_the_header():
    txt = open(os.path.join(HERE, "pairing_check_ops.h")).read()
    for name, val in (("F12_WORDS = 96", C.F12_WORDS), ("OPND = 4", C.OPND), ("DONE = 0x600d0000u", C.DONE), ("MAGIC_IN = 0x43524150u", C.MAGIC_IN),
                      ("MAGIC_OUT = 0x52524150u", C.MAGIC_OUT), ("MAGIC_TAB = 0x54524150u", C.MAGIC_TAB)):
        assert name in txt and int(name.split("= ")[1].rstrip("u"), 0) == val, name
    assert C.REC_WORDS == 228 and C.OUT_WORDS == 98
    for name in ("OP_F2_MUL = 1", "OP_F6_MUL = 10", "OP_F12_MUL = 20", "OP_FQ_CANON = 40"):
        assert name in txt
