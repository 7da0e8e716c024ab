"""csrc/placement.h, the host logic of zk_stream_placement, on made-up time stamps (tests/placement_logic_check.cpp): four classes
of ten streams, two classes, every stream on its own queue (unresolved after nine classes), an ambiguous stamp (one repeat, then
unresolved), and the deal on the layouts the documented runtime rule gives after 0 .. 5 foreign streams - all four invariants
afterwards, more streams asked for when a class is short, nothing dealt unless four classes were seen.  Plain g++: the header
needs no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_placement_logic(tmp_path):
    exe = str(tmp_path / "placement_logic_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "webauthn-halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "placement_logic_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "placement logic: 0 failures" in out.stdout, out.stdout + out.stderr


def test_report_struct_matches_the_binding():
    """The ctypes mirrors of zk_placement / zk_ctx_streams have the C structs' sizes and field offsets."""
    import ctypes
    import tempfile

    from webauthn_halo2_amd import engine as E

    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "zkmi355.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", '
           "sizeof(zk_placement), offsetof(zk_placement, main_queue), offsetof(zk_placement, role_queue), offsetof(zk_placement, spare_queue), "
           "offsetof(zk_placement, rounds), offsetof(zk_placement, probe_ms), sizeof(zk_ctx_streams), offsetof(zk_ctx_streams, counts)); return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, timeout=60).stdout.split()]
    P, S = E.PlacementC, E.CtxStreamsC
    assert got == [ctypes.sizeof(P), P.main_queue.offset, P.role_queue.offset, P.spare_queue.offset, P.rounds.offset, P.probe_ms.offset,
                   ctypes.sizeof(S), S.counts.offset]
