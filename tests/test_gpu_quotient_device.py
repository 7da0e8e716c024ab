"""The eight instantiations of csrc/quotient.hip — quotient_kernel and quotient_sliced_kernel, over the whole extended domain or
over three cosets, storing or accumulating — run directly (tests/quotient_device_check.hip) with any log_slices, on operands at
the bounds of the lazy 9 x 29-bit arithmetic, with the 32-term folds of q_acc reached up to nine times per sum.

The harness runs once, as a child process under its own time limit, over the data sets of tests/quotient_cases.py: every launch
form of every data set.  Every row of every launch must equal the plain-integer reference exactly, and the 256 guard rows on either
side of `out` must be unchanged.  What the set reaches is asserted by tests/test_quotient_cases.py from the term-count model alone
(no GPU).  The harness also prints quotient_log_slices for log_ext 8 .. 26 and 1 .. 352 gates; the model's restatement must agree.

Measured on an MI355X host (MEASURED below): 116 data sets, 2864 launches (2 to 40 launch forms per data set); generating the cases
and the expected rows of every launch takes 7.3 s of Python on the CPU; the harness run (process start to exit, 97 MB of cases
read, every `out` with its guards written) takes 1.5 s of wall time.

Checked against the test: harness variants with one arithmetic change each (never an index or a grid), run once.
  sub29<33> -> sub29<17> on l_0 (1 - z_0)           red in 1224 of 2192 launches (every all-(p - 1) round, most mixed ones)
  delta handed over without the factor 32           red in 1680 of 2192 launches
  sub29<9> -> sub29<4> on the chunk products        red in 248 of 2864 launches: the all-random rounds of exactly the shapes
                                                    whose last chunk holds one column (K = 4 is enough for longer chunks)
  no fold (the 32nd-term product removed)           red in 6 of 2864 launches: the widest legal key (302 gate terms in one lane),
  fold once, counter never reset                    all p - 1, divided by a stored t_inv of p - 1 — and green everywhere else,
                                                    the 96- to 264-term shapes included
The last two say what the fold is for.  A term is a product by a canonical power of y: (e y + m p) / 2^261 with m spread evenly,
so it lies below 1.09 p and near p / 2 on average — not at the 2p of its bound.  The top limb has three spare bits, so an unfolded
sum of 300 terms still holds its value; what fails is the last product of the row, which leaves the carry-free field below 2p
only while the row total is below 169 p.  With real operands that takes some 250 terms in one lane: the fold is needed for
the widest keys and for the bound to be provable, and no operand choice shows its absence at 96 terms.
"""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import quotient_cases as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]  # build.sh's
# on an MI355X host: data sets, launches, CPU seconds to generate the cases and the reference, wall seconds of the harness run
MEASURED = {"data_sets": 116, "launches": 2864, "generate_seconds": 7.3, "harness_wall_seconds": 1.5}
RUN_TIMEOUT = 120


def _binary():
    """build.sh makes the harness; a missing one is built here when hipcc is on the path.  Neither: fail."""
    exe = os.path.join(HERE, "quotient_device_check")
    if os.path.isfile(exe):
        return exe
    hipcc = shutil.which("hipcc")
    assert hipcc, "%s is missing (build.sh makes it) and there is no hipcc on the path to build it" % exe
    subprocess.check_call([hipcc] + FLAGS + ["-I", os.path.join(ROOT, "webauthn-halo2_amd", "csrc"),
                                             os.path.join(HERE, "quotient_device_check.hip"), "-o", exe])
    return exe


@pytest.mark.gpu
def test_every_quotient_kernel_form_against_the_reference(tmp_path):
    t0 = time.process_time()
    sets = Q.build_sets()
    want = {(si, li): Q.expected(ds, l) for si, ds in enumerate(sets) for li, l in enumerate(ds.launches)}
    gen = time.process_time() - t0
    case_file, out = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    Q.write_case_file(sets, case_file)
    exe = _binary()
    t0 = time.perf_counter()
    r = subprocess.run([exe, case_file, out], capture_output=True, text=True, timeout=RUN_TIMEOUT)
    wall = time.perf_counter() - t0
    print("%d data sets, %d launches; cases and reference %.1f s of CPU; harness wall time %.2f s; %s" % (
        len(sets), len(want), gen, wall, r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""))
    assert r.returncode == 0, "harness failed (%d): %s%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:])

    # the product's choice of lanes per row, as compiled
    table = {int(ln.split()[1]): ln.split()[2] for ln in r.stdout.splitlines() if ln.startswith("ls ")}
    assert sorted(table) == list(range(8, 27))
    for le, digits in table.items():
        assert digits == "".join(str(Q.quotient_log_slices(le, g)) for g in range(1, Q.MAX_ADV + 1)), "quotient_log_slices at log_ext %d" % le

    got = Q.read_result_file(out, sets)
    assert set(got) == set(want)
    canary = np.uint32(Q.CANARY)
    bad, guards = [], []
    for (si, li), (before, rows, after) in sorted(got.items()):
        ds, l = sets[si], sets[si].launches[li]
        if not ((before == canary).all() and (after == canary).all()):
            guards.append((si, li))
        miss = (rows != want[(si, li)]).any(axis=1)
        if miss.any():
            bad.append((si, li, int(miss.sum()), int(np.argmax(miss))))
    def describe(si, li):
        ds, l = sets[si], sets[si].launches[li]
        eff = Q.effective_log_slices(ds.log_ext, l.log_slices, l.c3)
        return "%s (A %d, L %d) log_ext %d %s: %s %s divide %d log_slices %d (%s), lane terms %s" % (
            ds.name, ds.lay.A, ds.lay.L, ds.log_ext, ds.round_kind, "ACC" if l.acc else "plain", "C3" if l.c3 else "4n", l.divide, l.log_slices,
            "%d lanes" % (1 << eff) if eff else "one lane per row", Q.launch_terms(ds.lay, ds.log_ext, l.log_slices, l.c3))
    assert not guards, "%d launches wrote outside `out`; first: %s" % (len(guards), describe(*guards[0]))
    if bad:
        si, li, cnt, row = bad[0]
        pytest.fail("%d of %d launches differ from the reference.  First: %s\n  %d rows differ, first row %d\n  got  %s\n  want %s\n  all: %s" % (
            len(bad), len(want), describe(si, li), cnt, row, [hex(int(w)) for w in got[(si, li)][1][row]],
            [hex(int(w)) for w in want[(si, li)][row]], "; ".join(sorted({"%s/%d" % (sets[s].name, sets[s].log_ext) for s, _, _, _ in bad}))))
