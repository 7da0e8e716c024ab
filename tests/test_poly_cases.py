"""The polynomial matrix's CPU side: the shapes of csrc/poly_plan.h through tests/poly_plan_check.cpp (built with the host compiler
under ASan + UBSan) against the Python restatement of tests/poly_cases.py, the classes the case set reaches, and its references —
the C oracle against plain Python at every length up to 2^13, against the sparse closed form and the division identity above.
No GPU."""
import os
import random
import shutil
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poly_cases as PC  # noqa: E402
from zkoracle import cops, fastprover as fp, prover  # noqa: E402
from zkoracle.field import R, omega  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "webauthn-halo2_amd", "csrc")
ALL_LENGTHS = sorted({n for n, _ in PC.lengths_eval()} | {n for n, _ in PC.lengths_kd()})


@pytest.fixture(scope="module")
def plan_output(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    exe = str(tmp_path_factory.mktemp("poly_plan") / "poly_plan_check")
    # host code only: plain C++ through hipcc's clang; the address and undefined-behaviour sanitizers go to the host side alone
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["hipcc", "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + san +
                          ["-I", CSRC, os.path.join(ROOT, "tests", "poly_plan_check.cpp"), "-o", exe])
    return subprocess.run([exe] + [str(n) for n in ALL_LENGTHS], capture_output=True, text=True, timeout=120)


def test_poly_plan_invariants(plan_output):
    """Every n in 1 .. 2^16 and 2^j + d, j in 16 .. 26, |d| <= 8: the strides reach n, 256 M blocks >= n, the non-empty batch
    workgroups cover [0, n) exactly, at most KD_TOP blocks, the partial results fit the context's small, the scratch formula covers
    the layout — and a clean run under the sanitizers."""
    assert plan_output.returncode == 0 and "0 failures" in plan_output.stdout, plan_output.stdout[-4000:] + plan_output.stderr[-4000:]
    assert "runtime error" not in plan_output.stderr and "AddressSanitizer" not in plan_output.stderr
    walked = int(plan_output.stdout.rsplit("poly plan: ", 1)[1].split()[0])
    assert walked == (1 << 16) + 11 * 17 - 9 - 8  # (2^16 - 8 .. 2^16 are in the first walk, 2^26 + 1 .. + 8 are not accepted)


def test_poly_plan_header_agrees_with_the_python_restatement(plan_output):
    got = [ln for ln in plan_output.stdout.splitlines() if ln.startswith("n=")]
    want = [PC.plan_line(n) for n in ALL_LENGTHS]
    assert len(got) == len(want) == len(ALL_LENGTHS)
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, diff[:5]


def test_restatement_landmarks():
    """The shapes the issue of this matrix names, from the restatement: where M, the empty workgroups, KD_L and the block counts
    change."""
    assert PC.plan_line(128) == "n=128 blocks=1 S=256 M=1 wg=1 live=128 L=8 m=16 nblk=1 scratch=290"
    n = (1 << 22) + 1
    assert (PC.eval_blocks(n), PC.eval_batch_per_lane(n), PC.eval_batch_workgroups(n)) == (1024, 17, (964, 256))
    assert PC.eval_batch_live(n, 17, 964) == 0 and PC.eval_batch_live(n, 17, 1023) == 0
    assert PC.eval_batch_per_lane(1 << 22) == 16 and PC.eval_batch_workgroups(1 << 22) == (1024, 256)
    assert PC.eval_blocks(70000) == 18 and PC.eval_blocks((1 << 20) + 4097) == 258
    assert [PC.kd_shape(x)[:3] for x in (2048, 2049, (1 << 19) + 1, 1 << 21, (1 << 21) + 1, (1 << 22) + 1, 1 << 26)] == [
        (8, 256, 1), (8, 257, 2), (8, 65537, 257), (8, 1 << 18, 1024), (16, 131073, 513), (32, 131073, 513), (256, 1 << 18, 1024)]
    assert PC.eval_blocks(1 << 26) + 1 <= PC.EVAL_SMALL_ELEMS


def test_every_class_is_in_the_case_set():
    """Counted from the restatement alone; the counts are pinned so that a later edit cannot drop a class."""
    ev, kd = PC.lengths_eval(), PC.lengths_kd()
    assert [n for n, _ in ev] == [1, 2, 100, 129, 255, 256, 257, 4095, 4096, 4097, 4196, 8193, (1 << 20) + 4097, (1 << 22) - 1, 1 << 22,
                                  (1 << 22) + 1]
    assert [n for n, _ in kd] == [1, 2, 7, 8, 9, 2041, 2047, 2048, 2049, 4104, (1 << 19) - 1, (1 << 19) + 1, (1 << 21) - 7, 1 << 21,
                                  (1 << 21) + 1, (1 << 21) + 8, (1 << 22) + 1]
    for n, tag in ev:
        assert tag in PC.classes_eval(n), (n, tag, PC.classes_eval(n))
    for n, tag in kd:
        assert tag in PC.classes_kd(n), (n, tag, PC.classes_kd(n))
    ce = Counter(c for n, _ in ev for c in PC.classes_eval(n))
    assert ce == {"one_workgroup": 9, "several_workgroups": 7, "M1": 6, "M9": 2, "M17": 1, "ragged_live": 3, "unequal_chains": 7,
                  "over_256_partials": 4, "block_cap": 3, "empty_workgroups": 1, "over_18_blocks": 4}, ce
    ck = Counter(c for n, _ in kd for c in PC.classes_kd(n))
    assert ck == {"single_chunk": 4, "short_last_chunk": 13, "m256": 3, "m257": 1, "single_chunk_last_block": 6, "nblk2": 1,
                  "nblk256": 1, "nblk257": 1, "nblk1024": 2, "L8_longest": 1, "L16": 2, "L32": 1}, ck
    assert set(ce) == set(PC.EVAL_CLASSES) and set(ck) == set(PC.KD_CLASSES)
    # the subsets of the GPU matrix
    assert PC.EVAL_LARGE == [(1 << 20) + 4097, (1 << 22) - 1, 1 << 22, (1 << 22) + 1] and len(PC.EVAL_SMALL) == 12
    assert PC.KD_FEW_Z == [(1 << 21) - 7, 1 << 21, (1 << 21) + 1, (1 << 21) + 8, (1 << 22) + 1] and len(PC.KD_ALL_Z) == 12
    assert set().union(*(PC.classes_eval(n) for n in PC.AUDIT_EVAL)) == set(PC.EVAL_CLASSES)
    assert set().union(*(PC.classes_kd(n) for n in PC.AUDIT_KD)) == set(PC.KD_CLASSES)
    assert set(PC.AUDIT_EVAL) <= {n for n, _ in ev} and set(PC.AUDIT_KD) <= {n for n, _ in kd}


def test_points_are_what_they_are_called():
    for n in ALL_LENGTHS:
        p = dict(PC.points(n))
        assert len(p) == 11 and (p["zero"], p["one"], p["minus_one"], p["two"]) == (0, 1, R - 1, 2)
        for name, order in (("w8", 8), ("w256", 256), ("w2048", 2048)):
            assert pow(p[name], order, R) == 1 and pow(p[name], order // 2, R) == R - 1
        S = PC.eval_stride(n)
        assert pow(p["w_stride"], S, R) == 1 and p["w_stride"] != 1 and pow(p["w_stride"], (S & -S) // 2, R) == R - 1
        assert len({p["random%d" % i] for i in range(3)}) == 3
        assert [k for k, _ in PC.points_few_eval(n)] == ["zero", "one", "w_stride", "random0"]
        assert [k for k, _ in PC.points_few_kd(n)] == ["zero", "one", "w8", "w2048", "random0"]
    # the multipliers that become one: Z = z^KD_L at w8, Z^256 at w2048, y = x^256 at w256
    assert pow(omega(3), 8, R) == 1 and pow(pow(omega(11), 8, R), 256, R) == 1 and pow(omega(8), 256, R) == 1


def test_sparse_vectors_sit_on_the_seams():
    one = PC.mont1(1)
    for n in ALL_LENGTHS:
        s = PC.seams(n)
        assert s == sorted(set(s)) and s[0] == 0 and s[-1] == n - 1 and all(0 <= i < n for i in s)
        M = PC.eval_batch_per_lane(n)
        wg, _ = PC.eval_batch_workgroups(n)
        L, m, nblk, _ = PC.kd_shape(n)
        first_of_last = (wg - 1) * 256 * M
        for i in (255, 256, first_of_last - 1, first_of_last, first_of_last + 255, first_of_last + 256, PC.eval_stride(n) - 1,
                  PC.eval_stride(n), L - 1, L, (m - 1) * L - 1, (m - 1) * L, 256 * L - 1, 256 * L, (nblk - 1) * 256 * L - 1,
                  (nblk - 1) * 256 * L):
            assert (i in s) == (0 <= i < n), (n, i)
        if n <= 8193:
            a = PC.coefficients(n, "sparse")
            assert [i for i in range(n) if a[i].any()] == s and all(np.array_equal(a[i], one) for i in s)
    assert cops.fr_ints(PC.coefficients(5, "max")) == [R - 1] * 5 and not PC.coefficients(5, "zero").any()
    a = PC.coefficients(300, "random")
    assert np.array_equal(a, PC.coefficients(300, "random")) and all(v < R for v in cops.arr_to_ints(a))


def test_table_pairs_fill_overflow_and_hit_the_table():
    """Restating launch_eval_batch's table of 16 distinct points over the pairs of each count: every launch of 64 that has more than
    16 pairs fills it, the counts of 18 and more meet a point behind the full table (computed again) and a point in it (copied)."""
    pts = PC.table_points(0)
    assert len(set(pts)) == 20
    order = PC.table_order()
    assert len(order) == 40 and Counter(order) == Counter({i: 2 for i in range(20)}) and order[:16] == list(range(16))
    assert order[16:24] == [16, 0, 17, 1, 18, 2, 19, 3]
    for count in PC.TABLE_COUNTS:
        pairs = PC.table_pairs(count, 3, pts)
        assert len(pairs) == count
        full = hit = again = 0
        for i0 in range(0, count, PC.EVAL_BATCH_PAIRS):
            table, seen = [], set()
            for _, x in pairs[i0:i0 + PC.EVAL_BATCH_PAIRS]:
                if x in table:
                    hit += 1
                elif len(table) < PC.EVAL_TABLE:
                    table.append(x)
                else:
                    full += 1
                    again += x in seen
                seen.add(x)
        assert (full >= 1) == (count >= 17) and (hit >= 1) == (count >= 18), (count, full, hit)
        if count >= 64:
            assert again >= 4 and hit >= 12, (count, again, hit)
    # a staging slot that is used by several calls holds another point in each of its first uses per call
    for i in range(18):
        uses = [PC.table_pairs(c, 3, pts)[i][1] for c in PC.TABLE_COUNTS if c > i]
        assert len(set(uses)) == len(uses), i


def test_c_oracle_equals_plain_python_up_to_2_13():
    """fastprover.eval_poly and kate_division against the plain-Python forms at every length of the set up to 2^13, every point and
    kind (the references of the GPU matrix switch between the two at 2^13)."""
    for n in [x for x in ALL_LENGTHS if x <= PC.PLAIN_MAX]:
        for kind in PC.KINDS:
            a = PC.coefficients(n, kind)
            ints = cops.fr_ints(a)
            for name, x in PC.points(n):
                assert fp.eval_poly(a, x) == prover.eval_poly(ints, x) == PC.eval_ref(a, x), (n, kind, name)
                q = fp.kate_division(a, x)
                assert cops.fr_ints(q) == prover.kate_division(ints, x) + [0], (n, kind, name)
                assert np.array_equal(q, PC.kd_ref(a, x))
                if kind == "sparse":
                    assert PC.eval_ref(a, x) == PC.sparse_value(n, x), (n, name)


@pytest.mark.parametrize("n", [x for x in ALL_LENGTHS if x > PC.PLAIN_MAX])
def test_c_oracle_at_the_large_lengths(n):
    """Above 2^13 the C oracle is the reference: it satisfies the sparse closed form (sum x^i by pow) at every point, and its
    quotients the identity p(x) = q(x) (x - z) + p(z) at two random x, for the random and the sparse vector."""
    rng = random.Random(n)
    sparse = PC.coefficients(n, "sparse")
    for name, x in PC.points(n):
        assert fp.eval_poly(sparse, x) == PC.sparse_value(n, x), (n, name)
    rnd = PC.coefficients(n, "random")
    xs = [rng.randrange(R) for _ in range(2)]
    for a in (rnd, sparse):
        for name, z in PC.points_few_kd(n)[0 if a is rnd else 3:]:
            q = fp.kate_division(a, z)
            assert not q[n - 1].any() and PC.division_identity_holds(a, q, z, xs), (n, name)
