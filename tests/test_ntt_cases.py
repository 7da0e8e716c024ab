"""The NTT matrix's CPU side: the pass planner (csrc/ntt_plan.h) over every size and option value, and tests/ntt_cases.py —
its references against the plain-Python definitions of zkoracle.prover, the impulse closed form against the oracle's
butterflies, non-standard primitive roots, the input generators.  No GPU."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ntt_cases as NC  # noqa: E402
from zkoracle import cops, prover  # noqa: E402
from zkoracle.field import R, ZETA, omega  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rand_fr(rng, n):
    return [rng.randrange(R) for _ in range(n)]


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    exe = str(tmp_path_factory.mktemp("ntt_plan") / "ntt_plan_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-x", "hip", "-I", os.path.join(ROOT, "webauthn-halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "ntt_plan_check.cpp"), "-o", exe])
    return exe


def test_ntt_plan_every_size_and_option(plan_check):
    """Every log_n in 0..26 under every ZK_OPT_NTT_MAX_RADIX_LOG2 in 0..11: the radices sum to log_n, each is >= 1, fits the tile
    and the requested maximum, the passes fit the array ntt_run plans into (the shared constant), the default plans are the table."""
    out = subprocess.run([plan_check], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "ntt plan: 0 failures" in out.stdout, out.stdout + out.stderr


def test_ntt_plan_check_rejects_an_eight_entry_array(plan_check):
    """The check has teeth: against the eight entries ntt_run used to plan into it names the first overrun of each option value —
    (1, 9), (2, 17), (3, 25) — and no pair of a value of 4 or more."""
    out = subprocess.run([plan_check, "8"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1
    over = {}
    for line in out.stdout.splitlines():
        if "overrun an array of 8" in line:
            opt, log_n = (int(t.split()[-1]) for t in line.split(":")[2].split(",")[:2])
            over.setdefault(opt, []).append(log_n)
    assert {o: min(v) for o, v in over.items()} == {1: 9, 2: 17, 3: 25}
    assert over[1] == list(range(9, 27)) and over[2] == list(range(17, 27)) and over[3] == [25, 26]
    assert sum(len(v) for v in over.values()) == int(out.stdout.rsplit("ntt plan: ", 1)[1].split()[0])


def test_default_first_radix_matches_plan_table():
    want = {0: 0, 1: 1, 8: 8, 9: 5, 10: 5, 16: 8, 17: 9, 18: 9, 19: 10, 20: 10, 21: 7, 22: 6, 23: 6, 24: 6, 25: 7, 26: 7}
    assert {k: NC.default_first_radix_log2(k) for k in want} == want
    assert NC.impulse_positions(9) == [0, 1, 16, 17, 256, 511] and NC.impulse_positions(0) == [0] and NC.impulse_positions(1) == [0, 1]


def test_canonical_random_is_canonical_and_reaches_the_top():
    a = NC.canonical_random(np.random.default_rng(1), 1 << 12)
    v = cops.arr_to_ints(a)
    assert all(x < R for x in v) and len(set(v)) == len(v)
    assert any(x >> 253 for x in v) and any((x >> 252) == 1 for x in v) and any(x >= 1 << 252 for x in v)
    # the same generator state gives the same rows
    assert np.array_equal(a, NC.canonical_random(np.random.default_rng(1), 1 << 12))
    edge = cops.ints_to_arr([R - 1, R, R + 1, 0, (1 << 256) - 1, R - (1 << 64), R + (1 << 192)])
    assert NC.below_r(edge).tolist() == [True, False, False, True, False, True, False]


def test_structured_vectors():
    n = 10
    assert cops.arr_to_ints(NC.all_max(n)) == [R - 1] * n
    assert cops.arr_to_ints(NC.alternating_max(n)) == [R - 1, 0] * 5
    for m in range(3):
        assert cops.arr_to_ints(NC.period3_max(n, m)) == [R - 1 if i % 3 == m else 0 for i in range(n)]
    assert [cops.arr_to_ints(NC.structured(n, name))[:3] for name in NC.STRUCTURED] == [[R - 1] * 3, [R - 1, 0, R - 1], [0, R - 1, 0]]
    assert cops.fr_ints(NC.impulse(8, 5, 77)) == [0, 0, 0, 0, 0, 77, 0, 0]


@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 5, 6, 9, 10])
def test_oracle_ntt_takes_any_primitive_root(log_n):
    """cops.ntt against the recursive definition, under omega, its inverse and odd powers of it."""
    n = 1 << log_n
    a = rand_fr(random.Random(log_n), n)
    a[0] = R - 1
    am = cops.fr_mont(a)
    w0 = omega(log_n)
    for e in sorted({1, 5 % max(n, 2), n - 1, (n - 3) % max(n, 2)}):
        if n > 1 and e % 2 == 0:
            continue
        w = pow(w0, e, R)
        assert cops.fr_ints(cops.ntt(am, w, log_n)) == prover.ntt(a, w), (log_n, e)


@pytest.mark.parametrize("log_n", [0, 1, 4, 9, 10])
def test_impulse_closed_form_matches_oracle_ntt(log_n):
    n = 1 << log_n
    rng = random.Random(100 + log_n)
    for w in (omega(log_n), NC.omega_inv(log_n), pow(omega(log_n), 5, R)):
        for j in NC.impulse_positions(log_n):
            c = rng.choice([1, R - 1, rng.randrange(R)])
            assert np.array_equal(NC.impulse_response(n, j, c, w), cops.ntt(NC.impulse(n, j, c), w, log_n)), (log_n, j)


@pytest.mark.parametrize("k", [0, 1, 3, 6, 10])
def test_domain_wrappers_match_plain_definitions(k):
    n = 1 << k
    a = rand_fr(random.Random(200 + k), n)
    am = cops.fr_mont(a)
    assert cops.fr_ints(NC.lagrange_to_coeff(am, k)) == prover.lagrange_to_coeff(a, k)
    assert cops.fr_ints(NC.coeff_to_lagrange(am, k)) == prover.ntt(a, omega(k))
    assert np.array_equal(NC.lagrange_to_coeff(NC.coeff_to_lagrange(am, k), k), am)
    assert cops.fr_ints(NC.extended_to_coeff(am, k)) == prover.extended_to_coeff(a, k)


@pytest.mark.parametrize("ext_k", [2, 3, 5, 8, 10])
def test_coeff_to_extended_any_length_matches_plain_definition(ext_k):
    N = 1 << ext_k
    rng = random.Random(300 + ext_k)
    for ln in sorted({1, 3, N // 4 - 1, N // 4, N // 4 + 1, 3 * N // 16 + 5, N // 2, N} - {0}):
        if ln > N:
            continue
        c = rand_fr(rng, ln)
        cm = cops.fr_mont(c)
        keep = cm.copy()
        got = NC.coeff_to_extended(cm, ext_k)
        assert cops.fr_ints(got) == prover.coeff_to_extended(c, ext_k - 2, ext_k), (ext_k, ln)
        assert np.array_equal(cm, keep)
        back = NC.extended_to_coeff(got, ext_k)
        assert np.array_equal(back[:ln], cm) and not back[ln:].any()
    # the definition itself at one point: ext[i] = f(zeta w^i)
    x = ZETA * pow(omega(ext_k), 3, R) % R
    assert cops.fr_ints(got[3:4])[0] == prover.eval_poly(c, x)
