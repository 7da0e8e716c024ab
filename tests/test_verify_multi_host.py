"""csrc/verifier.h with a circuit count, on the host (tests/verify_multi_host_check.cpp, built here with hipcc; no GPU): proofs of
tests/halo2_ref.py over two and three circuits — intact, with one flipped byte at five places, and read as proofs of another
circuit count — get the verdicts of halo2_ref.verify, in all four transcript x scheme combinations; with one circuit the
verdicts are those of the single-circuit layout."""
import os
import shutil
import subprocess

import pytest

from zkoracle import srs
from zkoracle.hashes import ChaCha20Rng
import halo2_ref
import verify_cases as vc
from multi_cases import SEED, setup, tampered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vmhc") / "verify_multi_host_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-x", "hip", "-I", os.path.join(ROOT, "webauthn-halo2_amd", "csrc"),
                           "-I", os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "verify_multi_host_check.cpp"), "-o", out])
    return out


def run_job(exe, N, vk, kind, scheme, proofs):
    sh = vk.shape
    lines = ["shape %d %d %d %d %d %d" % (sh.k, sh.num_advice, sh.num_lookup_advice, sh.num_fixed, sh.lookup_bits, sh.idle_gate_columns),
             "kind " + kind, "scheme " + scheme, "repr " + hex(vk.transcript_repr), "tau " + hex(srs.TAU)]
    lines += ["fixed %s %s" % (hex(p[0]), hex(p[1])) for p in vk.fixed_commitments]
    lines += ["perm %s %s" % (hex(p[0]), hex(p[1])) for p in vk.permutation_commitments]
    lines += ["proof " + (p.hex() or "-") for p in proofs]
    out = subprocess.run([exe, str(N)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    res = [ln.split()[1] == "1" for ln in out.stdout.splitlines()]
    assert len(res) == len(proofs)
    return res


@pytest.mark.parametrize("name,N", [("k18like", 2), ("k18like", 3), ("k17like", 2), ("wide", 2)])
def test_same_verdicts_as_the_reference(exe, name, N):
    pk, asgs = setup(name, N)
    vk = pk.vk
    for kind, scheme in vc.COMBOS:
        proof = halo2_ref.create_proof(pk, [a.advice for a in asgs], None, ChaCha20Rng(SEED), kind, scheme)
        cases = [proof] + [b for _, b in tampered(proof, vk.shape, N, kind, scheme)] + [proof[:-32], proof + bytes(32)]
        want = [halo2_ref.verify(vk, c, [[]] * N, kind, scheme) for c in cases]
        assert want == [True] + [False] * (len(cases) - 1)
        assert run_job(exe, N, vk, kind, scheme, cases) == want, (kind, scheme)
        for other in (N - 1, N + 1):  # a proof of another circuit count has another length
            assert run_job(exe, other, vk, kind, scheme, [proof]) == [False]


def test_one_circuit_is_the_single_layout(exe):
    pk, asg = vc.oracle_key("k17like")
    for kind, scheme in vc.COMBOS:
        proof = vc.oracle_proof(pk, asg, kind, scheme)
        assert run_job(exe, 1, pk.vk, kind, scheme, [proof, proof[:-1] + bytes([proof[-1] ^ 4])]) == [True, False]
