"""Public inputs on the host (tests/public_host_check.cpp, built here with hipcc; no GPU): csrc/verifier.h gives the verdicts of
tests/halo2_ref.py for its proofs - intact, under one changed value, a dropped value and an appended zero, and with one flipped
byte in the last z commitment and in the last sigma evaluation - in all four transcript x scheme combinations, and csrc/vkrepr.h
with csrc/pk.h renders the digest halo2_ref renders, at k19like, k17like, k18like and wide."""
import os
import shutil
import subprocess

import pytest

from zkoracle import srs
from zkoracle.hashes import ChaCha20Rng
import halo2_ref
from public_cases import COMBOS, SEED, reference_key, tampered, witness, wrong_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PUBLIC = 9

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("phc") / "public_host_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-x", "hip", "-I", os.path.join(ROOT, "webauthn-halo2_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "public_host_check.cpp"), "-o", out])
    return out


def job_lines(vk, kind="evm", scheme="gwc", proofs=()):
    sh = vk.shape
    lines = ["shape %d %d %d %d %d %d" % (sh.k, sh.num_advice, sh.num_lookup_advice, sh.num_fixed, sh.lookup_bits, sh.idle_gate_columns),
             "kind " + kind, "scheme " + scheme, "repr " + hex(vk.transcript_repr), "tau " + hex(srs.TAU)]
    lines += ["fixed %s %s" % (hex(p[0]), hex(p[1])) for p in vk.fixed_commitments]
    lines += ["perm %s %s" % (hex(p[0]), hex(p[1])) for p in vk.permutation_commitments]
    lines += ["proof " + (p.hex() or "-") for p in proofs]
    return "\n".join(lines) + "\n"


def verdicts(exe, tmp_path, vk, kind, scheme, instances, proofs):
    path = str(tmp_path / "instances")
    with open(path, "w") as f:
        f.write("".join(hex(v) + "\n" for v in instances))
    out = subprocess.run([exe, "verify", str(vk.shape.n_inst), path], input=job_lines(vk, kind, scheme, proofs), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    res = [ln.split()[1] == "1" for ln in out.stdout.splitlines()]
    assert len(res) == len(proofs)
    return res


@pytest.mark.parametrize("name", ["k19like", "k17like", "k18like", "wide"])
def test_same_verdicts_and_digest_as_the_reference(exe, tmp_path, name):
    asg = witness(name, N_PUBLIC)
    pk = reference_key(name, asg)
    vk, vals = pk.vk, asg.instance
    out = subprocess.run([exe, "repr", "1"], input=job_lines(vk), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["repr", "0x%064x" % vk.transcript_repr, "perm_cols", str(len(vk.shape.perm_cols)), "chunks", str(vk.shape.n_chunks)]
    for kind, scheme in COMBOS:
        proof = halo2_ref.create_proof(pk, [asg.advice], [vals], ChaCha20Rng(SEED), kind, scheme)
        cases = [proof] + [b for _, b in tampered(proof, vk.shape, 1, kind, scheme)] + [proof[:-32], proof + bytes(32)]
        want = [halo2_ref.verify(vk, c, [vals], kind, scheme) for c in cases]
        assert want == [True] + [False] * (len(cases) - 1)
        assert verdicts(exe, tmp_path, vk, kind, scheme, vals, cases) == want, (kind, scheme)
        for what, wrong in wrong_lists(vals):
            assert not halo2_ref.verify(vk, proof, [wrong], kind, scheme)
            assert verdicts(exe, tmp_path, vk, kind, scheme, wrong, [proof]) == [False], (kind, scheme, what)


def test_without_the_column_nothing_moves(exe, tmp_path):
    """A shape without the column: the digest and the verdicts are the oracle's (halo2_ref's with n_inst = 0 are those, byte for
    byte: tests/test_halo2_ref.py)."""
    asg = witness("k17like", 0, n_inst=0)
    pk = reference_key("k17like", asg, n_inst=0)
    out = subprocess.run([exe, "repr", "0"], input=job_lines(pk.vk), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.split()[1] == "0x%064x" % pk.vk.transcript_repr, out.stdout + out.stderr
    kind, scheme = COMBOS[0]
    proof = halo2_ref.create_proof(pk, [asg.advice], [[]], ChaCha20Rng(SEED), kind, scheme)
    assert verdicts(exe, tmp_path, pk.vk, kind, scheme, [], [proof, proof[:-1] + bytes([proof[-1] ^ 4])]) == [True, False]
