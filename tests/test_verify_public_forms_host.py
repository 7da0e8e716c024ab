"""csrc/verifier.h with one instance list per circuit, on the host (tests/verify_public_forms_host_check.cpp, built here with hipcc;
no GPU): proofs of tests/halo2_ref.py over two and three circuits get that reference's verdicts - intact, under every wrong
set of lists (one changed value in circuit 1's list only, the lists swapped, a dropped value, an appended zero, one circuit fewer
and one more) and with the flipped bytes of public_cases.PLACES - and likewise with one circuit.  For every
proof the program also prepares the term lists a second time from inst(x) values computed outside verifier::prepare_lists and
fails unless verdict, challenges and term lists are the same."""
import os
import shutil
import subprocess

import pytest

from zkoracle import srs
from zkoracle.hashes import ChaCha20Rng
import halo2_ref
from multi_public_cases import lanes, wrong_multi_lists
from public_cases import COMBOS, PAIRINGS, SEED, reference_key, tampered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vpfhc") / "verify_public_forms_host_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-x", "hip", "-I", os.path.join(ROOT, "webauthn-halo2_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests"),
                           os.path.join(ROOT, "tests", "verify_public_forms_host_check.cpp"), "-o", out])
    return out


def verdicts(exe, tmp_path, vk, kind, scheme, lists, proofs):
    sh = vk.shape
    lines = ["shape %d %d %d %d %d %d" % (sh.k, sh.num_advice, sh.num_lookup_advice, sh.num_fixed, sh.lookup_bits, sh.idle_gate_columns),
             "kind " + kind, "scheme " + scheme, "repr " + hex(vk.transcript_repr), "tau " + hex(srs.TAU)]
    lines += ["fixed %s %s" % (hex(p[0]), hex(p[1])) for p in vk.fixed_commitments]
    lines += ["perm %s %s" % (hex(p[0]), hex(p[1])) for p in vk.permutation_commitments]
    lines += ["proof " + (p.hex() or "-") for p in proofs]
    path = str(tmp_path / "lists")
    with open(path, "w") as f:
        f.write("".join((" ".join(hex(v) for v in l) or "-") + "\n" for l in lists))
    out = subprocess.run([exe, str(len(lists)), path], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    res = [ln.split()[1] == "1" for ln in out.stdout.splitlines()]
    assert len(res) == len(proofs)
    return res


@pytest.mark.parametrize("name,lengths", [("k19like", (9, 9)), ("k17like", (0, 9)), ("k17like", (1, 9, 2))])
def test_same_verdicts_as_the_reference(exe, tmp_path, name, lengths):
    made = lanes(name, lengths)
    pk = reference_key(name, made[0][0])
    vk = pk.vk
    lists = [vals for _, vals in made]
    for kind, scheme in (COMBOS if lengths == (9, 9) else PAIRINGS):
        proof = halo2_ref.create_proof(pk, [a.advice for a, _ in made], lists, ChaCha20Rng(SEED), kind, scheme)
        cases = [proof] + [b for _, b in tampered(proof, vk.shape, len(lists), kind, scheme)] + [proof[:-32], proof + bytes(32)]
        want = [halo2_ref.verify(vk, c, lists, kind, scheme) for c in cases]
        assert want == [True] + [False] * (len(cases) - 1)
        assert verdicts(exe, tmp_path, vk, kind, scheme, lists, cases) == want, (kind, scheme)
        for what, wrong in wrong_multi_lists(lists):
            assert not halo2_ref.verify(vk, proof, wrong, kind, scheme), what
            assert verdicts(exe, tmp_path, vk, kind, scheme, wrong, [proof]) == [False], (kind, scheme, what)


def test_one_circuit_has_the_single_proof_layout(exe, tmp_path):
    (asg, vals), = lanes("k17like", [9])
    pk = reference_key("k17like", asg)
    for kind, scheme in PAIRINGS:
        proof = halo2_ref.create_proof(pk, [asg.advice], [vals], ChaCha20Rng(SEED), kind, scheme)
        assert verdicts(exe, tmp_path, pk.vk, kind, scheme, [vals], [proof, proof[:-1] + bytes([proof[-1] ^ 4])]) == [True, False]
        assert verdicts(exe, tmp_path, pk.vk, kind, scheme, [vals + [0]], [proof]) == [False]
