"""zk_verify_public (csrc/verify.hip, csrc/verifier.h): verify_proof with the circuit's public inputs.  It accepts zk_prove_public's
proofs and tests/halo2_ref.py's own, on full and on verifying-only keys, in all four transcript x scheme pairs; under one changed
value, a dropped value and an appended zero, and after one flipped byte in the last z commitment and in the last sigma evaluation
it rejects - as a verdict, never an error - exactly where the reference verifier does."""
import json
import os

import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
from zkoracle.hashes import ChaCha20Rng
import halo2_ref
from public_cases import COMBOS, PAIRINGS, SEED, engine_key, mont, params_of, reference_key, tampered, witness, wrong_lists

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KIND = {"evm": E.ZK_TRANSCRIPT_EVM, "blake2b": E.ZK_TRANSCRIPT_BLAKE2B}
SCHEME = {"gwc": E.ZK_SCHEME_GWC, "shplonk": E.ZK_SCHEME_SHPLONK}
N_PUBLIC = 9


@pytest.mark.parametrize("name", ["k19like", "k17like", "k18like", "wide"])
def test_verdicts_of_the_reference(name):
    eng = zk.Engine(0)
    asg = witness(name, N_PUBLIC)
    rpk = reference_key(name, asg)
    pk, (polys,) = engine_key(eng, name, [asg])
    vk = eng.vk_read(params_of(name), eng.vk_write(pk))
    vals = asg.instance
    for kind, scheme in (COMBOS if name == "k17like" else PAIRINGS):
        t, s = KIND[kind], SCHEME[scheme]
        proof = eng.prove_public(pk, polys, mont(vals), SEED, t, s)
        if (kind, scheme) == PAIRINGS[0]:  # the reference's own proof: another blinding stream, made by the Python prover
            own = halo2_ref.create_proof(rpk, [asg.advice], [vals], ChaCha20Rng(b"\x4c" * 32), kind, scheme)
            assert own != proof and eng.verify_public(pk, own, mont(vals), t, s) and eng.verify_public(vk, own, mont(vals), t, s)
        assert halo2_ref.verify(rpk.vk, proof, [vals], kind, scheme)
        cases = [(vals, proof)] + [(wrong, proof) for _, wrong in wrong_lists(vals)]
        cases += [(vals, bad) for _, bad in tampered(proof, rpk.shape, 1, kind, scheme)] + [(vals, proof[:-32]), (vals, proof + bytes(32))]
        want = [halo2_ref.verify(rpk.vk, pf, [inst], kind, scheme) for inst, pf in cases]
        assert want == [True] + [False] * (len(cases) - 1)
        for key in (pk, vk):  # the full key and the verifying-only one
            assert [eng.verify_public(key, pf, mont(inst), t, s) for inst, pf in cases] == want, (kind, scheme)
    eng.close()


def test_the_fixture_proofs():
    """The committed k = 10 proofs (tests/golden/make_public_proofs.py) on a verifying-only key made from the engine's own key."""
    with open(os.path.join(HERE, "golden", "public_proofs.json")) as f:
        g = json.load(f)
    eng = zk.Engine(0)
    asg = witness(g["shape"], g["n_public"])
    pk, (polys,) = engine_key(eng, g["shape"], [asg])
    fc, pc, tr = eng.vk_export(pk)
    vk = eng.vk_from_parts(params_of(g["shape"]), fc, pc)
    vals = [int(v, 16) for v in g["instances"]]
    for kind, scheme in PAIRINGS:
        proof = bytes.fromhex(g["proofs"][kind + "/" + scheme])
        assert eng.verify_public(vk, proof, mont(vals), KIND[kind]) and eng.verify_public(pk, proof, mont(vals), KIND[kind])
        for what, wrong in wrong_lists(vals):
            assert not eng.verify_public(vk, proof, mont(wrong), KIND[kind]), what
    eng.close()
