"""Shared by the tests of one proof over N circuits (tests/test_multi_ref.py, tests/test_verify_multi_host.py,
tests/test_gpu_prove_multi.py, tests/test_gpu_verify_multi.py): the oracle key and witnesses of a shape of tests/prover_shapes.py
without the instance column, the same on an engine (tests/public_cases.py's, at n_inst = 0), and the tampered variants of a proof."""
import webauthn_halo2_amd as zk
from zkoracle import plonk, prover
import public_cases

PAIRINGS = [("evm", "gwc"), ("blake2b", "shplonk")]  # the reference's two: verify_evm and verify
SEED = b"\x2a" * 32
PLACES = ("advice commitment of circuit 1", "h piece", "shared fixed evaluation", "circuit-1 lookup evaluation", "last opening")


def params_of(name):
    return public_cases.params_of(name, 0)


def witnesses(name, count):
    """`count` assignments of the shape: one structure (selectors, copies), distinct witness seeds."""
    p = params_of(name)
    return [zk.circuit.synthesize(p, 0x5EED0700 + 13 * i) for i in range(count)]


def oracle_key(name, asg):
    p = params_of(name)
    sh = plonk.Shape(p.degree, p.num_advice, p.num_lookup_advice, p.num_fixed, p.lookup_bits, p.idle_gate_columns)
    return prover.keygen(prover.Circuit(sh, asg.fixed, asg.copies, asg.advice))


def setup(name, n_witnesses):
    asgs = witnesses(name, n_witnesses)
    return oracle_key(name, asgs[0]), asgs


def engine_key(eng, name, asgs):
    return public_cases.engine_key(eng, name, asgs, 0)


def tampered(proof, shape, N, kind, scheme):
    return public_cases.tampered(proof, shape, N, kind, scheme, PLACES)
