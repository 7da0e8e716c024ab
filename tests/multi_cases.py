"""Shared by the tests of one proof over N circuits (tests/test_multi_ref.py, tests/test_verify_multi_host.py,
tests/test_gpu_prove_multi.py, tests/test_gpu_verify_multi.py): the oracle key and witnesses of a shape of tests/prover_shapes.py,
the same on an engine, and the tampered variants of a proof."""
import numpy as np

import webauthn_halo2_amd as zk
from zkoracle import plonk, prover
from prover_shapes import SHAPES
import multi_ref

PAIRINGS = [("evm", "gwc"), ("blake2b", "shplonk")]  # the reference's two: verify_evm and verify
SEED = b"\x2a" * 32
PLACES = ("advice commitment of circuit 1", "h piece", "shared fixed evaluation", "circuit-1 lookup evaluation", "last opening")


def params_of(name):
    A, L, F, k, lb, idle = (tuple(SHAPES[name]) + (0,))[:6]
    return zk.circuit.CircuitParams(degree=k, num_advice=A, num_lookup_advice=L, num_fixed=F, lookup_bits=lb, idle_gate_columns=idle)


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
    """(pk, advice sets) of the shape on `eng`: SRS of the shape's k, the key, every witness's columns resident."""
    p = params_of(name)
    eng.srs_setup(p.degree)
    fixed = np.stack([asgs[0].to_limbs(c) for c in asgs[0].fixed])
    pk = eng.keygen(p, fixed, asgs[0].copies)
    sets = []
    for asg in asgs:
        polys = []
        for col in asg.advice:
            h = eng.poly(1 << p.degree)
            eng.upload_canonical(h, asg.to_limbs(col))
            polys.append(h)
        sets.append(polys)
    return pk, sets


def tampered(proof, shape, N, kind, scheme):
    """[(place, bytes)]: one flipped byte at each of PLACES."""
    off = multi_ref.proof_offsets(shape, N, kind, scheme)
    out = []
    for place in PLACES:
        b = bytearray(proof)
        b[off[place]] ^= 0x10
        out.append((place, bytes(b)))
    return out
