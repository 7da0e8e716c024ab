"""Shared by the tests of public inputs (tests/test_halo2_ref.py, tests/test_public_host.py, tests/test_gpu_prove_public.py,
tests/test_gpu_verify_public.py, tests/test_gpu_witness_check_public.py, tests/golden/make_public_proofs.py) and, through
tests/multi_cases.py and tests/multi_public_cases.py, of N circuits: the shapes of tests/prover_shapes.py with the instance
column, their witnesses with n_public exposed gate outputs, the reference key (tests/halo2_ref.py) and the same on an engine, and
the tampered variants of a proof."""
import numpy as np

import webauthn_halo2_amd as zk
from prover_shapes import SHAPES
import halo2_ref

PAIRINGS = [("evm", "gwc"), ("blake2b", "shplonk")]  # the reference's two: verify_evm and verify
COMBOS = [(k, s) for k in ("evm", "blake2b") for s in ("gwc", "shplonk")]
SEED = b"\x3b" * 32
WITNESS_SEED = 0x5EED0900
PLACES = ("last z commitment", "last sigma evaluation")


def params_of(name, n_inst=1):
    A, L, F, k, lb, idle = (tuple(SHAPES[name]) + (0,))[:6]
    return zk.circuit.CircuitParams(degree=k, num_advice=A, num_lookup_advice=L, num_fixed=F, lookup_bits=lb, idle_gate_columns=idle,
                                    num_instance_columns=n_inst)


def shape_of(name, n_inst=1):
    A, L, F, k, lb, idle = (tuple(SHAPES[name]) + (0,))[:6]
    return halo2_ref.public_shape(k, A, L, F, lb, idle, n_inst)


def witness(name, n_public, n_inst=1):
    """The assignment of the shape with n_public gate outputs exposed: .instance holds their values, .copies ties them."""
    return zk.circuit.synthesize(params_of(name, n_inst), WITNESS_SEED, n_public=n_public)


def reference_key(name, asg, n_inst=1):
    return halo2_ref.keygen(shape_of(name, n_inst), asg.fixed, asg.copies)


def engine_key(eng, name, asgs, n_inst=1):
    """(pk, advice sets) of the shape on `eng`: SRS of the shape's k, the key of asgs[0]'s structure, every witness's columns
    resident."""
    p = params_of(name, n_inst)
    eng.srs_setup(p.degree)
    pk = eng.keygen(p, np.stack([asgs[0].to_limbs(c) for c in asgs[0].fixed]), asgs[0].copies)
    sets = []
    for asg in asgs:
        polys = []
        for col in asg.advice:
            h = eng.poly(1 << p.degree)
            eng.upload_canonical(h, asg.to_limbs(col))
            polys.append(h)
        sets.append(polys)
    return pk, sets


def mont(vals):
    return zk.circuit.Assignment.to_mont_limbs(list(vals))


def tampered(proof, shape, N, kind, scheme, places=PLACES):
    """[(place, bytes)]: one flipped byte at each of `places` of a proof over N circuits."""
    off = halo2_ref.proof_offsets(shape, N, kind, scheme)
    out = []
    for place in places:
        b = bytearray(proof)
        b[off[place]] ^= 0x10
        out.append((place, bytes(b)))
    return out


def wrong_lists(vals):
    """[(what, list)]: instance lists under which a proof over `vals` must not verify."""
    changed = list(vals)
    changed[len(vals) // 2] = (changed[len(vals) // 2] + 1) % halo2_ref.R
    return [("one changed value", changed), ("a dropped value", list(vals[:-1])), ("an appended zero", list(vals) + [0])]
