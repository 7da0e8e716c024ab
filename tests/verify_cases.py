"""Proofs and their tampered variants for the verifier tests (tests/test_verify_host.py, tests/test_gpu_verify.py): oracle-made
proofs at small k in the four transcript x scheme combinations, and the byte-level ways a proof can be wrong — bit flips, wrong
length, invalid point encodings, non-canonical scalars."""
import random

import webauthn_halo2_amd as zk
from zkoracle import plonk, prover
from zkoracle.field import P, R
from zkoracle.hashes import ChaCha20Rng

COMBOS = [("evm", "gwc"), ("evm", "shplonk"), ("blake2b", "gwc"), ("blake2b", "shplonk")]
# (A, L, F, k, lookup_bits[, idle]): the one-column k = 19 shape and the four-column k = 17 shape, scaled down
SMALL_SHAPES = {"k19like": (1, 1, 1, 7, 6), "k17like": (4, 1, 1, 7, 5), "idle": (4, 1, 1, 6, 4, 1)}


# F = 2: the identity-commitment key (identity_assignment)
IDENTITY_SHAPE = (3, 1, 2, 7, 5)


def params_of(name):
    return params_of_shape(SMALL_SHAPES[name])


def params_of_shape(shape):
    A, L, F, k, lb, idle = (tuple(shape) + (0,))[:6]
    return zk.circuit.CircuitParams(degree=k, num_advice=A, num_lookup_advice=L, num_fixed=F, lookup_bits=lb, idle_gate_columns=idle)


def oracle_shape(p):
    return plonk.Shape(p.degree, p.num_advice, p.num_lookup_advice, p.num_fixed, p.lookup_bits, p.idle_gate_columns)


def identity_assignment(seed=0x5EED0019):
    """A circuit of IDENTITY_SHAPE whose second constants column holds no constants: the column is all zero and every copy into
    it is dropped, so its fixed commitment is the identity — None in the oracle's key, (0, 0) in the engine's."""
    p = params_of_shape(IDENTITY_SHAPE)
    asg = zk.circuit.synthesize(p, seed)
    col = asg.layout.perm_index("fixed", 1)
    assert any(asg.fixed[1]) and any(col in (a[0], b[0]) for a, b in asg.copies)  # (there was something to drop)
    asg.fixed[1] = [0] * len(asg.fixed[1])
    asg.copies = [(a, b) for a, b in asg.copies if col not in (a[0], b[0])]
    return p, asg


def oracle_key(name, seed=0x5EED0019):
    p = params_of(name) if isinstance(name, str) else params_of_shape(name)
    asg = zk.circuit.synthesize(p, seed)
    return prover.keygen(prover.Circuit(oracle_shape(p), asg.fixed, asg.copies, asg.advice)), asg


def oracle_proof(pk, asg, kind, scheme, seed=b"\x07" * 32):
    return prover.create_proof(pk, asg.advice, ChaCha20Rng(seed), kind, scheme)


def n_points(shape, scheme):
    return shape.n_points_before_multiopen() + (2 if scheme == "shplonk" else shape.gwc_sets())


def variants(proof, shape, kind, scheme, seed=1):
    """[(label, bytes)] of proofs that differ from `proof`: every one of them is expected to be rejected."""
    rnd = random.Random(seed)
    ps = 64 if kind == "evm" else 32
    npts = n_points(shape, scheme)
    ev0 = shape.n_points_before_multiopen() * ps  # first evaluation
    out = []
    for t in range(3):
        b = bytearray(proof)
        pos = rnd.randrange(len(b))
        b[pos] ^= 1 << rnd.randrange(8)
        out.append((f"flip{t}@{pos}", bytes(b)))
    out += [("truncated", proof[:-32]), ("extended", proof + bytes(32)), ("empty", b"")]
    last_pt = (npts - 1) * ps if scheme == "gwc" else None
    for label, off in (("first point", 0), ("h point", (shape.n_points_before_multiopen() - 1) * ps), ("opening point", last_pt)):
        if off is None:
            continue
        if kind == "evm":
            b = bytearray(proof)
            y = int.from_bytes(b[off + 32:off + 64], "big")
            b[off + 32:off + 64] = ((y + 1) % P).to_bytes(32, "big")  # off the curve
            out.append((f"{label}: off curve", bytes(b)))
            b = bytearray(proof)
            b[off:off + 64] = bytes(64)  # the identity encoding
            out.append((f"{label}: identity", bytes(b)))
            b = bytearray(proof)
            x = int.from_bytes(b[off:off + 32], "big")
            b[off:off + 32] = (x + P).to_bytes(32, "big") if x + P < 1 << 256 else bytes(b[off:off + 32])
            out.append((f"{label}: x not canonical", bytes(b)))
        else:
            b = bytearray(proof)
            b[off:off + 32] = bytes(32)  # x = 0: 3 is not a square mod p
            out.append((f"{label}: zero", bytes(b)))
            b = bytearray(proof)
            x = int.from_bytes(b[off:off + 31] + bytes([b[off + 31] & 0x7F]), "little")
            enc = bytearray((x + P).to_bytes(32, "little"))
            enc[31] |= b[off + 31] & 0x80
            if (x + P) >> 255 == 0:
                b[off:off + 32] = enc
                out.append((f"{label}: x not canonical", bytes(b)))
            b = bytearray(proof)
            b[off + 31] ^= 0x80  # the other root
            out.append((f"{label}: sign", bytes(b)))
    for label, val in (("scalar = r", R), ("scalar = 2^256 - 1", (1 << 256) - 1)):
        b = bytearray(proof)
        b[ev0:ev0 + 32] = val.to_bytes(32, "big" if kind == "evm" else "little")
        out.append((label, bytes(b)))
    return out
