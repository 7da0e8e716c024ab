"""zk_prove_multi_public (csrc/prover_lockstep.h): ONE proof over N circuits with every circuit's public inputs, byte for byte what
tests/halo2_ref.py - the plain-Python statement of the rule, tied to the pinned oracle and to recorded digests by
tests/test_halo2_ref.py - makes: N = 2 and 3 at k19like (the column joins a permutation chunk), k17like (it has a chunk of its
own) and wide, with lists of different lengths; the committed k = 10 fixture through the column-batched passes.  One circuit is
zk_prove_public, a key without the column zk_prove_multi; the refusals leave the outputs untouched."""
import ctypes
import json
import os

import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
from zkoracle.hashes import ChaCha20Rng
import halo2_ref
from multi_public_cases import engine_lanes, lanes
from public_cases import PAIRINGS, SEED, engine_key, mont, reference_key, shape_of, witness

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KIND = {"evm": E.ZK_TRANSCRIPT_EVM, "blake2b": E.ZK_TRANSCRIPT_BLAKE2B}
SCHEME = {"gwc": E.ZK_SCHEME_GWC, "shplonk": E.ZK_SCHEME_SHPLONK}
LENGTHS = {2: (0, 9), 3: (1, 9, 2)}


def golden():
    with open(os.path.join(HERE, "golden", "multi_public_proofs.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("name", ["k19like", "k17like", "wide"])
def test_bytes_of_the_reference(name, N):
    eng = zk.Engine(0)
    made = lanes(name, LENGTHS[N])
    rpk = reference_key(name, made[0][0])
    pk, sets, lists = engine_lanes(eng, name, made)
    for kind, scheme in (PAIRINGS if name == "k19like" else [PAIRINGS[N % 2]]):
        t, s = KIND[kind], SCHEME[scheme]
        got = eng.prove_multi_public(pk, sets, lists, SEED, t, s)
        want = halo2_ref.create_proof(rpk, [a.advice for a, _ in made], [v for _, v in made], ChaCha20Rng(SEED), kind, scheme)
        assert got == want, (kind, scheme)
        assert len(got) == eng.proof_size_multi(pk, N, t, s)
        for domain in (1, 2):  # the accumulating pass reads circuit c's extended coset, or its three-coset copy
            eng.set_option(E.ZK_OPT_QUOTIENT_DOMAIN, domain)
            assert eng.prove_multi_public(pk, sets, lists, SEED, t, s) == want, domain
        eng.set_option(E.ZK_OPT_QUOTIENT_DOMAIN, 0)
    eng.close()


def test_batched_passes_against_the_fixture():
    g = golden()
    eng = zk.Engine(0)
    made = lanes(g["shape"], g["lengths"])
    assert [[hex(v) for v in vals] for _, vals in made] == g["instances"]
    pk, sets, lists = engine_lanes(eng, g["shape"], made)
    for kind, scheme in PAIRINGS:
        assert eng.prove_multi_public(pk, sets, lists, SEED, KIND[kind]).hex() == g["proofs"][kind + "/" + scheme], kind
    eng.set_option(E.ZK_OPT_STREAM_AUDIT, 1)
    try:
        proof = eng.prove_multi_public(pk, sets, lists, SEED, E.ZK_TRANSCRIPT_EVM)
    except zk.ZkError as e:
        raise AssertionError("%s under the audit: %s" % (e, eng.audit_report())) from e
    checks, violations, msg = eng.audit_report()
    assert violations == 0, msg
    assert checks > 0 and proof.hex() == g["proofs"]["evm/gwc"]
    eng.close()


def test_one_circuit_and_a_key_without_the_column():
    eng = zk.Engine(0)
    name = "k17like"
    made = lanes(name, [9])
    pk, sets, lists = engine_lanes(eng, name, made)
    for kind, _ in PAIRINGS:
        t = KIND[kind]
        assert eng.prove_multi_public(pk, sets, lists, SEED, t) == eng.prove_public(pk, sets[0], lists[0], SEED, t)
    eng.close()
    eng = zk.Engine(0)
    asg = witness(name, 0, n_inst=0)
    pk, (polys,) = engine_key(eng, name, [asg], n_inst=0)
    for kind, _ in PAIRINGS:
        t = KIND[kind]
        want = eng.prove_multi(pk, [polys, polys], SEED, t)
        assert eng.prove_multi_public(pk, [polys, polys], None, SEED, t) == want
        assert eng.prove_multi_public(pk, [polys, polys], [None, None], SEED, t) == want
    with pytest.raises(zk.ZkError) as e:
        eng.prove_multi_public(pk, [polys, polys], [None, mont([1])], SEED, t)
    assert e.value.code == -1
    eng.close()


def test_refusals():
    eng = zk.Engine(0)
    name = "k19like"
    made = lanes(name, [9, 9])
    pk, sets, lists = engine_lanes(eng, name, made)
    usable = shape_of(name).usable_rows
    t = E.ZK_TRANSCRIPT_BLAKE2B
    want = eng.prove_multi_public(pk, sets, lists, SEED, t)
    too_long = mont([1] * (usable + 1))
    bad_value = lists[1].copy()
    bad_value[2] = [0xFFFFFFFFFFFFFFFF] * 4
    for bad in (too_long, bad_value):
        with pytest.raises(zk.ZkError) as e:
            eng.prove_multi_public(pk, sets, [lists[0], bad], SEED, t)
        assert e.value.code == -1
        assert eng.prove_multi_public(pk, sets, lists, SEED, t) == want  # (the context proves on)
    size = eng.proof_size_multi(pk, 2, t)
    hs = (ctypes.c_uint64 * (2 * len(sets[0])))(*[p.h for a in sets for p in a])
    keep, iptrs, ilens = eng._instance_lists_arg([lists[0], too_long], 2)
    buf = ctypes.create_string_buffer(b"\xa5" * size, size)
    ln = ctypes.c_size_t(0x5A5A)
    rc = eng.L.zk_prove_multi_public(eng.ctx, pk, 2, hs, len(sets[0]), iptrs, ilens, SEED, t, 0, buf, size, ctypes.byref(ln))
    assert (rc, ln.value, buf.raw) == (-1, 0x5A5A, b"\xa5" * size)
    with pytest.raises(zk.ZkError):
        eng.prove_multi(pk, sets, SEED, t)
    with pytest.raises(zk.ZkError):
        eng.prove_multi_public(pk, sets, None, SEED, t)
    eng.close()
