"""zk_prove_batch_public (csrc/prover_lockstep.h): the lock-step batch with every proof's public inputs.  Proof j is zk_prove_public's
with the same key, advice, list and seed on the same engine - every lane has its own witness seed and the lists have different
lengths - and, at the shapes the plain-Python prover reaches, tests/halo2_ref.py's.  Shapes: k19like (n = 128), k18like (n = 64:
fewer rows than a workgroup of the kernel that writes the columns), k17like (the column has a permutation chunk of its own), wide and
k10batched (column-batched passes); B = 2, 3, 5; both reference pairings and one cross pairing; both quotient domains; the stream
audit; a long list followed by a short one in the same lane (a stale tail would change the bytes); empty lists; a batch of one; a
key without the column; the refusals."""
import ctypes

import numpy as np
import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
from zkoracle.hashes import ChaCha20Rng
import halo2_ref
from multi_public_cases import engine_lanes, lanes
from public_cases import PAIRINGS, engine_key, mont, reference_key, shape_of, witness

pytestmark = pytest.mark.gpu

KIND = {"evm": E.ZK_TRANSCRIPT_EVM, "blake2b": E.ZK_TRANSCRIPT_BLAKE2B}
SCHEME = {"gwc": E.ZK_SCHEME_GWC, "shplonk": E.ZK_SCHEME_SHPLONK}


def seeds(B):
    return [bytes([0x61 + j]) * 32 for j in range(B)]


def lengths(name, B):
    usable = shape_of(name).usable_rows
    return [9, 0, usable, 1, 2][:B]


def lone(eng, pk, sets, lists, sd, t, s=E.ZK_SCHEME_DEFAULT):
    return [eng.prove_public(pk, sets[j], lists[j], sd[j], t, s) for j in range(len(sets))]


@pytest.mark.parametrize("B", [2, 3, 5])
@pytest.mark.parametrize("name", ["k19like", "k18like", "k17like", "wide", "k10batched"])
def test_every_proof_is_zk_prove_public(name, B):
    eng = zk.Engine(0)
    made = lanes(name, lengths(name, B))
    pk, sets, lists = engine_lanes(eng, name, made)
    sd = seeds(B)
    pairs = PAIRINGS + ([("blake2b", "gwc")] if name == "k17like" else [])
    for kind, scheme in pairs:
        t, s = KIND[kind], SCHEME[scheme]
        got = eng.prove_batch_public(pk, sets, lists, sd, t, s)
        assert got == lone(eng, pk, sets, lists, sd, t, s), (kind, scheme)
        assert len(set(got)) == B
    if B == 2 and name != "k10batched":  # the plain-Python prover (both pairings where the column changes the chunks or not)
        rpk = reference_key(name, made[0][0])
        for kind, scheme in (PAIRINGS if name in ("k19like", "k17like") else PAIRINGS[:1]):
            got = eng.prove_batch_public(pk, sets, lists, sd, KIND[kind], SCHEME[scheme])
            for j, (asg, vals) in enumerate(made):
                assert got[j] == halo2_ref.create_proof(rpk, [asg.advice], [vals], ChaCha20Rng(sd[j]), kind, scheme), (kind, j)
    eng.close()


@pytest.mark.parametrize("name", ["k17like", "k10batched"])
def test_both_quotient_domains_and_the_audit(name):
    eng = zk.Engine(0)
    B = 3
    made = lanes(name, lengths(name, B))
    pk, sets, lists = engine_lanes(eng, name, made)
    sd = seeds(B)
    t = E.ZK_TRANSCRIPT_EVM
    want = lone(eng, pk, sets, lists, sd, t)
    for domain in (1, 2):
        eng.set_option(E.ZK_OPT_QUOTIENT_DOMAIN, domain)
        assert eng.prove_batch_public(pk, sets, lists, sd, t) == want, domain
    eng.set_option(E.ZK_OPT_QUOTIENT_DOMAIN, 0)
    eng.set_option(E.ZK_OPT_STREAM_AUDIT, 1)
    try:
        got = eng.prove_batch_public(pk, sets, lists, sd, t)
    except zk.ZkError as e:
        raise AssertionError("%s under the audit: %s" % (e, eng.audit_report())) from e
    checks, violations, msg = eng.audit_report()
    assert violations == 0, msg
    assert checks > 0 and got == want
    eng.close()


@pytest.mark.parametrize("name", ["k19like", "k17like"])
def test_a_longer_list_leaves_no_tail(name):
    """(usable, 1), then (1, usable), on one key in consecutive calls: lane 0 held `usable` values and then holds one."""
    eng = zk.Engine(0)
    usable = shape_of(name).usable_rows
    made = lanes(name, [9, 9])
    pk, sets, _ = engine_lanes(eng, name, made)
    pr = np.random.default_rng(7)
    long_ = mont([int(v) + 1 for v in pr.integers(0, 1 << 62, usable)])
    short = mont([12345])
    sd = seeds(2)
    t = E.ZK_TRANSCRIPT_BLAKE2B
    first = eng.prove_batch_public(pk, sets, [long_, short], sd, t)
    second = eng.prove_batch_public(pk, sets, [short, long_], sd, t)
    empty = eng.prove_batch_public(pk, sets, [None, None], sd, t)
    assert first == lone(eng, pk, sets, [long_, short], sd, t)
    assert second == lone(eng, pk, sets, [short, long_], sd, t)
    assert empty == lone(eng, pk, sets, [None, None], sd, t) and empty[0] != second[0]
    # a batch of one is zk_prove_public
    assert eng.prove_batch_public(pk, sets[:1], [short], sd[:1], t) == [eng.prove_public(pk, sets[0], short, sd[0], t)]
    eng.close()


def test_a_key_without_the_column():
    eng = zk.Engine(0)
    name = "k17like"
    asg = witness(name, 0, n_inst=0)
    pk, (polys,) = engine_key(eng, name, [asg], n_inst=0)
    sd = seeds(3)
    for kind, _ in PAIRINGS:
        t = KIND[kind]
        want = eng.prove_batch(pk, [polys] * 3, sd, t)
        assert eng.prove_batch_public(pk, [polys] * 3, None, sd, t) == want
        assert eng.prove_batch_public(pk, [polys] * 3, [None] * 3, sd, t) == want
    with pytest.raises(zk.ZkError) as e:
        eng.prove_batch_public(pk, [polys] * 3, [None, mont([1]), None], sd, t)
    assert e.value.code == -1
    eng.close()


def test_refusals():
    eng = zk.Engine(0)
    name = "k19like"
    made = lanes(name, [9, 9, 9])
    pk, sets, lists = engine_lanes(eng, name, made)
    usable = shape_of(name).usable_rows
    sd = seeds(3)
    t = E.ZK_TRANSCRIPT_BLAKE2B
    want = eng.prove_batch_public(pk, sets, lists, sd, t)
    modulus = np.array([[(halo2_ref.R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]], dtype=np.uint64)
    for bad in (mont([1] * (usable + 1)), np.concatenate([lists[1][:4], modulus, lists[1][5:]])):
        with pytest.raises(zk.ZkError) as e:
            eng.prove_batch_public(pk, sets, [lists[0], bad, lists[2]], sd, t)
        assert e.value.code == -1
        assert eng.prove_batch_public(pk, sets, lists, sd, t) == want  # (the context proves on)
    # the outputs are untouched, and the forms without instances still refuse the key
    size = eng.proof_size(pk, t)
    hs = (ctypes.c_uint64 * (3 * len(sets[0])))(*[p.h for a in sets for p in a])
    keep, iptrs, ilens = eng._instance_lists_arg([lists[0], mont([1] * (usable + 1)), lists[2]], 3)
    buf = ctypes.create_string_buffer(b"\xa5" * (3 * size), 3 * size)
    ln = ctypes.c_size_t(0x5A5A)
    rc = eng.L.zk_prove_batch_public(eng.ctx, pk, 3, hs, len(sets[0]), iptrs, ilens, b"".join(sd), t, 0, buf, size, ctypes.byref(ln))
    assert (rc, ln.value, buf.raw) == (-1, 0x5A5A, b"\xa5" * (3 * size))
    with pytest.raises(zk.ZkError):
        eng.prove_batch(pk, sets, sd, t)
    with pytest.raises(zk.ZkError) as e:  # a key with the column takes no NULL length array
        eng.prove_batch_public(pk, sets, None, sd, t)
    assert e.value.code == -1
    eng.close()
