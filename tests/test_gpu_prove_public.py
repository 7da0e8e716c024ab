"""zk_prove_public (csrc/prover.hip): create_proof with the circuit's public inputs - ONE instance column, absorbed into the
transcript, copy-constrained, neither committed nor opened.

The bytes are compared with tests/halo2_ref.py, the plain-Python statement of the rule (tied to the pinned oracle where they
overlap by tests/test_halo2_ref.py): at the shape where the column joins a full permutation chunk (k19like), where it starts a
chunk of its own (k17like), k18like, where it fills a free slot (wide) and - against the committed fixture - through the
column-batched MSM passes and transforms (k10batched); with 0, 1, 9 and `usable` instance values; under both quotient domains;
after the key went through its file forms; under the stream audit with the lone proof's side streams.  The entry points that carry
no instances refuse a key that has the column; a key without it is what it was."""
import ctypes
import functools
import json
import os

import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
from zkoracle.hashes import ChaCha20Rng
import halo2_ref
from public_cases import PAIRINGS, SEED, engine_key, mont, params_of, reference_key, shape_of, witness

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KIND = {"evm": E.ZK_TRANSCRIPT_EVM, "blake2b": E.ZK_TRANSCRIPT_BLAKE2B}
SCHEME = {"gwc": E.ZK_SCHEME_GWC, "shplonk": E.ZK_SCHEME_SHPLONK}
N_PUBLIC = 9


@functools.lru_cache(maxsize=None)
def made(name, n_public):
    """(witness, reference key) of the shape with n_public public inputs - made once, never changed."""
    asg = witness(name, n_public)
    return asg, reference_key(name, asg)


@functools.lru_cache(maxsize=None)
def reference(name, n_public, kind, scheme, extra_zeros=0):
    asg, rpk = made(name, n_public)
    return halo2_ref.create_proof(rpk, [asg.advice], [asg.instance + [0] * extra_zeros], ChaCha20Rng(SEED), kind, scheme)


def golden():
    with open(os.path.join(HERE, "golden", "public_proofs.json")) as f:
        return json.load(f)


def canon(limbs):
    return sum(int(limbs[i]) << (64 * i) for i in range(4)) * pow(1 << 256, -1, halo2_ref.R) % halo2_ref.R


@pytest.mark.parametrize("name", ["k19like", "k17like", "k18like", "wide"])
def test_bytes_of_the_reference(name):
    eng = zk.Engine(0)
    asg, rpk = made(name, N_PUBLIC)
    pk, (polys,) = engine_key(eng, name, [asg])
    sh = rpk.shape
    assert eng.pk_num_instance_columns(pk) == 1
    assert (eng.pk_shape(pk)["n_perm"], eng.pk_shape(pk)["n_chunks"]) == (len(sh.perm_cols), sh.n_chunks)
    assert canon(eng.vk_export(pk)[2]) == rpk.vk.transcript_repr
    pairs = PAIRINGS + ([("blake2b", "gwc"), ("evm", "shplonk")] if name == "k17like" else [])
    for kind, scheme in pairs:
        t, s = KIND[kind], SCHEME[scheme]
        got = eng.prove_public(pk, polys, mont(asg.instance), SEED, t, s)
        assert got == reference(name, N_PUBLIC, kind, scheme), (kind, scheme)
        assert len(got) == eng.proof_size(pk, t, s) == halo2_ref.proof_size(sh, 1, kind, scheme)
    # the same bytes over the whole extended domain and over three of its cosets
    kind, scheme = PAIRINGS[0]
    for domain in (1, 2):
        eng.set_option(E.ZK_OPT_QUOTIENT_DOMAIN, domain)
        assert eng.prove_public(pk, polys, mont(asg.instance), SEED, KIND[kind]) == reference(name, N_PUBLIC, kind, scheme), domain
    eng.close()


@pytest.mark.parametrize("name,m", [("k19like", 0), ("k19like", 1), ("k17like", 1), ("k19like", "usable"), ("k17like", "usable")])
def test_instance_lengths(name, m):
    """No value, one, and as many as the column holds (n - 7); one more is halo2's InstanceTooLarge from prover and verifier."""
    eng = zk.Engine(0)
    usable = shape_of(name).usable_rows
    m = usable if m == "usable" else m
    asg, rpk = made(name, m)
    assert len(asg.instance) == m
    pk, (polys,) = engine_key(eng, name, [asg])
    kind, scheme = PAIRINGS[1 if name == "k19like" else 0]
    t = KIND[kind]
    got = eng.prove_public(pk, polys, mont(asg.instance), SEED, t)
    assert got == reference(name, m, kind, scheme)
    assert eng.verify_public(pk, got, mont(asg.instance), t)
    if m == usable:
        too_many = mont(asg.instance + [0])
        with pytest.raises(zk.ZkError) as e:
            eng.prove_public(pk, polys, too_many, SEED, t)
        assert e.value.code == -1
        with pytest.raises(zk.ZkError) as e:
            eng.verify_public(pk, got, too_many, t)
        assert e.value.code == -1
        assert eng.prove_public(pk, polys, mont(asg.instance), SEED, t) == got  # (the context proves on)
    eng.close()


def test_trailing_zeros_are_part_of_the_transcript():
    """[v..] and [v.., 0]: the same column, another transcript - other bytes, and neither proof verifies under the other list."""
    eng = zk.Engine(0)
    name = "k17like"
    asg, rpk = made(name, N_PUBLIC)
    pk, (polys,) = engine_key(eng, name, [asg])
    for kind, scheme in PAIRINGS:
        t = KIND[kind]
        v, vz = mont(asg.instance), mont(asg.instance + [0])
        a, b = eng.prove_public(pk, polys, v, SEED, t), eng.prove_public(pk, polys, vz, SEED, t)
        assert a == reference(name, N_PUBLIC, kind, scheme) and b == reference(name, N_PUBLIC, kind, scheme, 1) and a != b
        assert eng.verify_public(pk, a, v, t) and eng.verify_public(pk, b, vz, t)
        assert not eng.verify_public(pk, a, vz, t) and not eng.verify_public(pk, b, v, t)
    eng.close()


def test_batched_passes_against_the_fixture():
    """k = 10: window tables exist, so the commitments take the column-batched MSM passes and the batched transforms; the bytes are
    the committed ones of tests/golden/make_public_proofs.py.  Once more under the stream audit with everything forced onto the
    side streams - the lone proof's rules: the instance column is written on the main stream and transformed on another."""
    g = golden()
    eng = zk.Engine(0)
    asg = witness(g["shape"], g["n_public"])
    assert [hex(v) for v in asg.instance] == g["instances"]
    pk, (polys,) = engine_key(eng, g["shape"], [asg])
    assert hex(canon(eng.vk_export(pk)[2])) == g["transcript_repr"]
    for kind, scheme in PAIRINGS:
        assert eng.prove_public(pk, polys, mont(asg.instance), SEED, KIND[kind]).hex() == g["proofs"][kind + "/" + scheme], kind
    eng.set_option(E.ZK_OPT_STREAM_AUDIT, 1)
    for opt in (E.ZK_OPT_MSM_TAIL_STREAM, E.ZK_OPT_XFORM_STREAM, E.ZK_OPT_MSM_STREAM):
        eng.set_option(opt, 1)
    try:
        proof = eng.prove_public(pk, polys, mont(asg.instance), SEED, E.ZK_TRANSCRIPT_EVM)
    except zk.ZkError as e:
        raise AssertionError("%s under the audit: %s" % (e, eng.audit_report())) from e
    checks, violations, msg = eng.audit_report()
    assert violations == 0, msg
    assert checks > 0
    assert proof.hex() == g["proofs"]["evm/gwc"]
    eng.close()


def test_a_key_without_the_column_is_what_it_was():
    eng = zk.Engine(0)
    name = "k17like"
    asg = witness(name, 0, n_inst=0)
    pk, (polys,) = engine_key(eng, name, [asg], n_inst=0)
    assert eng.pk_num_instance_columns(pk) == 0
    for kind, scheme in PAIRINGS:
        t = KIND[kind]
        want = eng.prove(pk, polys, SEED, t)
        assert eng.prove_public(pk, polys, None, SEED, t) == want
        assert eng.verify_public(pk, want, None, t) and eng.verify(pk, want, t)
    for call in (lambda: eng.prove_public(pk, polys, mont([5]), SEED), lambda: eng.verify_public(pk, want, mont([0]), E.ZK_TRANSCRIPT_BLAKE2B),
                 lambda: eng.witness_check_public(pk, polys, mont([0]))):
        with pytest.raises(zk.ZkError) as e:
            call()
        assert e.value.code == -1
    assert eng.witness_check_public(pk, polys, None) == eng.witness_check(pk, polys)
    eng.close()


def test_entry_points_without_instances_refuse_the_key():
    """zk_prove, zk_prove_batch, zk_prove_multi, zk_verify, zk_verify_batch, zk_verify_multi, zk_witness_check,
    zk_permutation_product and zk_quotient return ZK_EINVAL (halo2's InvalidInstances); the lookup phases, the shape and the
    key functions work; a value that is not below the modulus is ZK_EINVAL too."""
    eng = zk.Engine(0)
    name = "k17like"
    asg, rpk = made(name, N_PUBLIC)
    pk, (polys,) = engine_key(eng, name, [asg])
    t = E.ZK_TRANSCRIPT_EVM
    proof = eng.prove_public(pk, polys, mont(asg.instance), SEED, t)
    sh = eng.pk_shape(pk)
    n = 1 << sh["k"]
    ext = [eng.poly(4 * n) for _ in range(sh["n_advice"] + sh["n_chunks"] + 3 * sh["n_lookups"] + 1)]
    one = mont([1])[0]
    refused = {
        "zk_prove": lambda: eng.prove(pk, polys, SEED, t),
        "zk_prove_batch": lambda: eng.prove_batch(pk, [polys, polys], [SEED, SEED], t),
        "zk_prove_multi": lambda: eng.prove_multi(pk, [polys, polys], SEED, t),
        "zk_verify": lambda: eng.verify(pk, proof, t),
        "zk_verify_batch": lambda: eng.verify_batch(pk, [proof, proof], t),
        "zk_verify_multi": lambda: eng.verify_multi(pk, 2, proof, t),
        "zk_witness_check": lambda: eng.witness_check(pk, polys),
        "zk_permutation_product": lambda: eng.permutation_product(pk, polys, one, one),
        "zk_quotient": lambda: eng.quotient(pk, ext[:sh["n_advice"]], ext[sh["n_advice"]:sh["n_advice"] + sh["n_chunks"]],
                                            [tuple(ext[sh["n_advice"] + sh["n_chunks"] + 3 * l:][:3]) for l in range(sh["n_lookups"])],
                                            one, one, one, ext[-1]),
    }
    for what, call in refused.items():
        with pytest.raises(zk.ZkError) as e:
            call()
        assert e.value.code == -1, what
    # a batch / a multi proof of one is zk_prove / zk_verify: refused alike
    with pytest.raises(zk.ZkError):
        eng.prove_batch(pk, [polys], [SEED], t)
    with pytest.raises(zk.ZkError):
        eng.verify_multi(pk, 1, proof, t)
    # a Montgomery image that is not below the modulus
    bad = mont(asg.instance)
    bad[3] = [0xFFFFFFFFFFFFFFFF] * 4
    for call in (lambda: eng.prove_public(pk, polys, bad, SEED, t), lambda: eng.verify_public(pk, proof, bad, t),
                 lambda: eng.witness_check_public(pk, polys, bad)):
        with pytest.raises(zk.ZkError) as e:
            call()
        assert e.value.code == -1
    # what carries no permutation column works
    a, s = eng.lookup_permute(pk, polys)
    z = eng.lookup_product(pk, polys, a, s, one, one)
    for h in a + s + z + ext:
        h.free()
    assert eng.prove_public(pk, polys, mont(asg.instance), SEED, t) == proof
    eng.close()


@pytest.mark.parametrize("name", ["k19like", "k17like"])
def test_the_key_through_its_files(name):
    """zk_pk_write -> zk_pk_read and zk_vk_write -> zk_vk_read -> zk_vk_export -> zk_vk_from_parts of a key with the column: the
    same digest, the same proof bytes, a clean audit; zk_vk_load adopts the key's own image; a file read WITHOUT the column in the
    shape has one permutation commitment too many."""
    eng = zk.Engine(0)
    asg, rpk = made(name, N_PUBLIC)
    pk, (polys,) = engine_key(eng, name, [asg])
    p = params_of(name)
    kind, scheme = PAIRINGS[0]
    t = KIND[kind]
    want = reference(name, N_PUBLIC, kind, scheme)
    inst = mont(asg.instance)
    assert eng.pk_check(pk) == (E.ZK_PK_CHECK_ALL | E.ZK_PK_CHECK_REPR, [])
    img, vimg = eng.pk_write(pk), eng.vk_write(pk)
    pk2 = eng.pk_read(p, img)
    assert eng.pk_num_instance_columns(pk2) == 1 and eng.pk_shape(pk2) == eng.pk_shape(pk)
    assert eng.pk_check(pk2) == (E.ZK_PK_CHECK_ALL | E.ZK_PK_CHECK_REPR, [])
    assert eng.prove_public(pk2, polys, inst, SEED, t) == want
    assert bytes(eng.pk_write(pk2)) == bytes(img) and bytes(eng.vk_write(pk2)) == bytes(vimg)
    eng.vk_load(pk2, vimg)
    sigma = eng.poly(1 << p.degree)
    eng.pk_export_poly(pk2, E.ZK_PK_SIGMA_POLY, eng.pk_shape(pk)["n_perm"] - 1, sigma)  # the instance column's sigma polynomial
    sigma.free()
    vk = eng.vk_read(p, vimg)
    fc, pc, tr = eng.vk_export(vk)
    assert canon(tr) == rpk.vk.transcript_repr and len(pc) == len(rpk.shape.perm_cols)
    vk2 = eng.vk_from_parts(p, fc, pc)
    for key in (vk, vk2):
        assert eng.pk_num_instance_columns(key) == 1 and eng.verify_public(key, want, inst, t)
        with pytest.raises(zk.ZkError) as e:
            eng.prove_public(key, polys, inst, SEED, t)
        assert e.value.code == -5  # a verifying-only key proves nothing
    for read in (lambda: eng.vk_read(params_of(name, 0), vimg), lambda: eng.pk_read(params_of(name, 0), img)):
        with pytest.raises(zk.ZkError):
            read()
    bad = params_of(name)
    bad.num_instance_columns = 2
    with pytest.raises(zk.ZkError) as e:
        eng.vk_read(bad, vimg)
    assert e.value.code == -1
    eng.close()


def test_refusals_leave_the_outputs_untouched():
    eng = zk.Engine(0)
    name = "k19like"
    asg, rpk = made(name, N_PUBLIC)
    pk, (polys,) = engine_key(eng, name, [asg])
    size = eng.proof_size(pk)
    hs = (ctypes.c_uint64 * len(polys))(*[p.h for p in polys])
    inst = mont(asg.instance + [0] * (rpk.shape.usable_rows + 1 - N_PUBLIC))
    buf = ctypes.create_string_buffer(b"\xa5" * size, size)
    ln = ctypes.c_size_t(0x5A5A)
    rc = eng.L.zk_prove_public(eng.ctx, pk, hs, len(polys), inst.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(inst), SEED, 0, 0, buf,
                               size, ctypes.byref(ln))
    assert (rc, ln.value, buf.raw) == (-1, 0x5A5A, b"\xa5" * size)
    ok = ctypes.c_int(7)
    rc = eng.L.zk_verify_public(eng.ctx, pk, 0, 0, inst.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(inst), buf, size, ctypes.byref(ok))
    assert (rc, ok.value) == (-1, 7)
    # length alone without a buffer, as zk_prove
    v = mont(asg.instance)
    rc = eng.L.zk_prove_public(eng.ctx, pk, hs, len(polys), v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(v), SEED, 0, 0, None, 0,
                               ctypes.byref(ln))
    assert (rc, ln.value) == (0, size)
    eng.close()
