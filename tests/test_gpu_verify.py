"""zk_verify / zk_verify_batch on an MI355X: a real pairing against the resident SRS (csrc/verify.hip, csrc/verifier.h,
csrc/pairing.h).  The reference's golden proof through zk_vk_from_parts, device proofs of small shapes in all four transcript x
scheme combinations with their tampered variants (verdicts equal to the oracle verifier's), full-size proofs, batches whose
verdicts equal the per-proof ones, SRS separation, the ecdsa_p256 / proving_server surface, and the stream audit."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
from zkoracle import cops, plonk
from zkoracle.field import P
import verify_cases as vc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
T = {"evm": E.ZK_TRANSCRIPT_EVM, "blake2b": E.ZK_TRANSCRIPT_BLAKE2B}
S = {"gwc": E.ZK_SCHEME_GWC, "shplonk": E.ZK_SCHEME_SHPLONK}


def mont_points(pts):
    """[(x, y)] canonical ints -> (n, 8) uint64 affine Montgomery"""
    xs = []
    for x, y in pts:
        xs += [x * (1 << 256) % P, y * (1 << 256) % P]
    return cops.ints_to_arr(xs).reshape(-1, 8)


def fr_mont_limbs(v):
    return cops.fr_mont([v])[0]


def test_golden_proof_through_vk_from_parts(engine):
    d = json.load(open(os.path.join(GOLD, "vk_k17.json")))
    proof = bytes.fromhex(open(os.path.join(GOLD, "golden_proof_k17_evm.hex")).read().strip())
    pt = lambda p: (int(p[0], 16), int(p[1], 16))
    engine.srs_setup(17, bytes(32))
    vk = engine.vk_from_parts(zk.circuit.K17, mont_points([pt(p) for p in d["fixed_commitments"]]),
                              mont_points([pt(p) for p in d["permutation_commitments"]]), fr_mont_limbs(int(d["transcript_repr"], 16)))
    assert engine.verify(vk, proof, E.ZK_TRANSCRIPT_EVM)
    flip = json.load(open(os.path.join(GOLD, "yul_verdicts.json")))["golden"]["flip"]
    bad = []
    for pos in (5, 0x1c0 + 40, 0x3c0 + 7, 0x3c0 + 32 * 20 + 31, 0x920 + 3, len(proof) - 1, flip[0]):
        b = bytearray(proof)
        b[pos] ^= flip[1] if pos == flip[0] else 1
        bad.append(bytes(b))
    bad += [proof[:-32], proof + bytes(32), b""]
    assert not any(engine.verify(vk, b, E.ZK_TRANSCRIPT_EVM) for b in bad)
    assert engine.verify_batch(vk, [proof] + bad + [proof], E.ZK_TRANSCRIPT_EVM) == [True] + [False] * len(bad) + [True]
    # a verifying-only key proves nothing and writes no proving key; its shape and vk are there
    with pytest.raises(zk.ZkError) as ei:
        engine.pk_write(vk)
    assert ei.value.code == -5
    assert engine.pk_shape(vk)["k"] == 17 and engine.vk_export(vk)[2].tolist() == fr_mont_limbs(int(d["transcript_repr"], 16)).tolist()
    engine.pk_free(vk)


def device_key(engine, name):
    p = vc.params_of(name)
    asg = zk.circuit.synthesize(p, 0x5EED0019)
    engine.srs_setup(p.degree, bytes(32))
    pk = engine.keygen(p, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
    adv = [engine.poly(1 << p.degree) for _ in asg.advice]
    for h, col in zip(adv, asg.advice):
        engine.upload_canonical(h, asg.to_limbs(col))
    fc, pc, tr = engine.vk_export(pk)
    sh = plonk.Shape(p.degree, p.num_advice, p.num_lookup_advice, p.num_fixed, p.lookup_bits, p.idle_gate_columns)
    ovk = plonk.VerifyingKey(sh, cops.affine_arr_to_ints(fc), cops.affine_arr_to_ints(pc), cops.fr_ints(tr.reshape(1, 4))[0])
    return p, pk, adv, ovk, (fc, pc, tr)


@pytest.mark.parametrize("name", ["k19like", "k17like"])
def test_device_proofs_all_combinations(engine, name):
    p, pk, adv, ovk, (fc, pc, tr) = device_key(engine, name)
    vko = engine.vk_from_parts(p, fc, pc, tr)
    try:
        for kind, scheme in vc.COMBOS:
            proof = engine.prove(pk, adv, b"\x31" * 32, T[kind], S[scheme])
            cases = [("intact", proof)] + vc.variants(proof, ovk.shape, kind, scheme, seed=sum(map(ord, name + kind + scheme)))
            want = [plonk.verify(ovk, c[1], kind, scheme) for c in cases]
            assert want[0]
            got = [engine.verify(pk, c[1], T[kind], S[scheme]) for c in cases]
            assert got == want, [c[0] for c, g, w in zip(cases, got, want) if g != w]
            assert engine.verify_batch(vko, [c[1] for c in cases], T[kind], S[scheme]) == want
        with pytest.raises(zk.ZkError) as ei:
            engine.prove(vko, adv, b"\x31" * 32, E.ZK_TRANSCRIPT_EVM)
        assert ei.value.code == -5
    finally:
        engine.pk_free(vko)
        engine.pk_free(pk)
        for h in adv:
            h.free()


FIX = json.load(open(os.path.join(GOLD, "fullsize_proofs.json")))


@pytest.mark.parametrize("case", ["k17_evm_gwc", "k19_blake2b_shplonk"])
def test_fullsize_proofs_accepted(engine, case):
    c = FIX[case]
    proof = bytes.fromhex(c["proof"])
    assert hashlib.sha256(proof).hexdigest() == c["sha256"]
    p = zk.circuit.K17 if c["degree"] == 17 else zk.circuit.K19
    engine.srs_setup(c["degree"], bytes(32))
    pt = lambda q: (int(q[0], 16), int(q[1], 16))
    vk = engine.vk_from_parts(p, mont_points([pt(q) for q in c["vk_fixed_commitments"]]), mont_points([pt(q) for q in c["vk_permutation_commitments"]]),
                              fr_mont_limbs(int(c["transcript_repr"], 16)))
    kind = c["transcript"]
    scheme = E.ZK_SCHEME_DEFAULT
    try:
        if c["degree"] == 17:  # made again on the device from its seeds: the same bytes
            asg = zk.circuit.synthesize(p, c["witness_seed"], worst_case=c["worst_case"])
            pk = engine.keygen(p, np.stack([asg.to_limbs(col) for col in asg.fixed]), asg.copies)
            adv = [engine.poly(1 << 17) for _ in asg.advice]
            for h, col in zip(adv, asg.advice):
                engine.upload_canonical(h, asg.to_limbs(col))
            again = engine.prove(pk, adv, bytes.fromhex(c["rng_seed"]), T[kind])
            for h in adv:
                h.free()
            assert hashlib.sha256(again).hexdigest() == c["sha256"]
            assert engine.verify(pk, again, T[kind])
            engine.pk_free(pk)
        assert engine.verify(vk, proof, T[kind], scheme)
        bad = bytearray(proof)
        bad[len(bad) // 2] ^= 8
        assert engine.verify_batch(vk, [proof, bytes(bad)], T[kind], scheme) == [True, False]
    finally:
        engine.pk_free(vk)


def test_batches_equal_single_verdicts(engine):
    p, pk, adv, ovk, (fc, pc, tr) = device_key(engine, "k19like")
    vko = engine.vk_from_parts(p, fc, pc, tr)
    rnd = random.Random(7)
    try:
        for kind, scheme in (("evm", "gwc"), ("blake2b", "shplonk")):
            good = [engine.prove(pk, adv, bytes([i]) * 32, T[kind], S[scheme]) for i in range(12)]
            bad = []
            for g in good[:6]:
                bad += [v for _, v in vc.variants(g, ovk.shape, kind, scheme, seed=rnd.randrange(1 << 16))][:4]
            single = {}

            def verdict(x):
                if x not in single:
                    single[x] = engine.verify(vko, x, T[kind], S[scheme])
                return single[x]

            assert all(verdict(g) for g in good)
            masks = []
            for B in (1, 7, 64, 256):
                masks += [[True] * B, [False] * B]
                if B > 1:
                    for at in (0, B // 2, B - 1):
                        m = [True] * B
                        m[at] = False
                        masks.append(m)
                    masks.append([rnd.random() < 0.5 for _ in range(B)])
            for m in masks:
                batch = [rnd.choice(good) if ok else rnd.choice(bad) for ok in m]
                got = engine.verify_batch(vko, batch, T[kind], S[scheme])
                assert got == [verdict(x) for x in batch]
            # the oracle on a few of them
            for x in [good[0], good[5]] + bad[:3]:
                assert verdict(x) == plonk.verify(ovk, x, kind, scheme)
    finally:
        engine.pk_free(vko)
        engine.pk_free(pk)
        for h in adv:
            h.free()


def test_another_srs_rejects(engine):
    p = vc.params_of("k19like")
    asg = zk.circuit.synthesize(p, 0x5EED0019)
    engine.srs_setup(p.degree, b"\xaa" * 32)
    pk = engine.keygen(p, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
    adv = [engine.poly(1 << p.degree) for _ in asg.advice]
    for h, col in zip(adv, asg.advice):
        engine.upload_canonical(h, asg.to_limbs(col))
    proofs = [engine.prove(pk, adv, b"\x01" * 32, E.ZK_TRANSCRIPT_EVM), engine.prove(pk, adv, b"\x02" * 32, E.ZK_TRANSCRIPT_BLAKE2B)]
    fc, pc, tr = engine.vk_export(pk)
    vko = engine.vk_from_parts(p, fc, pc, tr)
    try:
        assert engine.verify(vko, proofs[0], E.ZK_TRANSCRIPT_EVM) and engine.verify(vko, proofs[1], E.ZK_TRANSCRIPT_BLAKE2B)
        engine.srs_setup(p.degree, b"\xbb" * 32)
        assert not engine.verify(vko, proofs[0], E.ZK_TRANSCRIPT_EVM)
        assert engine.verify_batch(vko, proofs[1:] * 3, E.ZK_TRANSCRIPT_BLAKE2B) == [False] * 3
        with pytest.raises(zk.ZkError) as ei:  # the full key belongs to the replaced SRS
            engine.verify(pk, proofs[0], E.ZK_TRANSCRIPT_EVM)
        assert ei.value.code == -5
        engine.srs_setup(p.degree, b"\xaa" * 32)
        assert engine.verify(vko, proofs[0], E.ZK_TRANSCRIPT_EVM)
    finally:
        engine.pk_free(vko)
        engine.pk_free(pk)
        for h in adv:
            h.free()


def test_bad_arguments(engine):
    p, pk, adv, ovk, _ = device_key(engine, "k19like")
    try:
        L = engine.L
        import ctypes
        ok = ctypes.c_int(7)
        assert L.zk_verify(engine.ctx, pk, 5, 0, b"", 0, ctypes.byref(ok)) == -1  # unknown transcript
        assert L.zk_verify(engine.ctx, pk, 0, 9, b"", 0, ctypes.byref(ok)) == -1  # unknown scheme
        assert L.zk_verify(engine.ctx, 999999, 0, 0, b"", 0, ctypes.byref(ok)) == -1
        assert L.zk_verify(engine.ctx, pk, 0, 0, b"", 0, None) == -1
        assert L.zk_verify(engine.ctx, pk, 0, 0, b"", 0, ctypes.byref(ok)) == 0 and ok.value == 0  # a verdict, not an error
        v = (ctypes.c_uint8 * 1)()
        lens = (ctypes.c_size_t * 1)(0)
        ptrs = (ctypes.c_char_p * 1)(b"")
        assert L.zk_verify_batch(engine.ctx, pk, 0, 0, 0, ptrs, lens, v) == -1
        assert L.zk_verify_batch(engine.ctx, pk, E.ZK_VERIFY_BATCH_MAX + 1, 0, 0, ptrs, lens, v) == -1
        fc, pc, tr = engine.vk_export(pk)
        with pytest.raises(zk.ZkError):
            bad = fc.copy()
            bad[0, 4] ^= 1  # y changed: off the curve
            engine.vk_from_parts(p, bad, pc, tr)
        with pytest.raises(zk.ZkError):
            engine.vk_from_parts(p, fc[:-1], pc, tr)
        # zk_srs_load without zk_srs_set_g2: no G2 half, ZK_ESTATE
        g = engine.srs_export(E.ZK_BASIS_MONOMIAL, 0, 1 << p.degree)
        gl = engine.srs_export(E.ZK_BASIS_LAGRANGE, 0, 1 << p.degree)
        engine.srs_load(p.degree, g, gl)
        vko = engine.vk_from_parts(p, fc, pc, tr)
        assert L.zk_verify(engine.ctx, vko, 0, 0, b"", 0, ctypes.byref(ok)) == -5
        engine.pk_free(vko)
    finally:
        engine.pk_free(pk)
        for h in adv:
            h.free()


def test_server_verify_endpoints(tmp_path):
    from webauthn_halo2_amd import ecdsa_p256 as api, proving_server as srv

    api.shutdown()
    pkp, vkp = str(tmp_path / "proving_key.pk"), str(tmp_path / "verifying_key.vk")
    try:
        api.download_keys(17, pkp, vkp)
        d, kk, z = 0x1234567, 0x7654321, 0xABCDEF  # an ES256 signature made here: the synthetic provers check it on the host
        q, r = api._p256_mul(d, api._G), api._p256_mul(kk, api._G)[0] % api._N
        sig_s = pow(kk, -1, api._N) * (z + r * d) % api._N
        req = [v.to_bytes(32, "little") for v in (q[0], q[1], r, sig_s, z)]
        pf = api.generate_proof_synthetic(*req, pkp, 17, rng_seed=bytes(32))
        pe = api.generate_proof_evm_synthetic(*req, pkp, 17, rng_seed=bytes(32))
        assert api.verify(17, pf, vkp) and api.verify_evm(17, pe, vkp)
        assert not api.verify(17, pe, vkp) and not api.verify_evm(17, pf, vkp)
        bad = bytearray(pe)
        bad[100] ^= 1
        assert not api.verify_evm(17, bytes(bad), vkp)
        body = lambda proof: json.dumps({"verifying_key_path": vkp, "proof": proof})
        assert srv.verify(body(pf.hex())) == "verified" and srv.verify_evm(body(pe.hex())) == "verified"
        assert srv.verify_evm(body(pe.hex().upper())) == "verified"  # hex::decode takes either case
        assert srv.verify_evm(body(bytes(bad).hex())) == "rejected" and srv.verify(body(pe.hex())) == "rejected"
        for broken in ("0x" + pe.hex(), pe.hex()[:-1], pe.hex() + " ", " " + pe.hex(), pe.hex()[:-2] + "zz"):
            with pytest.raises(ValueError):
                srv.verify_evm(body(broken))
        with pytest.raises(FileNotFoundError):
            api.verify_evm(17, pe, str(tmp_path / "missing.vk"))
        outs = srv.verify_batch([body(pe.hex()), body(bytes(bad).hex()), body("0"), body(pe.hex())], evm=True)
        assert outs[0] == "verified" and outs[1] == "rejected" and isinstance(outs[2], ValueError) and outs[3] == "verified"
    finally:
        api.shutdown()


def test_stream_audit_refuses_nothing(engine):
    p, pk, adv, ovk, (fc, pc, tr) = device_key(engine, "k17like")
    engine.set_option(E.ZK_OPT_STREAM_AUDIT, 1)
    try:
        proof = engine.prove(pk, adv, b"\x44" * 32, E.ZK_TRANSCRIPT_EVM)
        bad = bytearray(proof)
        bad[-1] ^= 1
        vko = engine.vk_from_parts(p, fc, pc, tr)
        assert engine.verify(pk, proof, E.ZK_TRANSCRIPT_EVM)
        assert engine.verify_batch(vko, [proof, bytes(bad), proof, proof], E.ZK_TRANSCRIPT_EVM) == [True, False, True, True]
        checks, violations, msg = engine.audit_report()
        assert checks > 0 and violations == 0, msg
        engine.pk_free(vko)
    finally:
        engine.set_option(E.ZK_OPT_STREAM_AUDIT, 0)
        engine.pk_free(pk)
        for h in adv:
            h.free()
