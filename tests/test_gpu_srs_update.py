"""One ceremony contribution on an MI355X: zk_srs_update (the scaling pass of csrc/g1_ntt.hip feeding the G1 transform, the G2 step
and the receipt of csrc/srs_update.h) against the Python rule (tests/srs_update_ref.py) and the closed forms of the product
secret, zk_srs_contribution_check, what becomes of keys and shared contexts, the failure rules, the stream audit, and the way up
to the server (ecdsa_p256.contribute_params / check_contributions)."""
import ctypes
import json
import random

import numpy as np
import pytest

import srs_update_ref as ref
import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
from zkoracle import cops, curve, fastprover as fp, field as F, plonk, srs
from zkoracle.hashes import ChaCha20Rng
from prover_shapes import SHAPES

pytestmark = pytest.mark.gpu
FMTS = [E.ZK_SERDE_PROCESSED, E.ZK_SERDE_RAW_BYTES, E.ZK_SERDE_RAW_BYTES_UNCHECKED]
ALL = E.ZK_SRS_CHECK_POWERS | E.ZK_SRS_CHECK_LAGRANGE | E.ZK_SRS_CHECK_GENERATORS
SEED_A, SEED_B, SEED_C = bytes(range(32)), bytes(range(100, 132)), b"\xc3" * 32
TAU_A, S_B, S_C = (ref.secret_of_seed(s) for s in (SEED_A, SEED_B, SEED_C))


def G(s):
    return srs.g1_of_scalar(s)


def g1_arr(scalars):
    """[s] G1 for every scalar as the engine's affine Montgomery image (the oracle's C fixed-base multiplication)"""
    return cops.fixed_base_g1(cops.fr_mont([s % F.R for s in scalars]))


def lagrange_scalar(k, x, i):
    """L_i(x) over the 2^k domain"""
    n, wi = 1 << k, pow(F.omega(k), i, F.R)
    return wi * (pow(x, n, F.R) - 1) % F.R * F.inv(n * (x - wi) % F.R, F.R) % F.R


def s_g2_of_image(img, k, fmt=E.ZK_SERDE_RAW_BYTES):
    assert fmt == E.ZK_SERDE_RAW_BYTES
    off = 4 + 2 * (64 << k) + 128
    return ref.g2_from_words(np.frombuffer(img[off:off + 128], dtype=np.uint64))


def fresh(k, seed):
    e = zk.Engine(0)
    e.srs_setup(k, seed)
    return e


# ---- 1. small SRS, every point ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(1, 9))
def test_update_of_a_seed_setup_is_the_srs_of_the_product(k):
    n, t = 1 << k, TAU_A * S_B % F.R
    eng = fresh(k, SEED_A)
    rec = eng.srs_update(SEED_B)
    g, gl = eng.srs_export(0, 0, n), eng.srs_export(1, 0, n)
    assert np.array_equal(g, g1_arr([pow(t, i, F.R) for i in range(n)]))
    assert np.array_equal(gl, g1_arr(srs.lagrange_at(k, t)))
    if k <= 5:  # the Python rule itself, from the SRS of tau_A
        want_g, want_gl = ref.update_both([G(pow(TAU_A, i, F.R)) for i in range(n)], S_B, k)
        assert ref.from_mont_limbs(g) == want_g and ref.from_mont_limbs(gl) == want_gl
    img = eng.srs_write().tobytes()
    assert s_g2_of_image(img, k) == curve.g2_mul(curve.G2_GEN, t)
    assert eng.srs_check(bytes([k]) * 32) == ALL
    assert eng.L.zk_srs_k(eng.ctx) == k
    assert ref.contribution_from_limbs(rec) == ref.contribution(G(TAU_A), S_B)
    eng.close()


# ---- 2. degenerate bases -----------------------------------------------------------------------------------------------------
def inputs(kind, k, rnd):
    """the input kinds of tests/test_gpu_srs_downsize.py"""
    n = 1 << k
    if kind == "random":
        return [G(rnd.randrange(1, F.R)) for _ in range(n)]
    if kind == "identity":
        return [None] * n
    if kind == "repeated":
        return [G(rnd.randrange(1, F.R))] * n
    if kind == "single":
        pts = [None] * n
        pts[rnd.randrange(n)] = G(rnd.randrange(1, F.R))
        return pts
    if kind == "opposite":
        P = G(rnd.randrange(1, F.R))
        return [P if i % 2 == 0 else curve.neg(P) for i in range(n)]
    P, Q = G(rnd.randrange(1, F.R)), G(rnd.randrange(1, F.R))
    return [[P, curve.neg(P), P, Q][i % 4] if i < n // 2 else [P, P, curve.neg(Q), Q][i % 4] for i in range(n)]


@pytest.mark.parametrize("kind", ["random", "identity", "repeated", "single", "opposite", "meet"])
def test_update_of_degenerate_bases_equals_the_reference(engine, kind):
    rnd = random.Random(sum(map(ord, kind)))
    g2, s_g2 = ref.g2_to_words(curve.G2_GEN), curve.g2_mul(curve.G2_GEN, 0x51EC7)
    for k in range(1, 6):
        n = 1 << k
        pts = inputs(kind, k, rnd)
        for seed in ([SEED_B] if k != 3 else [SEED_B, SEED_C]):
            s = ref.secret_of_seed(seed)
            engine.srs_load(k, ref.to_mont_limbs(pts), ref.to_mont_limbs(pts[::-1]))
            engine.srs_set_g2(g2, ref.g2_to_words(s_g2))
            rec = engine.srs_update(seed)
            want_g, want_gl = ref.update_both(pts, s, k)
            assert ref.from_mont_limbs(engine.srs_export(0, 0, n)) == want_g, (kind, k)
            assert ref.from_mont_limbs(engine.srs_export(1, 0, n)) == want_gl, (kind, k)
            if kind == "identity":
                assert want_g == [None] * n and want_gl == [None] * n
            assert s_g2_of_image(engine.srs_write().tobytes(), k) == curve.g2_mul(s_g2, s)
            got = ref.contribution_from_limbs(rec)
            assert got == ref.contribution(pts[1], s), (kind, k)


# ---- 3. commutativity, whole files -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 14, 17, 19])
def test_contributions_commute(k):
    ab = fresh(k, SEED_A)
    ab.srs_update(SEED_B)
    ba = fresh(k, SEED_B)
    ba.srs_update(SEED_A)
    for fmt in FMTS:
        assert ab.srs_write(fmt).tobytes() == ba.srs_write(fmt).tobytes(), (k, fmt)
    ba.close()
    assert ab.srs_check(b"\x05" * 32) == ALL
    rec = ab.srs_update(SEED_C)  # two updates in a row
    assert ab.srs_check(b"\x06" * 32) == ALL
    t = TAU_A * S_B % F.R * S_C % F.R
    assert np.array_equal(ab.srs_export(0, 1, 1), g1_arr([t]))
    assert ref.contribution_from_limbs(rec) == ref.contribution(G(TAU_A * S_B), S_C)
    assert ab.srs_contribution_check(rec) == 15
    ab.close()


# ---- 4. full size ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [19, 21])
def test_full_size_update(k):
    n, t = 1 << k, TAU_A * S_B % F.R
    eng = fresh(k, SEED_A)
    eng.srs_update(SEED_B)
    for i in (0, 1, 2, n // 2, n - 1):
        assert np.array_equal(eng.srs_export(0, i, 1), g1_arr([pow(t, i, F.R)])), (k, i)
        assert np.array_equal(eng.srs_export(1, i, 1), g1_arr([lagrange_scalar(k, t, i)])), (k, i)
    assert eng.srs_check(b"\x07" * 32) == ALL
    a = np.frombuffer(np.random.default_rng(k).bytes(n * 32), dtype=np.uint64).reshape(n, 4).copy()
    a[:, 3] &= 0x0FFFFFFFFFFFFFFF
    want = g1_arr([srs.commit_scalar_monomial(cops.fr_ints(a), x=t)])[0]  # [f(tau')] G1, Horner
    p = eng.poly(n, a)
    assert np.array_equal(eng.commit(p, E.ZK_BASIS_MONOMIAL), want)
    eng.upload(p, cops.ntt(a, F.omega(k), k))  # the values of f over the domain: sum_i f(w^i) L_i(tau') = f(tau')
    assert np.array_equal(eng.commit(p, E.ZK_BASIS_LAGRANGE), want)
    p.free()
    eng.close()


# ---- 5. receipts -----------------------------------------------------------------------------------------------------------------
def test_receipts():
    k = 6
    eng = fresh(k, SEED_A)
    other = fresh(k, SEED_C)
    empty = zk.Engine(0)
    rec = eng.srs_update(SEED_B)
    honest = (TAU_A, TAU_A * S_B % F.R, S_B, S_B)
    want = ref.contribution_of_scalars(*honest)
    assert ref.contribution_from_limbs(rec) == want == ref.contribution(G(TAU_A), S_B)
    assert ref.expected_flags(*honest) == 7
    assert eng.srs_contribution_check(rec) == 15
    assert other.srs_contribution_check(rec) == 7  # a context holding another SRS: only RESIDENT goes
    assert empty.srs_contribution_check(rec) == 7  # (and one holding none)
    rnd = random.Random(5)
    for field in range(4):
        t = list(honest)
        t[field] = rnd.randrange(2, F.R)
        bad = ref.contribution_to_limbs(ref.contribution_of_scalars(*t))
        for f in ref.FIELDS:  # (only the one field differs from the engine's own receipt)
            assert np.array_equal(bad[f], rec[f]) == (f != ref.FIELDS[field])
        predicted = ref.expected_flags(*t) | (0 if ref.FIELDS[field] == "after_g1" else ref.RESIDENT)
        assert eng.srs_contribution_check(bad) == predicted, ref.FIELDS[field]
        assert bin(15 ^ predicted).count("1") == {"before_g1": 1, "after_g1": 2, "s_g1": 1, "s_g2": 2}[ref.FIELDS[field]]
    off = {f: np.array(rec[f]) for f in ref.FIELDS}
    off["s_g1"][0] ^= np.uint64(1)  # off the curve
    assert eng.srs_contribution_check(off) == ref.RESIDENT
    unit = ref.contribution_to_limbs(ref.contribution_of_scalars(TAU_A * S_B, TAU_A * S_B, 1, 1))  # the step by s = 1
    assert eng.srs_contribution_check(unit) == ref.SAME_SECRET | ref.LINKS | ref.RESIDENT
    flags = ctypes.c_uint32(99)
    assert eng.L.zk_srs_contribution_check(eng.ctx, None, ctypes.byref(flags)) == -1 and flags.value == 99
    for e in (eng, other, empty):
        e.close()


# ---- 6. keys and contexts --------------------------------------------------------------------------------------------------------
def test_keys_and_shared_contexts():
    A, L, Fx, k, lb = SHAPES["k19like"]
    p = zk.circuit.CircuitParams(degree=k, num_advice=A, num_lookup_advice=L, num_fixed=Fx, lookup_bits=lb)
    asg = zk.circuit.synthesize(p, 11)
    fixed = np.stack([asg.to_limbs(c) for c in asg.fixed])
    n, seed = 1 << k, b"\x44" * 32
    eng = fresh(k, SEED_A)
    pk_old = eng.keygen(p, fixed, asg.copies)
    child = zk.Engine(0, share_with=eng)
    pk_child = child.keygen(p, fixed, asg.copies)

    def advice(e):
        hs = []
        for col in asg.advice:
            h = e.poly(n)
            e.upload_canonical(h, asg.to_limbs(col))
            hs.append(h)
        return hs

    def prove(e, pk):
        hs = advice(e)
        try:
            return e.prove(pk, hs, seed, E.ZK_TRANSCRIPT_EVM)
        finally:
            for h in hs:
                h.free()

    want_old = prove(eng, pk_old)
    assert prove(child, pk_child) == want_old
    old_image = eng.srs_write().tobytes()
    eng.srs_update(SEED_B)
    hs = advice(eng)
    for call in (lambda: eng.prove(pk_old, hs, seed, E.ZK_TRANSCRIPT_EVM), lambda: eng.witness_check(pk_old, hs), lambda: eng.pk_check(pk_old)):
        with pytest.raises(zk.ZkError) as ex:
            call()
        assert ex.value.code == -5
    for h in hs:
        h.free()
    assert child.srs_write().tobytes() == old_image  # shared before the call: the old SRS, and its key proves the same bytes
    assert prove(child, pk_child) == want_old
    # a key made after the update: the oracle prover over a committer built on the exported bases gives the same bytes
    pk_new = eng.keygen(p, fixed, asg.copies)
    proof = prove(eng, pk_new)
    assert proof != want_old
    cm = fp.Committer(k, "msm", g=eng.srs_export(0, 0, n), g_lagrange=eng.srs_export(1, 0, n))
    sh = plonk.Shape(k, A, L, Fx, lb)
    opk = fp.keygen(sh, asg.fixed, asg.copies, cm)
    assert proof == fp.create_proof(opk, asg.advice, ChaCha20Rng(seed), "evm", committer=cm)
    assert cm.count > 0
    assert eng.verify(pk_new, proof, E.ZK_TRANSCRIPT_EVM, E.ZK_SCHEME_GWC)
    # verifying-only keys: each SRS accepts its own proofs and rejects the other's
    vk_new_on_old = child.vk_read(p, eng.vk_write(pk_new).tobytes())
    vk_old_on_new = eng.vk_read(p, child.vk_write(pk_child).tobytes())
    vk_new_on_new = eng.vk_read(p, eng.vk_write(pk_new).tobytes())
    assert eng.verify(vk_new_on_new, proof, E.ZK_TRANSCRIPT_EVM, E.ZK_SCHEME_GWC)
    assert not child.verify(vk_new_on_old, proof, E.ZK_TRANSCRIPT_EVM, E.ZK_SCHEME_GWC)
    assert not eng.verify(vk_old_on_new, want_old, E.ZK_TRANSCRIPT_EVM, E.ZK_SCHEME_GWC)
    assert child.verify(pk_child, want_old, E.ZK_TRANSCRIPT_EVM, E.ZK_SCHEME_GWC)
    for e, h in ((eng, pk_old), (eng, pk_new), (eng, vk_old_on_new), (eng, vk_new_on_new), (child, pk_child), (child, vk_new_on_old)):
        e.pk_free(h)
    child.close()
    eng.close()


# ---- 7. errors and atomicity -----------------------------------------------------------------------------------------------------
def test_errors_and_atomicity():
    k = 7
    A, L, Fx, _, lb = SHAPES["k19like"]
    p = zk.circuit.CircuitParams(degree=k, num_advice=A, num_lookup_advice=L, num_fixed=Fx, lookup_bits=lb)
    asg = zk.circuit.synthesize(p, 12)
    eng = zk.Engine(0)
    rec = E.SrsContributionC()
    marker = bytes(range(64)) * 5
    ctypes.memmove(ctypes.byref(rec), marker, 320)
    assert eng.L.zk_srs_update(eng.ctx, SEED_B, ctypes.byref(rec)) == -5  # no SRS
    assert bytes(rec) == marker
    src = fresh(k, SEED_A)
    n = 1 << k
    g, gl = src.srs_export(0, 0, n), src.srs_export(1, 0, n)
    eng.srs_load(k, g, gl)  # no G2 half
    pk = eng.keygen(p, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
    h = eng.poly(n)
    eng.upload_canonical(h, asg.to_limbs(asg.advice[0]))
    proof = eng.prove(pk, [h], b"\x09" * 32, E.ZK_TRANSCRIPT_EVM)
    assert eng.L.zk_srs_update(eng.ctx, SEED_B, ctypes.byref(rec)) == -5
    assert bytes(rec) == marker
    assert np.array_equal(eng.srs_export(0, 0, n), g) and np.array_equal(eng.srs_export(1, 0, n), gl)
    assert eng.L.zk_srs_k(eng.ctx) == k
    assert eng.prove(pk, [h], b"\x09" * 32, E.ZK_TRANSCRIPT_EVM) == proof
    assert eng.L.zk_srs_update(None, SEED_B, ctypes.byref(rec)) == -1
    assert eng.L.zk_srs_update(src.ctx, None, ctypes.byref(rec)) == -1
    assert bytes(rec) == marker
    assert src.srs_write().tobytes() == fresh_image(k, SEED_A)
    with pytest.raises(ValueError):
        src.srs_update(bytes(31))
    # out == NULL works, and the same start and seed give the same bytes
    assert src.L.zk_srs_update(src.ctx, SEED_B, None) == 0
    again = fresh(k, SEED_A)
    r2 = again.srs_update(SEED_B)
    assert src.srs_write().tobytes() == again.srs_write().tobytes()
    third = fresh(k, SEED_A)
    r3 = third.srs_update(SEED_B)
    assert all(np.array_equal(r2[f], r3[f]) for f in ref.FIELDS)
    assert src.srs_contribution_check(r2) == 15
    # the G2 half given, the loaded SRS updates like the set-up one
    img = fresh_image(k, SEED_A)
    off = 4 + 2 * n * 64
    eng.srs_set_g2(np.frombuffer(img[off:off + 128], dtype=np.uint64), np.frombuffer(img[off + 128:off + 256], dtype=np.uint64))
    eng.srs_update(SEED_B)
    assert eng.srs_write().tobytes() == src.srs_write().tobytes()
    with pytest.raises(zk.ZkError) as ex:
        eng.prove(pk, [h], b"\x09" * 32, E.ZK_TRANSCRIPT_EVM)
    assert ex.value.code == -5
    h.free()
    eng.pk_free(pk)
    for e in (eng, src, again, third):
        e.close()


def fresh_image(k, seed):
    e = fresh(k, seed)
    img = e.srs_write().tobytes()
    e.close()
    return img


# ---- 8. stream audit -------------------------------------------------------------------------------------------------------------
def test_update_under_the_stream_audit():
    eng = zk.Engine(0)
    eng.set_option(E.ZK_OPT_STREAM_AUDIT, 1)
    eng.srs_setup(12, SEED_A)
    rec = eng.srs_update(SEED_B)
    checks, violations, msg = eng.audit_report()
    assert violations == 0, msg
    assert eng.srs_contribution_check(rec) == 15 and eng.srs_check() == ALL
    assert eng.audit_report()[1] == 0
    eng.close()


# ---- 9. through the server -------------------------------------------------------------------------------------------------------
def es256_request():
    from webauthn_halo2_amd import ecdsa_p256 as api

    d, kk, z = 0x1234567, 0x7654321, 0xABCDEF
    q, r = api._p256_mul(d, api._G), api._p256_mul(kk, api._G)[0] % api._N
    sig_s = pow(kk, -1, api._N) * (z + r * d) % api._N
    return [v.to_bytes(32, "little") for v in (q[0], q[1], r, sig_s, z)]


def test_contribution_through_the_server(tmp_path):
    import hashlib

    from webauthn_halo2_amd import ecdsa_p256 as api, proving_server as srv

    f, f2 = str(tmp_path / "kzg_bn254_17_mine.srs"), str(tmp_path / "kzg_bn254_17_ours.srs")
    receipt = api.contribute_params(None, f, SEED_B, degree=17)
    json.dumps(receipt)
    assert receipt["k"] == 17 and receipt["src_sha256"] is None
    assert receipt["dst_sha256"] == hashlib.sha256(open(f, "rb").read()).hexdigest()
    assert receipt["before_g1"] == ref.to_mont_limbs([G(srs.TAU)])[0].astype("<u8").tobytes().hex()
    assert receipt["after_g1"] == ref.to_mont_limbs([G(srs.TAU * S_B)])[0].astype("<u8").tobytes().hex()
    assert api.check_contributions(f, [receipt])
    second = api.contribute_params(f, f2, SEED_C)
    assert second["src_sha256"] == receipt["dst_sha256"] and second["before_g1"] == receipt["after_g1"]
    assert api.check_contributions(f2, [receipt, second])
    assert not api.check_contributions(f2, [receipt])  # the file is one step further
    assert not api.check_contributions(f, [receipt, second])
    assert not api.check_contributions(f2, [second, receipt])
    assert not api.check_contributions(f2, [receipt, dict(second, s_g1=receipt["s_g1"])])
    with pytest.raises(ValueError):
        api.contribute_params(f, f, SEED_C)
    req = es256_request()
    body = {"pubkey_x": list(req[0]), "pubkey_y": list(req[1]), "r": list(req[2]), "s": list(req[3]), "msghash": list(req[4])}
    pkp, vkp, vk0 = str(tmp_path / "proving_key.pk"), str(tmp_path / "verifying_key.vk"), str(tmp_path / "verifying_key_0.vk")
    b = dict(body, proving_key_path=pkp)
    vbody = lambda path, proof: json.dumps({"verifying_key_path": path, "proof": proof})
    api.shutdown()
    try:
        srv.setup(0, 17, pkp, vk0)  # the seed-0 SRS
        under_seed0 = srv.prove_evm(b, rng_seed=bytes(32))
        assert srv.verify_evm(vbody(vk0, under_seed0)) == "verified"
        srv.setup(0, 17, pkp, vkp, params_path=f)
        proof = srv.prove_evm(b, rng_seed=bytes(32))
        assert proof != under_seed0
        assert srv.verify_evm(vbody(vkp, proof)) == "verified"
        assert srv.verify_evm(vbody(vkp, under_seed0)) == "rejected"  # the same request proved under the seed-0 SRS
        assert srv.verify_evm(vbody(vk0, under_seed0)) == "rejected"  # (its own key's commitments belong to the other SRS too)
    finally:
        api.set_params_file(None)
        api.shutdown()
