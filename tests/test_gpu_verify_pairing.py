"""zk_verify_pairing_mode on an MI355X: the verdicts of batches with pairing-failing proofs are the same under the host bisection
(mode 1), the device pairing (mode 2, csrc/pairing.hip through settle() of csrc/verify.hip) and auto, and zk_verify_pairing_stats
shows which route ran: under mode 2 a failing fold of B live proofs costs exactly one host check and B device pairs, an all-good
batch one host check and none.  Failing proofs decode: one evaluation altered, or the same circuit's proof under another SRS.
Small shapes of tests/verify_cases.py; the server surface at the k = 17 shape its keys have."""
import ctypes
import json

import numpy as np
import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
from zkoracle.field import P, R
import public_cases as pub
import verify_cases as vc

pytestmark = pytest.mark.gpu

T = {"evm": E.ZK_TRANSCRIPT_EVM, "blake2b": E.ZK_TRANSCRIPT_BLAKE2B}
S = {"gwc": E.ZK_SCHEME_GWC, "shplonk": E.ZK_SCHEME_SHPLONK}
PAIRINGS = [("evm", "gwc"), ("blake2b", "shplonk")]
HOST, DEVICE = E.ZK_VERIFY_PAIRING_HOST, E.ZK_VERIFY_PAIRING_DEVICE


def altered_evaluation(proof, shape, kind):
    """the proof with its first evaluation replaced by the next scalar: canonical, so the proof decodes and fails at the pairing"""
    ps = 64 if kind == "evm" else 32
    off = shape.n_points_before_multiopen() * ps
    order = "big" if kind == "evm" else "little"
    b = bytearray(proof)
    b[off:off + 32] = ((int.from_bytes(b[off:off + 32], order) + 1) % R).to_bytes(32, order)
    return bytes(b)


@pytest.fixture(scope="module")
def made():
    """One engine with the k19like key under SRS A resident; per transcript: good proofs, proofs with an altered evaluation, and
    the same circuit's proofs made under SRS B."""
    eng = zk.Engine(0)
    p = vc.params_of("k19like")
    asg = zk.circuit.synthesize(p, 0x5EED0019)
    fixed = np.stack([asg.to_limbs(c) for c in asg.fixed])
    adv = [eng.poly(1 << p.degree) for _ in asg.advice]
    for h, col in zip(adv, asg.advice):
        eng.upload_canonical(h, asg.to_limbs(col))
    shape = vc.oracle_shape(p)
    out = {"eng": eng, "shape": shape, "good": {}, "altered": {}, "other_srs": {}}
    eng.srs_setup(p.degree, b"\xbb" * 32)
    pk_b = eng.keygen(p, fixed, asg.copies)
    for kind, scheme in PAIRINGS:
        out["other_srs"][kind] = [eng.prove(pk_b, adv, bytes([0x60 + i]) * 32, T[kind], S[scheme]) for i in range(2)]
    eng.pk_free(pk_b)
    eng.srs_setup(p.degree, b"\xaa" * 32)
    pk = eng.keygen(p, fixed, asg.copies)
    for kind, scheme in PAIRINGS:
        out["good"][kind] = [eng.prove(pk, adv, bytes([0x40 + i]) * 32, T[kind], S[scheme]) for i in range(4)]
        out["altered"][kind] = [altered_evaluation(g, shape, kind) for g in out["good"][kind][:2]]
    fc, pc, tr = eng.vk_export(pk)
    out["vk"] = eng.vk_from_parts(p, fc, pc, tr)
    for h in adv:
        h.free()
    yield out
    eng.close()


def bisection_checks(live_ok):
    """host pairing checks of settle() over the live proofs' own verdicts: one per set, halves on failure"""
    if not live_ok:
        return 0
    if all(live_ok) or len(live_ok) == 1:
        return 1
    h = len(live_ok) // 2
    return 1 + bisection_checks(live_ok[:h]) + bisection_checks(live_ok[h:])


def run(made, mode, kind, batch):
    """(verdicts, host checks, device pairs) of one zk_verify_batch call under `mode`"""
    eng = made["eng"]
    eng.verify_pairing_mode(mode)
    h0, d0 = eng.verify_pairing_stats()
    scheme = dict(PAIRINGS)[kind]
    got = eng.verify_batch(made["vk"], batch, T[kind], S[scheme])
    h1, d1 = eng.verify_pairing_stats()
    eng.verify_pairing_mode(E.ZK_VERIFY_PAIRING_AUTO)
    return got, h1 - h0, d1 - d0


def batch_of(made, kind, B, bad_at):
    good, bad = made["good"][kind], made["altered"][kind] + made["other_srs"][kind]
    return [bad[j % len(bad)] if j in bad_at else good[j % len(good)] for j in range(B)]


@pytest.mark.parametrize("kind", ["evm", "blake2b"])
@pytest.mark.parametrize("B", [2, 8, 65])
def test_failing_batches(made, kind, B):
    for bad_at in ({0}, {B // 2}, {B - 1}, {0, B // 2, B - 1}, set(range(B)), set()):
        batch = batch_of(made, kind, B, bad_at)
        want = [j not in bad_at for j in range(B)]
        got_h, hh, hd = run(made, HOST, kind, batch)
        got_d, dh, dd = run(made, DEVICE, kind, batch)
        assert got_h == want and got_d == want, sorted(bad_at)
        assert (hh, hd) == (bisection_checks(want), 0), sorted(bad_at)
        if len(bad_at) <= 1:  # auto is the host: the same verdicts and the same counters
            assert run(made, E.ZK_VERIFY_PAIRING_AUTO, kind, batch) == (want, hh, hd), sorted(bad_at)
        if bad_at:
            assert hh > 1 and (dh, dd) == (1, B), sorted(bad_at)
        else:
            assert (hh, dh, dd) == (1, 1, 0)


def test_both_kinds_of_failing_proof_fail_alone(made):
    eng = made["eng"]
    for kind, scheme in PAIRINGS:
        for proof in made["altered"][kind] + made["other_srs"][kind]:
            assert not eng.verify(made["vk"], proof, T[kind], S[scheme])
        assert all(eng.verify(made["vk"], g, T[kind], S[scheme]) for g in made["good"][kind])


def test_proofs_that_fail_before_the_pairing_are_not_device_pairs(made):
    good, bad = made["good"]["evm"], made["altered"]["evm"]
    off = (made["shape"].n_points_before_multiopen() - 1) * 64
    pt = bytearray(good[1])
    y = int.from_bytes(pt[off + 32:off + 64], "big")
    pt[off + 32:off + 64] = ((y + 1) % P).to_bytes(32, "big")  # a point off the curve
    batch = [good[0], good[1][:-32], bad[0], bytes(pt), good[2], bad[1], good[3], b""]
    want = [True, False, False, False, True, False, True, False]
    live = [True, False, True, False, True]  # the five proofs that reach the fold
    got_h, hh, hd = run(made, HOST, "evm", batch)
    got_d, dh, dd = run(made, DEVICE, "evm", batch)
    assert got_h == want and got_d == want
    assert (hh, hd) == (bisection_checks(live), 0) and (dh, dd) == (1, 5)
    # one live proof left: a set of one stays on the host
    got_d, dh, dd = run(made, DEVICE, "evm", [good[0][:-32], bad[0], b""])
    assert got_d == [False, False, False] and (dh, dd) == (1, 0)


def test_single_verify_stays_on_the_host(made):
    eng = made["eng"]
    eng.verify_pairing_mode(DEVICE)
    try:
        for proof, want in ((made["good"]["evm"][0], True), (made["altered"]["evm"][0], False)):
            before = eng.verify_pairing_stats()
            assert eng.verify(made["vk"], proof, E.ZK_TRANSCRIPT_EVM, E.ZK_SCHEME_GWC) == want
            after = eng.verify_pairing_stats()
            assert (after[0] - before[0], after[1] - before[1]) == (1, 0)
    finally:
        eng.verify_pairing_mode(E.ZK_VERIFY_PAIRING_AUTO)


def test_mode_outside_the_three_is_refused(made):
    eng = made["eng"]
    assert eng.L.zk_verify_pairing_mode(eng.ctx, 3) == -1 and eng.L.zk_verify_pairing_mode(eng.ctx, -1) == -1
    assert eng.L.zk_verify_pairing_mode(None, 1) == -1
    assert eng.L.zk_verify_pairing_stats(eng.ctx, None) == -1
    out = (ctypes.c_uint64 * 2)()
    assert eng.L.zk_verify_pairing_stats(None, out) == -1
    with pytest.raises(zk.ZkError):
        eng.verify_pairing_mode(3)
    # the refused calls changed nothing: a failing batch still goes the host's way
    batch = batch_of(made, "evm", 4, {1})
    assert run(made, E.ZK_VERIFY_PAIRING_AUTO, "evm", batch)[1:] == (bisection_checks([True, False, True, True]), 0)


def test_public_batch_follows():
    eng = zk.Engine(0)
    try:
        name, t, s = "k17like", E.ZK_TRANSCRIPT_BLAKE2B, E.ZK_SCHEME_SHPLONK
        asg = pub.witness(name, 9)
        pk, sets = pub.engine_key(eng, name, [asg])
        proof = eng.prove_public(pk, sets[0], pub.mont(asg.instance), pub.SEED, t, s)
        right, wrong = pub.mont(asg.instance), pub.mont(pub.wrong_lists(asg.instance)[0][1])  # one changed value: fails at the pairing
        B = 5
        lists = [wrong if j in (1, 4) else right for j in range(B)]
        want = [j not in (1, 4) for j in range(B)]
        res = {}
        for mode in (HOST, DEVICE):
            eng.verify_pairing_mode(mode)
            before = eng.verify_pairing_stats()
            got = eng.verify_batch_public(pk, [proof] * B, lists, t, s)
            after = eng.verify_pairing_stats()
            assert got == want, mode
            res[mode] = (after[0] - before[0], after[1] - before[1])
        assert res[HOST] == (bisection_checks(want), 0) and res[DEVICE] == (1, B)
    finally:
        eng.close()


def test_server_outputs_are_the_same_strings(tmp_path):
    from webauthn_halo2_amd import ecdsa_p256 as api, proving_server as srv

    api.shutdown()
    pkp, vkp = str(tmp_path / "proving_key.pk"), str(tmp_path / "verifying_key.vk")
    try:
        api.download_keys(17, pkp, vkp)
        d, kk, z = 0x1234567, 0x7654321, 0xABCDEF
        q, r = api._p256_mul(d, api._G), api._p256_mul(kk, api._G)[0] % api._N
        sig_s = pow(kk, -1, api._N) * (z + r * d) % api._N
        req = [v.to_bytes(32, "little") for v in (q[0], q[1], r, sig_s, z)]
        pe = api.generate_proof_evm_synthetic(*req, pkp, 17, rng_seed=bytes(32))
        bad = altered_evaluation(pe, vc.oracle_shape(zk.circuit.K17), "evm")
        body = lambda proof: json.dumps({"verifying_key_path": vkp, "proof": proof.hex()})
        bodies = [body(pe), body(bad), body(pe), body(bad)]
        outs = {}
        for mode in ("host", "device"):
            api.set_verify_pairing(mode)
            eng, _ = api._resident_vk(17, vkp, 0)
            before = eng.verify_pairing_stats()
            outs[mode] = srv.verify_batch(bodies, evm=True)
            after = eng.verify_pairing_stats()
            assert (after[1] - before[1]) == (4 if mode == "device" else 0)
            assert srv.verify_evm(body(pe)) == "verified" and srv.verify_evm(body(bad)) == "rejected"
        assert outs["host"] == outs["device"] == ["verified", "rejected", "verified", "rejected"]
    finally:
        api.set_verify_pairing("auto")
        api.shutdown()
