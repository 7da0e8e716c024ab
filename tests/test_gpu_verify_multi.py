"""zk_verify_multi (csrc/verifier.h with a circuit count, csrc/verify.hip): verify_proof of ONE proof over N circuits.  Proofs of
zk_prove_multi and of tests/halo2_ref.py are accepted; one flipped byte in a circuit's advice commitment, an h piece, a shared fixed
evaluation, a circuit's lookup evaluation or the last opening, another circuit count, or the single-circuit verifier each give the
verdict 0 — a verdict, never an error — and a verifying-only key read from the key's own image says the same as the full key."""
import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
from zkoracle.hashes import ChaCha20Rng
import halo2_ref
from multi_cases import PAIRINGS, SEED, engine_key, oracle_key, params_of, tampered, witnesses

pytestmark = pytest.mark.gpu

KIND = {"evm": E.ZK_TRANSCRIPT_EVM, "blake2b": E.ZK_TRANSCRIPT_BLAKE2B}
SCHEME = {"gwc": E.ZK_SCHEME_GWC, "shplonk": E.ZK_SCHEME_SHPLONK}


@pytest.mark.parametrize("name,N", [("k17like", 2), ("wide", 3)])
def test_verdicts(name, N):
    eng = zk.Engine(0)
    asgs = witnesses(name, N)
    opk = oracle_key(name, asgs[0])
    pk, sets = engine_key(eng, name, asgs)
    vk = eng.vk_read(params_of(name), eng.vk_write(pk))
    for kind, scheme in PAIRINGS:
        t, s = KIND[kind], SCHEME[scheme]
        proof = eng.prove_multi(pk, sets, SEED, t, s)
        cases = [("intact", proof, N, True)]
        cases += [(place, bad, N, False) for place, bad in tampered(proof, opk.shape, N, kind, scheme)]
        cases += [("N - 1", proof, N - 1, False), ("N + 1", proof, N + 1, False), ("truncated", proof[:-32], N, False), ("empty", b"", N, False)]
        for label, data, count, want in cases:
            assert eng.verify_multi(pk, count, data, t, s) is want, (kind, label)
            assert eng.verify_multi(vk, count, data, t, s) is want, (kind, label, "verifying-only key")
        assert not eng.verify(pk, proof, t, s)  # the single-circuit verifier reads another layout
        assert halo2_ref.verify(opk.vk, proof, [[]] * N, kind, scheme)
    eng.close()


def test_reference_proofs_and_argument_errors():
    eng = zk.Engine(0)
    asgs = witnesses("k18like", 2)
    opk = oracle_key("k18like", asgs[0])
    pk, _ = engine_key(eng, "k18like", asgs[:1])
    for kind, scheme in PAIRINGS:
        proof = halo2_ref.create_proof(opk, [a.advice for a in asgs], None, ChaCha20Rng(SEED), kind, scheme)
        assert eng.verify_multi(pk, 2, proof, KIND[kind], SCHEME[scheme])
        assert not eng.verify_multi(pk, 2, proof, KIND["blake2b" if kind == "evm" else "evm"], SCHEME[scheme])
    for bad_n in (0, E.ZK_PROVE_MULTI_MAX + 1):
        with pytest.raises(zk.ZkError) as e:
            eng.verify_multi(pk, bad_n, proof, KIND[kind])
        assert e.value.code == -1
    eng.close()


def test_server_multi_endpoints(tmp_path):
    """proving_server.prove_multi / verify_multi (extensions of the reference's JSON contract): a list of request bodies in, one
    hex proof out; each body passes the ES256 check first; the verifier must be told the same count."""
    import json

    from webauthn_halo2_amd import ecdsa_p256 as api, proving_server as srv

    api.shutdown()
    pkp, vkp = str(tmp_path / "proving_key.pk"), str(tmp_path / "verifying_key.vk")
    try:
        api.download_keys(17, pkp, vkp)
        bodies = []
        for d, kk, z in ((0x1234567, 0x7654321, 0xABCDEF), (0x2345671, 0x6543217, 0xBCDEFA)):  # ES256 signatures made here
            q, r = api._p256_mul(d, api._G), api._p256_mul(kk, api._G)[0] % api._N
            sig_s = pow(kk, -1, api._N) * (z + r * d) % api._N
            vals = dict(zip(("pubkey_x", "pubkey_y", "r", "s", "msghash"), (list(v.to_bytes(32, "little")) for v in (q[0], q[1], r, sig_s, z))))
            bodies.append(json.dumps(dict(vals, proving_key_path=pkp)))
        body = lambda proof, n: json.dumps({"verifying_key_path": vkp, "proof": proof, "num_proof": n})
        for evm in (True, False):
            proof = srv.prove_multi(bodies, evm=evm, rng_seed=bytes(32))
            assert srv.verify_multi(body(proof, 2), evm=evm) == "verified"
            assert srv.verify_multi(body(proof, 3), evm=evm) == "rejected" and srv.verify_multi(body(proof, 1), evm=evm) == "rejected"
            assert srv.verify_multi(body(proof, 2), evm=not evm) == "rejected"
            assert (srv.verify_evm if evm else srv.verify)(json.dumps({"verifying_key_path": vkp, "proof": proof})) == "rejected"
            one = srv.prove_multi(bodies[:1], evm=evm, rng_seed=bytes(32))
            assert one == (srv.prove_evm if evm else srv.prove)(bodies[0], rng_seed=bytes(32))  # one request: the reference's proof
        forged = json.loads(bodies[1])
        forged["msghash"][0] ^= 1
        with pytest.raises(ValueError):
            srv.prove_multi([bodies[0], json.dumps(forged)])
        with pytest.raises(ValueError):
            srv.verify_multi(json.dumps({"verifying_key_path": vkp, "proof": proof}))  # no count
    finally:
        api.shutdown()
