"""proving_server / ecdsa_p256 / batch with public inputs in the batch and multi forms, at a k = 10 config (ECDSA_CONFIG: the
smallest the request path is exercised at): prove_batch(public=True) strings verify through verify_batch(public=9) and one string
with a changed instance word is "rejected"; prove_multi(public=True) answers all circuits' instance words in circuit order, then
the proof, which verify_multi(public=9) accepts with the same count only; Pipeline.prove_lockstep(instances=...) gives
Engine.prove_public's bytes.  Every default is the form without instances."""
import json

import numpy as np
import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E

pytestmark = pytest.mark.gpu


def requests(api, pkp, count):
    """`count` request bodies with ES256 signatures made here (plain secp256r1 arithmetic of the module itself)."""
    out = []
    for i in range(count):
        d, kk, z = 0x1234567 + 11 * i, 0x7654321 + 7 * i, int.from_bytes(bytes([0x21 + i]) * 32, "big") % api._N
        q, r = api._p256_mul(d, api._G), api._p256_mul(kk, api._G)[0] % api._N
        s = pow(kk, -1, api._N) * (z + r * d) % api._N
        vals = dict(zip(("pubkey_x", "pubkey_y", "r", "s", "msghash"), (list(v.to_bytes(32, "little")) for v in (q[0], q[1], r, s, z))))
        out.append(dict(vals, proving_key_path=pkp))
    return out


def words_of(api, body):
    return api.public_inputs(bytes(body["msghash"]), bytes(body["pubkey_x"]), bytes(body["pubkey_y"]))


def test_batch_and_multi_endpoints(tmp_path, monkeypatch):
    api, srv = zk.ecdsa_p256, zk.proving_server
    api.shutdown()
    cfg = tmp_path / "ecdsa_circuit.config"
    cfg.write_text(json.dumps({"degree": 10, "num_advice": 3, "num_lookup_advice": 2, "num_fixed": 1, "lookup_bits": 8}) + "\n")
    monkeypatch.setenv("ECDSA_CONFIG", str(cfg))
    pkp, vkp = str(tmp_path / "proving_key.pk"), str(tmp_path / "verifying_key.vk")
    try:
        srv.setup(degree=10, proving_key_path=pkp, verifying_key_path=vkp, public=True)
        bodies = requests(api, pkp, 3)
        vbody = lambda proof, **kw: json.dumps(dict({"verifying_key_path": vkp, "proof": proof}, **kw))
        for evm in (True, False):
            # -- the batch: every answer carries its nine words; one changed word is one "rejected"
            hexed = srv.prove_batch(bodies, evm=evm, degree=10, public=True)
            assert all(isinstance(h, str) for h in hexed), hexed
            for h, b in zip(hexed, bodies):
                assert bytes.fromhex(h)[:288] == b"".join(v.to_bytes(32, "big") for v in words_of(api, b))
            assert srv.verify_batch([vbody(h) for h in hexed], evm=evm, degree=10, public=9) == ["verified"] * 3
            forged = bytearray(bytes.fromhex(hexed[1]))
            forged[31] ^= 1  # the lowest byte of the first instance word
            got = srv.verify_batch([vbody(hexed[0]), vbody(bytes(forged).hex()), vbody(hexed[2]), vbody("00" * 64)], evm=evm, degree=10, public=9)
            assert got[:3] == ["verified", "rejected", "verified"] and isinstance(got[3], ValueError)
            assert srv.verify_batch([vbody(hexed[0])], evm=not evm, degree=10, public=9) == ["rejected"]
            # -- one proof over the three requests
            multi = srv.prove_multi(bodies, evm=evm, degree=10, rng_seed=bytes(32), public=True)
            raw = bytes.fromhex(multi)
            assert raw[:3 * 288] == b"".join(v.to_bytes(32, "big") for b in bodies for v in words_of(api, b))
            assert srv.verify_multi(vbody(multi, num_proof=3), evm=evm, degree=10, public=9) == "verified"
            swapped = raw[288:576] + raw[:288] + raw[576:]  # circuits 0 and 1 exchange their words
            assert srv.verify_multi(vbody(swapped.hex(), num_proof=3), evm=evm, degree=10, public=9) == "rejected"
            changed = bytearray(raw)
            changed[288 + 31] ^= 1  # one word of circuit 1
            assert srv.verify_multi(vbody(bytes(changed).hex(), num_proof=3), evm=evm, degree=10, public=9) == "rejected"
            assert srv.verify_multi(vbody(multi, num_proof=2), evm=evm, degree=10, public=9) == "rejected"
            one = srv.prove_multi(bodies[:1], evm=evm, degree=10, rng_seed=bytes(32), public=True)
            assert one == (srv.prove_evm if evm else srv.prove)(bodies[0], degree=10, rng_seed=bytes(32), public=True)
        with pytest.raises(ValueError):
            srv.prove_multi(bodies, degree=10)  # public=False on this key
        # the advice-level function, with the witness check
        _, p, _ = api._resident_key(pkp, 10, 0)
        lists = [words_of(api, b) for b in bodies[:2]]
        sets = [[a.to_limbs(c) for c in a.advice] for a in (zk.circuit.synthesize(p, 5 + i, n_public=9, public_values=l) for i, l in enumerate(lists))]
        pf = api.create_proof_multi_from_advice(sets, pkp, 10, rng_seed=bytes(32), check=True, instances=lists)
        assert api.verify_multi(10, pf, vkp, 2, False, instances=lists) and not api.verify_multi(10, pf, vkp, 2, False, instances=lists[::-1])
        with pytest.raises(api.WitnessError) as e:
            api.create_proof_multi_from_advice(sets, pkp, 10, rng_seed=bytes(32), check=True, instances=[lists[0], lists[0]])
        assert e.value.circuit == 1
        assert api.verify_batch(10, [pf], vkp, False, instances=[lists[0]]) == [False]  # (a multi proof is no single proof)
    finally:
        api.shutdown()


def test_pipeline_lockstep_with_instances():
    from webauthn_halo2_amd import batch

    p = zk.circuit.CircuitParams(degree=7, num_advice=4, num_lookup_advice=1, num_fixed=1, lookup_bits=5, num_instance_columns=1)
    asgs = [zk.circuit.synthesize(p, 0x5EED0C00 + i, n_public=9) for i in range(3)]
    pipe = batch.Pipeline(0, p, fixed=np.stack([asgs[0].to_limbs(c) for c in asgs[0].fixed]), copies=asgs[0].copies, deterministic_seeds=True)
    try:
        for j, a in enumerate(asgs):
            pipe.load(j, [a.to_limbs(c) for c in a.advice])
        seeds = [bytes([j + 1]) * 32 for j in range(3)]
        lists = [a.instance for a in asgs]
        want = [pipe.eng.prove_public(pipe.pk, pipe.resident[j], zk.circuit.Assignment.to_mont_limbs(lists[j]), seeds[j], E.ZK_TRANSCRIPT_EVM)
                for j in range(3)]
        got = pipe.prove_lockstep(range(3), E.ZK_TRANSCRIPT_EVM, keep=True, rng_seeds=seeds, instances=lists)
        assert got == want
        assert all(pipe.eng.verify_public(pipe.pk, pf, zk.circuit.Assignment.to_mont_limbs(l), E.ZK_TRANSCRIPT_EVM) for pf, l in zip(got, lists))
    finally:
        pipe.close()
