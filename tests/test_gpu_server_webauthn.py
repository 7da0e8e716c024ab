"""The proving server's assertion entry points at the k = 10 config the other server tests use: prove_assertion / prove_assertion_evm
with a fixed rng_seed give the hex of prove / prove_evm for the classic body an honest web client would have posted, under both
signature-check modes; a refused assertion raises an error naming the reason; prove_assertions_batch puts that error into the bad
assertion's slot and proofs that verify into the others, with one device launch for the whole batch; the public form's nine
instance words are those of the msghash the engine computed; the mode is put back afterwards.
"""
import base64
import hashlib
import json

import pytest

import webauthn_halo2_amd as zk
import webauthn_cases as C
import webauthn_ref as W

pytestmark = pytest.mark.gpu

NAMES = ("valid/1", "cdlen/193", "adlen/96")  # UV set, a clientDataJSON with a trailing member, extension bytes


def b64(b):
    return base64.urlsafe_b64encode(b).rstrip(b"=").decode()


def assertion_body(a, pkp):
    return {"authenticator_data": b64(a.authenticator_data), "client_data_json": b64(a.client_data_json), "signature": b64(a.signature),
            "pubkey_x": list(a.x.to_bytes(32, "little")), "pubkey_y": list(a.y.to_bytes(32, "little")), "proving_key_path": pkp}


def classic_body(a, pkp):
    """What the reference's web client posts for the same assertion: both hashes, the ASN.1 parse, everything little-endian."""
    r, s = W.der_parse(a.signature)
    z = hashlib.sha256(a.authenticator_data + hashlib.sha256(a.client_data_json).digest()).digest()
    vals = {"pubkey_x": a.x.to_bytes(32, "little"), "pubkey_y": a.y.to_bytes(32, "little"), "r": r.to_bytes(32, "little"),
            "s": s.to_bytes(32, "little"), "msghash": z[::-1]}
    return dict({k: list(v) for k, v in vals.items()}, proving_key_path=pkp)


def config(tmp_path, monkeypatch):
    cfg = tmp_path / "ecdsa_circuit.config"
    cfg.write_text(json.dumps({"degree": 10, "num_advice": 3, "num_lookup_advice": 2, "num_fixed": 1, "lookup_bits": 8}) + "\n")
    monkeypatch.setenv("ECDSA_CONFIG", str(cfg))


def test_same_answers_as_the_classic_bodies_under_both_modes(tmp_path, monkeypatch):
    api, srv = zk.ecdsa_p256, zk.proving_server
    cs = C.build()
    api.shutdown()
    config(tmp_path, monkeypatch)
    pkp, vkp = str(tmp_path / "proving_key.pk"), str(tmp_path / "verifying_key.vk")
    assert api.signature_check() == "host"
    calls = []
    real = api.webauthn_verify_many
    monkeypatch.setattr(api, "webauthn_verify_many", lambda reqs, device=0: calls.append(len(list(reqs))) or real(reqs, device))
    good = [cs.assertions[cs.index(n)] for n in NAMES]
    assert all(cs.reasons[cs.index(n)] == W.VALID for n in NAMES)
    expect = dict(origin=C.ORIGIN, rp_id=C.RP_ID)
    try:
        srv.setup(degree=10, proving_key_path=pkp, verifying_key_path=vkp)
        want = {"prove": srv.prove(classic_body(good[0], pkp), degree=10, rng_seed=bytes(32)),
                "prove_evm": srv.prove_evm(classic_body(good[0], pkp), degree=10, rng_seed=bytes(32)),
                "prove long": srv.prove(classic_body(good[1], pkp), degree=10, rng_seed=bytes(32))}
        bad = good[1].replace(client_data_json=C.client_data(origin="https://a.example.evil"))
        seen = {}
        for mode in ("host", "device"):
            api.set_signature_check(mode)
            del calls[:]
            got = {"prove": srv.prove_assertion(assertion_body(good[0], pkp), C.CHALLENGE, degree=10, rng_seed=bytes(32), require_uv=True, **expect),
                   "prove_evm": srv.prove_assertion_evm(json.dumps(assertion_body(good[0], pkp)), C.CHALLENGE, degree=10, rng_seed=bytes(32), **expect),
                   "prove long": srv.prove_assertion(assertion_body(good[1], pkp), C.CHALLENGE, degree=10, rng_seed=bytes(32), **expect)}
            assert got == want, mode
            refused = {}
            for name, a, kw in (("CLIENTDATA", bad, {}), ("FLAGS", good[1], {"require_uv": True}),
                                ("RPID", good[0], {"rp_id": "b.example"}), ("CLIENTDATA", good[0], {"expected_challenge": C.CHALLENGE[::-1]}),
                                ("MISMATCH", good[0].replace(y=W.R.P - good[0].y), {})):
                args = dict(expect, expected_challenge=C.CHALLENGE, degree=10, rng_seed=bytes(32))
                args.update(kw)
                with pytest.raises(ValueError) as e:
                    srv.prove_assertion(assertion_body(a, pkp), **args)
                assert str(e.value) == "WebAuthn assertion refused: " + name
                refused[name] = str(e.value)
            n_before = len(calls)
            bodies = [assertion_body(good[0], pkp), assertion_body(bad, pkp), assertion_body(good[2], pkp), {"signature": "="}]
            batch = srv.prove_assertions_batch(bodies, [C.CHALLENGE] * 4, degree=10, **expect)
            assert isinstance(batch[0], str) and isinstance(batch[2], str), batch
            assert isinstance(batch[1], ValueError) and str(batch[1]) == "WebAuthn assertion refused: CLIENTDATA"
            assert isinstance(batch[3], ValueError)  # the body that does not parse: its own slot's error
            # the neighbours' proofs are what prove_batch gives for their classic bodies: the same length, and they verify
            vbody = lambda proof: json.dumps({"verifying_key_path": vkp, "proof": proof})
            assert len(batch[0]) == len(batch[2]) == len(want["prove_evm"])
            assert srv.verify_batch([vbody(batch[0]), vbody(batch[2])], evm=True, degree=10) == ["verified"] * 2
            # the device route: one launch per entry point call, every assertion of the batch in ONE
            assert calls == ([] if mode == "host" else [1] * 8 + [3]), calls
            assert calls[n_before:] == ([] if mode == "host" else [3])
            seen[mode] = (got, refused)
        assert seen["host"] == seen["device"]
    finally:
        api.set_signature_check("host")
        api.shutdown()
    assert api.signature_check() == "host"


def test_public_form_is_bound_to_the_msghash_made_here(tmp_path, monkeypatch):
    api, srv = zk.ecdsa_p256, zk.proving_server
    cs = C.build()
    api.shutdown()
    config(tmp_path, monkeypatch)
    pkp = str(tmp_path / "proving_key.pk")
    a = cs.assertions[cs.index(NAMES[2])]
    try:
        srv.setup(degree=10, proving_key_path=pkp, public=True)
        z = hashlib.sha256(a.authenticator_data + hashlib.sha256(a.client_data_json).digest()).digest()
        words = api.public_inputs(z[::-1], a.x.to_bytes(32, "little"), a.y.to_bytes(32, "little"))
        for mode in ("host", "device"):
            api.set_signature_check(mode)
            got = srv.prove_assertion_evm(assertion_body(a, pkp), C.CHALLENGE, C.ORIGIN, C.RP_ID, degree=10, rng_seed=bytes(32), public=True)
            assert bytes.fromhex(got)[:288] == b"".join(v.to_bytes(32, "big") for v in words)
            assert got == srv.prove_evm(classic_body(a, pkp), degree=10, rng_seed=bytes(32), public=True)
            batch = srv.prove_assertions_batch([assertion_body(a, pkp)], [C.CHALLENGE], C.ORIGIN, C.RP_ID, degree=10, public=True)
            assert bytes.fromhex(batch[0])[:288] == bytes.fromhex(got)[:288]
    finally:
        api.set_signature_check("host")
        api.shutdown()
