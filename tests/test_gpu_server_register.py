"""The proving server's registration entry points: register_credential gives one dict on the host route and on the device route;
the dict's key arrays placed into an assertion body pass parse_assertion and are the key zk_webauthn_verify accepts the
credential's assertions under; a refused body raises an error naming the reason, the same on both routes; register_credentials_batch
keeps each exception in its own slot and checks the whole batch in one device launch; the mode is put back afterwards.  No proof
is made, so no SRS and no key are needed.
"""
import base64
import json

import pytest

import webauthn_halo2_amd as zk
import webauthn_cases as A
import webauthn_register_cases as C
import webauthn_register_ref as G

pytestmark = pytest.mark.gpu

NAMES = ("valid/packed-self/policy=1", "head/id=255", "cred/ed-set-credProtect-self-attested")


def b64(b):
    return base64.urlsafe_b64encode(b).rstrip(b"=").decode()


def body(g):
    return {"attestation_object": b64(g.attestation_object), "client_data_json": b64(g.client_data_json)}


def test_one_credential_on_both_routes():
    api, srv = zk.ecdsa_p256, zk.proving_server
    cs = C.build()
    api.shutdown()
    assert api.signature_check() == "host"
    calls = []
    real = api.webauthn_register_many
    good = [cs.regs[cs.index(n)] for n in NAMES]
    assert all(cs.reasons[cs.index(n)] == G.VALID for n in NAMES)
    expect = dict(origin=C.ORIGIN, rp_id=C.RP_ID)
    refused_cases = (("CLIENTDATA", "cd/wrong-origin", {}), ("FLAGS", NAMES[0], {"require_uv": True}), ("RPID", NAMES[0], {"rp_id": "b.example"}),
                     ("CLIENTDATA", NAMES[0], {"expected_challenge": C.CHALLENGE[::-1]}), ("CBOR", "head/indefinite/bf", {}),
                     ("CREDENTIAL", "cred/at-clear", {}), ("COSE_KEY", "cose/okp", {}), ("OFF_CURVE", "cose/key-off-the-curve", {}),
                     ("ATTESTATION", "valid/tpm/policy=0", {"attestation": "none-or-self"}), ("MISMATCH", "self/s+1", {"attestation": "none-or-self"}),
                     ("SIGNATURE_DER", "self/der-byte-after-s", {"attestation": "none-or-self"}), ("SIZE", "cap/object=8193", {}))
    try:
        api.webauthn_register_many = lambda reqs, device=0: calls.append(len(list(reqs))) or real(reqs, device)
        seen = {}
        for mode in ("host", "device"):
            api.set_signature_check(mode)
            del calls[:]
            got = [srv.register_credential(body(g), C.CHALLENGE, attestation="none-or-self", **expect) for g in good]
            got.append(srv.register_credential(json.dumps(body(good[0])), C.CHALLENGE, **expect))  # a JSON string; the statement not judged
            got.append(srv.register_credential(body(cs.regs[cs.index("valid/uv-required-and-set")]), C.CHALLENGE, require_uv=True, **expect))
            for name, d in zip(NAMES, got):
                ref = cs.creds[cs.index(name)]
                assert d == {"credential_id": C.cred_id(ref["credential_id_len"]).hex(), "pubkey_x": list(ref["pubkey_x"][::-1]),
                             "pubkey_y": list(ref["pubkey_y"][::-1]), "aaguid": C.AAGUID.hex(), "sign_count": ref["sign_count"], "flags": ref["flags"],
                             "attestation": "self"}, mode
            assert got[3] == dict(got[0], attestation="not-judged") and got[4]["flags"] & 0x04
            refused = []
            for name, case, kw in refused_cases:
                args = dict(expect, expected_challenge=C.CHALLENGE)
                args.update(kw)
                with pytest.raises(ValueError) as e:
                    srv.register_credential(body(cs.regs[cs.index(case)]), **args)
                assert str(e.value) == "WebAuthn registration refused: " + name, case
                refused.append(str(e.value))
            n_before = len(calls)
            bodies = [body(good[0]), body(cs.regs[cs.index("cose/okp")]), body(good[2]), {"attestation_object": "="}, body(good[1])]
            batch = srv.register_credentials_batch(bodies, [C.CHALLENGE] * 5, attestation="none-or-self", **expect)
            assert batch[0] == got[0] and batch[2] == got[2] and batch[4] == got[1]
            assert isinstance(batch[1], ValueError) and str(batch[1]) == "WebAuthn registration refused: COSE_KEY"
            assert isinstance(batch[3], ValueError)  # the body that does not parse: its own slot's error
            # the device route: one launch per entry point call, every registration of the batch in ONE
            assert calls[n_before:] == ([] if mode == "host" else [4])
            assert len(calls) == (0 if mode == "host" else 5 + len(refused_cases) + 1)
            seen[mode] = (got, refused, [b if isinstance(b, dict) else str(b) for b in batch])
        assert seen["host"] == seen["device"]
        with pytest.raises(ValueError):
            srv.register_credential(body(good[0]), C.CHALLENGE, attestation="full", **expect)
        with pytest.raises(ValueError):
            srv.register_credentials_batch([body(good[0])], [], **expect)
    finally:
        api.webauthn_register_many = real
        api.set_signature_check("host")
        api.shutdown()
    assert api.signature_check() == "host"


def test_a_stored_credential_drops_into_an_assertion_body():
    """The dict's key arrays are the little-endian ones parse_assertion takes; the assertion of the same private key is accepted
    under them on the device, and refused under the key of another registration."""
    api, srv = zk.ecdsa_p256, zk.proving_server
    cs = C.build()
    api.shutdown()
    other = C.reg(C.att_obj(C.auth_data(key=C.cose_key(A._key(A.D + 1)))))
    try:
        api.set_signature_check("device")
        mine = srv.register_credential(body(cs.regs[cs.index(NAMES[0])]), C.CHALLENGE, C.ORIGIN, C.RP_ID, attestation="none-or-self")
        theirs = srv.register_credential(body(other), C.CHALLENGE, C.ORIGIN, C.RP_ID)
        a = A.make(ad=A.auth_data(counter=mine["sign_count"] + 1))
        verdicts = []
        for cred in (mine, theirs):
            q = srv.parse_assertion({"authenticator_data": b64(a.authenticator_data), "client_data_json": b64(a.client_data_json),
                                     "signature": b64(a.signature), "pubkey_x": cred["pubkey_x"], "pubkey_y": cred["pubkey_y"],
                                     "proving_key_path": "unused.pk"})
            assert q["pubkey_x"] == bytes(cred["pubkey_x"]) and len(q["pubkey_y"]) == 32
            verdicts.append(api.webauthn_check([srv._expectation(q, A.CHALLENGE, A.ORIGIN, A.RP_ID, False, False)])[0])
        assert verdicts[0][:2] == (True, api.ZK_WEBAUTHN_VALID) and verdicts[0][3] == mine["sign_count"] + 1
        assert verdicts[1][:2] == (False, api.ZK_WEBAUTHN_MISMATCH)
        assert bytes(mine["pubkey_x"]) == a.x.to_bytes(32, "little") and bytes(mine["pubkey_y"]) == a.y.to_bytes(32, "little")
    finally:
        api.set_signature_check("host")
        api.shutdown()
