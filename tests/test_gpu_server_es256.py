"""The proving server with the ES256 check on the device (ecdsa_p256.set_signature_check("device")), at the k = 10 config the other
server tests use: prove with a fixed rng_seed gives the same hex under both modes; a spoiled request raises the same ValueError
under both; prove_multi with one bad body of three is refused under both; prove_batch puts the exception into the bad request's
slot and proofs into the others; every signature goes through the device check exactly once; the mode is put back afterwards.
"""
import json

import pytest

import webauthn_halo2_amd as zk

pytestmark = pytest.mark.gpu


def requests(api, pkp, count):
    out = []
    for i in range(count):
        d, kk, z = 0x1234567 + 11 * i, 0x7654321 + 7 * i, int.from_bytes(bytes([0x21 + i]) * 32, "big") % api._N
        q, r = api._p256_mul(d, api._G), api._p256_mul(kk, api._G)[0] % api._N
        s = pow(kk, -1, api._N) * (z + r * d) % api._N
        vals = dict(zip(("pubkey_x", "pubkey_y", "r", "s", "msghash"), (list(v.to_bytes(32, "little")) for v in (q[0], q[1], r, s, z))))
        out.append(dict(vals, proving_key_path=pkp))
    return out


def spoiled(body):
    bad = dict(body)
    bad["s"] = [body["s"][0] ^ 1] + body["s"][1:]
    return bad


def test_same_answers_under_both_modes(tmp_path, monkeypatch):
    api, srv = zk.ecdsa_p256, zk.proving_server
    api.shutdown()
    cfg = tmp_path / "ecdsa_circuit.config"
    cfg.write_text(json.dumps({"degree": 10, "num_advice": 3, "num_lookup_advice": 2, "num_fixed": 1, "lookup_bits": 8}) + "\n")
    monkeypatch.setenv("ECDSA_CONFIG", str(cfg))
    pkp = str(tmp_path / "proving_key.pk")
    assert api.signature_check() == "host"
    calls = []
    real = api.es256_verify_many
    monkeypatch.setattr(api, "es256_verify_many", lambda reqs, device=0: calls.append(len(list(reqs))) or real(reqs, device))
    try:
        srv.setup(degree=10, proving_key_path=pkp)
        bodies = requests(api, pkp, 3)
        bad = spoiled(bodies[1])
        seen = {}
        for mode in ("host", "device"):
            api.set_signature_check(mode)
            del calls[:]
            got = {"prove": srv.prove(bodies[0], degree=10, rng_seed=bytes(32)), "prove_evm": srv.prove_evm(bodies[0], degree=10, rng_seed=bytes(32))}
            with pytest.raises(ValueError) as e:
                srv.prove(bad, degree=10, rng_seed=bytes(32))
            got["refused"] = str(e.value)
            got["multi"] = srv.prove_multi(bodies, degree=10, rng_seed=bytes(32))
            with pytest.raises(ValueError) as e:
                srv.prove_multi([bodies[0], bad, bodies[2]], degree=10, rng_seed=bytes(32))
            got["multi refused"] = str(e.value)
            n_before = len(calls)
            batch = srv.prove_batch([bodies[0], bad, bodies[2], {"r": []}], degree=10)
            assert isinstance(batch[0], str) and isinstance(batch[2], str), batch
            assert isinstance(batch[1], ValueError) and str(batch[1]) == got["refused"]
            assert isinstance(batch[3], ValueError)  # the body that does not parse: its own slot's error
            assert len(batch[0]) == len(got["prove_evm"])
            # the device check: one launch per entry point call, every signature once
            assert calls == ([] if mode == "host" else [1, 1, 1, 3, 3, 3]), calls
            assert calls[n_before:] == ([] if mode == "host" else [3])
            seen[mode] = got
        assert seen["host"] == seen["device"]
        assert seen["host"]["refused"] == "invalid ES256 signature (or non-canonical field encoding): request refused"
        assert seen["host"]["multi refused"].startswith("request 1: invalid ES256 signature")
    finally:
        api.set_signature_check("host")
        api.shutdown()
    assert api.signature_check() == "host"
