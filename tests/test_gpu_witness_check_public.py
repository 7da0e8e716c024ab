"""zk_witness_check_public (csrc/witness_check.hip): MockProver::verify with the instance column - the last permutation column of
the copy check - and the Python layer over the three public entry points.  A clean witness has no failure; one changed instance
value is exactly the ZK_FAIL_COPY pair the rule predicts, reported from both sides; zk_prove_public still proves that witness (the
prover checks no copy) and zk_verify_public rejects the proof."""
import json

import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
from public_cases import PAIRINGS, SEED, engine_key, mont, witness
import halo2_ref

pytestmark = pytest.mark.gpu

N_PUBLIC = 9


@pytest.mark.parametrize("name", ["k19like", "k17like", "wide"])
def test_one_changed_instance_value_is_one_copy_pair(name):
    eng = zk.Engine(0)
    asg = witness(name, N_PUBLIC)
    pk, (polys,) = engine_key(eng, name, [asg])
    lay = asg.layout
    inst_col = len(lay.perm_cols) - 1
    assert lay.perm_cols[inst_col] == ("instance", 0) and eng.pk_shape(pk)["n_perm"] == inst_col + 1
    assert eng.witness_check_public(pk, polys, mont(asg.instance)) == ([0, 0, 0, 0, 0], [])
    i = 4
    # instance row i is tied to exactly one advice cell: its copy constraint (every public gate's output is exposed once here)
    (a, b), = [c for c in asg.copies if (inst_col, i) in c]
    cell = b if a == (inst_col, i) else a
    others = [c for c in asg.copies if cell in c and (inst_col, i) not in c]
    assert not others  # (a two-cell cycle: sigma swaps the two)
    bad = list(asg.instance)
    bad[i] = (bad[i] + 1) % halo2_ref.R
    counts, failures = eng.witness_check_public(pk, polys, mont(bad))
    want = sorted([(E.ZK_FAIL_COPY, cell[0], cell[1], inst_col, i), (E.ZK_FAIL_COPY, inst_col, i, cell[0], cell[1])])
    assert counts == [2, 0, 0, 0, 2] and failures == want
    # a dropped value: row N_PUBLIC - 1 reads zero
    counts, failures = eng.witness_check_public(pk, polys, mont(asg.instance[:-1]))
    assert counts == [2, 0, 0, 0, 2] and {f[1:3] for f in failures} >= {(inst_col, N_PUBLIC - 1)}
    # the prover does not check copies: it proves, and the verifier rejects
    kind, _ = PAIRINGS[0]
    t = E.ZK_TRANSCRIPT_EVM
    proof = eng.prove_public(pk, polys, mont(bad), SEED, t)
    assert not eng.verify_public(pk, proof, mont(bad), t) and not eng.verify_public(pk, proof, mont(asg.instance), t)
    good = eng.prove_public(pk, polys, mont(asg.instance), SEED, t)
    assert eng.verify_public(pk, good, mont(asg.instance), t)
    assert eng.witness_check_public(pk, polys, mont(asg.instance)) == ([0, 0, 0, 0, 0], [])
    eng.close()


def test_python_layer(tmp_path, monkeypatch):
    """ecdsa_p256 / proving_server with public=True at a k = 10 config: the proof is bound to msghash and the public key."""
    api, srv = zk.ecdsa_p256, zk.proving_server
    api.shutdown()
    cfg = tmp_path / "ecdsa_circuit.config"
    cfg.write_text(json.dumps({"degree": 10, "num_advice": 3, "num_lookup_advice": 2, "num_fixed": 1, "lookup_bits": 8}) + "\n")
    monkeypatch.setenv("ECDSA_CONFIG", str(cfg))
    pkp, vkp = str(tmp_path / "proving_key.pk"), str(tmp_path / "verifying_key.vk")
    # an ES256 signature made here: d = 7, k = 11 (plain secp256r1 arithmetic of the module itself)
    d, k, z = 7, 11, int.from_bytes(b"\x21" * 32, "big") % api._N
    Q, Rp = api._p256_mul(d, api._G), api._p256_mul(k, api._G)
    r = Rp[0] % api._N
    s = pow(k, -1, api._N) * (z + r * d) % api._N
    le = lambda v: v.to_bytes(32, "little")
    req = dict(pubkey_x=le(Q[0]), pubkey_y=le(Q[1]), r=le(r), s=le(s), msg_hash=le(z))
    assert api.es256_verify(req["pubkey_x"], req["pubkey_y"], req["r"], req["s"], req["msg_hash"])
    try:
        api.download_keys(10, pkp, vkp, public=True)
        vals = api.public_inputs(req["msg_hash"], req["pubkey_x"], req["pubkey_y"])
        assert len(vals) == 9 and sum(v << (88 * (i % 3)) for i, v in enumerate(vals[:3])) == z
        proof = api.generate_proof_evm_synthetic(proving_key_path=pkp, degree=10, rng_seed=bytes(32), check=True, public=True, **req)
        data = api.encode_calldata(vals, proof)
        assert len(data) == 32 * 9 + len(proof) and data[:32] == vals[0].to_bytes(32, "big") and data[288:] == proof
        assert api.verify_evm(10, proof, vkp, instances=vals)
        other = list(vals)
        other[0] ^= 1  # another message hash
        assert not api.verify_evm(10, proof, vkp, instances=other)
        with pytest.raises(ValueError):
            api.generate_proof_evm_synthetic(proving_key_path=pkp, degree=10, rng_seed=bytes(32), **req)  # public=False on this key
        # the advice-level functions
        _, p, _ = api._resident_key(pkp, 10, 0)
        asg = zk.circuit.synthesize(p, 5, n_public=9, public_values=vals)
        cols = [asg.to_limbs(c) for c in asg.advice]
        assert api.mock_verify_advice(cols, pkp, 10, instances=vals) == []
        assert [f[0] for f in api.mock_verify_advice(cols, pkp, 10, instances=other)] == [E.ZK_FAIL_COPY] * 2
        with pytest.raises(api.WitnessError):
            api.create_proof_from_advice(cols, pkp, 10, rng_seed=bytes(32), check=True, instances=other)
        pf = api.create_proof_from_advice(cols, pkp, 10, rng_seed=bytes(32), check=True, instances=vals)
        assert api.verify(10, pf, vkp, instances=vals) and not api.verify(10, pf, vkp, instances=other)
        # the server's contract: instance words in front of the proof
        body = {"r": list(req["r"]), "s": list(req["s"]), "pubkey_x": list(req["pubkey_x"]), "pubkey_y": list(req["pubkey_y"]),
                "msghash": list(req["msg_hash"]), "proving_key_path": pkp}
        hexed = srv.prove_evm(body, degree=10, rng_seed=bytes(32), public=True)
        assert bytes.fromhex(hexed) == data
        assert srv.verify_evm({"verifying_key_path": vkp, "proof": hexed}, degree=10, public=9) == "verified"
        forged = (other[0].to_bytes(32, "big") + data[32:]).hex()
        assert srv.verify_evm({"verifying_key_path": vkp, "proof": forged}, degree=10, public=9) == "rejected"
        hexed2 = srv.prove(body, degree=10, rng_seed=bytes(32), public=True)
        assert srv.verify({"verifying_key_path": vkp, "proof": hexed2}, degree=10, public=9) == "verified"
    finally:
        api.shutdown()
