"""K5/K3 pin: the oracle's generic PLONK verifier, fed the k=17
verifying key constants baked into the reference's generated verifier, accepts
the reference's golden EVM proof and reproduces its Fiat-Shamir challenges.
CPU only."""
import hashlib
import json
import os

from zkoracle import plonk

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def load_k17():
    d = json.load(open(os.path.join(GOLD, "vk_k17.json")))
    shape = plonk.Shape(k=17, num_advice=4, num_lookup_advice=1, num_fixed=1, lookup_bits=16)
    pt = lambda p: (int(p[0], 16), int(p[1], 16))
    vk = plonk.VerifyingKey(shape, [pt(p) for p in d["fixed_commitments"]],
                            [pt(p) for p in d["permutation_commitments"]], int(d["transcript_repr"], 16))
    proof = bytes.fromhex(open(os.path.join(GOLD, "golden_proof_k17_evm.hex")).read().strip())
    return d, vk, proof


def test_shape_model_matches_published_proof_sizes():
    # K6: halo2-circuits/src/results/ecdsa_bench.csv:2-7 (Blake2b sizes) and the 2720-byte EVM proof
    rows = {19: (1, 1, 1, 960), 18: (2, 1, 1, 1344), 17: (4, 1, 1, 1920), 16: (8, 2, 1, 3552),
            15: (17, 3, 1, 6560), 14: (34, 6, 1, 12704)}
    for k, (A, L, F, size) in rows.items():
        sh = plonk.Shape(k, A, L, F)
        pts = sh.n_points_before_multiopen() + 2  # SHPLONK: 2 more points
        assert 32 * (pts + sh.n_evals()) == size, k
    sh = plonk.Shape(17, 4, 1, 1)
    assert 64 * (sh.n_points_before_multiopen() + sh.gwc_sets()) + 32 * sh.n_evals() == 2720
    sh = plonk.Shape(19, 1, 1, 1)
    assert 64 * (sh.n_points_before_multiopen() + sh.gwc_sets()) + 32 * sh.n_evals() == 1536


def test_golden_proof_accepted_and_challenges_match():
    d, vk, proof = load_k17()
    ok, pf = plonk.verify(vk, proof, "evm", return_detail=True)
    assert ok
    for name, val in d["golden_challenges"].items():
        assert pf.challenges[name] == int(val, 16), name


def test_tampered_golden_proof_rejected():
    _, vk, proof = load_k17()
    for pos in (5, 0x1c0 + 40, 0x3c0 + 7, 0x3c0 + 32 * 20 + 31, 0x920 + 3, len(proof) - 1):
        bad = bytearray(proof)
        bad[pos] ^= 1
        assert not plonk.verify(vk, bytes(bad), "evm")
    assert not plonk.verify(vk, proof[:-32], "evm")
    assert not plonk.verify(vk, proof + b"\x00" * 32, "evm")
    assert not plonk.verify(vk, b"", "evm")  # contracts/test/P256Account.t.sol:106-118: empty proof must fail


def yul_verdicts():
    """What the reference's generated verifier (P256Verifier.yul, run by oracle/tools/yul_exec.py) decided on the suite's two EVM
    proofs: recorded by tests/golden/make_yul_verdicts.py where the reference tree is."""
    return json.load(open(os.path.join(GOLD, "yul_verdicts.json")))


def flipped(proof, pos_mask):
    bad = bytearray(proof)
    bad[pos_mask[0]] ^= pos_mask[1]
    return bytes(bad)


def test_reference_yul_verifier_agrees():
    """The oracle verifier reaches the reference's generated verifier's verdicts on the same bytes: the golden proof, and the
    golden proof with one bit flipped."""
    rec = yul_verdicts()["golden"]
    _, vk, proof = load_k17()
    assert hashlib.sha256(proof).hexdigest() == rec["proof_sha256"]
    assert rec["accepted"] and rec["precompile_calls"] == {"5": 1, "6": 38, "7": 39, "8": 1}
    assert plonk.verify(vk, proof, "evm") == rec["accepted"]
    assert plonk.verify(vk, flipped(proof, rec["flip"]), "evm") == rec["flipped_accepted"] == False  # noqa: E712


def load_engine_fixture():
    d = json.load(open(os.path.join(GOLD, "engine_proof_k17_evm.json")))
    shape = plonk.Shape(d["k"], d["num_advice"], d["num_lookup_advice"], d["num_fixed"], d["lookup_bits"])
    pt = lambda p: (int(p[0], 16), int(p[1], 16))
    vk = plonk.VerifyingKey(shape, [pt(p) for p in d["fixed_commitments"]],
                            [pt(p) for p in d["permutation_commitments"]], int(d["transcript_repr"], 16))
    return vk, bytes.fromhex(d["proof"])


def test_engine_proof_fixture_verifies():
    """A proof the device prover made on an MI355X for the k=17 bench shape
    (tests/golden/make_engine_fixture.py) is accepted by the golden-proof-pinned verifier."""
    vk, proof = load_engine_fixture()
    assert len(proof) == 2720
    assert plonk.verify(vk, proof, "evm")
    # the digest the device stamped on its key is halo2's own: the hash of the pinned verifying key's Debug rendering
    # (zkoracle/vkrepr.py, pinned by the reference's k = 17 literal in tests/test_oracle_kat.py)
    from zkoracle import vkrepr
    assert vk.transcript_repr == vkrepr.transcript_repr(vk.shape, vk.fixed_commitments, vk.permutation_commitments)


def test_reference_yul_verifier_accepts_engine_proof():
    """BASELINE config 3: the reference's GENERATED verifier program (proving-server/P256Verifier.yul) accepted the device
    prover's EVM proof bytes unchanged (tests/golden/yul_verdicts.json).  The program is vk-specific, so the synthetic circuit's 12
    vk commitments and transcript_repr replaced the ECDSA circuit's literals in memory; every instruction of the verification
    logic was the reference's.  The oracle verifier reaches the same verdicts on the same bytes and squeezes the same
    Fiat-Shamir challenges; the unmodified program (ECDSA circuit's key) rejected the proof, and so does the oracle under that key."""
    rec = yul_verdicts()["engine"]
    vk, proof = load_engine_fixture()
    assert hashlib.sha256(proof).hexdigest() == rec["proof_sha256"]
    assert rec["accepted_with_its_key"] and rec["precompile_calls"] == {"5": 1, "6": 38, "7": 39, "8": 1}
    ok, pf = plonk.verify(vk, proof, "evm", return_detail=True)
    assert ok == rec["accepted_with_its_key"]
    for name, val in rec["challenges"].items():
        assert pf.challenges[name] == int(val, 16), name
    _, ecdsa_vk, _ = load_k17()
    assert ecdsa_vk.shape == vk.shape
    assert plonk.verify(ecdsa_vk, proof, "evm") == rec["accepted_with_the_programs_key"] == False  # noqa: E712
    assert plonk.verify(vk, flipped(proof, rec["flip"]), "evm") == rec["flipped_accepted_with_its_key"] == False  # noqa: E712
