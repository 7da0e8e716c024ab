"""tests/halo2_ref.py at N circuits without the instance column, under the oracle's own key (zk_prove_multi / zk_verify_multi) - tied
to the pinned oracle and checked against itself.  No GPU.  The rest of that reference's tests are in tests/test_halo2_ref.py; this
file keeps its name so that its ten tests keep their ids.

  N = 1   create_proof gives zkoracle.prover.create_proof's bytes (k18like, k19like; both reference pairings): the reference
          restates the pinned one where they overlap
  N = 2, 3  verify accepts the proofs; rejects them after one flipped byte in an advice commitment of circuit 1, an h piece,
          a shared fixed evaluation, a circuit-1 lookup evaluation and the last opening; rejects them as proofs over N - 1 and
          N + 1 circuits; the circuits' order is part of the proof; a circuit with one broken gate is refused.

Measured on the build machine: about 10 s for the file."""
import pytest

from zkoracle import plonk, prover
from zkoracle.hashes import ChaCha20Rng
import halo2_ref
from multi_cases import PAIRINGS, SEED, setup, tampered


@pytest.fixture(scope="module")
def k18():
    """k18like with three witnesses and, per pairing, its proofs over the first two and over all three (made once)."""
    pk, asgs = setup("k18like", 3)
    proofs = {}
    for kind, scheme in PAIRINGS:
        for N in (2, 3):
            proofs[(kind, N)] = halo2_ref.create_proof(pk, [a.advice for a in asgs[:N]], None, ChaCha20Rng(SEED), kind, scheme)
    return pk, asgs, proofs


@pytest.mark.parametrize("kind,scheme", PAIRINGS)
@pytest.mark.parametrize("name", ["k18like", "k19like"])
def test_one_circuit_is_the_pinned_oracle(name, kind, scheme):
    pk, asgs = setup(name, 1)
    got = halo2_ref.create_proof(pk, [asgs[0].advice], None, ChaCha20Rng(SEED), kind, scheme)
    assert got == prover.create_proof(pk, asgs[0].advice, ChaCha20Rng(SEED), kind, scheme)
    assert halo2_ref.verify(pk.vk, got, [[]], kind, scheme) and plonk.verify(pk.vk, got, kind, scheme)
    assert len(got) == halo2_ref.proof_offsets(pk.shape, 1, kind, scheme)["length"]


@pytest.mark.parametrize("kind,scheme", PAIRINGS)
@pytest.mark.parametrize("N", [2, 3])
def test_accepts_its_proofs_and_rejects_tampered_ones(k18, N, kind, scheme):
    pk, asgs, proofs = k18
    proof = proofs[(kind, N)]
    off = halo2_ref.proof_offsets(pk.shape, N, kind, scheme)
    assert len(proof) == off["length"]
    assert off["length"] - halo2_ref.proof_offsets(pk.shape, N - 1, kind, scheme)["length"] == off["per circuit"]
    assert halo2_ref.verify(pk.vk, proof, [[]] * N, kind, scheme)
    for place, bad in tampered(proof, pk.shape, N, kind, scheme):
        assert not halo2_ref.verify(pk.vk, bad, [[]] * N, kind, scheme), place
    assert not halo2_ref.verify(pk.vk, proof, [[]] * (N - 1), kind, scheme)
    assert not halo2_ref.verify(pk.vk, proof, [[]] * (N + 1), kind, scheme)
    if N == 2:
        assert not plonk.verify(pk.vk, proof, kind, scheme)  # (the single-circuit verifier reads another layout)


def test_the_order_of_the_circuits_is_part_of_the_proof(k18):
    pk, asgs, proofs = k18
    kind, scheme = PAIRINGS[0]
    swapped = halo2_ref.create_proof(pk, [asgs[1].advice, asgs[0].advice], None, ChaCha20Rng(SEED), kind, scheme)
    assert swapped != proofs[(kind, 2)] and len(swapped) == len(proofs[(kind, 2)])
    assert halo2_ref.verify(pk.vk, swapped, [[], []], kind, scheme)


def test_a_circuit_with_a_broken_gate_is_refused(k18):
    """Circuit 1 of 2 violates one gate row (a[r] + a[r+1] a[r+2] - a[r+3] with its selector on): the combined quotient no
    longer has degree below n_h n - the reference's assertion fires - or, were it made anyway, the verifier rejects."""
    pk, asgs, _ = k18
    lay = asgs[1].layout
    sel = asgs[1].fixed[lay.fx_sel[0]]
    row = next(r for r in range(lay.usable_rows - 3) if sel[r])
    bad = [list(c) for c in asgs[1].advice]
    bad[0][row + 3] = (bad[0][row + 3] + 1) % halo2_ref.R
    kind, scheme = PAIRINGS[0]
    try:
        proof = halo2_ref.create_proof(pk, [asgs[0].advice, bad], None, ChaCha20Rng(SEED), kind, scheme)
    except AssertionError as e:
        assert "quotient degree" in str(e)
        return
    assert not halo2_ref.verify(pk.vk, proof, [[], []], kind, scheme)
