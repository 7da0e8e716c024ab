"""tests/multi_public_ref.py - the plain-Python reference of one proof over N circuits WITH public inputs (zk_prove_multi_public /
zk_verify_multi_public) - tied to the two references it is built on and checked against itself.  No GPU.

  N = 1           its bytes are public_ref.create_proof's (k19like, k17like; both reference pairings)
  no column       on a shape without the instance column its bytes are multi_ref.create_proof_multi's (N = 2)
  N = 2, 3        k19like and k17like, lists of lengths (9, 9), (0, 9) and (1, 9, 2): its tau-based verifier accepts, and rejects
                  one changed value in circuit 1's list only, the two circuits' lists swapped, a dropped value, an appended zero,
                  N - 1 and N + 1 lists, and the flipped bytes of public_cases.PLACES
The instance lists are absorbed once, in circuit order, before any commitment: swapping two lists of equal length changes the
transcript alone, and must already be rejected."""
import pytest

from zkoracle.hashes import ChaCha20Rng
import multi_public_ref
import multi_ref
import public_ref
from multi_public_cases import lanes, wrong_multi_lists
from public_cases import PAIRINGS, SEED, reference_key, tampered, witness

LENGTHS = [(9, 9), (0, 9), (1, 9, 2)]


@pytest.mark.parametrize("name", ["k19like", "k17like"])
def test_one_circuit_is_public_ref(name):
    (asg, vals), = lanes(name, [9])
    pk = reference_key(name, asg)
    for kind, scheme in PAIRINGS:
        got = multi_public_ref.create_proof_multi(pk, [asg.advice], [vals], ChaCha20Rng(SEED), kind, scheme)
        assert got == public_ref.create_proof(pk, asg.advice, vals, ChaCha20Rng(SEED), kind, scheme)
        assert multi_public_ref.verify_multi(pk.vk, got, [vals], kind, scheme) and public_ref.verify(pk.vk, got, vals, kind, scheme)


def test_without_the_column_it_is_multi_ref():
    name = "k19like"
    asgs = [witness(name, 0, n_inst=0), witness(name, 0, n_inst=0)]
    pk = reference_key(name, asgs[0], n_inst=0)
    kind, scheme = PAIRINGS[1]
    got = multi_public_ref.create_proof_multi(pk, [a.advice for a in asgs], [[], []], ChaCha20Rng(SEED), kind, scheme)
    assert got == multi_ref.create_proof_multi(pk, [a.advice for a in asgs], ChaCha20Rng(SEED), kind, scheme)
    assert multi_public_ref.verify_multi(pk.vk, got, [[], []], kind, scheme) and multi_ref.verify_multi(pk.vk, got, 2, kind, scheme)
    with pytest.raises(public_ref.InstanceTooLarge):
        multi_public_ref.verify_multi(pk.vk, got, [[], [0]], kind, scheme)


@pytest.mark.parametrize("lengths", LENGTHS, ids=lambda l: "-".join(map(str, l)))
@pytest.mark.parametrize("name", ["k19like", "k17like"])
def test_accepts_its_proofs_and_rejects_the_wrong_ones(name, lengths):
    made = lanes(name, lengths)
    pk = reference_key(name, made[0][0])
    lists = [vals for _, vals in made]
    assert [len(l) for l in lists] == list(lengths)
    # (both pairings at the first list set, one each at the others: the pairing does not meet the lists)
    pairs = PAIRINGS if lengths == LENGTHS[0] else [PAIRINGS[LENGTHS.index(lengths) % 2]]
    for kind, scheme in pairs:
        proof = multi_public_ref.create_proof_multi(pk, [a.advice for a, _ in made], lists, ChaCha20Rng(SEED), kind, scheme)
        assert len(proof) == multi_ref.proof_offsets(pk.shape, len(lists), kind, scheme)["length"]
        assert multi_public_ref.verify_multi(pk.vk, proof, lists, kind, scheme)
        for what, wrong in wrong_multi_lists(lists):
            assert not multi_public_ref.verify_multi(pk.vk, proof, wrong, kind, scheme), what
        for place, bad in tampered(proof, pk.shape, kind, scheme):
            assert not multi_public_ref.verify_multi(pk.vk, bad, lists, kind, scheme), place


def test_swapped_lists_of_equal_length_are_rejected():
    """(9, 9): the swap is in wrong_multi_lists above; here the witnesses are swapped WITH their lists - another, valid proof."""
    name = "k19like"
    made = lanes(name, (9, 9))
    pk = reference_key(name, made[0][0])
    kind, scheme = PAIRINGS[0]
    a, b = made
    proof = multi_public_ref.create_proof_multi(pk, [b[0].advice, a[0].advice], [b[1], a[1]], ChaCha20Rng(SEED), kind, scheme)
    assert multi_public_ref.verify_multi(pk.vk, proof, [b[1], a[1]], kind, scheme)
    assert not multi_public_ref.verify_multi(pk.vk, proof, [a[1], b[1]], kind, scheme)
