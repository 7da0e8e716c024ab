"""tests/halo2_ref.py - the plain-Python reference of public inputs and of one proof over N circuits (zk_prove_public, zk_prove_multi,
zk_prove_multi_public and the zk_verify* forms) - tied to the pinned oracle, to recorded digests, and checked against itself.  No GPU.
N circuits without the column, under the oracle's own key, are in tests/test_multi_ref.py, which keeps its tests' ids.

  the pinned oracle
      without the column its key (commitments, transcript_repr) and its proofs are zkoracle.prover's, byte for byte (k19like,
      k17like; both reference pairings): the reference restates the pinned one where they overlap
  recorded digests
      every proof this file, tests/test_multi_ref.py and tests/test_phase_public_ref.py make has the SHA-256 that tests/golden/ref_proof_sha256.json
      records (tests/golden/make_ref_digests.py: written by the three modules this one replaced, which agreed where they overlapped)
  one circuit with the column (k19like, k17like; 9 public inputs)
      its verifier accepts its own proofs and rejects them under one changed value, a dropped value and an appended zero, and
      after one flipped byte in the last z commitment (k17like: the new chunk's) and in the last sigma evaluation (the instance
      column's); [v] and [v, 0] are the same polynomial, different transcripts and different proofs.  The proof grows as the rule
      says: by formula, and 960 -> 992 (k = 19, Blake2b) and 2720 -> 2912 (k = 17, EVM + GWC; Blake2b + 160) at the full-size
      rows, whose sizes depend on the column counts alone
  N = 2, 3 with the column (k19like, k17like; lists of lengths (9, 9), (0, 9) and (1, 9, 2))
      accepts, and rejects one changed value in circuit 1's list only, the two circuits' lists swapped, a dropped value, an
      appended zero, N - 1 and N + 1 lists, and the flipped bytes of public_cases.PLACES.  The instance lists are absorbed once, in
      circuit order, before any commitment: swapping two lists of equal length changes the transcript alone, and must already be
      rejected."""
import json
import os
import sys

import pytest

from zkoracle import plonk, prover
from zkoracle.hashes import ChaCha20Rng
import halo2_ref
from multi_public_cases import lanes, wrong_multi_lists
from public_cases import PAIRINGS, SEED, reference_key, shape_of, tampered, witness, wrong_lists

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_ref_digests  # noqa: E402

N_PUBLIC = 9
LENGTHS = make_ref_digests.LENGTHS
with open(os.path.join(GOLDEN, "ref_proof_sha256.json")) as f:
    DIGESTS = json.load(f)


# ---- the recorded digests

def test_the_digest_file_has_the_cases():
    assert list(DIGESTS) == list(make_ref_digests.cases())


@pytest.mark.parametrize("cid", list(DIGESTS))
def test_its_proofs_have_the_recorded_digests(cid):
    assert make_ref_digests.digest(make_ref_digests.cases()[cid], halo2_ref.create_proof) == DIGESTS[cid]


# ---- the pinned oracle

@pytest.mark.parametrize("name", ["k19like", "k17like"])
def test_without_the_column_it_is_the_pinned_oracle(name):
    asg = witness(name, 0, n_inst=0)
    pk = reference_key(name, asg, n_inst=0)
    sh = pk.shape
    opk = prover.keygen(prover.Circuit(plonk.Shape(sh.k, sh.num_advice, sh.num_lookup_advice, sh.num_fixed, sh.lookup_bits, sh.idle_gate_columns),
                                       asg.fixed, asg.copies, asg.advice))
    assert pk.vk.fixed_commitments == opk.vk.fixed_commitments and pk.vk.permutation_commitments == opk.vk.permutation_commitments
    assert pk.vk.transcript_repr == opk.vk.transcript_repr and pk.sigma == opk.sigma
    for kind, scheme in PAIRINGS:
        got = halo2_ref.create_proof(pk, [asg.advice], [[]], ChaCha20Rng(SEED), kind, scheme)
        assert got == prover.create_proof(opk, asg.advice, ChaCha20Rng(SEED), kind, scheme)
        assert halo2_ref.verify(pk.vk, got, [[]], kind, scheme) and plonk.verify(opk.vk, got, kind, scheme)
        assert len(got) == halo2_ref.proof_size(sh, 1, kind, scheme)
        with pytest.raises(halo2_ref.InstanceTooLarge):
            halo2_ref.verify(pk.vk, got, [[0]], kind, scheme)


# ---- one circuit with the column

@pytest.fixture(scope="module", params=["k19like", "k17like"])
def made(request):
    """The shape with the column: key, witness with nine public inputs, and per pairing its proof and the proof over [v.., 0]."""
    name = request.param
    asg = witness(name, N_PUBLIC)
    pk = reference_key(name, asg)
    proofs = {}
    for kind, scheme in PAIRINGS:
        proofs[kind] = (halo2_ref.create_proof(pk, [asg.advice], [asg.instance], ChaCha20Rng(SEED), kind, scheme),
                        halo2_ref.create_proof(pk, [asg.advice], [asg.instance + [0]], ChaCha20Rng(SEED), kind, scheme))
    return name, pk, asg, proofs


def test_the_key_has_the_column(made):
    name, pk, asg, _ = made
    base = shape_of(name, 0)
    assert pk.shape.perm_cols == base.perm_cols + [halo2_ref.INSTANCE] and len(pk.vk.permutation_commitments) == len(base.perm_cols) + 1
    assert len(asg.instance) == N_PUBLIC and any(v > 1 for v in asg.instance)
    s = halo2_ref.pinned_debug(pk.shape, pk.vk.fixed_commitments, pk.vk.permutation_commitments)
    assert "num_instance_columns: 1, " in s and "instance_queries: [(Column { index: 0, column_type: Instance }, Rotation(0))], " in s
    assert "column_type: Advice }, Column { index: 0, column_type: Instance }] }, lookups: [" in s
    # the same commitments without the column in the constraint system hash to another value
    assert pk.vk.transcript_repr != prover.transcript_repr(base, pk.vk.fixed_commitments, pk.vk.permutation_commitments)


@pytest.mark.parametrize("kind,scheme", PAIRINGS)
def test_accepts_its_proofs_and_rejects_the_wrong_ones(made, kind, scheme):
    name, pk, asg, proofs = made
    vals = asg.instance
    proof, proof_z = proofs[kind]
    assert len(proof) == len(proof_z) == halo2_ref.proof_size(pk.shape, 1, kind, scheme) == halo2_ref.proof_offsets(pk.shape, 1, kind, scheme)["length"]
    assert halo2_ref.verify(pk.vk, proof, [vals], kind, scheme)
    for what, wrong in wrong_lists(vals):
        assert not halo2_ref.verify(pk.vk, proof, [wrong], kind, scheme), what
    for place, bad in tampered(proof, pk.shape, 1, kind, scheme):
        assert not halo2_ref.verify(pk.vk, bad, [vals], kind, scheme), place
    # trailing zeros: the same polynomial, another transcript
    assert proof_z != proof
    assert halo2_ref.verify(pk.vk, proof_z, [vals + [0]], kind, scheme) and not halo2_ref.verify(pk.vk, proof_z, [vals], kind, scheme)
    with pytest.raises(halo2_ref.InstanceTooLarge):
        halo2_ref.verify(pk.vk, proof, [[0] * (pk.shape.usable_rows + 1)], kind, scheme)


def test_a_witness_that_disagrees_with_its_public_input_is_refused(made):
    name, pk, asg, _ = made
    bad = list(asg.instance)
    bad[0] = (bad[0] + 1) % halo2_ref.R
    kind, scheme = PAIRINGS[0]
    try:
        proof = halo2_ref.create_proof(pk, [asg.advice], [bad], ChaCha20Rng(SEED), kind, scheme)
    except AssertionError as e:
        assert "quotient degree" in str(e)
        return
    assert not halo2_ref.verify(pk.vk, proof, [bad], kind, scheme)


def test_size_deltas():
    size = lambda sh, kind: halo2_ref.proof_size(sh, 1, kind)
    for name, d_blake, d_evm in (("k19like", 32, 32), ("k17like", 160, 192)):
        a, b = shape_of(name, 0), shape_of(name, 1)
        assert b.n_chunks - a.n_chunks == (1 if name == "k17like" else 0)
        assert size(b, "blake2b") - size(a, "blake2b") == d_blake and size(b, "evm") - size(a, "evm") == d_evm
    k19 = lambda n_inst: halo2_ref.public_shape(19, 1, 1, 1, 18, 0, n_inst)
    k17 = lambda n_inst: halo2_ref.public_shape(17, 4, 1, 1, 16, 0, n_inst)
    assert (len(k19(1).perm_cols), k19(1).n_chunks) == (3, 1) and (len(k17(1).perm_cols), k17(0).n_chunks, k17(1).n_chunks) == (7, 3, 4)
    assert (size(k19(0), "blake2b"), size(k19(1), "blake2b")) == (960, 992)
    assert (size(k17(0), "evm"), size(k17(1), "evm")) == (2720, 2912)
    assert size(k17(1), "blake2b") - size(k17(0), "blake2b") == 160


# ---- N circuits with the column

def test_without_the_column_a_list_is_too_large():
    name = "k19like"
    asgs = [witness(name, 0, n_inst=0), witness(name, 0, n_inst=0)]
    pk = reference_key(name, asgs[0], n_inst=0)
    kind, scheme = PAIRINGS[1]
    got = halo2_ref.create_proof(pk, [a.advice for a in asgs], [[], []], ChaCha20Rng(SEED), kind, scheme)
    assert got == halo2_ref.create_proof(pk, [a.advice for a in asgs], None, ChaCha20Rng(SEED), kind, scheme)
    assert halo2_ref.verify(pk.vk, got, [[], []], kind, scheme)
    with pytest.raises(halo2_ref.InstanceTooLarge):
        halo2_ref.verify(pk.vk, got, [[], [0]], kind, scheme)
    with pytest.raises(halo2_ref.InstanceTooLarge):
        halo2_ref.create_proof(pk, [a.advice for a in asgs], [[], [0]], ChaCha20Rng(SEED), kind, scheme)


@pytest.mark.parametrize("lengths", LENGTHS, ids=lambda l: "-".join(map(str, l)))
@pytest.mark.parametrize("name", ["k19like", "k17like"])
def test_n_circuits_accept_their_proofs_and_reject_the_wrong_ones(name, lengths):
    made = lanes(name, lengths)
    pk = reference_key(name, made[0][0])
    lists = [vals for _, vals in made]
    assert [len(l) for l in lists] == list(lengths)
    # (both pairings at the first list set, one each at the others: the pairing does not meet the lists)
    pairs = PAIRINGS if lengths == LENGTHS[0] else [PAIRINGS[LENGTHS.index(lengths) % 2]]
    for kind, scheme in pairs:
        proof = halo2_ref.create_proof(pk, [a.advice for a, _ in made], lists, ChaCha20Rng(SEED), kind, scheme)
        assert len(proof) == halo2_ref.proof_offsets(pk.shape, len(lists), kind, scheme)["length"]
        assert halo2_ref.verify(pk.vk, proof, lists, kind, scheme)
        for what, wrong in wrong_multi_lists(lists):
            assert not halo2_ref.verify(pk.vk, proof, wrong, kind, scheme), what
        for place, bad in tampered(proof, pk.shape, len(lists), kind, scheme):
            assert not halo2_ref.verify(pk.vk, bad, lists, kind, scheme), place


def test_swapped_lists_of_equal_length_are_rejected():
    """(9, 9): the swap is in wrong_multi_lists above; here the witnesses are swapped WITH their lists - another, valid proof."""
    name = "k19like"
    made = lanes(name, (9, 9))
    pk = reference_key(name, made[0][0])
    kind, scheme = PAIRINGS[0]
    a, b = made
    proof = halo2_ref.create_proof(pk, [b[0].advice, a[0].advice], [b[1], a[1]], ChaCha20Rng(SEED), kind, scheme)
    assert halo2_ref.verify(pk.vk, proof, [b[1], a[1]], kind, scheme)
    assert not halo2_ref.verify(pk.vk, proof, [a[1], b[1]], kind, scheme)
