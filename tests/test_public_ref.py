"""tests/public_ref.py — the plain-Python reference of public inputs (zk_prove_public / zk_verify_public) — tied to the pinned
oracle and checked against itself.  No GPU.

  (a) without the column its key (commitments, transcript_repr) and its proofs are zkoracle.prover's, byte for byte (k19like,
      k17like; both reference pairings): the new reference restates the pinned one where they overlap
  (b) with the column its verifier accepts its own proofs
  (c) and rejects them under one changed value, a dropped value and an appended zero, and after one flipped byte in the last z
      commitment (k17like: the new chunk's) and in the last sigma evaluation (the instance column's); [v] and [v, 0] are the same
      polynomial, different transcripts and different proofs
  (d) the proof grows as the rule says: by formula at k19like / k17like, and 960 -> 992 (k = 19, Blake2b) and 2720 -> 2912
      (k = 17, EVM + GWC; Blake2b + 160) at the full-size rows, whose sizes depend on the column counts alone"""
import pytest

from zkoracle import plonk, prover
from zkoracle.hashes import ChaCha20Rng
import public_ref
from public_cases import PAIRINGS, SEED, reference_key, shape_of, tampered, witness, wrong_lists

N_PUBLIC = 9


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
        got = public_ref.create_proof(pk, asg.advice, [], ChaCha20Rng(SEED), kind, scheme)
        assert got == prover.create_proof(opk, asg.advice, ChaCha20Rng(SEED), kind, scheme)
        assert public_ref.verify(pk.vk, got, [], kind, scheme) and plonk.verify(opk.vk, got, kind, scheme)
        assert len(got) == public_ref.proof_size(sh, kind, scheme)
        with pytest.raises(public_ref.InstanceTooLarge):
            public_ref.verify(pk.vk, got, [0], kind, scheme)


@pytest.fixture(scope="module", params=["k19like", "k17like"])
def made(request):
    """The shape with the column: key, witness with nine public inputs, and per pairing its proof and the proof over [v.., 0]."""
    name = request.param
    asg = witness(name, N_PUBLIC)
    pk = reference_key(name, asg)
    proofs = {}
    for kind, scheme in PAIRINGS:
        proofs[kind] = (public_ref.create_proof(pk, asg.advice, asg.instance, ChaCha20Rng(SEED), kind, scheme),
                        public_ref.create_proof(pk, asg.advice, asg.instance + [0], ChaCha20Rng(SEED), kind, scheme))
    return name, pk, asg, proofs


def test_the_key_has_the_column(made):
    name, pk, asg, _ = made
    base = shape_of(name, 0)
    assert pk.shape.perm_cols == base.perm_cols + [public_ref.INSTANCE] and len(pk.vk.permutation_commitments) == len(base.perm_cols) + 1
    assert len(asg.instance) == N_PUBLIC and any(v > 1 for v in asg.instance)
    s = public_ref.pinned_debug(pk.shape, pk.vk.fixed_commitments, pk.vk.permutation_commitments)
    assert "num_instance_columns: 1, " in s and "instance_queries: [(Column { index: 0, column_type: Instance }, Rotation(0))], " in s
    assert "column_type: Advice }, Column { index: 0, column_type: Instance }] }, lookups: [" in s
    # the same commitments without the column in the constraint system hash to another value
    assert pk.vk.transcript_repr != prover.transcript_repr(base, pk.vk.fixed_commitments, pk.vk.permutation_commitments)


@pytest.mark.parametrize("kind,scheme", PAIRINGS)
def test_accepts_its_proofs_and_rejects_the_wrong_ones(made, kind, scheme):
    name, pk, asg, proofs = made
    vals = asg.instance
    proof, proof_z = proofs[kind]
    assert len(proof) == len(proof_z) == public_ref.proof_size(pk.shape, kind, scheme) == public_ref.proof_offsets(pk.shape, kind, scheme)["length"]
    assert public_ref.verify(pk.vk, proof, vals, kind, scheme)
    for what, wrong in wrong_lists(vals):
        assert not public_ref.verify(pk.vk, proof, wrong, kind, scheme), what
    for place, bad in tampered(proof, pk.shape, kind, scheme):
        assert not public_ref.verify(pk.vk, bad, vals, kind, scheme), place
    # trailing zeros: the same polynomial, another transcript
    assert proof_z != proof
    assert public_ref.verify(pk.vk, proof_z, vals + [0], kind, scheme) and not public_ref.verify(pk.vk, proof_z, vals, kind, scheme)
    with pytest.raises(public_ref.InstanceTooLarge):
        public_ref.verify(pk.vk, proof, [0] * (pk.shape.usable_rows + 1), kind, scheme)


def test_a_witness_that_disagrees_with_its_public_input_is_refused(made):
    name, pk, asg, _ = made
    bad = list(asg.instance)
    bad[0] = (bad[0] + 1) % public_ref.R
    kind, scheme = PAIRINGS[0]
    try:
        proof = public_ref.create_proof(pk, asg.advice, bad, ChaCha20Rng(SEED), kind, scheme)
    except AssertionError as e:
        assert "quotient degree" in str(e)
        return
    assert not public_ref.verify(pk.vk, proof, bad, kind, scheme)


def test_size_deltas():
    size = public_ref.proof_size
    for name, d_blake, d_evm in (("k19like", 32, 32), ("k17like", 160, 192)):
        a, b = shape_of(name, 0), shape_of(name, 1)
        assert b.n_chunks - a.n_chunks == (1 if name == "k17like" else 0)
        assert size(b, "blake2b") - size(a, "blake2b") == d_blake and size(b, "evm") - size(a, "evm") == d_evm
    k19 = lambda n_inst: public_ref.public_shape(19, 1, 1, 1, 18, 0, n_inst)
    k17 = lambda n_inst: public_ref.public_shape(17, 4, 1, 1, 16, 0, n_inst)
    assert (len(k19(1).perm_cols), k19(1).n_chunks) == (3, 1) and (len(k17(1).perm_cols), k17(0).n_chunks, k17(1).n_chunks) == (7, 3, 4)
    assert (size(k19(0), "blake2b"), size(k19(1), "blake2b")) == (960, 992)
    assert (size(k17(0), "evm"), size(k17(1), "evm")) == (2720, 2912)
    assert size(k17(1), "blake2b") - size(k17(0), "blake2b") == 160
