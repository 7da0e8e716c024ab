"""tests/phase_public_ref.py is tied to the whole proofs of the reference it restates: fed what tests/halo2_ref.py `create_proof`
commits to on its way (the blinded columns, a', s', zL) and the challenges it squeezes (beta, gamma, y), its functions give back the
z those proofs commit to - on every row they promise - and their h pieces.  The reference is traced from outside (a recording
committer and transcript in its namespace); it is not changed.  CPU only.

  one circuit  k19like (the column joins a chunk) and k17like (it opens one), 9 public inputs
  N circuits   k19like N = 3 with lists of 9, 0 and 1 values; k17like N = 2 with 1 and 9
  no column    N = 2 on k19like without the instance column: `instances` are ignored
  divide       the undivided quotient times 1 / (X^n - 1) is the divided one; a wrong y moves every piece"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import halo2_ref  # noqa: E402
import phase_public_ref as PPR  # noqa: E402
from multi_public_cases import lanes  # noqa: E402
from public_cases import SEED, reference_key, witness  # noqa: E402
from zkoracle.field import R, ZETA, inv, omega  # noqa: E402
from zkoracle.hashes import ChaCha20Rng  # noqa: E402


def traced(monkeypatch, run):
    """run() with halo2_ref's commitments and challenges recorded -> dict(lagrange=[columns], coeff=[polynomials], squeezed=[..])."""
    rec = dict(lagrange=[], coeff=[], squeezed=[])
    module = halo2_ref
    real_committer, real_commit_coeff, real_make = module.Committer, module.commit_coeff, module.make_transcript

    class Committer(real_committer):
        def lagrange(self, col):
            rec["lagrange"].append(list(col))
            return super().lagrange(col)

    def commit_coeff(c):
        rec["coeff"].append(list(c))
        return real_commit_coeff(c)

    def make_transcript(kind, proof=None):
        tr = real_make(kind, proof)
        squeeze = tr.squeeze

        def recording():
            v = squeeze()
            rec["squeezed"].append(v)
            return v

        tr.squeeze = recording
        return tr

    monkeypatch.setattr(module, "Committer", Committer)
    monkeypatch.setattr(module, "commit_coeff", commit_coeff)
    monkeypatch.setattr(module, "make_transcript", make_transcript)
    rec["proof"] = run()
    return rec


def split(sh, rec, N):
    """The recorded commitments in the rule's order -> (per-circuit column sets, beta, gamma, y, the h pieces the proof commits to)."""
    cols = iter(rec["lagrange"])
    circuits = [dict(adv=[next(cols) for _ in range(sh.n_adv)]) for _ in range(N)]
    for d in circuits:
        d["ap"], d["sp"] = [], []
        for _ in range(sh.n_lookups):
            d["ap"].append(next(cols))
            d["sp"].append(next(cols))
    for d in circuits:
        d["z"] = [next(cols) for _ in range(sh.n_chunks)]
    for d in circuits:
        d["zl"] = [next(cols) for _ in range(sh.n_lookups)]
    assert next(cols, None) is None
    _theta, beta, gamma, y = rec["squeezed"][:4]
    return circuits, beta, gamma, y, rec["coeff"][1:1 + sh.n_h]  # (coeff[0] is the random polynomial)


def check(sh, pk, rec, lists):
    circuits, beta, gamma, y, pieces = split(sh, rec, len(lists))
    usable = sh.usable_rows
    for d, vals in zip(circuits, lists):
        d["instances"] = vals
        zs = PPR.permutation_products_public(sh, pk.fixed, pk.sigma, d["adv"], vals, beta, gamma)
        assert len(zs) == sh.n_chunks
        for z, want in zip(zs, d["z"]):
            assert z == want[:usable + 1]
    hv = PPR.quotient_multi(sh, pk.fixed, pk.sigma, circuits, beta, gamma, y)
    got, above = PPR.h_pieces(sh, hv)
    assert got == pieces and not any(above)
    return circuits, beta, gamma, y, hv


@pytest.mark.parametrize("name", ["k19like", "k17like"])
def test_one_circuit_against_the_whole_proof(monkeypatch, name):
    asg = witness(name, 9)
    pk = reference_key(name, asg)
    sh = pk.shape
    assert sh.perm_cols[-1] == halo2_ref.INSTANCE and (len(sh.perm_cols) % sh.chunk_len == 1) == (name == "k17like")
    vals = list(asg.instance)
    rec = traced(monkeypatch, lambda: halo2_ref.create_proof(pk, [asg.advice], [vals], ChaCha20Rng(SEED), "evm"))
    check(sh, pk, rec, [vals])


@pytest.mark.parametrize("name,lengths", [("k19like", (9, 0, 1)), ("k17like", (1, 9))], ids=["k19like-9-0-1", "k17like-1-9"])
def test_n_circuits_against_the_whole_proof(monkeypatch, name, lengths):
    made = lanes(name, lengths)
    pk = reference_key(name, made[0][0])
    lists = [vals for _, vals in made]
    rec = traced(monkeypatch, lambda: halo2_ref.create_proof(pk, [a.advice for a, _ in made], lists, ChaCha20Rng(SEED), "blake2b"))
    sh = pk.shape
    circuits, beta, gamma, y, hv = check(sh, pk, rec, lists)
    if name != "k19like":
        return
    # the division is the product by 1 / (X^n - 1) on the coset; another y is another quotient in every piece
    raw = PPR.quotient_multi(sh, pk.fixed, pk.sigma, circuits, beta, gamma, y, divide=False)
    x, w = ZETA, omega(sh.ext_k)
    for i in range(len(raw)):
        assert raw[i] * inv((pow(x, sh.n, R) - 1) % R, R) % R == hv[i]
        x = x * w % R
    other, _ = PPR.h_pieces(sh, PPR.quotient_multi(sh, pk.fixed, pk.sigma, circuits, beta, gamma, (y + 1) % R))
    mine, _ = PPR.h_pieces(sh, hv)
    assert all(a != b for a, b in zip(other, mine))
    # circuit order matters: the chain runs through circuit 0 first
    swapped = PPR.quotient_multi(sh, pk.fixed, pk.sigma, circuits[::-1], beta, gamma, y)
    assert swapped != hv


def test_without_the_column_instances_are_ignored(monkeypatch):
    name = "k19like"
    asgs = [witness(name, 0, n_inst=0), witness(name, 0, n_inst=0)]
    pk = reference_key(name, asgs[0], n_inst=0)
    rec = traced(monkeypatch, lambda: halo2_ref.create_proof(pk, [a.advice for a in asgs], [[], []], ChaCha20Rng(SEED), "evm"))
    check(pk.shape, pk, rec, [[], []])
    with pytest.raises(halo2_ref.InstanceTooLarge):
        PPR.permutation_products_public(pk.shape, pk.fixed, pk.sigma, asgs[0].advice, [1], 2, 3)
