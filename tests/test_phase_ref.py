"""tests/phase_ref.py is the oracle's own code: fed the trace of zkoracle.prover.create_proof (advice as blinded, beta, gamma) its
functions give back create_proof's permuted columns and grand products on every row they promise; the array forms agree with the
integer forms, zero denominators included; chacha_fr is ChaCha20Rng's stream.  CPU only."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phase_ref as PR  # noqa: E402
import webauthn_halo2_amd as zk  # noqa: E402
from zkoracle import cops, plonk, prover  # noqa: E402
from zkoracle.field import R  # noqa: E402
from zkoracle.hashes import ChaCha20Rng  # noqa: E402


def _keyed(t, seed=0x5EED0019):
    A, L, F, k, lb = t
    p = zk.circuit.CircuitParams(degree=k, num_advice=A, num_lookup_advice=L, num_fixed=F, lookup_bits=lb)
    asg = zk.circuit.synthesize(p, seed)
    sh = plonk.Shape(k, A, L, F, lb)
    return sh, asg, prover.keygen(prover.Circuit(sh, asg.fixed, asg.copies, asg.advice))


@pytest.mark.parametrize("t", [(1, 1, 1, 6, 4), (3, 2, 2, 7, 5)], ids=["one-column", "multi-column"])
def test_phase_ref_reproduces_create_proof_trace(t):
    sh, asg, pk = _keyed(t)
    trace = {}
    prover.create_proof(pk, asg.advice, ChaCha20Rng(b"\x09" * 32), "evm", trace=trace)
    adv, beta, gamma, usable = trace["adv"], trace["beta"], trace["gamma"], sh.usable_rows
    assert sh.single or sh.n_chunks >= 3  # the chained start of a chunk is in play
    zs = PR.permutation_products(sh, pk.fixed, pk.sigma, adv, beta, gamma)
    assert len(zs) == sh.n_chunks == len(trace["zs"])
    for z, want in zip(zs, trace["zs"]):
        assert z == want[:usable + 1]
    aps, sps = [], []
    for l, d in enumerate(trace["lk"]):
        inp = PR.lookup_input(sh, pk.fixed, adv, l)
        assert inp[:usable] == d["inp"][:usable]
        ap, sp = PR.permuted_pair(inp, pk.fixed[sh.fx_table], usable)
        assert ap == d["ap"][:usable] and sp == d["sp"][:usable]
        aps.append(ap)
        sps.append(sp)
    zl = PR.lookup_products(sh, pk.fixed, adv, aps, sps, beta, gamma)
    assert len(zl) == sh.n_lookups
    for z, d in zip(zl, trace["lk"]):
        assert z == d["z"][:usable + 1]
    # nothing reads a row the host blinds: other values there, the same answers
    pr = random.Random(3)
    other = [c[:usable] + [pr.randrange(R) for _ in range(sh.n - usable)] for c in adv]
    assert PR.permutation_products(sh, pk.fixed, pk.sigma, other, beta, gamma) == zs
    assert PR.lookup_products(sh, pk.fixed, other, aps, sps, beta, gamma) == zl


def test_array_forms_agree_with_integer_forms_with_a_zero_denominator():
    sh, asg, pk = _keyed((3, 2, 1, 7, 5))
    usable = sh.usable_rows
    pr = random.Random(11)
    adv = [list(c) for c in asg.advice]
    for l in range(sh.n_lookups):  # arbitrary lookup columns: no zero at all / two values
        adv[sh.n_gate + l] = [pr.randrange(1, 32) if l == 0 else pr.choice((1, 31)) for _ in range(sh.n)]
    fx = [cops.fr_mont(c) for c in pk.fixed]
    sg = [cops.fr_mont(c) for c in pk.sigma]
    av = [cops.fr_mont(c) for c in adv]
    aps, sps, apf, spf = [], [], [], []
    for l in range(sh.n_lookups):
        a, s = PR.permuted_pair(adv[sh.n_gate + l], pk.fixed[sh.fx_table], usable)
        af, sf = PR.permuted_pair_fast(av[sh.n_gate + l], fx[sh.fx_table], usable)
        assert cops.fr_ints(af) == a and cops.fr_ints(sf) == s
        aps.append(a), sps.append(s), apf.append(af), spf.append(sf)
    beta = pr.randrange(R)
    r, c = 40, 3  # a zero denominator in the middle chunk, and none
    zero_at = (-(adv[c - sh.num_fixed][r] + beta * pk.sigma[c][r])) % R
    for gamma in (zero_at, pr.randrange(R)):
        zs = PR.permutation_products(sh, pk.fixed, pk.sigma, adv, beta, gamma)
        zf = PR.permutation_products_fast(sh, fx, sg, av, beta, gamma)
        assert [cops.fr_ints(z) for z in zf] == zs
        if gamma == zero_at:
            ci = c // sh.chunk_len
            assert 0 < ci < sh.n_chunks - 1
            assert zs[ci][r] != 0 and not any(zs[ci][r + 1:]) and all(not any(z) for z in zs[ci + 1:])
    for gamma in ((-sps[1][17]) % R, pr.randrange(R)):
        zl = PR.lookup_products(sh, pk.fixed, adv, aps, sps, beta, gamma)
        zlf = PR.lookup_products_fast(sh, fx, av, apf, spf, beta, gamma)
        assert [cops.fr_ints(z) for z in zlf] == zl


def test_lincomb_and_chacha_fr():
    pr = random.Random(5)
    ins = [[pr.randrange(R) for _ in range(5)] for _ in range(3)]
    cs = [pr.randrange(R), 1, R - 1]
    low = [7, R - 1, 3, 4, 5, 6, 8, 9]
    want = [(cs[0] * ins[0][i] + ins[1][i] - ins[2][i] - low[i]) % R for i in range(5)]
    assert PR.lincomb(ins, cs, low) == want   # of 8 low coefficients the 5 that exist
    assert PR.lincomb(ins, cs) == [(w + l) % R for w, l in zip(want, low)]
    key = bytes(range(32))
    rng = ChaCha20Rng(key)
    assert PR.chacha_fr(key, 0, 5) == [rng.fr() for _ in range(5)]
    rng.block = (1 << 32) - 2
    got = PR.chacha_fr(key, (1 << 32) - 2, 4)
    assert got == [rng.fr() for _ in range(4)] and len(set(got)) == 4 and all(v < R for v in got)
    assert PR.chacha_fr(key, 1 << 32, 1) != PR.chacha_fr(key, 0, 1)  # the carry reaches counter word 13
    from zkoracle import fastprover as FP
    for first in (0, (1 << 32) - 3, 1 << 63):
        assert cops.fr_ints(FP.chacha_fr(key, first, 6)) == PR.chacha_fr(key, first, 6)
