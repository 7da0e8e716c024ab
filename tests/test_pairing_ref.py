"""tests/pairing_ref.py anchored on facts that do not involve the code under test: the Frobenius map is the p-th power (by
square-and-multiply in the reference's own Fq12), a a^-1 = 1 at every level of the tower, e(G1, G2) has order r, bilinearity at
x, t in {1, 2, r - 1, one random}, the verdicts pairing_cases.mixed_pairs knows from scalars, and the G2 walk against
zkoracle.curve's G2 arithmetic.  No GPU, nothing compiled.  Measured: the file runs in about 3 s on one CPU core.
"""
import random

import pytest

import pairing_cases as pc
import pairing_ref as R
from zkoracle import curve, field as F

T = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % F.R  # tests/test_gpu_pairing.py's s_g2 = [T] G2


def rand_f2(rnd):
    return (rnd.randrange(R.P), rnd.randrange(R.P))


def rand_f12(rnd):
    return tuple(rand_f2(rnd) for _ in range(6))


@pytest.fixture(scope="module")
def e_gen():
    return R.pairing(curve.G1_GEN, curve.G2_GEN)


def test_frobenius_is_the_pth_power():
    rnd = random.Random(1201)
    for _ in range(2):
        a = rand_f12(rnd)
        assert R.frobenius(a) == R.f12_pow(a, R.P)
    assert R.GAMMA[0] == R.F2_ONE and R.f2_pow(R.GAMMA[1], 6) == R.f2_pow(R.XI, R.P - 1)


def test_inverses_at_every_level():
    rnd = random.Random(1202)
    for _ in range(8):
        a = rand_f2(rnd)
        assert R.f2_mul(a, R.f2_inv(a)) == R.F2_ONE
        b = tuple(rand_f2(rnd) for _ in range(3))
        assert R.f6_mul(b, R.f6_inv(b)) == R.F6_ONE
        c = rand_f12(rnd)
        assert R.f12_mul(c, R.f12_inv(c)) == R.F12_ONE
    assert R.f2_inv(R.F2_ZERO) == R.F2_ZERO and R.f6_inv(R.F6_ZERO) == R.F6_ZERO and R.f12_inv(R.F12_ZERO) == R.F12_ZERO
    # the defining relations: u^2 = -1, v^3 = xi, w^2 = v
    assert R.f2_mul((0, 1), (0, 1)) == (R.P - 1, 0)
    v = (R.F2_ZERO, R.F2_ONE, R.F2_ZERO)
    assert R.f6_mul(R.f6_mul(v, v), v) == (R.XI, R.F2_ZERO, R.F2_ZERO)
    w = (R.F2_ZERO, R.F2_ONE) + (R.F2_ZERO,) * 4
    assert R.f12_c0(R.f12_mul(w, w)) == v and R.f12_c1(R.f12_mul(w, w)) == R.F6_ZERO


def test_the_generators_pair_to_an_element_of_order_r(e_gen):
    assert e_gen != R.F12_ONE
    assert R.f12_pow(e_gen, R.R) == R.F12_ONE


def test_bilinearity(e_gen):
    rnd = random.Random(1203)
    xs, ts = [1, 2, F.R - 1, rnd.randrange(3, F.R)], [1, 2, F.R - 1, rnd.randrange(3, F.R)]
    for x in xs:
        for t in ts:
            assert R.pairing(pc.g1(x), pc.g2(t)) == R.f12_pow(e_gen, x * t % F.R), (x, t)


def test_verdicts_known_from_scalars():
    xy = pc.mixed_pairs(12, T, 41)
    table = R.make_table(curve.G2_GEN, pc.g2(T))
    want = [pc.holds(x, y, T) for x, y in xy]
    assert any(want) and not all(want)
    rows = pc.g1_words([pc.g1(x) for x, _ in xy]), pc.g1_words([pc.g1(y) for _, y in xy])
    got = [R.check(R.g1_row_to_words(a), R.g1_row_to_words(b), table) for a, b in zip(*rows)]
    assert got == [R.VALID if w else R.MISMATCH for w in want]
    # the rows are the same images the reference makes itself
    assert R.g1_row_to_words(rows[0][3]) == R.g1_words(pc.g1(xy[3][0]))


def test_the_walk_against_the_oracles_g2_arithmetic():
    for t in (1, 12345, T):
        q = pc.g2(t)
        walk, (t_loop, t_frob1, t_frob2) = R.prepared_walk(q, with_t=True)
        assert len(walk) == R.STEPS == 64 + bin(R.SIX_U_PLUS_2 & (2**64 - 1)).count("1") + 2
        assert t_loop == curve.g2_mul(q, R.SIX_U_PLUS_2)
        pi_q = curve.g2_mul(q, F.P % F.R)  # on G2 the Frobenius map is multiplication by p
        assert R.g2_frobenius(q) == pi_q
        assert t_frob1 == curve.g2_add(t_loop, pi_q)
        pi2_q = curve.g2_mul(q, F.P * F.P % F.R)
        assert t_frob2 == curve.g2_add(t_frob1, R.g2_neg(pi2_q))
        assert t_frob2 == R.g2_neg(curve.g2_mul(q, pow(F.P, 3, F.R)))  # [6u + 2] Q + pi(Q) - pi^2(Q) + pi^3(Q) = O


def test_limb_images_round_trip():
    rnd = random.Random(1204)
    a = rand_f12(rnd)
    assert R.f12_from_words(R.f12_words(a)) == a and len(R.f12_words(a)) == 96
    assert R.f12_words(R.F12_ONE)[:8] == R.to_words((1 << 256) % R.P) and not any(R.f12_words(R.F12_ONE)[8:])
    assert R.f12_words(R.f12_of_halves(R.F6_ZERO, R.F6_ONE))[48:56] == R.to_words((1 << 256) % R.P)
