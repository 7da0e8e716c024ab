"""The limb-exact model of the lazy 29-bit field and curve (tests/field29_model.py) against big integers, at the extremes
of the contracts written in csrc/field29.hip.h, csrc/ec29.hip.h and at the call sites.  No GPU, no compiler.

What is pinned here:
  * every product at the largest operands its contract admits: no 64-bit column wraps, the result limbs are normalised,
    the value is below p (1 + k_a k_b p / 2^261) and congruent to a b 2^-261;
  * every sub29<K, E> instantiation of csrc/ at the largest subtrahend its call site admits: no limb goes negative and the
    value is a + K p - b exactly;
  * the three curve routines on every lifted representative of their accumulator, with the exceptional cases;
  * that the model does raise one step beyond each limit (so a loosened check in the model cannot pass unnoticed).
"""
import itertools
import random

import pytest

import field29_model as M
from field29_model import FQ, FR, M29, Wrap, extreme, value
from zkoracle import curve as C
from zkoracle import field as F

FIELDS = [pytest.param(FR, id="Fr"), pytest.param(FQ, id="Fq")]


def _check_product(f, r, want_num, kk):
    """r: result limbs; want_num: the integer sum of products; kk: sum of k_a k_b."""
    p = f.p
    assert all(0 <= l <= M29 for l in r), "result limbs not normalised"
    v = value(r)
    assert (v << 261) < p * ((1 << 261) + kk * p), "value above p (1 + kk p / 2^261)"
    # the bound as the issue states it, p (1 + kk / 169.28): 2^261 / p = 169.2819 > 169.28, so the line above implies it
    assert (1 << 261) * 100 > 16928 * p
    assert v * 16928 < p * (16928 + 100 * kk)
    assert v % p == want_num * pow(1 << 261, -1, p) % p


# ---- products at the extremes of their contracts ------------------------------------------------------------------------
# (limb bits of a, limb bits of b, k_a, k_b).  The header's contract: a_i b_j < 2^60.6 "e.g. 2^30.6 x 2^30", k_a k_b <= 168;
# the quotient's uses above 168 with the limb widths written at their call sites (csrc/quotient.hip).
MUL29_CASES = [(30.6, 30, ka, kb) for ka, kb in [(12, 14), (168, 1), (1, 168), (84, 2), (32, 5), (13, 12)]] + [
    (30, 30.6, 14, 12), (29, 31.6, 2, 84), (31.6, 29, 84, 2),
    (29, 31.3, 65, 65),   # dd = norm29(d) * (pa - pam + 33 p)
    (29, 31.3, 32, 73),   # g = q * w
    (29, 30, 32, 35),     # q (2 - q), left * (vg + bs)
    (29, 29, 32, 32),     # m = a1 * a2
    (29, 29, 66, 1),      # q_acc's fold
    (29, 29, 108, 1),     # the row's last product (quotient_row's result times its constant)
]


@pytest.mark.parametrize("f", FIELDS)
@pytest.mark.parametrize("ba,bb,ka,kb", MUL29_CASES)
def test_mul29_at_contract_extremes(f, ba, bb, ka, kb):
    a, b = extreme(ba, ka, f.p), extreme(bb, kb, f.p)
    r = f.mul29(a, b)
    _check_product(f, r, value(a) * value(b), ka * kb)
    if ka * kb <= 168:
        assert value(r) < 2 * f.p


# sqr29: limbs a_i^2 < 2^60.6, k^2 <= 168; the quotient squares a loaded value (32 ; 29)
@pytest.mark.parametrize("f", FIELDS)
@pytest.mark.parametrize("bits,k", [(30.3, 12), (30.3, 8), (30.3, 1), (29, 12), (29, 5), (29, 32)])
def test_sqr29_at_contract_extremes(f, bits, k):
    a = extreme(bits, k, f.p)
    r = f.sqr29(a)
    _check_product(f, r, value(a) ** 2, k * k)
    assert r == f.mul29(a, a), "sqr29 and mul29(a, a) are the same columns"


# mul2add29: a, c normalised, b, d limbs < 2^30.7, k_a k_b + k_c k_d <= 168.  (8, 12, 5, 3) and (5, 12, 2, 3) are the two
# call sites of ec29.hip.h.
MUL2ADD_CASES = [(8, 12, 5, 3), (5, 12, 2, 3), (12, 7, 12, 7), (1, 84, 1, 84), (84, 1, 84, 1), (168, 1, 0, 0), (1, 167, 1, 1)]


@pytest.mark.parametrize("f", FIELDS)
@pytest.mark.parametrize("ka,kb,kc,kd", MUL2ADD_CASES)
def test_mul2add29_at_contract_extremes(f, ka, kb, kc, kd):
    zero = [0] * 9
    a, b = extreme(29, ka, f.p), extreme(30.7, kb, f.p)
    c, d = (extreme(29, kc, f.p), extreme(30.7, kd, f.p)) if kc else (zero, zero)
    r = f.mul2add29(a, b, c, d)
    _check_product(f, r, value(a) * value(b) + value(c) * value(d), ka * kb + kc * kd)
    assert value(r) < 2 * f.p


# mulKadd29<K>: all operands normalised, sum k_a k_b <= 168, K <= 5
MULK_CASES = [(1, [(168, 1)]), (1, [(12, 14)]), (2, [(12, 7), (7, 12)]), (3, [(8, 7), (7, 8), (56, 1)]),
              (4, [(6, 7)] * 4), (4, [(42, 1)] * 4), (4, [(1, 42)] * 4), (5, [(33, 1)] * 5), (5, [(5, 6)] * 5 + []),
              (5, [(1, 33)] * 5), (5, [(164, 1), (1, 1), (1, 1), (1, 1), (1, 1)])]


@pytest.mark.parametrize("f", FIELDS)
@pytest.mark.parametrize("K,ks", MULK_CASES)
def test_mulKadd29_at_contract_extremes(f, K, ks):
    assert len(ks) == K and sum(x * y for x, y in ks) <= 168
    a = [extreme(29, x, f.p) for x, _ in ks]
    b = [extreme(29, y, f.p) for _, y in ks]
    r = f.mulKadd29(a, b)
    _check_product(f, r, sum(value(x) * value(y) for x, y in zip(a, b)), sum(x * y for x, y in ks))
    assert value(r) < 2 * f.p


@pytest.mark.parametrize("f", FIELDS)
def test_products_on_random_and_all_ones_operands(f):
    rng = random.Random(0x29 + f.p % 97)
    ones = [M29] * 9  # all limbs at the normalised maximum: 2^261 - 1 = 169.28 p
    for _ in range(200):
        a, b = M.split29(rng.randrange(12 * f.p)), M.split29(rng.randrange(14 * f.p))
        _check_product(f, f.mul29(a, b), value(a) * value(b), 168)
        _check_product(f, f.sqr29(a), value(a) ** 2, 144)
    one = f.pow2(261)
    r = f.mul29(ones, one)  # 169.28 x 1: beyond the < 2p contract by a hair, still no wrap and still congruent
    assert value(r) % f.p == value(ones) % f.p and all(l <= M29 for l in r)
    assert value(f.mul29(ones, ones)) % f.p == value(ones) ** 2 * pow(1 << 261, -1, f.p) % f.p


# ---- the model raises one step beyond each limit ------------------------------------------------------------------------
@pytest.mark.parametrize("f", FIELDS)
def test_model_raises_on_a_wrapped_column(f):
    # nine terms of 2^31 * floor(2^30.5): column 8 lands in [2^64, 2^65) — a check loosened by one bit would let it pass
    a, b = [1 << 31] * 9, [int(2 ** 30.5)] * 9
    assert 64 <= f.worst_column([(a, b)]) < 65
    with pytest.raises(Wrap, match="column"):
        f.mul29(a, b)
    with pytest.raises(Wrap, match="column"):
        f.mul2add29(a, b, [0] * 9, [0] * 9)
    with pytest.raises(Wrap, match="column"):
        f.mulKadd29([a], [b])
    # and the largest operands that do fit, found by bisection on the limb size, are within one unit of the first that wrap
    lo, hi = 1 << 29, 1 << 32
    while hi - lo > 1:
        mid = (lo + hi) // 2
        try:
            f.mul29([mid] * 9, [mid] * 9)
            lo = mid
        except Wrap:
            hi = mid
    assert f.worst_column([([lo] * 9, [lo] * 9)]) < 64 <= f.worst_column([([hi] * 9, [hi] * 9)])


@pytest.mark.parametrize("f", FIELDS)
def test_model_raises_on_limb_and_top_limb_overflow(f):
    top = [0] * 8 + [(1 << 32) - 1]
    with pytest.raises(Wrap, match="top limb"):
        f.mul29(top, top)
    with pytest.raises(Wrap, match="doubled"):
        f.sqr29([1 << 31] + [0] * 8)
    f.sqr29([(1 << 31) - 1] + [0] * 8)
    z = [0] * 9
    assert f.add29([(1 << 32) - 1] * 9, z) == [(1 << 32) - 1] * 9
    with pytest.raises(Wrap):
        f.add29([(1 << 32) - 1] + z[1:], [1] + z[1:])
    with pytest.raises(Wrap):
        f.norm29([(1 << 32) - 1, (1 << 32) - 1] + z[2:])  # the carry of limb 0 pushes limb 1 over
    assert f.norm29([(1 << 32) - 1] + z[1:]) == [M29, 7] + z[2:]
    with pytest.raises(Wrap):
        f.norm29(z[:7] + [(1 << 32) - 1, (1 << 32) - 1])


# ---- sub29<K, E>: every instantiation of csrc/, at the largest b its call site admits ----------------------------------
# (K, E, limb bits of a, k of b, limb bits of b, call site)
SUB29_SITES = [
    (2, 29, 29, 1, 29, "prover_kernels: acc - to29(canonical)"),
    (3, 29, 29, 2, 29, "ntt bfly_mul / ec29: minus a product output"),
    (4, 29, 29, 3, 29, "quotient: left - right, (3 ; 29)"),
    (5, 30, 29, 4, 30, "g1x29_dbl_rare: mm - 2 s"),
    (6, 29, 29, 5, 29, "g1x29_add_affine: s2 - Y, Y < 5p"),
    (7, 29, 29, None, 29, "ntt round0<6>: minus a loaded value < 2^256"),
    (7, 31, 29, 6, 30.6, "rr - (ppp + 2 q), limbs < 3 * 2^29"),
    (8, 29, 29, 7, 29, "g1x29_dbl_rare: s - x3, (7 ; 29)"),
    (9, 29, 29, 8, 29, "quotient: left - right, (8 ; 29)"),
    (10, 29, 29, 9, 29, "u2 - X and q - x3, X < 9p"),
    (13, 30, 30, 12, 30, "ntt round0<6>: sums of two loaded values"),
    (33, 29, 30, 32, 29, "quotient / ntt round0<32>: minus a loaded value (32 ; 29)"),
    (65, 30, 30, 64, 30, "ntt round0<32>: sums of two loaded values"),
]


def _sub29_operands(f, K, E, abits, kb, bbits):
    if kb is None:  # limbs of the largest 256-bit integer (5.29 p for both moduli)
        b = f.to29((1 << 256) - 1)
        assert value(b) < 6 * f.p
    elif bbits == 30.6:  # ppp + 2 q with three normalised product outputs: limbs <= 3 (2^29 - 1), value < 6p
        lo = 3 * M29
        low = sum(lo << (29 * i) for i in range(8))
        b = [lo] * 8 + [(kb * f.p - 1 - low) >> 232]
    else:
        b = extreme(bbits, kb, f.p)
    a = [(1 << abits) - 1] * 9
    return a, b


@pytest.mark.parametrize("f", FIELDS)
@pytest.mark.parametrize("K,E,abits,kb,bbits,site", SUB29_SITES)
def test_sub29_at_every_call_site(f, K, E, abits, kb, bbits, site):
    C = f.spread(K, E)
    assert value(C) == K * f.p, "the spread constant is not K p"
    assert all(c >= (1 << E) for c in C[:8]), "a lower limb of the spread constant is below 2^E"
    a, b = _sub29_operands(f, K, E, abits, kb, bbits)
    assert all(l < (1 << E) for l in b[:8])
    r = f.sub29(K, E, a, b)
    assert value(r) == value(a) + K * f.p - value(b)
    assert value(f.norm29(r)) == value(r)
    # the header's own statement of the condition: b's top limb may be as large as (K - 1) p's
    b2 = [(1 << E) - 1] * 8 + [((K - 1) * f.p) >> 232]
    if value(b2) < K * f.p:
        r2 = f.sub29(K, E, [0] * 9, b2)
        assert value(r2) == K * f.p - value(b2)
    # one past the constant in any single limb must raise
    for i in range(9):
        over = [0] * 9
        over[i] = C[i] + 1
        with pytest.raises(Wrap, match="exceeds"):
            f.sub29(K, E, [0] * 9, over)
        over[i] = C[i]
        assert f.sub29(K, E, [0] * 9, over)[i] == 0


def test_sub29_site_list_matches_the_sources():
    """The (K, E) list above is read off the call sites; a new instantiation in csrc/ must be added to it."""
    import os
    import re

    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "webauthn-halo2_amd", "csrc")
    found = set()
    for name in sorted(os.listdir(root)):
        src = open(os.path.join(root, name)).read()
        for m in re.finditer(r"(?<![\w/])sub29<(\d+), (\d+)>\(", src):
            found.add((int(m.group(1)), int(m.group(2))))
        for kin in re.findall(r"ntt_pass_kernel<(\d+),", src):  # round0<KIN>: bfly_plain<KIN + 1, 29>, <2 KIN + 1, 30>
            found |= {(int(kin) + 1, 29), (2 * int(kin) + 1, 30)}
    assert found == {(K, E) for K, E, *_ in SUB29_SITES}


# ---- conversions, norm29, is_zero29 --------------------------------------------------------------------------------------
def _edge_values(f):
    p = f.p
    vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, f.R256, f.R256 * f.R256 % p, pow(1 << 256, -1, p)]
    vals += [1 << (29 * i) for i in range(9) if (1 << (29 * i)) < p] + [(1 << (29 * i)) - 1 for i in range(1, 9)]
    vals += [1 << (32 * i) for i in range(8) if (1 << (32 * i)) < p] + [(1 << (32 * i)) - 1 for i in range(1, 8)]
    return vals


@pytest.mark.parametrize("f", FIELDS)
def test_conversions(f):
    p = f.p
    rng = random.Random(5)
    for v in _edge_values(f) + [rng.randrange(p) for _ in range(100)] + [(1 << 256) - 1, (1 << 254) - 1]:
        a = f.to29(v)
        assert value(a) == v and all(l <= M29 for l in a) and f.from29(a) == v
        if v < (1 << 254):
            x = f.to29_x32(v)
            assert value(x) == 32 * v and all(l <= M29 for l in x)
        if v < p:
            i = f.std_to_internal(v)
            assert value(i) < 2 * p and value(i) % p == 32 * v % p and all(l <= M29 for l in i)
            assert f.internal_to_std(i) == v
            assert f.internal_to_std(f.to29_x32(v)) == v
    # internal_to_std at the top of its contract (k_a = 168) and on both sides of its conditional subtraction
    sides = set()
    for a in [extreme(29, 168, p), extreme(30.6, 168, p)] + [M.split29(rng.randrange(168 * p)) for _ in range(200)]:
        raw = f.from29(f.mul29(a, f.pow2(256)))
        assert raw < 2 * p
        sides.add(raw >= p)
        assert f.internal_to_std(a) == value(a) * pow(32, -1, p) % p
    assert sides == {True, False}


@pytest.mark.parametrize("f", FIELDS)
def test_norm29_and_is_zero29(f):
    p = f.p
    rng = random.Random(6)
    for _ in range(200):
        a = [rng.randrange(1 << 31) for _ in range(8)] + [rng.randrange(1 << 24)]
        n = f.norm29(a)
        assert value(n) == value(a) and all(l <= M29 for l in n[:8])
    for v, want in [(0, True), (p, True), (p + 1, False), (p - 1, False), (2 * p - 1, False), (1, False)]:
        a = M.split29(v)
        assert f.is_zero29(a) is want
        for i in range(9):  # one limb perturbed: zero only where that lands on 0 or p itself (1 -> 0, p +- 1 -> p)
            b = list(a)
            b[i] ^= 1
            assert f.is_zero29(b) is (value(b) in (0, p))


# ---- the curve routines on lifted representatives -------------------------------------------------------------------------
LIFTS = list(itertools.product(range(9), range(5), range(2), range(2)))
SETTINGS = [(True, True), (False, False)]  # (ZK_EC29_SQR, ZK_EC29_FUSE)
P_, S261, S256 = F.P, (1 << 261) % F.P, (1 << 256) % F.P


def _pts():
    rng = random.Random(0xEC29)
    return [C.mul(C.G1_GEN, rng.randrange(1, F.R)) for _ in range(3)] + [C.G1_GEN]


def _addend(pt, internal):
    s = S261 if internal else S256
    return pt[0] * s % P_, pt[1] * s % P_


def _check_invariants(a, xk=9, yk=5):
    assert not a.inf
    for c in (a.x, a.y, a.zz, a.zzz):
        assert all(0 <= l <= M29 for l in c[:8]) and c[8] < (1 << 29)
    assert value(a.x) < xk * P_ and value(a.y) < yk * P_ and value(a.zz) < 2 * P_ and value(a.zzz) < 2 * P_


@pytest.mark.parametrize("sqr,fuse", SETTINGS)
@pytest.mark.parametrize("check,internal", list(itertools.product([True, False], repeat=2)))
def test_g1x29_add_affine_on_lifted_accumulators(check, internal, sqr, fuse):
    pts = _pts()
    rng = random.Random(11)
    for q, pt in [(pts[0], pts[1]), (pts[3], pts[2])]:
        z = rng.randrange(1, P_)
        x, y = _addend(pt, internal)
        want = C.add(q, pt)
        for lift in LIFTS:
            acc = M.lifted(q, z, *lift)
            assert M.g1x29_add_affine(acc, x, y, check, internal, sqr, fuse) is True
            _check_invariants(acc, 9, 2 if fuse else 5)
            assert M.affine_of(acc) == want


@pytest.mark.parametrize("sqr,fuse", SETTINGS)
@pytest.mark.parametrize("internal", [False, True])
def test_g1x29_add_affine_exceptional_cases(internal, sqr, fuse):
    pts = _pts()
    q = pts[0]
    z = 0x1234567
    for pt, what in [(q, "same"), (C.neg(q), "negated")]:
        x, y = _addend(pt, internal)
        for lift in LIFTS:
            acc = M.lifted(q, z, *lift)
            before = acc.key()
            assert M.g1x29_add_affine(acc, x, y, True, internal, sqr, fuse) is False
            assert acc.key() == before, "CHECK = true must leave the accumulator unchanged"
            assert M.g1x29_add_affine(acc, x, y, False, internal, sqr, fuse) is True
            assert value(acc.zz) % P_ == 0 and FQ.is_zero29(acc.zz), "CHECK = false must leave ZZ = 0 (mod p)"
            # and ZZ stays zero through a further, ordinary, step
            x2, y2 = _addend(pts[1], internal)
            M.g1x29_add_affine(acc, x2, y2, False, internal, sqr, fuse)
            assert FQ.is_zero29(acc.zz)
    # identity as accumulator
    for pt in pts:
        x, y = _addend(pt, internal)
        acc = M.g1x29_identity()
        assert M.g1x29_add_affine(acc, x, y, True, internal, sqr, fuse) is True
        _check_invariants(acc, 2, 2)
        assert M.affine_of(acc) == pt
    # chains from the identity
    for n in (1, 2, 40):
        acc = M.g1x29_identity()
        want = None
        for k in range(n):
            pt = C.mul(C.G1_GEN, 3 * k + 2)
            assert M.g1x29_add_affine(acc, *_addend(pt, internal), True, internal, sqr, fuse)
            want = C.add(want, pt) if want is not None else pt
            _check_invariants(acc, 9, 2 if fuse or k == 0 else 5)
        assert M.affine_of(acc) == want
        sx, sy, szz, szzz = M.g1x29_to_std(acc)
        zi = pow(szz, -1, P_)
        assert sx * zi % P_ == want[0] and sy * pow(szzz, -1, P_) % P_ == want[1]


B_LIFTS = [(0, 0, 0, 0), (8, 4, 1, 1), (8, 0, 0, 1), (0, 4, 1, 0)]


def test_g1x29_add_on_lifted_accumulators():
    pts = _pts()
    a, b = pts[0], pts[1]
    want = C.add(a, b)
    for bl in B_LIFTS:
        bb = M.lifted(b, 0xBEEF, *bl)
        for lift in LIFTS:
            acc = M.lifted(a, 0xACC, *lift)
            assert M.g1x29_add(acc, bb) == "add"
            _check_invariants(acc, 9, 2)
            assert M.affine_of(acc) == want


def test_g1x29_add_exceptional_cases_and_dbl_rare():
    pts = _pts()
    a = pts[2]
    dbl = C.add(a, a)
    for bl in B_LIFTS:
        same = M.lifted(a, 0x5A5A5, *bl)          # the same point under another Z
        minus = M.lifted(C.neg(a), 0x77, *bl)
        for lift in LIFTS:
            acc = M.lifted(a, 0xACC, *lift)
            assert M.g1x29_add(acc, same) == "dbl"  # P + P goes through g1x29_dbl_rare
            _check_invariants(acc, 7, 5)
            assert M.affine_of(acc) == dbl
            acc = M.lifted(a, 0xACC, *lift)
            assert M.g1x29_add(acc, minus) == "cancel" and acc.inf
            assert M.g1x29_store(acc) == [0] * 36
    for lift in LIFTS:
        acc = M.lifted(a, 0x31337, *lift)
        M.g1x29_dbl_rare(acc)
        _check_invariants(acc, 7, 5)
        assert M.affine_of(acc) == dbl
        # identity on either side, and both
        acc = M.lifted(a, 0x31337, *lift)
        before = acc.key()
        assert M.g1x29_add(acc, M.g1x29_identity()) == "b_inf" and acc.key() == before
        idn = M.g1x29_identity()
        assert M.g1x29_add(idn, acc) == "acc_inf" and idn.key() == before
    idn = M.g1x29_identity()
    assert M.g1x29_add(idn, M.g1x29_identity()) == "b_inf" and idn.inf
    M.g1x29_dbl_rare(idn)
    assert idn.inf


def test_g1x29_store_load_and_std_round_trip():
    pts = _pts()
    for lift in LIFTS[::7]:
        acc = M.lifted(pts[1], 0x99, *lift)
        w = M.g1x29_store(acc)
        assert len(w) == 36 and M.g1x29_load(w).key() == acc.key()
        sx, sy, szz, szzz = M.g1x29_to_std(acc)
        back = M.g1x29_from_std(sx, sy, szz, szzz)
        _check_invariants(back, 2, 2)
        assert M.affine_of(back) == pts[1]
    assert M.g1x29_load([0] * 36).inf and M.g1x29_store(M.g1x29_identity()) == [0] * 36
    assert M.g1x29_to_std(M.g1x29_identity()) == (S256, S256, 0, 0)
    assert M.g1x29_from_std(S256, S256, 0, 0).inf
