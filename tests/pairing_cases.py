"""Pairs for the pairing-check tests, given by their scalars: with a = [x] G1, b = [y] G1, g2 = G2 and s_g2 = [t] G2 the check
e(a, s_g2) = e(b, g2) holds exactly when x t = y (mod r) — no pairing is needed to know the verdict.  Points go to the engine
as Montgomery limb arrays: G1 as 8 words (x, y; the identity all zero), G2 as the 16 words of zk_srs_set_g2."""
import random

import numpy as np

from srs_update_ref import g2_to_words, to_mont_limbs
from zkoracle import curve, field as F

VALID, RANGE, OFF_CURVE, MISMATCH = 0, 1, 2, 3


def g1(x):
    """[x] G1 (None for x = 0 mod r)"""
    x %= F.R
    return curve.mul(curve.G1_GEN, x) if x else None


def g2(t):
    t %= F.R
    return curve.g2_mul(curve.G2_GEN, t) if t else None


def g1_words(points):
    """points (tuples or None) -> (n, 8) uint64 Montgomery limbs"""
    return np.ascontiguousarray(to_mont_limbs(list(points)).astype(np.uint64).reshape(len(points), 8))


def holds(x, y, t):
    return (x * t - y) % F.R == 0


def mixed_pairs(count, t, seed):
    """`count` (x, y) scalar pairs against s_g2 = [t] G2, two holding ones to every non-holding one (so every wave of 64 has both),
    with the special cases in the first places: x = 1, x t wrapping mod r, and b the negative of the correct point."""
    rnd = random.Random(seed)
    out = []
    for i in range(count):
        x = rnd.randrange(1, F.R)
        if i == 0:
            x = 1
        elif i == 1:
            x = F.R - 1  # x t wraps for every t > 1
        y = x * t % F.R
        if i % 3 == 2:
            y = (F.R - y) % F.R if i % 2 else rnd.randrange(1, F.R)  # -(correct b), or an unrelated point
        out.append((x, y))
    return out


def with_p_added(words, col):
    """the limb row `words` (8 uint64) with p added to the coordinate starting at word `col` (0: x, 4: y): an image not below p"""
    w = np.array(words, dtype=np.uint64).copy()
    v = sum(int(w[col + q]) << (64 * q) for q in range(4)) + F.P
    assert v < 1 << 256
    w[col:col + 4] = [(v >> (64 * q)) & 0xFFFFFFFFFFFFFFFF for q in range(4)]
    return w


def p_words():
    return np.array([(F.P >> (64 * q)) & 0xFFFFFFFFFFFFFFFF for q in range(4)], dtype=np.uint64)


# ---- a point of the twist outside G2 (the twist's group has a cofactor) ----------------------------------------------------
def _fq_sqrt(a):
    s = pow(a, (F.P + 1) // 4, F.P)  # p = 3 (mod 4)
    return s if s * s % F.P == a % F.P else None


def _f2_sqrt(a):
    a0, a1 = a
    if a1 == 0:
        s = _fq_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = _fq_sqrt(-a0 % F.P)
        return None if s is None else (0, s)
    n = _fq_sqrt((a0 * a0 + a1 * a1) % F.P)
    if n is None:
        return None
    half = F.inv(2, F.P)
    for sign in (1, -1):
        x0 = _fq_sqrt((a0 + sign * n) * half % F.P)
        if x0:
            x1 = a1 * F.inv(2 * x0 % F.P, F.P) % F.P
            if curve.f2mul((x0, x1), (x0, x1)) == (a0 % F.P, a1 % F.P):
                return (x0, x1)
    return None


TWIST_B = curve.f2mul((3, 0), curve.f2inv((9, 1)))


def g2_on_twist(pt):
    (x, y) = pt
    return curve.f2mul(y, y) == curve.f2add(curve.f2mul(curve.f2mul(x, x), x), TWIST_B)


def twist_point_outside_g2():
    """the first point (x, y) of the twist with x = (i, 1) that [r] does not send to the identity"""
    for i in range(1, 200):
        x = (i, 1)
        y = _f2_sqrt(curve.f2add(curve.f2mul(curve.f2mul(x, x), x), TWIST_B))
        if y is None:
            continue
        pt = (x, y)
        assert g2_on_twist(pt)
        if curve.g2_mul(pt, F.R) is not None:
            return pt
    raise AssertionError("no twist point found")


__all__ = ["g1", "g2", "g1_words", "g2_to_words", "holds", "mixed_pairs", "with_p_added", "p_words", "twist_point_outside_g2", "g2_on_twist",
           "VALID", "RANGE", "OFF_CURVE", "MISMATCH"]
