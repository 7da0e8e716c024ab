"""A pure-Python restatement of one ceremony contribution (zk_srs_update) on zkoracle.curve: the update of the monomial basis,
its Lagrange basis by g_to_lagrange (tests/g1_lagrange_ref.py), the receipt, and the flag word zk_srs_contribution_check owes a
receipt whose points are given by their scalars — no pairing needed: e([a] G1, [b] G2) = e(G1, G2)^(ab).
Points are affine int tuples, identity None; G2 points ((x0, x1), (y0, y1))."""
import numpy as np

from g1_lagrange_ref import from_mont_limbs, g_to_lagrange, to_mont_limbs  # noqa: F401  (re-exported)
from zkoracle import curve, field as F
from zkoracle.hashes import ChaCha20Rng

SAME_SECRET, LINKS, NONTRIVIAL, RESIDENT = 1, 2, 4, 8
FIELDS = ("before_g1", "after_g1", "s_g1", "s_g2")


def secret_of_seed(seed):
    """the first Fr draw of ChaCha20Rng::from_seed(seed): zk_srs_setup's tau and zk_srs_update's s"""
    return ChaCha20Rng(bytes(seed)).fr()


def update(g, s):
    """g'[i] = [s^i] g[i]"""
    out, p = [], 1
    for pt in g:
        out.append(curve.mul(pt, p) if pt is not None else None)
        p = p * s % F.R
    return out


def update_both(g, s, k):
    """(g', g_lagrange') of a contribution by s to the monomial basis g of degree k"""
    g2 = update(g, s)
    return g2, g_to_lagrange(g2, k)


def contribution(before_g1, s):
    """the receipt of a step by s from an SRS whose g[1] is before_g1"""
    return {"before_g1": before_g1, "after_g1": curve.mul(before_g1, s) if before_g1 is not None else None,
            "s_g1": curve.mul(curve.G1_GEN, s), "s_g2": curve.g2_mul(curve.G2_GEN, s)}


def contribution_of_scalars(b, a, u, v):
    """a receipt whose four points are [b] G1, [a] G1, [u] G1, [v] G2 (an honest one has a = b v, u = v)"""
    return {"before_g1": curve.mul(curve.G1_GEN, b % F.R), "after_g1": curve.mul(curve.G1_GEN, a % F.R),
            "s_g1": curve.mul(curve.G1_GEN, u % F.R), "s_g2": curve.g2_mul(curve.G2_GEN, v % F.R)}


def expected_flags(b, a, u, v):
    """SAME_SECRET | LINKS | NONTRIVIAL of contribution_of_scalars(b, a, u, v).  An identity among the four points (a scalar
    that is 0 mod r) is an improper receipt: no bit at all, as for a point off its curve."""
    b, a, u, v = (x % F.R for x in (b, a, u, v))
    if 0 in (b, a, u, v):
        return 0
    f = 0
    if u != 1:
        f |= NONTRIVIAL
    if u == v:
        f |= SAME_SECRET  # e([u] G1, G2) == e(G1, [v] G2)
    if a == b * v % F.R:
        f |= LINKS        # e([a] G1, G2) == e([b] G1, [v] G2)
    return f


def g2_to_words(pt):
    """G2 affine ((x0, x1), (y0, y1)) -> the 16-word Montgomery image of zk_srs_set_g2 (identity: zeros)"""
    if pt is None:
        return np.zeros(16, dtype=np.uint64)
    words = []
    for c in (pt[0][0], pt[0][1], pt[1][0], pt[1][1]):
        m = c * (1 << 256) % F.P
        words += [(m >> (64 * q)) & 0xFFFFFFFFFFFFFFFF for q in range(4)]
    return np.array(words, dtype=np.uint64)


def g2_from_words(w):
    rinv = F.inv(1 << 256, F.P)
    c = [sum(int(w[4 * q + i]) << (64 * i) for i in range(4)) * rinv % F.P for q in range(4)]
    return None if not any(c) else ((c[0], c[1]), (c[2], c[3]))


def contribution_to_limbs(c):
    """a receipt of points -> the dict of limb arrays Engine.srs_contribution_check takes"""
    out = {f: to_mont_limbs([c[f]])[0] for f in FIELDS[:3]}
    out["s_g2"] = g2_to_words(c["s_g2"])
    return out


def contribution_from_limbs(c):
    out = {f: from_mont_limbs(np.asarray(c[f]))[0] for f in FIELDS[:3]}
    out["s_g2"] = g2_from_words(c["s_g2"])
    return out
