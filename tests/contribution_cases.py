"""Receipts for the tests of the receipt rule with a G2 point per lane (csrc/pairing.h contribution_check_lanes,
zk_srs_contribution_check_batch): every kind of receipt with the flag word it owes.  The words come from the receipt's scalars
(srs_update_ref.expected_flags) or, for a malformed point, are 0 by the rule itself — no pairing is needed to know them.
A receipt travels as the dict of limb arrays Engine.srs_contribution_check takes."""
import functools
import random

import numpy as np

import pairing_cases as pc
from srs_update_ref import FIELDS, expected_flags, g2_to_words
from zkoracle import field as F

WAVE = 64


def receipt(b, a, u, v):
    """the limbs of ([b] G1, [a] G1, [u] G1, [v] G2); a scalar that is 0 mod r gives the identity"""
    g = pc.g1_words([pc.g1(b), pc.g1(a), pc.g1(u)])
    return {"before_g1": g[0].copy(), "after_g1": g[1].copy(), "s_g1": g[2].copy(), "s_g2": g2_to_words(pc.g2(v))}


def _with(rec, field, words):
    out = {f: rec[f].copy() for f in FIELDS}
    out[field] = np.asarray(words, dtype=np.uint64)
    return out


def _g2_with_p_added(words, col):
    w = np.array(words, dtype=np.uint64).copy()
    v = sum(int(w[col + q]) << (64 * q) for q in range(4)) + F.P
    assert v < 1 << 256
    w[col:col + 4] = [(v >> (64 * q)) & 0xFFFFFFFFFFFFFFFF for q in range(4)]
    return w


@functools.lru_cache(maxsize=None)
def honest_pool(n=6, seed=0x5eed):
    """n distinct honest receipts as (receipt, 7)"""
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        b, v = rnd.randrange(2, F.R), rnd.randrange(2, F.R)
        out.append((receipt(b, b * v, v, v), expected_flags(b, b * v, v, v)))
        assert out[-1][1] == 7
    return tuple(out)


@functools.lru_cache(maxsize=None)
def kinds():
    """(name, receipt, flag word) of every kind of receipt the rule tells apart"""
    rnd = random.Random(0xC0FFEE)
    b, v, w = (rnd.randrange(2, F.R) for _ in range(3))
    good = receipt(b, b * v, v, v)
    out = [("honest", good, expected_flags(b, b * v, v, v))]

    def scalars(name, *s):
        out.append((name, receipt(*s), expected_flags(*s)))

    scalars("u != v", b, b * v, w, v)
    scalars("a != b v", b, b * v + 1, v, v)
    scalars("u = v = 1", b, b, 1, 1)
    scalars("before_g1 = O", 0, b * v, v, v)
    scalars("after_g1 = O", b, 0, v, v)
    scalars("s_g1 = O", b, b * v, 0, v)
    scalars("s_g2 = O", b, b * v, v, 0)
    scalars("s_g2 = -G2", b, -b, -1, -1)
    scalars("s_g2 = -G2, u = 1", b, -b, 1, -1)
    for f in FIELDS[:3]:
        for col, c in ((0, "x"), (4, "y")):
            out.append(("%s.%s + p" % (f, c), _with(good, f, pc.with_p_added(good[f], col)), 0))
    for col, c in ((0, "x.c0"), (4, "x.c1"), (8, "y.c0"), (12, "y.c1")):
        out.append(("s_g2.%s + p" % c, _with(good, "s_g2", _g2_with_p_added(good["s_g2"], col)), 0))
    off = good["s_g2"].copy()
    off[0] ^= np.uint64(1)
    out.append(("s_g2 off the twist", _with(good, "s_g2", off), 0))
    outside = pc.twist_point_outside_g2()
    assert pc.g2_on_twist(outside)
    out.append(("s_g2 outside the subgroup", _with(good, "s_g2", g2_to_words(outside)), 0))
    words = {n: fl for n, _, fl in out}
    assert words["honest"] == 7 and words["u != v"] == 6 and words["a != b v"] == 5 and words["u = v = 1"] == 3
    assert words["s_g2 = -G2"] == 7 and words["s_g2 = -G2, u = 1"] == 2
    assert all(words[n] == 0 for n in words if n.endswith("= O") or "+ p" in n or "twist" in n or "subgroup" in n)
    return tuple(out)


def honest_batch(count):
    pool = honest_pool()
    return [pool[i % len(pool)] for i in range(count)]


def mixed_batch(count):
    """`count` (receipt, word): in every wave of 64 the first and the last lane (and the batch's last lane) hold a receipt with no
    bit, which returns before it walks; in between, honest receipts alternate with every kind in turn, so lanes that return early sit
    beside lanes that walk"""
    ks, pool = kinds(), honest_pool()
    bad = [k for k in ks if k[2] == 0]
    out, nk, nb = [], 0, 0
    for i in range(count):
        lane = i % WAVE
        if lane in (0, WAVE - 1) or i == count - 1:
            out.append(bad[nb % len(bad)][1:])
            nb += 1
        elif lane % 2:
            out.append(pool[i % len(pool)])
        else:
            out.append(ks[nk % len(ks)][1:])
            nk += 1
    return out
