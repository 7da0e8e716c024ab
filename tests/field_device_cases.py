"""Cases and expected results for tests/field_device_check.hip (one record per case, one case per lane).

Groups A and C (field.hip.h, ec.hip.h: canonical outputs) are computed with big integers; groups B and D (field29.hip.h,
ec29.hip.h: lazy outputs) limb for limb with tests/field29_model.py, which tests/test_field29_model.py anchors to big
integers.  Everything is seeded; `build()` returns the same arrays on every call.

The branch classes the GPU test must see (both sides of every final conditional subtraction, the exceptional curve steps,
every lift of an accumulator, ...) are counted here, from the model — never from what the device returns.
"""
import itertools
import random
from collections import Counter

import numpy as np

import field29_model as M
from field29_model import FQ, FR, M29, extreme, split29, value, words8
from zkoracle import curve as C
from zkoracle import field as F

REC_WORDS, OPND, OUT_WORDS, DONE = 100, 4, 40, 0x600D0000
MAGIC_IN, MAGIC_OUT = 0x43464B5A, 0x52464B5A

# the harness's op codes
(FE_ADD, FE_SUB, FE_NEG, FE_DBL, FE_MUL, FE_SQR, FE_TO_MONT, FE_FROM_MONT, FE_INV, REDUCE_ONCE, REDUCE_ONCE_ASM,
 FE_LOAD_STORE) = range(1, 13)
(TO29, TO29_X32, FROM29, MUL29_S, MUL29_C, SQR29_S, SQR29_C, MUL2ADD29_S, MUL2ADD29_C, MUL1ADD29_S, MUL1ADD29_C, MUL4ADD29_S,
 MUL4ADD29_C, MUL5ADD29_S, MUL5ADD29_C, ADD29, NORM29, IS_ZERO29, STD_TO_INTERNAL, INTERNAL_TO_STD) = range(20, 40)
SUB29_OPS = {(2, 29): 40, (3, 29): 41, (4, 29): 42, (5, 30): 43, (6, 29): 44, (7, 29): 45, (7, 31): 46, (8, 29): 47, (9, 29): 48,
             (10, 29): 49, (13, 30): 50, (33, 29): 51, (65, 30): 52}
G1X_DBL, G1X_DBL_AFFINE, G1X_ADD_AFFINE, G1X_ADD, G1X_TO_JAC, G1X_LOAD_STORE = range(60, 66)
(G1X29_FROM_STD, G1X29_TO_STD, G1X29_ADD_AFFINE_CS, G1X29_ADD_AFFINE_CI, G1X29_ADD_AFFINE_NS, G1X29_ADD_AFFINE_NI, G1X29_ADD_S,
 G1X29_ADD_C, G1X29_DBL_RARE, G1X29_LOAD_STORE, MUL29_CALL, INTERNAL_TO_STD_CALL, G1X29_SHFL_DOWN, G1X29_CHAIN) = range(70, 84)
OP_NAMES = {v: k for k, v in list(globals().items()) if k.isupper() and isinstance(v, int) and 1 <= v < 84 and k not in (
    "REC_WORDS", "OPND", "OUT_WORDS", "M29")}
OP_NAMES.update({v: "SUB29_%d_%d" % k for k, v in SUB29_OPS.items()})

N_FIELD = 2048            # cases per field op and modulus (padded with random operands up to this)
SHFL_OFFSETS = (1, 2, 4, 8, 16, 32, 63)  # the MSM tails' tree steps, plus 1 and 63
LIFTS = list(itertools.product(range(9), range(5), range(2), range(2)))
P = F.P


class CaseSet:
    def __init__(self):
        self.rows = []
        self.classes = Counter()

    def add(self, op, mod, words, expect, aux=0, alt=None, cls=None):
        """expect / alt: list of (first result word, words); alt is what the ZK_EC29_SQR=0 ZK_EC29_FUSE=0 build gives."""
        assert len(words) <= REC_WORDS - OPND and all(0 <= w < (1 << 32) for w in words)
        self.rows.append((op, mod, aux, words, expect, alt if alt is not None else expect))
        for c in ([cls] if isinstance(cls, str) else cls or []):
            self.classes[(OP_NAMES[op], mod, c)] += 1

    def arrays(self):
        order = sorted(range(len(self.rows)), key=lambda i: (self.rows[i][0], self.rows[i][1]))  # stable
        n = len(order)
        recs = np.zeros((n, REC_WORDS), dtype=np.uint32)
        exp = np.zeros((2, n, OUT_WORDS), dtype=np.uint32)
        mask = np.zeros((n, OUT_WORDS), dtype=bool)
        for k, i in enumerate(order):
            op, mod, aux, words, expect, alt = self.rows[i]
            recs[k, 0], recs[k, 1], recs[k, 2] = op, mod, aux
            recs[k, OPND:OPND + len(words)] = words
            for which, e in ((0, expect), (1, alt)):
                for off, ws in e:
                    exp[which, k, off:off + len(ws)] = ws
                    mask[k, off:off + len(ws)] = True
            exp[:, k, OUT_WORDS - 1] = DONE | op
            mask[k, OUT_WORDS - 1] = True
        return recs, exp, mask


# ---- operands ----------------------------------------------------------------------------------------------------------
def edge_values(p):
    """Canonical edge values: small, p - small, halves, the Montgomery constants, single bits and runs of ones in both limb
    widths (words of all ones wherever the value stays below p)."""
    r = (1 << 256) % p
    v = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, r, r * r % p, pow(1 << 256, -1, p)]
    v += [1 << (32 * i) for i in range(8)] + [(1 << (32 * i)) - 1 for i in range(1, 8)]
    v += [1 << (29 * i) for i in range(9) if (1 << (29 * i)) < p] + [(1 << (29 * i)) - 1 for i in range(1, 9)]
    v += [(1 << 253) - 1, ((1 << 253) - 1) ^ 0xFFFFFFFF]  # the largest all-ones value below p; the same with a zero low word
    assert all(0 <= x < p for x in v)
    return v


def field_pairs(p, rng):
    e = edge_values(p)
    pairs = [(a, b) for a in e[:14] for b in e] + [(a, a) for a in e]
    for a in e + [rng.randrange(p) for _ in range(60)]:
        pairs += [(a, (p - a) % p), (a, (p + 1 - a) % p), (a, (p - 1 - a) % p), (a, a)]  # a + b = p, p + 1, p - 1; a = b
        pairs += [(a, (a + 1) % p)]                                                      # a - b borrows through all eight words
    pairs += [(p - 1, p - 1), (0, 1), (0, p - 1), (1 << 224, 1), (1 << 224, (1 << 224) + 1)]   # 2p - 2; long borrows
    return pairs


def pad(cases, n, make):
    while len(cases) < n:
        cases.append(make())
    return cases


def lazy29(rng, p, k, bits=29):
    """A random lazy operand: value below k p, lower limbs below 2^bits (non-normalised when bits > 29)."""
    v = rng.randrange(k * p)
    a = split29(v)
    if bits > 29:  # move whole units of 2^29 from limb i + 1 down into limb i: the value is unchanged
        for i in range(7, -1, -1):
            t = min(a[i + 1], rng.randrange(1 << (bits - 29)))
            a[i + 1] -= t
            a[i] += t << 29
    assert value(a) == v and all(l < (1 << 32) for l in a)
    return a


# ---- groups A and B -----------------------------------------------------------------------------------------------------
def field_cases(cs, f, mod):
    p = f.p
    rng = random.Random(0xF1E1D + mod)
    r = (1 << 256) % p
    ri = pow(r, -1, p)
    e = edge_values(p)
    rand = lambda: rng.randrange(p)

    pairs = pad(field_pairs(p, rng), N_FIELD, lambda: (rand(), rand()))
    for a, b in pairs:
        w = words8(a) + words8(b)
        s = a + b
        cs.add(FE_ADD, mod, w, [(0, words8(s % p))], cls="sum<p" if s < p else ("sum=p" if s == p else "sum>p"))
        cs.add(FE_SUB, mod, w, [(0, words8((a - b) % p))], cls="borrow" if a < b else ("equal" if a == b else "plain"))
    singles = pad(list(e), N_FIELD, rand)
    for a in singles:
        w = words8(a)
        cs.add(FE_NEG, mod, w, [(0, words8(-a % p))], cls="zero" if a == 0 else "nonzero")
        cs.add(FE_DBL, mod, w, [(0, words8(2 * a % p))], cls="2a<p" if 2 * a < p else "2a>=p")
        cs.add(FE_TO_MONT, mod, w, [(0, words8(a * r % p))])
        cs.add(FE_FROM_MONT, mod, w, [(0, words8(a * ri % p))])
        cs.add(FE_LOAD_STORE, mod, w, [(0, w)])
        cs.add(FE_SQR, mod, w, [(0, words8(a * a * ri % p))], cls=_mont_side(a, a, p))
    for _ in range(1024):  # squares of large elements: the unreduced total passes p about one time in six
        a = rng.randrange(p - p // 10, p)
        cs.add(FE_SQR, mod, words8(a), [(0, words8(a * a * ri % p))], cls=_mont_side(a, a, p))
    for a in pad([x for x in e if x], 512, lambda: rng.randrange(1, p)):  # 256 squarings and up to 256 products per lane
        cs.add(FE_INV, mod, words8(a), [(0, words8(pow(a, -1, p) * r * r % p))])
    cs.add(FE_INV, mod, words8(0), [(0, words8(0))])
    # Montgomery products on both sides of the final conditional subtraction: picked by the unreduced total
    mp = [(a, b) for a in e[:12] for b in e] + [(a, b) for a in e[18:] for b in e[18:]]  # and the runs of ones with each other
    want = {"total<p": 0, "total>=p": 0}
    for a, b in mp:
        want[_mont_side(a, b, p)] += 1
    while len(mp) < N_FIELD or min(want.values()) < 300:
        a, b = rand(), rand()
        side = _mont_side(a, b, p)
        if len(mp) >= N_FIELD - 400 and want[side] >= 300 and min(want.values()) < 300:
            continue
        want[side] += 1
        mp.append((a, b))
    for a, b in mp:
        cs.add(FE_MUL, mod, words8(a) + words8(b), [(0, words8(a * b * ri % p))], cls=_mont_side(a, b, p))
    # reduce_once: a < 2p on both sides, at the edges
    ro = [0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p - 2, (1 << 253) - 1, 1 << 253, p + (1 << 224), p - (1 << 224)]
    ro += [x + p for x in e] + e
    ro = pad(ro, N_FIELD, lambda: rng.randrange(2 * p))
    for a in ro:
        for op in (REDUCE_ONCE, REDUCE_ONCE_ASM):
            cs.add(op, mod, words8(a), [(0, words8(a - p if a >= p else a))], cls="a>=p" if a >= p else "a<p")

    # ---- B: conversions
    big = [(1 << 256) - 1, (1 << 254) - 1, 1 << 255, p, 2 * p, 5 * p]
    for a in pad(e + big, N_FIELD, lambda: rng.randrange(1 << 256)):
        cs.add(TO29, mod, words8(a), [(0, f.to29(a))])
    for a in pad(e + [(1 << 254) - 1, p], N_FIELD, lambda: rng.randrange(1 << 254)):
        cs.add(TO29_X32, mod, words8(a), [(0, f.to29_x32(a))], cls="largest" if a == p - 1 else None)
    for a in pad(e + big, N_FIELD, lambda: rng.randrange(1 << 256)):
        cs.add(FROM29, mod, f.to29(a), [(0, words8(f.from29(f.to29(a))))])
    for a in pad(list(e), N_FIELD, rand):
        cs.add(STD_TO_INTERNAL, mod, words8(a), [(0, f.std_to_internal(a))], cls="largest" if a == p - 1 else None)

    # ---- B: products.  Operand lists: the contract extremes of tests/test_field29_model.py, all-limbs-max normalised
    # operands, zero in a non-zero representative (the total is then exactly p), the edge values, random lazy operands.
    ones = [M29] * 9
    plimbs = split29(p)
    ext = [(extreme(ba, ka, p), extreme(bb, kb, p), ka * kb) for ba, bb, ka, kb in MUL29_EXTREMES]
    ext += [(ones, f.pow2(261), 170), (f.pow2(261), ones, 170), (ones, f.to29(1), 170)]
    ext += [(plimbs, f.to29(x), 1) for x in e if x] + [(f.to29(x), plimbs, 1) for x in e[1:8]] + [(split29(2 * p), f.pow2(261), 2)]
    ext += [(f.to29(a), f.to29(b), 1) for a in e[:12] for b in e]
    ext = pad(ext, N_FIELD, lambda: (lazy29(rng, p, 12, 30), lazy29(rng, p, 14, 30), 168))
    for a, b, _ in ext:
        want_r = f.mul29(a, b)
        cl = _lazy_side(want_r, p)
        for op in (MUL29_S, MUL29_C):
            cs.add(op, mod, a + b, [(0, want_r)], cls=cl)
    sq = [extreme(bits, k, p) for bits, k in SQR29_EXTREMES] + [ones, plimbs, split29(2 * p)] + [f.to29(x) for x in e]
    sq = pad(sq, N_FIELD, lambda: lazy29(rng, p, 12, 30))
    for a in sq:
        want_r = f.sqr29(a)
        for op in (SQR29_S, SQR29_C):
            cs.add(op, mod, a, [(0, want_r)], cls=_lazy_side(want_r, p))
    zero = [0] * 9
    m2 = [(extreme(29, ka, p), extreme(30.7, kb, p), extreme(29, kc, p) if kc else zero, extreme(30.7, kd, p) if kd else zero)
          for ka, kb, kc, kd in MUL2ADD_EXTREMES]
    m2 += [(ones, f.to29(1), zero, zero), (ones, f.to29(1), ones, f.to29(1))]
    m2 += [(plimbs, f.to29(x), zero, f.to29(x)) for x in e[1:8]] + [(plimbs, f.to29(x), split29(2 * p), f.to29(1)) for x in e[1:8]]
    m2 += [(f.to29(a), f.to29(b), f.to29(b), f.to29(a)) for a in e[:8] for b in e]
    m2 = pad(m2, N_FIELD, lambda: (lazy29(rng, p, 8), lazy29(rng, p, 12, 30), lazy29(rng, p, 5), lazy29(rng, p, 14, 30)))
    for a, b, c, d in m2:
        want_r = f.mul2add29(a, b, c, d)
        for op in (MUL2ADD29_S, MUL2ADD29_C):
            cs.add(op, mod, a + b + c + d, [(0, want_r)], cls=_lazy_side(want_r, p))
    for K, ops in ((1, (MUL1ADD29_S, MUL1ADD29_C)), (4, (MUL4ADD29_S, MUL4ADD29_C)), (5, (MUL5ADD29_S, MUL5ADD29_C))):
        mk = [([extreme(29, x, p) for x, _ in ks], [extreme(29, y, p) for _, y in ks]) for kk, ks in MULK_EXTREMES if kk == K]
        mk += [([ones] * K, [f.to29(1)] * K), ([plimbs] + [zero] * (K - 1), [f.to29(3)] + [zero] * (K - 1)),
               ([plimbs] * K, [f.to29(x) for x in e[1:K + 1]])]
        mk += [([f.to29(e[(i + j) % len(e)]) for j in range(K)], [f.to29(e[(3 * i + j) % len(e)]) for j in range(K)]) for i in range(64)]
        kmax = [x for x in (12, 6, 5, 5, 5)][K - 1]
        mk = pad(mk, N_FIELD, lambda: ([lazy29(rng, p, kmax) for _ in range(K)], [lazy29(rng, p, kmax + 1) for _ in range(K)]))
        for a, b in mk:
            want_r = f.mulKadd29(a, b)
            w = [0] * 90
            for j in range(K):
                w[9 * j:9 * j + 9] = a[j]
                w[45 + 9 * j:45 + 9 * j + 9] = b[j]
            for op in ops:
                cs.add(op, mod, w, [(0, want_r)], cls=_lazy_side(want_r, p))

    # ---- B: additions
    ad = [([(1 << 31) - 1] * 9, [1 << 31] * 9), (ones, ones), (zero, zero)] + [(f.to29(a), f.to29(b)) for a in e[:10] for b in e[:10]]
    for a, b in pad(ad, N_FIELD, lambda: (lazy29(rng, p, 40, 31), lazy29(rng, p, 40, 31))):
        cs.add(ADD29, mod, a + b, [(0, f.add29(a, b))])
    nm = [[(1 << 32) - 1] + [0] * 8, [(1 << 32) - 1 - 7] * 8 + [5], [M29] * 8 + [0], [M29 + 1] * 8 + [0], zero] + [f.to29(x) for x in e]
    for a in pad(nm, N_FIELD, lambda: lazy29(rng, p, 160, 31)):
        cs.add(NORM29, mod, a, [(0, f.norm29(a))])
    for (K, E), op in SUB29_OPS.items():
        abits, kb, bbits = SUB29_SITE[(K, E)]
        sb = [sub29_extreme(f, K, E)]
        C_ = f.spread(K, E)
        sb += [(zero, list(C_)), ([(1 << 29) - 1] * 9, list(C_)), (zero, zero), (zero, [(1 << E) - 1] * 8 + [((K - 1) * p) >> 232])]
        sb += [(f.to29(a), f.to29(b)) for a in e[:8] for b in e[:8]]
        kk = kb if kb else 5
        sb = pad(sb, N_FIELD, lambda: (lazy29(rng, p, 4, abits), lazy29(rng, p, kk, int(bbits))))
        for a, b in sb:
            cs.add(op, mod, a + b, [(0, f.sub29(K, E, a, b))])
    # is_zero29: 0, p, p +- 1, 2p - 1, each with one limb perturbed
    iz = []
    for v in (0, p, p + 1, p - 1, 2 * p - 1, 1):
        a = split29(v)
        iz.append(a)
        for i in range(9):
            for d in (1, 1 << 28):
                b = list(a)
                b[i] ^= d
                iz.append(b)
    for a in pad(iz, 512, lambda: lazy29(rng, p, 2)):
        z = f.is_zero29(a)
        cs.add(IS_ZERO29, mod, a, [(36, [int(z)])], cls="zero" if z else "nonzero")
    # internal_to_std: both sides of its reduce_once, the top of its contract, zero as p
    its = [extreme(29, 168, p), extreme(30.6, 168, p), ones[:8] + [0], plimbs, split29(2 * p), zero, f.to29_x32(p - 1), f.std_to_internal(p - 1)]
    its += [f.to29_x32(x) for x in e] + [f.std_to_internal(x) for x in e]
    cnt = Counter()
    its2 = []
    for a in its:
        its2.append(a)
        cnt[_its_side(f, a)] += 1
    while len(its2) < N_FIELD or min(cnt["raw<p"], cnt["raw>=p"]) < 300:
        a = lazy29(rng, p, rng.choice((2, 32, 168)))
        s = _its_side(f, a)
        if len(its2) >= N_FIELD - 400 and cnt[s] >= 300 and min(cnt["raw<p"], cnt["raw>=p"]) < 300:
            continue
        cnt[s] += 1
        its2.append(a)
    for a in its2:
        cs.add(INTERNAL_TO_STD, mod, a, [(0, words8(f.internal_to_std(a)))], cls=_its_side(f, a))
        if mod == 1:
            cs.add(INTERNAL_TO_STD_CALL, 1, a, [(0, words8(f.internal_to_std(a)))], cls=_its_side(f, a))
    if mod == 1:
        for a, b, _ in ext:
            want_r = f.mul29(a, b)
            cs.add(MUL29_CALL, 1, a + b, [(0, want_r)], cls=_lazy_side(want_r, p))


def _mont_side(a, b, p):
    m = (-a * b * pow(p, -1, 1 << 256)) % (1 << 256)
    t = (a * b + m * p) >> 256
    assert t < 2 * p
    return "total>=p" if t >= p else "total<p"


def _lazy_side(r, p):
    v = value(r)
    return "total=p" if v == p else ("total>=p" if v > p else "total<p")


def _its_side(f, a):
    return "raw>=p" if f.from29(f.mul29(a, f.pow2(256))) >= f.p else "raw<p"


# the contract extremes, shared with tests/test_field29_model.py (which checks them against big integers)
MUL29_EXTREMES = [(30.6, 30, 12, 14), (30.6, 30, 168, 1), (30.6, 30, 1, 168), (30.6, 30, 84, 2), (30.6, 30, 32, 5), (30.6, 30, 13, 12),
                  (30, 30.6, 14, 12), (29, 31.6, 2, 84), (31.6, 29, 84, 2), (29, 31.3, 65, 65), (29, 31.3, 32, 73), (29, 30, 32, 35),
                  (29, 29, 32, 32), (29, 29, 66, 1), (29, 29, 108, 1)]
SQR29_EXTREMES = [(30.3, 12), (30.3, 8), (30.3, 1), (29, 12), (29, 5), (29, 32)]
MUL2ADD_EXTREMES = [(8, 12, 5, 3), (5, 12, 2, 3), (12, 7, 12, 7), (1, 84, 1, 84), (84, 1, 84, 1), (168, 1, 0, 0), (1, 167, 1, 1)]
MULK_EXTREMES = [(1, [(168, 1)]), (1, [(12, 14)]), (2, [(12, 7), (7, 12)]), (3, [(8, 7), (7, 8), (56, 1)]), (4, [(6, 7)] * 4),
                 (4, [(42, 1)] * 4), (4, [(1, 42)] * 4), (5, [(33, 1)] * 5), (5, [(5, 6)] * 5), (5, [(1, 33)] * 5),
                 (5, [(164, 1), (1, 1), (1, 1), (1, 1), (1, 1)])]
# sub29<K, E> of csrc/: (K, E) -> (limb bits of a, k of b or None for "a 256-bit integer", limb bits of b) at the call site
SUB29_SITE = {(2, 29): (29, 1, 29), (3, 29): (29, 2, 29), (4, 29): (29, 3, 29), (5, 30): (29, 4, 30), (6, 29): (29, 5, 29),
              (7, 29): (29, None, 29), (7, 31): (29, 6, 30.6), (8, 29): (29, 7, 29), (9, 29): (29, 8, 29), (10, 29): (29, 9, 29),
              (13, 30): (30, 12, 30), (33, 29): (30, 32, 29), (65, 30): (30, 64, 30)}
assert set(SUB29_SITE) == set(SUB29_OPS)


def sub29_extreme(f, K, E):
    """(a, b): a with every limb at its call site's maximum, b the largest its call site admits."""
    abits, kb, bbits = SUB29_SITE[(K, E)]
    if kb is None:  # limbs of the largest 256-bit integer (5.29 p for both moduli)
        b = f.to29((1 << 256) - 1)
        assert value(b) < 6 * f.p
    elif bbits == 30.6:  # ppp + 2 q with three normalised product outputs: limbs <= 3 (2^29 - 1), value < 6p
        lo = 3 * M29
        low = sum(lo << (29 * i) for i in range(8))
        b = [lo] * 8 + [(kb * f.p - 1 - low) >> 232]
    else:
        b = extreme(bbits, kb, f.p)
    return [(1 << abits) - 1] * 9, b


# ---- groups C and D -----------------------------------------------------------------------------------------------------
R256 = (1 << 256) % P
S261 = (1 << 261) % P


def _std(v):
    return words8(v * R256 % P)


def _xyzz(pt, z):
    """Plain field values (X, Y, ZZ, ZZZ) of pt under Z = z; the identity as G1X::identity() (1, 1, 0, 0)."""
    if pt is None:
        return (1, 1, 0, 0)
    zz, zzz = z * z % P, z * z * z % P
    return (pt[0] * zz % P, pt[1] * zzz % P, zz, zzz)


def _g1x_words(q):
    return [w for c in q for w in _std(c)]


def _dbl(q):
    X, Y, ZZ, ZZZ = q
    if ZZ == 0:
        return q
    u = 2 * Y % P
    v = u * u % P
    w = u * v % P
    s = X * v % P
    m = 3 * X * X % P
    x3 = (m * m - 2 * s) % P
    return (x3, (m * (s - x3) - w * Y) % P, v * ZZ % P, w * ZZZ % P)


def _add(a, b):
    """add-2008-s as ec.hip.h's g1x_add, on plain field values; returns (result, branch)."""
    if b[2] == 0:
        return a, "b_inf"
    if a[2] == 0:
        return b, "acc_inf"
    u1, u2, s1, s2 = a[0] * b[2] % P, b[0] * a[2] % P, a[1] * b[3] % P, b[1] * a[3] % P
    p_, r_ = (u2 - u1) % P, (s2 - s1) % P
    if p_ == 0:
        return (_dbl(a), "dbl") if r_ == 0 else ((1, 1, 0, 0), "cancel")
    pp = p_ * p_ % P
    ppp = p_ * pp % P
    q = u1 * pp % P
    x3 = (r_ * r_ - ppp - 2 * q) % P
    return (x3, (r_ * (q - x3) - s1 * ppp) % P, a[2] * b[2] % P * pp % P, a[3] * b[3] % P * ppp % P), "add"


def _add_affine(a, pt):
    """madd-2008-s as ec.hip.h's g1x_add_affine."""
    x, y = pt
    if a[2] == 0:
        return (x, y, 1, 1), "acc_inf"
    p_, r_ = (x * a[2] - a[0]) % P, (y * a[3] - a[1]) % P
    if p_ == 0:
        return (_dbl((x, y, 1, 1)), "dbl") if r_ == 0 else ((1, 1, 0, 0), "cancel")
    pp = p_ * p_ % P
    ppp = p_ * pp % P
    q = a[0] * pp % P
    x3 = (r_ * r_ - ppp - 2 * q) % P
    return (x3, (r_ * (q - x3) - a[1] * ppp) % P, a[2] * pp % P, a[3] * ppp % P), "add"


def _affine(q):
    if q[2] == 0:
        return None
    return (q[0] * pow(q[2], -1, P) % P, q[1] * pow(q[3], -1, P) % P)


def _x0_point():
    """An affine point with x = 0 exists iff 3 is a square mod p."""
    return pow(3, (P - 1) // 2, P) == 1


def curve_points():
    rng = random.Random(0xC0FFEE)
    pts = [C.G1_GEN] + [C.mul(C.G1_GEN, rng.randrange(1, F.R)) for _ in range(23)] + [C.mul(C.G1_GEN, k) for k in (2, 3, F.R - 1)]
    return pts


def curve_cases(cs):
    rng = random.Random(0xD1CE)
    pts = curve_points()
    assert not _x0_point(), "y^2 = 3 has no root mod p: no affine point with x = 0 on BN254 G1, so no such case is made"
    rz = lambda: rng.randrange(1, P)
    f = FQ

    # ---- C: ec.hip.h on canonical words, against the same formulas in big integers; the affine result against the oracle
    pairs = [(a, b) for a in pts[:8] for b in pts[:8]] + [(a, a) for a in pts] + [(a, C.neg(a)) for a in pts]
    pairs += [(None, a) for a in pts[:6]] + [(a, None) for a in pts[:6]] + [(None, None)]
    pairs = pad(pairs, 1024, lambda: (rng.choice(pts), rng.choice(pts)))
    for a, b in pairs:
        qa, qb = _xyzz(a, rz()), _xyzz(b, rz())
        got, br = _add(qa, qb)
        assert _affine(got) == C.add(a, b)
        cs.add(G1X_ADD, 1, _g1x_words(qa) + _g1x_words(qb), [(0, _g1x_words(got))], cls=br)
        if b is not None:
            got, br = _add_affine(qa, b)
            assert _affine(got) == C.add(a, b)
            cs.add(G1X_ADD_AFFINE, 1, _g1x_words(qa) + _std(b[0]) + _std(b[1]), [(0, _g1x_words(got))], cls=br)
        got = _dbl(qa)
        assert _affine(got) == C.add(a, a)
        cs.add(G1X_DBL, 1, _g1x_words(qa), [(0, _g1x_words(got))], cls="inf" if a is None else "point")
        cs.add(G1X_LOAD_STORE, 1, _g1x_words(qa), [(0, _g1x_words(qa))])
        jac = (1, 1, 0) if a is None else (qa[0] * qa[2] % P, qa[1] * qa[3] % P, qa[2])
        assert C.to_affine(jac) == a
        cs.add(G1X_TO_JAC, 1, _g1x_words(qa), [(0, [w for c in jac for w in _std(c)])], cls="inf" if a is None else "point")
        if a is not None:
            got = _dbl((a[0], a[1], 1, 1))
            assert _affine(got) == C.add(a, a)
            cs.add(G1X_DBL_AFFINE, 1, _std(a[0]) + _std(a[1]), [(0, _g1x_words(got))])

    # ---- D: ec29.hip.h, limb for limb against the model
    def stored(a):
        return M.g1x29_store(a)

    def out29(a, ret=None):
        e = [(0, stored(a)), (38, [int(a.inf)])]
        if ret is not None:
            e += [(36, [int(ret)]), (37, [int(f.is_zero29(a.zz))])]
        return e

    for a, _ in pairs[:600]:
        q = _xyzz(a, rz())
        m = M.g1x29_from_std(*(c * R256 % P for c in q))
        assert M.affine_of(m) == a
        cs.add(G1X29_FROM_STD, 1, _g1x_words(q), out29(m), cls="inf" if a is None else "point")

    variants = [(G1X29_ADD_AFFINE_CS, True, False), (G1X29_ADD_AFFINE_CI, True, True), (G1X29_ADD_AFFINE_NS, False, False),
                (G1X29_ADD_AFFINE_NI, False, True)]

    def add_affine_case(acc, pt, tag):
        for op, check, internal in variants:
            s = S261 if internal else R256
            x, y = pt[0] * s % P, pt[1] * s % P
            res = []
            for sqr, fuse in ((True, True), (False, False)):
                a = acc.copy()
                ret = M.g1x29_add_affine(a, x, y, check, internal, sqr, fuse)
                res.append((a, ret))
            (a1, r1), (a0, r0) = res
            cl = [tag]
            if check and not r1:
                assert a1.key() == acc.key() and not r0
                cl.append("refused")
            if not check and tag in ("same", "negated"):
                assert f.is_zero29(a1.zz) and f.is_zero29(a0.zz) and r1 and r0
                cl.append("zz=0")
            if tag == "generic":
                assert M.affine_of(a1) == M.affine_of(a0) == C.add(M.affine_of(acc), pt)
            cs.add(op, 1, stored(acc) + words8(x) + words8(y), out29(a1, r1), alt=out29(a0, r0), cls=cl)

    # every lift of the accumulator, for a generic step, the same point and the negated point
    for k, (qa, pb) in enumerate([(pts[1], pts[2]), (pts[0], pts[3]), (pts[4], pts[0]), (pts[5], pts[6])]):
        z = rz()
        for lift in LIFTS:
            add_affine_case(M.lifted(qa, z, *lift), pb, "generic")
            cs.classes[("lift", 1, lift)] += 1
            if k < 2:
                add_affine_case(M.lifted(qa, z, *lift), qa, "same")
                add_affine_case(M.lifted(qa, z, *lift), C.neg(qa), "negated")
    for pt in pts:
        add_affine_case(M.g1x29_identity(), pt, "acc_inf")

    # g1x29_add / g1x29_dbl_rare / to_std / load-store on every lift
    b_lifts = [(0, 0, 0, 0), (8, 4, 1, 1), (8, 0, 0, 1), (0, 4, 1, 0)]

    def add_case(acc, b):
        a = acc.copy()
        br = M.g1x29_add(a, b)
        want = C.add(M.affine_of(acc), M.affine_of(b))
        assert M.affine_of(a) == want
        for op in (G1X29_ADD_S, G1X29_ADD_C):
            cs.add(op, 1, stored(acc) + stored(b), out29(a), cls=br)

    for k, (qa, qb) in enumerate([(pts[1], pts[2]), (pts[7], pts[0]), (pts[8], pts[9])]):
        za, zb = rz(), rz()
        for lift in LIFTS:
            acc = M.lifted(qa, za, *lift)
            bl = b_lifts[(lift[0] + lift[1]) % 4]
            add_case(acc, M.lifted(qb, zb, *bl))
            if k == 0:
                add_case(acc, M.lifted(qa, zb, *bl))           # P + P: through g1x29_dbl_rare
                add_case(acc, M.lifted(C.neg(qa), zb, *bl))    # P - P
                add_case(acc, M.g1x29_identity())
                add_case(M.g1x29_identity(), acc)
            d = acc.copy()
            M.g1x29_dbl_rare(d)
            assert M.affine_of(d) == C.add(qa, qa)
            cs.add(G1X29_DBL_RARE, 1, stored(acc), out29(d), cls="point")
            cs.add(G1X29_LOAD_STORE, 1, stored(acc), out29(acc), cls="point")
            cs.add(G1X29_TO_STD, 1, stored(acc), [(0, [w for c in M.g1x29_to_std(acc) for w in words8(c)])], cls="point")
    add_case(M.g1x29_identity(), M.g1x29_identity())
    idn = M.g1x29_identity()
    cs.add(G1X29_DBL_RARE, 1, stored(idn), out29(idn), cls="inf")
    cs.add(G1X29_LOAD_STORE, 1, stored(idn), out29(idn), cls="inf")
    cs.add(G1X29_TO_STD, 1, stored(idn), [(0, [w for c in M.g1x29_to_std(idn) for w in words8(c)])], cls="inf")

    # chains of 1, 2 and 40 steps from the identity, compared after g1x29_to_std
    for n in (1, 2, 40):
        for _ in range(128 if n < 40 else 256):
            five = rng.sample(pts[:24], 5)
            res = []
            for sqr, fuse in ((True, True), (False, False)):
                a = M.g1x29_identity()
                ok = True
                want = None
                for k in range(n):
                    pt = five[k % 5]
                    ok &= M.g1x29_add_affine(a, pt[0] * R256 % P, pt[1] * R256 % P, True, False, sqr, fuse)
                    want = C.add(want, pt)
                assert ok and M.affine_of(a) == want
                res.append([(0, [w for c in M.g1x29_to_std(a) for w in words8(c)]), (36, [1])])
            cs.add(G1X29_CHAIN, 1, [w for pt in five for w in _std(pt[0]) + _std(pt[1])], res[0], aux=n, alt=res[1], cls="n=%d" % n)

    # g1x29_shfl_down: full waves of 64 distinct points, some lanes the identity
    for off in SHFL_OFFSETS:
        for wave in range(5):
            lanes = []
            for l in range(64):
                if (l * 7 + wave + off) % 9 == 0:
                    lanes.append(M.g1x29_identity())
                else:
                    lanes.append(M.lifted(C.mul(C.G1_GEN, 64 * wave + l + 5), rz(), l % 9, l % 5, l & 1, (l >> 1) & 1))
            assert len({a.key() for a in lanes if not a.inf}) == sum(not a.inf for a in lanes)
            for l in range(64):
                src = lanes[(l + off) & 63]
                cs.add(G1X29_SHFL_DOWN, 1, stored(lanes[l]), out29(src), aux=off, cls=["off=%d" % off, "inf" if src.inf else "point"])


_CACHE = {}


def build():
    """-> (records, expected[2], mask, class counts); expected[1] is for the ZK_EC29_SQR=0 ZK_EC29_FUSE=0 build."""
    if "v" not in _CACHE:
        cs = CaseSet()
        field_cases(cs, FR, 0)
        field_cases(cs, FQ, 1)
        curve_cases(cs)
        _CACHE["v"] = cs.arrays() + (cs.classes,)
    return _CACHE["v"]
