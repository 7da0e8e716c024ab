"""Cases and model of csrc/p256.hip.h's field, point and x-compare routines, for the two harnesses that run the header directly:
tests/p256_host_check.cpp (the portable forms on the CPU, under the sanitizers) and tests/p256_device_check.hip (one case per lane
on the device).  Both read the case file written by write_case_file() and write one result record per case; check_results()
compares with Python integers.

Case file (32-bit little-endian words): MAGIC_IN, n, REC_WORDS, 0, then n records: [0] op  [1] modulus (0 = p, 1 = n)  [2] [3] 0
[4 ..] operand words.  The records are sorted by (op, modulus).  Result record (OUT_WORDS words): [0 .. 24) result words, [24] a
flag (the x-compare's verdict), [25] DONE | op.

Field elements travel as eight words; the operands of MUL / SQR / INV are taken as they are (any reduced value is the Montgomery
form of something), so the expected value of MUL is a b / 2^256 mod m.  Points travel in Montgomery coordinates; results are
compared as affine points, because a Jacobian triple is not unique.

The branch classes counted here come from the model alone:
  ADD   sum<m, m<=sum<2^256, sum>=2^256        (the middle band is 2^224 wide: those cases are constructed)
  SUB   borrow, equal, plain
  MUL / SQR   by the Montgomery total T = (a b + q m) / 2^256:  T<m, m<=T<2^256 (constructed: pick a result below 2^256 - m and b,
              solve for a, keep what the model puts in the band), T>=2^256
"""
import functools
import random

import numpy as np

import es256_ref as R

MAGIC_IN, MAGIC_OUT = 0x43503235, 0x52503235
REC_WORDS, OPND, OUT_WORDS, DONE = 56, 4, 26, 0x600D0000
ADD, SUB, NEG, MUL, SQR, TO_MONT, FROM_MONT, INV = 1, 2, 3, 4, 5, 6, 7, 8
DBL, ADD_MIXED, ADD_FULL, XCMP = 20, 21, 22, 30
OP_NAMES = {ADD: "ADD", SUB: "SUB", NEG: "NEG", MUL: "MUL", SQR: "SQR", TO_MONT: "TO_MONT", FROM_MONT: "FROM_MONT", INV: "INV",
            DBL: "DBL", ADD_MIXED: "ADD_MIXED", ADD_FULL: "ADD_FULL", XCMP: "XCMP"}
FIELD_OPS = (ADD, SUB, NEG, MUL, SQR, TO_MONT, FROM_MONT, INV)
MODULI = (R.P, R.N)
W = 1 << 256
SEED = 0x503235362D31


def words(v, n=8):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def unwords(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def mont_total(a, b, m):
    """T = (a b + q m) / 2^256 with q = -a b / m mod 2^256: what a Montgomery product holds before its final subtraction."""
    ab = a * b
    q = (-ab * pow(m, -1, W)) % W
    return (ab + q * m) >> 256


def mont_class(a, b, m):
    t = mont_total(a, b, m)
    return "T<m" if t < m else ("m<=T<2^256" if t < W else "T>=2^256")


def add_class(a, b, m):
    s = a + b
    return "sum<m" if s < m else ("m<=sum<2^256" if s < W else "sum>=2^256")


def sub_class(a, b):
    return "borrow" if a < b else ("equal" if a == b else "plain")


def sqrt_mod(a, m):
    """A square root of a mod the prime m, or None (Tonelli-Shanks)."""
    a %= m
    if a == 0:
        return 0
    if pow(a, (m - 1) // 2, m) != 1:
        return None
    q, s = m - 1, 0
    while q % 2 == 0:
        q //= 2
        s += 1
    zz = 2
    while pow(zz, (m - 1) // 2, m) != m - 1:
        zz += 1
    mm, c, t, r = s, pow(zz, q, m), pow(a, q, m), pow(a, (q + 1) // 2, m)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % m
            i += 1
        b = pow(c, 1 << (mm - i - 1), m)
        mm, c = i, b * b % m
        t, r = t * c % m, r * b % m
    return r


def specials(m):
    """Edge operands below m: 0, 1, m - 1, and values whose words are all ones."""
    out = [0, 1, 2, m - 1, m - 2, 2**32 - 1, 2**64 - 1, 2**96 - 1, 2**128 - 1, 2**192 - 1, 2**224 - 1, 2**255 - 1, 2**255,
           (2**32 - 1) << 192, ((2**32 - 1) << 224) - 1, W % m, W * W % m, (m - 1) // 2, (m + 1) // 2]
    assert all(0 <= v < m for v in out)
    return out


class Cases:
    def __init__(self):
        self.recs, self.expect, self.classes = [], [], {}

    def add(self, op, mod, opnd, expect, cls=None):
        assert len(opnd) <= REC_WORDS - OPND
        self.recs.append([op, mod, 0, 0] + list(opnd) + [0] * (REC_WORDS - OPND - len(opnd)))
        self.expect.append(expect)
        if cls is not None:
            key = (OP_NAMES[op], mod, cls)
            self.classes[key] = self.classes.get(key, 0) + 1


def _field_cases(cs, rng):
    rinv = {m: pow(W, -1, m) for m in MODULI}
    for mod, m in enumerate(MODULI):
        sp = specials(m)
        rnd = lambda: rng.randrange(m)
        pairs = [(a, b) for a in sp for b in sp] + [(rnd(), rnd()) for _ in range(700)]
        # ADD: the middle band m <= a + b < 2^256, constructed
        add_pairs = list(pairs)
        for _ in range(260):
            target = rng.randrange(m, W)
            a = rng.randrange(target - m + 1, m)
            add_pairs.append((a, target - a))
        add_pairs += [(m - 1, 1), (m - 1, m - 1), (m - 1, W - m), (m - 1, W - m + 1), (1, m - 2)]
        for a, b in add_pairs:
            cs.add(ADD, mod, words(a) + words(b), ("fe", (a + b) % m), add_class(a, b, m))
        sub_pairs = list(pairs) + [(v, v) for v in (rnd() for _ in range(60))]
        for a, b in sub_pairs:
            cs.add(SUB, mod, words(a) + words(b), ("fe", (a - b) % m), sub_class(a, b))
        for a in sp + [rnd() for _ in range(200)]:
            cs.add(NEG, mod, words(a), ("fe", (-a) % m), "zero" if a == 0 else "nonzero")
            cs.add(TO_MONT, mod, words(a), ("fe", a * W % m))
            cs.add(FROM_MONT, mod, words(a), ("fe", a * rinv[m] % m))
        # MUL: the band m <= T < 2^256, constructed: res < 2^256 - m, b random, a = res R / b; T is res or res + m
        mul_pairs = list(pairs) + [(rng.randrange(m // 2, m), rng.randrange(m // 2, m)) for _ in range(400)]  # (large a b: T >= 2^256 more often)
        made = 0
        while made < 80:
            res, b = rng.randrange(W - m), rng.randrange(1, m)
            a = res * W * pow(b, -1, m) % m
            if mont_class(a, b, m) == "m<=T<2^256":
                mul_pairs.append((a, b))
                made += 1
        for a, b in mul_pairs:
            cs.add(MUL, mod, words(a) + words(b), ("fe", a * b * rinv[m] % m), mont_class(a, b, m))
        sqr_ops = sp + [rnd() for _ in range(700)]
        made = 0
        while made < 80:
            res = rng.randrange(W - m)
            a = sqrt_mod(res * W, m)
            if a is None:
                continue
            for cand in (a, m - a):
                if mont_class(cand, cand, m) == "m<=T<2^256":
                    sqr_ops.append(cand)
                    made += 1
        for a in sqr_ops:
            cs.add(SQR, mod, words(a), ("fe", a * a * rinv[m] % m), mont_class(a, a, m))
        # INV: Montgomery in, Montgomery out: (a / R)^-1 R = R^2 / a; 0 -> 0
        inv_ops = [0, W % m, (m - 1) * W % m, 1, m - 1] + [rnd() for _ in range(507)]
        for a in inv_ops:
            cs.add(INV, mod, words(a), ("fe", W * W * pow(a, -1, m) % m if a else 0), "zero" if a == 0 else "nonzero")


def to_mont(v):
    return v * W % R.P


def lift(rng, pt, z=None):
    """Jacobian Montgomery words of the affine point pt (None: the identity, with arbitrary X and Y)."""
    if pt is None:
        return words(to_mont(rng.randrange(R.P))) + words(to_mont(rng.randrange(R.P))) + words(0)
    z = rng.randrange(1, R.P) if z is None else z
    return words(to_mont(pt[0] * z * z % R.P)) + words(to_mont(pt[1] * z * z * z % R.P)) + words(to_mont(z))


def affine_words(pt):
    return [0] * 16 if pt is None else words(to_mont(pt[0])) + words(to_mont(pt[1]))


def neg(pt):
    return None if pt is None else (pt[0], (-pt[1]) % R.P)


def _point_cases(cs, rng):
    step = R.affine_mul(rng.randrange(1, R.N), R.G)
    pts = [R.affine_mul(rng.randrange(1, R.N), R.G)]
    for _ in range(199):
        pts.append(R.affine_add(pts[-1], step))
    pts += [R.G, neg(R.G), R.affine_add(R.G, R.G)]
    pick = lambda: pts[rng.randrange(len(pts))]
    for i, p in enumerate(pts[:80] + pts[-3:]):
        cs.add(DBL, 0, lift(rng, p, 1 if i % 4 == 0 else None), ("pt", R.affine_add(p, p)), "point")
    for _ in range(8):
        cs.add(DBL, 0, lift(rng, None), ("pt", None), "identity")
    for op in (ADD_MIXED, ADD_FULL):
        second = affine_words if op == ADD_MIXED else (lambda q: lift(rng, q))
        for i in range(96):
            p, q = pick(), pick()
            if p == q or p == neg(q):
                continue
            cs.add(op, 0, lift(rng, p, 1 if i % 8 == 0 else None) + second(q), ("pt", R.affine_add(p, q)), "generic")
        for _ in range(24):
            p = pick()
            cs.add(op, 0, lift(rng, p) + second(p), ("pt", R.affine_add(p, p)), "equal")
            cs.add(op, 0, lift(rng, p) + second(neg(p)), ("pt", None), "opposite")
            cs.add(op, 0, lift(rng, None) + second(p), ("pt", p), "accumulator identity")
            cs.add(op, 0, lift(rng, p) + second(None), ("pt", p), "addend identity")
        for _ in range(4):
            cs.add(op, 0, lift(rng, None) + second(None), ("pt", None), "both identity")


def _xcmp_cases(cs, rng):
    gap = R.P - R.N
    def one(x, z, r, want, cls):
        cs.add(XCMP, 0, words(to_mont(x * z * z % R.P)) + words(to_mont(z)) + words(r), ("flag", int(want)), cls)
    for _ in range(64):
        r, z = rng.randrange(1, R.N), rng.randrange(1, R.P)
        one(r, z, r, True, "x=r")
        one((r + 1) % R.P, z, r, False, "near miss")
        one(r, z, r - 1 if r > 1 else 2, False, "near miss")
        one(r, 0, r, False, "Z=0")
        small = rng.randrange(1, gap)
        one(small + R.N, z, small, True, "x=r+n, r<p-n")
        one(small, z, small, True, "x=r, r<p-n")
        one(small + R.N - 1, z, small, False, "near miss")
        big = rng.randrange(gap, R.N)
        one((big + R.N) % R.P, z, big, False, "x=r+n mod p, r>=p-n")
    one(gap - 1 + R.N, 1, gap - 1, True, "x=r+n, r<p-n")          # x = p - 1, the last r of the second clause
    one((gap + R.N) % R.P, 5, gap, False, "x=r+n mod p, r>=p-n")  # r = p - n: r + n = p, which is 0 in Fp
    one(0, 0, 1, False, "Z=0")


@functools.lru_cache(maxsize=None)
def build():
    """(records: (n, REC_WORDS) uint32 sorted by (op, modulus), expectations, class counts)."""
    rng = random.Random(SEED)
    cs = Cases()
    _field_cases(cs, rng)
    _point_cases(cs, rng)
    _xcmp_cases(cs, rng)
    order = sorted(range(len(cs.recs)), key=lambda i: (cs.recs[i][0], cs.recs[i][1]))
    recs = np.array([cs.recs[i] for i in order], dtype=np.uint32)
    return recs, [cs.expect[i] for i in order], cs.classes


def write_case_file(path):
    recs = build()[0]
    with open(path, "wb") as f:
        np.array([MAGIC_IN, recs.shape[0], REC_WORDS, 0], dtype="<u4").tofile(f)
        recs.astype("<u4").tofile(f)
    return recs.shape[0]


def assert_classes(classes):
    c = lambda *k: classes.get(k, 0)
    for mod in (0, 1):
        for cls in ("sum<m", "m<=sum<2^256", "sum>=2^256"):
            assert c("ADD", mod, cls) >= 200, ("ADD", mod, cls, c("ADD", mod, cls))
        assert c("SUB", mod, "borrow") >= 200 and c("SUB", mod, "equal") >= 50 and c("SUB", mod, "plain") >= 200
        for op in ("MUL", "SQR"):
            assert c(op, mod, "T<m") >= 200 and c(op, mod, "T>=2^256") >= 200, (op, mod)
            assert c(op, mod, "m<=T<2^256") >= 50, (op, mod, c(op, mod, "m<=T<2^256"))
        assert c("INV", mod, "zero") + c("INV", mod, "nonzero") >= 512
    assert c("DBL", 0, "point") >= 50 and c("DBL", 0, "identity") >= 1
    for op in ("ADD_MIXED", "ADD_FULL"):
        assert c(op, 0, "generic") >= 50
        for cls in ("equal", "opposite", "accumulator identity", "addend identity"):
            assert c(op, 0, cls) >= 20, (op, cls)
        assert c(op, 0, "both identity") >= 1
    for cls in ("x=r", "x=r+n, r<p-n", "x=r+n mod p, r>=p-n", "Z=0", "near miss"):
        assert c("XCMP", 0, cls) >= 20, cls


def check_results(got, label=""):
    """got: (n, OUT_WORDS) uint32, one result record per case of build().  Raises AssertionError naming the first mismatch."""
    recs, expect, _ = build()
    assert got.shape == (recs.shape[0], OUT_WORDS), "%s: result shape %s" % (label, got.shape)
    rinv = pow(W, -1, R.P)
    bad = []
    for i, (kind, want) in enumerate(expect):
        op, mod = int(recs[i, 0]), int(recs[i, 1])
        if int(got[i, OUT_WORDS - 1]) != (DONE | op):
            bad.append((i, "no result written"))
            continue
        if kind == "fe":
            have = unwords(got[i, :8])
            if have != want:
                bad.append((i, "got %x want %x" % (have, want)))
        elif kind == "flag":
            if int(got[i, 24]) != want:
                bad.append((i, "got %d want %d" % (int(got[i, 24]), want)))
        else:
            X, Y, Z = (unwords(got[i, 8 * k:8 * k + 8]) for k in range(3))
            if max(X, Y, Z) >= R.P:
                bad.append((i, "a coordinate is not reduced"))
                continue
            X, Y, Z = X * rinv % R.P, Y * rinv % R.P, Z * rinv % R.P
            if Z == 0:
                have = None
            else:
                zi = pow(Z, -1, R.P)
                have = (X * zi * zi % R.P, Y * zi * zi * zi % R.P)
            if have != want:
                bad.append((i, "got %s want %s" % (have, want)))
    if bad:
        i, why = bad[0]
        per_op = {}
        for j, _ in bad:
            k = "%s/%s" % (OP_NAMES[int(recs[j, 0])], "n" if recs[j, 1] else "p")
            per_op[k] = per_op.get(k, 0) + 1
        raise AssertionError("%s: %d mismatches, by op %s.  First: case %d op %s modulus %s: %s\n  operands %s" % (
            label, len(bad), per_op, i, OP_NAMES[int(recs[i, 0])], "n" if recs[i, 1] else "p", why,
            [hex(int(w)) for w in recs[i, OPND:]]))
