"""Cases and expected results of csrc/pairing.h's tower, Frobenius map, line product, Miller loop, final exponentiation and whole
check, for tests/pairing_device_check.hip (one case per lane on the device, or the same code on the CPU under --host).  Every
expected word comes from tests/pairing_ref.py's Python integers; all comparisons are exact, limb for limb on the Montgomery
images.  build() makes the set once per session; measured: about 7 s on one CPU core.

Case file (32-bit little-endian words): MAGIC_IN, n, REC_WORDS, n_tables; n records sorted by op; the n words of the second
pass's order; n_tables x 64 words, the raw images of g2 then s_g2.  A record: [0] op  [1] aux  [2] table  [3] 0  [4 ..) a (an Fq12,
smaller operands from its start)  [100 ..) b  [196 ..) p0  [212 ..) p1 (G1 rows).  A result: [0 .. 96) an Fq12 (smaller results
from its start, the rest zero)  [96] a flag  [97] DONE | op.  The layouts are those of tests/pairing_check_ops.h.

Tables: 0 (G2, [T] G2)  1 ([v] G2, [t v] G2)  2 (G2, G2)  3 (G2, O): inf[0] set  4 (O, [T] G2): inf[1] set.  No public entry point
makes the last two: the harness calls pairing_table_make itself.

The second pass's order puts different ops into consecutive lanes, gives every wave of 64 a CHECK lane that returns early (RANGE
or OFF_CURVE) and a CHECK lane that runs a whole VALID check, and leaves no case at the place it has in the first pass.
"""
import functools
import os
import random
import shutil
import subprocess

import numpy as np

import pairing_cases as pc
import pairing_ref as R
from zkoracle import curve, field as F

P = R.P
MAGIC_IN, MAGIC_OUT, MAGIC_TAB = 0x43524150, 0x52524150, 0x54524150
F12_WORDS, OPND = 96, 4
REC_WORDS, OUT_WORDS, DONE = OPND + 2 * F12_WORDS + 32, F12_WORDS + 2, 0x600D0000
OFF_A, OFF_B, OFF_P0, OFF_P1 = OPND, OPND + F12_WORDS, OPND + 2 * F12_WORDS, OPND + 2 * F12_WORDS + 16
F2_MUL, F2_MUL_XI, F2_MUL_FQ, F2_INV = 1, 2, 3, 4
F6_MUL, F6_MUL_01, F6_MUL_V, F6_INV = 10, 11, 12, 13
F12_MUL, F12_SQR, F12_INV, F12_CONJ, F12_FROB, F12_MUL_LINE, F12_POW_U, F12_IS_ONE = 20, 21, 22, 23, 24, 25, 26, 27
FQ_CANON, MILLER, FEXP, CHECK = 40, 41, 42, 43
OP_NAMES = {F2_MUL: "F2_MUL", F2_MUL_XI: "F2_MUL_XI", F2_MUL_FQ: "F2_MUL_FQ", F2_INV: "F2_INV", F6_MUL: "F6_MUL", F6_MUL_01: "F6_MUL_01",
            F6_MUL_V: "F6_MUL_V", F6_INV: "F6_INV", F12_MUL: "F12_MUL", F12_SQR: "F12_SQR", F12_INV: "F12_INV", F12_CONJ: "F12_CONJ",
            F12_FROB: "F12_FROB", F12_MUL_LINE: "F12_MUL_LINE", F12_POW_U: "F12_POW_U", F12_IS_ONE: "F12_IS_ONE", FQ_CANON: "FQ_CANON",
            MILLER: "MILLER", FEXP: "FEXP", CHECK: "CHECK"}
TOWER_OPS = ("F2_MUL", "F2_MUL_XI", "F2_MUL_FQ", "F2_INV", "F6_MUL", "F6_MUL_01", "F6_MUL_V", "F6_INV", "F12_MUL", "F12_SQR", "F12_INV",
             "F12_CONJ", "F12_FROB", "F12_MUL_LINE")
WAVE = 64
SEED = 0x424E3235342D3132
T = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % F.R
V1, T1 = 0xABCDEF123456789, F.R - 3
# (g2 scalar, s_g2 scalar) of each table, 0 for the identity; RATIO: the t with s_g2 = [t] g2 where both are points
TABLE_SCALARS = ((1, T), (V1, T1 * V1 % F.R), (1, 1), (1, 0), (0, T))
RATIO = (T, T1, 1)

# the canonical value whose Montgomery image has all-ones low words (the top word one below p's)
ALL_ONES = R.unmont((((P >> 224) - 1) << 224) | ((1 << 224) - 1))
SPECIAL = (0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, R.W256 % P, ALL_ONES)
assert R.to_words(R.mont(ALL_ONES))[:7] == [0xFFFFFFFF] * 7

Z2, ONE2 = R.F2_ZERO, R.F2_ONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]  # build.sh's


def binary():
    """build.sh makes it; a missing one is built here when hipcc is on the path.  Neither: fail."""
    exe = os.path.join(HERE, "pairing_device_check")
    if os.path.isfile(exe):
        return exe
    hipcc = shutil.which("hipcc")
    assert hipcc, "%s is missing (build.sh makes it) and there is no hipcc on the path to build it" % exe
    subprocess.check_call([hipcc] + FLAGS + ["-I", os.path.join(ROOT, "webauthn-halo2_amd", "csrc"), os.path.join(HERE, "pairing_device_check.hip"), "-o", exe])
    return exe


# ---- operands ----------------------------------------------------------------------------------------------------------------
def fq_pick(rng):
    return SPECIAL[rng.randrange(len(SPECIAL))] if rng.randrange(4) == 0 else rng.randrange(P)


def f2_rand(rng):
    return (rng.randrange(P), rng.randrange(P))


def f2_mixed(rng):
    return (fq_pick(rng), fq_pick(rng))


def f6_rand(rng):
    return tuple(f2_rand(rng) for _ in range(3))


def f12_rand(rng):
    return tuple(f2_rand(rng) for _ in range(6))


def of_fq_coeffs(cs):
    """Fq coefficients in MEMORY order (c0 first, each Fq2 as c0, c1) -> an element of Fq2 (2), Fq6 (6) or Fq12 (12)"""
    f2s = tuple((cs[2 * i], cs[2 * i + 1]) for i in range(len(cs) // 2))
    if len(f2s) == 1:
        return f2s[0]
    if len(f2s) == 3:
        return f2s
    return tuple(f2s[R.F12_ORDER.index(i)] for i in range(6))


def cyclotomic(rng):
    """the easy part of the final exponentiation of a random element: conj is its inverse"""
    f = f12_rand(rng)
    t = R.f12_mul(R.f12_conj(f), R.f12_inv(f))
    t = R.f12_mul(R.frobenius(R.frobenius(t)), t)
    assert R.f12_mul(t, R.f12_conj(t)) == R.F12_ONE
    return t


def fq_sqrt(a):
    s = pow(a, (P + 1) // 4, P)
    return s if s * s % P == a % P else None


def f2_of_norm(rng, n):
    """a random Fq2 element with a0^2 + a1^2 = n"""
    while True:
        a0 = rng.randrange(1, P)
        a1 = fq_sqrt((n - a0 * a0) % P)
        if a1:
            return (a0, a1 if rng.randrange(2) else P - a1)


def common_operands(rng, level, n_random, n_special):
    """(class, element) at level 2, 6 or 12: every coefficient position alone, the subfields, one, -1, zero, special and random
    coefficients"""
    out = []
    for k in range(level):
        for val in (1, P - 1, rng.randrange(2, P)):
            out.append(("position %d" % k, of_fq_coeffs([val if i == k else 0 for i in range(level)])))
    one = of_fq_coeffs([1] + [0] * (level - 1))
    out += [("one", one), ("minus one", of_fq_coeffs([P - 1] + [0] * (level - 1))), ("zero", of_fq_coeffs([0] * level))]
    for _ in range(4):
        out.append(("in Fq", of_fq_coeffs([rng.randrange(1, P)] + [0] * (level - 1))))
        if level > 2:
            out.append(("in Fq2", of_fq_coeffs(list(f2_rand(rng)) + [0] * (level - 2))))
        if level == 12:
            out.append(("in Fq6", R.f12_of_halves(f6_rand(rng), R.F6_ZERO)))
            out.append(("pure w", R.f12_of_halves(R.F6_ZERO, f6_rand(rng))))
    for _ in range(n_special):
        out.append(("special", of_fq_coeffs([fq_pick(rng) for _ in range(level)])))
    for _ in range(n_random):
        out.append(("random", of_fq_coeffs([rng.randrange(P) for _ in range(level)])))
    return out


def f2_cancel(rng):
    a0 = rng.randrange(1, P)
    return (a0, P - a0)  # a0 + a1 = 0: the Karatsuba sum of f2_mul


def f6_cancel(rng, which):
    """c_i + c_j = 0 for the named pair of positions"""
    c = list(f6_rand(rng))
    i, j = {"c0+c1=0": (0, 1), "c1+c2=0": (1, 2), "c0+c2=0": (0, 2)}[which]
    c[j] = R.f2_neg(c[i])
    return tuple(c)


def f12_cancel(rng, which):
    c1 = f6_rand(rng)
    c0 = R.f6_neg(c1) if which == "c0+c1=0" else R.f6_neg(R.f6_mul_v(c1))
    return R.f12_of_halves(c0, c1)





class Cases:
    def __init__(self):
        self.recs, self.expect, self.kind, self.classes = [], [], [], {}

    def add(self, op, cls, a=(), b=(), p0=(), p1=(), aux=0, table=0, value=(), flag=0, kind=None):
        """a, b, p0, p1, value: word lists.  kind: for CHECK, 'early' / 'valid' / 'mismatch' (the second pass's order needs it)"""
        assert len(a) <= F12_WORDS and len(b) <= F12_WORDS and len(p0) in (0, 16) and len(p1) in (0, 16) and len(value) <= F12_WORDS
        pad = lambda ws, n: list(ws) + [0] * (n - len(ws))
        self.recs.append([op, aux, table, 0] + pad(a, F12_WORDS) + pad(b, F12_WORDS) + pad(p0, 16) + pad(p1, 16))
        self.expect.append(pad(value, F12_WORDS) + [flag, DONE | op])
        self.kind.append(kind)
        key = (OP_NAMES[op], cls)
        self.classes[key] = self.classes.get(key, 0) + 1


# ---- tower cases -------------------------------------------------------------------------------------------------------------
def _f2_cases(cs, rng):
    w = R.f2_words
    ops = common_operands(rng, 2, 90, 90)
    grid = [(x, y) for x in SPECIAL for y in SPECIAL]
    pairs = [(c, a, f2_mixed(rng)) for c, a in ops] + [(c, f2_mixed(rng), a) for c, a in ops[:40]]
    pairs += [("a0+a1=0", f2_cancel(rng), f2_rand(rng)) for _ in range(8)] + [("a0+a1=0", f2_rand(rng), f2_cancel(rng)) for _ in range(8)]
    pairs += [("a0+a1=0", f2_cancel(rng), f2_cancel(rng)) for _ in range(4)]
    for _ in range(8):
        a = f2_rand(rng)
        pairs += [("b=inverse", a, R.f2_inv(a)), ("b=a", a, a)]
    pairs += [("special", grid[i], grid[(7 * i + 3) % len(grid)]) for i in range(len(grid))]
    for c, a, b in pairs:
        cs.add(F2_MUL, c, w(a), w(b), value=w(R.f2_mul(a, b)))
    xi_ops = [("p-1 in c0", (P - 1, v)) for v in SPECIAL + (rng.randrange(P),)] + [("p-1 in c1", (v, P - 1)) for v in SPECIAL + (rng.randrange(P),)]
    for c, a in xi_ops + [("special", g) for g in grid] + ops:
        cs.add(F2_MUL_XI, c, w(a), value=w(R.f2_mul(a, R.XI)))
    for c, a in [("special", g) for g in grid] + ops:
        s = fq_pick(rng)
        cs.add(F2_MUL_FQ, c, w(a), R.fq_words(s), value=w(R.f2_mul_fq(a, s)))
    for s in SPECIAL:
        a = f2_rand(rng)
        cs.add(F2_MUL_FQ, "special scalar", w(a), R.fq_words(s), value=w(R.f2_mul_fq(a, s)))
    inv_ops = [("a0=0", (0, v)) for v in SPECIAL[1:] + (rng.randrange(1, P),)] + [("a1=0", (v, 0)) for v in SPECIAL[1:] + (rng.randrange(1, P),)]
    inv_ops += [("norm 1", f2_of_norm(rng, 1)) for _ in range(6)] + [("norm p-1", f2_of_norm(rng, P - 1)) for _ in range(6)]
    for c, a in inv_ops + [("special", g) for g in grid] + ops:
        if c.startswith("norm"):
            assert R.f2_norm(a) == (1 if c == "norm 1" else P - 1)
        cs.add(F2_INV, c, w(a), value=w(R.f2_inv(a)))


def _f6_cases(cs, rng):
    w = R.f6_words
    ops = common_operands(rng, 6, 120, 120)
    kinds = ("c0+c1=0", "c1+c2=0", "c0+c2=0")
    pairs = [(c, a, of_fq_coeffs([fq_pick(rng) for _ in range(6)])) for c, a in ops] + [(c, f6_rand(rng), a) for c, a in ops[:40]]
    for k in kinds:
        pairs += [(k, f6_cancel(rng, k), f6_rand(rng)) for _ in range(4)] + [(k, f6_rand(rng), f6_cancel(rng, k)) for _ in range(4)]
        pairs += [(k, f6_cancel(rng, k), f6_cancel(rng, k)) for _ in range(2)]
    for _ in range(8):
        a = f6_rand(rng)
        pairs += [("b=inverse", a, R.f6_inv(a)), ("b=a", a, a)]
    for c, a, b in pairs:
        cs.add(F6_MUL, c, w(a), w(b), value=w(R.f6_mul(a, b)))
    m01 = [(c, a, f2_mixed(rng), f2_mixed(rng)) for c, a in ops]
    for k in kinds:
        m01 += [(k, f6_cancel(rng, k), f2_rand(rng), f2_rand(rng)) for _ in range(6)]
    for _ in range(8):
        b0 = f2_rand(rng)
        m01.append(("b0+b1=0", f6_rand(rng), b0, R.f2_neg(b0)))
        m01.append(("b0+b1=0", f6_cancel(rng, "c0+c1=0"), b0, R.f2_neg(b0)))
    m01 += [("b0=0", f6_rand(rng), Z2, f2_rand(rng)) for _ in range(4)] + [("b1=0", f6_rand(rng), f2_rand(rng), Z2) for _ in range(4)]
    for c, a, b0, b1 in m01:
        cs.add(F6_MUL_01, c, w(a), R.f2_words(b0) + R.f2_words(b1), value=w(R.f6_mul(a, (b0, b1, Z2))))
    v = (Z2, ONE2, Z2)
    for c, a in ops + [("p-1 in c2", (f2_rand(rng), f2_rand(rng), (P - 1, P - 1)))]:
        cs.add(F6_MUL_V, c, w(a), value=w(R.f6_mul(a, v)))
    for c, a in ops + [(k, f6_cancel(rng, k)) for k in kinds]:
        cs.add(F6_INV, c, w(a), value=w(R.f6_inv(a)))


def _f12_cases(cs, rng):
    w = R.f12_words
    ops = common_operands(rng, 12, 100, 100)
    kinds = ("c0+c1=0", "c0+v*c1=0")
    cancels = [(k, f12_cancel(rng, k)) for k in kinds for _ in range(6)]
    pairs = [(c, a, of_fq_coeffs([fq_pick(rng) for _ in range(12)])) for c, a in ops] + [(c, f12_rand(rng), a) for c, a in ops[:48]]
    pairs += [(k, a, f12_rand(rng)) for k, a in cancels] + [(k, f12_rand(rng), a) for k, a in cancels[::2]]
    pairs += [(k, f12_cancel(rng, k), f12_cancel(rng, k)) for k in kinds for _ in range(2)]
    same = []
    for _ in range(8):
        a = f12_rand(rng)
        pairs.append(("b=inverse", a, R.f12_inv(a)))
        same.append(a)
        cy = cyclotomic(rng)
        pairs.append(("b=conj(a), a cyclotomic", cy, R.f12_conj(cy)))
    for c, a, b in pairs:
        cs.add(F12_MUL, c, w(a), w(b), value=w(R.f12_mul(a, b)))
    for a in same:  # F12_MUL of (a, a) and F12_SQR of a: the same expected words
        sq = w(R.f12_mul(a, a))
        cs.add(F12_MUL, "b=a", w(a), w(a), value=sq)
        cs.add(F12_SQR, "b=a of F12_MUL", w(a), value=sq)
    cyc = [("cyclotomic", cyclotomic(rng)) for _ in range(6)]
    for c, a in ops + cancels + cyc:
        cs.add(F12_SQR, c, w(a), value=w(R.f12_mul(a, a)))
        cs.add(F12_CONJ, c, w(a), value=w(R.f12_conj(a)))
    for c, a in ops + cancels + cyc:
        cs.add(F12_INV, c, w(a), value=w(R.f12_inv(a)))
    for i, (c, a) in enumerate(ops + cancels + cyc):
        cs.add(F12_FROB, c, w(a), table=i % len(TABLE_SCALARS), value=w(R.frobenius(a)))  # (every table holds the same gamma)
    # is_one: one, and one with each single coefficient off by one
    cs.add(F12_IS_ONE, "one", w(R.F12_ONE), flag=1)
    for k in range(12):
        cs.add(F12_IS_ONE, "off by one at %d" % k, w(of_fq_coeffs([(1 if i == 0 else 0) + (1 if i == k else 0) for i in range(12)])), flag=0)
    for c, a in (("zero", R.F12_ZERO), ("minus one", R.f12_neg(R.F12_ONE)), ("random", f12_rand(rng)), ("in Fq", of_fq_coeffs([2] + [0] * 11))):
        cs.add(F12_IS_ONE, c, w(a), flag=0)
    # pow_u
    pw = [("one", R.F12_ONE), ("minus one", R.f12_neg(R.F12_ONE))] + [("random", f12_rand(rng)) for _ in range(30)]
    pw += [("cyclotomic", cyclotomic(rng)) for _ in range(32)]
    for c, a in pw:
        cs.add(F12_POW_U, c, w(a), value=w(R.f12_pow(a, R.U)))


def _canon_cases(cs, rng):
    for c, img, want in (("p-1", P - 1, 1), ("p", P, 0), ("p+1", P + 1, 0), ("2^256-1", R.W256 - 1, 0), ("zero", 0, 1),
                         ("top word below", P - (1 << 224), 1), ("top word above", P + (1 << 224), 0), ("bottom word below", P - 5, 1),
                         ("bottom word above", P + 5, 0), ("middle word below", P - (1 << 96), 1), ("middle word above", P + (1 << 96), 0)):
        cs.add(FQ_CANON, c, R.to_words(img), flag=want)
    for _ in range(8):
        lo, hi = rng.randrange(P), rng.randrange(P, R.W256)
        cs.add(FQ_CANON, "random below", R.to_words(lo), flag=1)
        cs.add(FQ_CANON, "random above", R.to_words(hi), flag=0)


def addition_steps():
    """the walk's step kinds in order: 'dbl', 'add', then the two 'frob'"""
    kinds = []
    for b in range(63, -1, -1):
        kinds.append("dbl")
        if (R.SIX_U_PLUS_2 >> b) & 1:
            kinds.append("add")
    return kinds + ["frob", "frob"]


def _line_cases(cs, rng, tables):
    kinds = addition_steps()
    assert len(kinds) == R.STEPS
    mid = next(i for i in range(10, R.STEPS) if kinds[i] == "dbl" and kinds[i + 1] == "add")
    steps = [(0, "first step"), (mid, "doubling before an addition"), (mid + 1, "addition after a doubling"), (R.STEPS - 3, "last loop step"),
             (R.STEPS - 2, "Frobenius step 1"), (R.STEPS - 1, "Frobenius step 2")]
    pts = [curve.G1_GEN, pc.g1(F.R - 1), pc.g1(rng.randrange(2, F.R)), pc.g1(rng.randrange(2, F.R))]
    for ti in (0, 1):
        for walk in (0, 1):
            for step, cls in steps:
                fs = [("f one", R.F12_ONE)]
                fs += [("f sparse", of_fq_coeffs([rng.randrange(1, P) if i == k else 0 for i in range(12)])) for k in rng.sample(range(12), 4)]
                fs += [("f sparse", R.f12_of_halves(f6_rand(rng), R.F6_ZERO)), ("f sparse", R.f12_of_halves(R.F6_ZERO, f6_rand(rng)))]
                fs += [("f random", f12_rand(rng)) for _ in range(4)]
                for j, (fc, f) in enumerate(fs):
                    pt = pts[(j + step) % len(pts)]
                    want = R.f12_mul(f, R.line_value(tables[ti]["walks"][walk][step], pt))
                    cs.add(F12_MUL_LINE, cls, R.f12_words(f), p0=R.g1_words(pt), aux=(walk << 8) | step, table=ti, value=R.f12_words(want))
                    cs.classes[("F12_MUL_LINE", fc)] = cs.classes.get(("F12_MUL_LINE", fc), 0) + 1


# ---- Miller loop, final exponentiation, whole checks -----------------------------------------------------------------------------
def _pair_cases(cs, rng, tables):
    @functools.lru_cache(maxsize=None)
    def miller(p0, p1, ti):
        return R.miller(p0, p1, tables[ti]["walks"][0], tables[ti]["walks"][1])

    holding, failing = [], []  # Miller values, for FEXP
    for ti in range(len(TABLE_SCALARS)):
        t = RATIO[ti] if ti < 3 else T
        xs = [rng.randrange(2, F.R) for _ in range(3)]
        rows = [("holding pair" if ti < 3 else "table with an identity", x, x * t) for x in xs]
        rows += [("non-holding pair" if ti < 3 else "table with an identity", x, rng.randrange(1, F.R)) for x in xs]
        rows += [("p0 identity", 0, rng.randrange(1, F.R)) for _ in range(2)] + [("p1 identity", rng.randrange(1, F.R), 0) for _ in range(2)]
        rows += [("both identities", 0, 0), ("x=1", 1, t), ("x=r-1", F.R - 1, (F.R - 1) * t)]
        for cls, x, y in rows:
            p0, p1 = pc.g1(x), R.g1_neg(pc.g1(y))
            val = miller(p0, p1, ti)
            if cls == "both identities":
                assert val == R.F12_ONE
            cs.add(MILLER, cls, p0=R.g1_words(p0), p1=R.g1_words(p1), table=ti, value=R.f12_words(val))
            if ti < 3 and x and y:
                (holding if pc.holds(x, y, t) else failing).append(val)
    assert len(holding) >= 12 and len(failing) >= 8
    fe = [("Miller value of a holding pair", v) for v in holding[:16]] + [("Miller value of a non-holding pair", v) for v in failing[:12]]
    fe += [("random", f12_rand(rng)) for _ in range(24)] + [("c1=0", R.f12_of_halves(f6_rand(rng), R.F6_ZERO)) for _ in range(10)]
    fe += [("one", R.F12_ONE), ("minus one", R.f12_neg(R.F12_ONE)), ("zero", R.F12_ZERO), ("pure w", R.f12_of_halves(R.F6_ZERO, f6_rand(rng)))]
    fe += [("cyclotomic", cyclotomic(rng)) for _ in range(4)]
    for i, (cls, a) in enumerate(fe):
        val = R.final_exponentiation(a)
        if cls in ("Miller value of a holding pair", "c1=0", "one", "minus one"):
            assert val == R.F12_ONE, cls
        if cls == "Miller value of a non-holding pair":
            assert val != R.F12_ONE
        cs.add(FEXP, cls, R.f12_words(a), table=i % len(TABLE_SCALARS), value=R.f12_words(val))

    # whole checks: the reason comes from the reference's check() on the very words of the record
    def chk(cls, a_words, b_words, ti, expect_reason=None):
        reason = R.check(a_words, b_words, tables[ti])
        if expect_reason is not None:
            assert reason == expect_reason, (cls, reason)
        kind = "early" if reason in (R.RANGE, R.OFF_CURVE) else ("valid" if reason == R.VALID else "mismatch")
        cs.add(CHECK, cls, p0=a_words, p1=b_words, table=ti, flag=reason, kind=kind)
        cs.classes[("CHECK", "reason %d" % reason)] = cs.classes.get(("CHECK", "reason %d" % reason), 0) + 1

    g = lambda x: R.g1_words(pc.g1(x))
    for i in range(78):  # VALID: holding pairs on the three full tables
        ti = i % 3
        x = (1, F.R - 1)[i // 3] if i < 6 else rng.randrange(2, F.R)
        chk("holding pair", g(x), g(x * RATIO[ti]), ti, R.VALID)
    zero = [0] * 16
    for ti in range(5):
        chk("both identities", zero, zero, ti, R.VALID)
    chk("s_g2 identity, b identity", g(5), zero, 3, R.VALID)   # e(a, O) e(O, g2) = 1
    chk("g2 identity, a identity", zero, g(5), 4, R.VALID)     # e(O, s_g2) e(-b, O) = 1
    for i in range(18):
        ti = i % 3
        x = rng.randrange(2, F.R)
        y = (F.R - x * RATIO[ti]) % F.R if i % 2 else rng.randrange(1, F.R)  # -(correct b), or an unrelated point
        chk("non-holding pair", g(x), g(y), ti, R.MISMATCH)
    ga, gb = g(3), g(21)  # test_gpu_pairing.py's test_reasons, against s_g2 = [7] G2's place taken by table 0
    chk("a identity", zero, gb, 0, R.MISMATCH)
    chk("b identity", ga, zero, 0, R.MISMATCH)
    chk("b=a", ga, ga, 0, R.MISMATCH)
    chk("s_g2 identity, b a point", ga, gb, 3, R.MISMATCH)
    chk("g2 identity, a a point", ga, gb, 4, R.MISMATCH)
    one_one = R.fq_words(1) + R.fq_words(1)

    def with_image(words, col, img):
        out = list(words)
        out[col:col + 8] = R.to_words(img)
        return out

    def plus_p(words, col):
        return with_image(words, col, R.from_words(words[col:col + 8]) + P)

    early = []
    for i in range(12):
        a, b, ti = g(rng.randrange(2, F.R)), g(rng.randrange(2, F.R)), i % 5
        early += [("a.x = p", with_image(a, 0, P), b, ti, R.RANGE), ("b.y + p", a, plus_p(b, 8), ti, R.RANGE),
                  ("a off the curve", one_one, b, ti, R.OFF_CURVE), ("b off the curve", a, one_one, ti, R.OFF_CURVE),
                  ("RANGE before OFF_CURVE", one_one, plus_p(b, 0), ti, R.RANGE), ("a.y = 2^256-1", with_image(a, 8, R.W256 - 1), b, ti, R.RANGE),
                  ("y off by one", a, with_image(b, 8, (R.from_words(b[8:]) + 1) % P), ti, R.OFF_CURVE)]
    early += [("x = 0, y = 1", R.fq_words(0) + R.fq_words(1), gb, 0, R.OFF_CURVE), ("x = 1, y = 0", ga, R.fq_words(1) + R.fq_words(0), 0, R.OFF_CURVE)]
    for cls, a, b, ti, want in early:
        chk(cls, a, b, ti, want)


# ---- the set -----------------------------------------------------------------------------------------------------------------
def second_pass_order(ops, kinds):
    """the order of the interleaved pass (position -> case): every wave of 64 gets one early-returning and one VALID CHECK case,
    the other places are dealt in proportion over the ops; within a wave the lanes go round the ops; no case keeps its place."""
    n = len(ops)
    waves = (n + WAVE - 1) // WAVE
    early = [i for i in range(n) if kinds[i] == "early"]
    valid = [i for i in range(n) if kinds[i] == "valid"]
    assert len(early) >= waves and len(valid) >= waves, (len(early), len(valid), waves)
    reserved = set(early[:waves]) | set(valid[:waves])
    size, rank, key = {}, {}, {}
    for i in range(n):
        if i not in reserved:
            rank[i] = size.get(ops[i], 0)
            size[ops[i]] = rank[i] + 1
    rest = sorted((i for i in range(n) if i not in reserved), key=lambda i: ((rank[i] + 0.5) / size[ops[i]], ops[i]))
    order, at = [], 0
    for w in range(waves):
        room = min(WAVE, n - WAVE * w) - 2
        members = [early[w], valid[w]] + rest[at:at + room]
        at += room
        by_op = {}
        for i in members:
            by_op.setdefault(ops[i], []).append(i)
        lanes = []
        while any(by_op.values()):
            for op in sorted(by_op):
                if by_op[op] and (not lanes or ops[lanes[-1]] != op or sum(1 for q in by_op.values() if q) == 1):
                    lanes.append(by_op[op].pop())
        # the two CHECK lanes apart from each other, and nobody at the place of the first pass
        for shift in range(len(lanes)):
            cand = lanes[shift:] + lanes[:shift]
            if all(WAVE * w + j != i for j, i in enumerate(cand)) and all(ops[cand[j]] != ops[cand[j + 1]] for j in range(len(cand) - 1)):
                lanes = cand
                break
        else:
            raise AssertionError("no arrangement of wave %d" % w)
        order += lanes
    assert at == len(rest) and sorted(order) == list(range(n))
    return order


@functools.lru_cache(maxsize=None)
def build():
    """a dict: recs (n, REC_WORDS) uint32 sorted by op, expect (n, OUT_WORDS) uint32, classes, order (n,) uint32: the second
    pass, kinds, tables_raw (n_tables, 64) uint32, tables: the reference's walks"""
    rng = random.Random(SEED)
    points = [(pc.g2(a), pc.g2(b)) for a, b in TABLE_SCALARS]
    tables = [R.make_table(g2, s_g2) for g2, s_g2 in points]
    cs = Cases()
    _f2_cases(cs, rng)
    _f6_cases(cs, rng)
    _f12_cases(cs, rng)
    _canon_cases(cs, rng)
    _line_cases(cs, rng, tables)
    _pair_cases(cs, rng, tables)
    idx = sorted(range(len(cs.recs)), key=lambda i: cs.recs[i][0])
    recs = np.array([cs.recs[i] for i in idx], dtype=np.uint32)
    expect = np.array([cs.expect[i] for i in idx], dtype=np.uint32)
    kinds = [cs.kind[i] for i in idx]
    order = np.array(second_pass_order([int(o) for o in recs[:, 0]], kinds), dtype=np.uint32)
    raw = np.array([[int(w) & 0xFFFFFFFF if h == 0 else int(w) >> 32 for w in list(pc.g2_to_words(g2)) + list(pc.g2_to_words(s_g2)) for h in (0, 1)]
                    for g2, s_g2 in points], dtype=np.uint32)
    return {"recs": recs, "expect": expect, "classes": cs.classes, "order": order, "kinds": kinds, "tables_raw": raw, "tables": tables}


def write_case_file(path):
    s = build()
    with open(path, "wb") as f:
        np.array([MAGIC_IN, s["recs"].shape[0], REC_WORDS, s["tables_raw"].shape[0]], dtype="<u4").tofile(f)
        s["recs"].astype("<u4").tofile(f)
        s["order"].astype("<u4").tofile(f)
        s["tables_raw"].astype("<u4").tofile(f)
    return s["recs"].shape[0]


def read_results(path, passes):
    n = build()["recs"].shape[0]
    raw = np.fromfile(path, dtype="<u4")
    assert raw[:4].tolist() == [MAGIC_OUT, n, OUT_WORDS, passes] and raw.size == 4 + passes * n * OUT_WORDS, "result file malformed"
    return raw[4:].reshape(passes, n, OUT_WORDS)


def expected_table_words(ti):
    """the words of table ti as pairing_table_make lays it out: 6 gamma, inf[8], then line[2][102] of (lambda, c)"""
    t = build()["tables"][ti]
    out = [w for g in R.GAMMA for w in R.f2_words(g)]
    out += [int(t["walks"][0] is None), int(t["walks"][1] is None), 0, 0, 0, 0, 0, 0]
    for walk in t["walks"]:
        for step in range(R.STEPS):
            out += [0] * 32 if walk is None else R.f2_words(walk[step][0]) + R.f2_words(walk[step][1])
    return out


def check_tables(path):
    """the harness's dump of the tables it made against the reference's walks: 6 gamma, the two identity flags, 2 x 102 lines"""
    n_tables = len(TABLE_SCALARS)
    per = 6 * 16 + 8 + 2 * R.STEPS * 32
    raw = np.fromfile(path, dtype="<u4")
    assert raw[:4].tolist() == [MAGIC_TAB, n_tables, per, 0] and raw.size == 4 + n_tables * per, "table file malformed"
    got = raw[4:].reshape(n_tables, per)
    for ti in range(n_tables):
        want = np.array(expected_table_words(ti), dtype=np.uint32)
        bad = np.nonzero(got[ti] != want)[0]
        if bad.size:
            k = int(bad[0])
            where = "gamma[%d]" % (k // 16) if k < 96 else ("inf[%d]" % (k - 96) if k < 104 else "line[%d][%d] %s" % (
                (k - 104) // (R.STEPS * 32), (k - 104) // 32 % R.STEPS, "lambda" if (k - 104) % 32 < 16 else "c"))
            raise AssertionError("table %d: %d words differ from the reference's walk, first at word %d (%s): got %08x want %08x" % (
                ti, bad.size, k, where, int(got[ti][k]), int(want[k])))


def assert_classes(s=None):
    """the class counts the set promises, from the generator's own bookkeeping and the records"""
    s = s or build()
    classes, recs, order, kinds = s["classes"], s["recs"], s["order"], s["kinds"]
    c = lambda *k: classes.get(k, 0)
    per_op = {}
    for op in recs[:, 0]:
        per_op[OP_NAMES[int(op)]] = per_op.get(OP_NAMES[int(op)], 0) + 1
    for op in TOWER_OPS:
        assert per_op[op] >= 256, (op, per_op[op])
    assert per_op["F12_POW_U"] >= 64 and per_op["MILLER"] >= 64 and per_op["FEXP"] >= 64 and per_op["CHECK"] >= 128, per_op
    levels = {2: ("F2_MUL", "F2_MUL_XI", "F2_MUL_FQ", "F2_INV"), 6: ("F6_MUL", "F6_MUL_01", "F6_MUL_V", "F6_INV"),
              12: ("F12_MUL", "F12_SQR", "F12_INV", "F12_CONJ", "F12_FROB")}
    for level, ops in levels.items():
        for op in ops:
            for k in range(level):
                assert c(op, "position %d" % k) >= 3, (op, k)
            for cls in ("one", "minus one", "zero", "in Fq") + (("in Fq2",) if level > 2 else ()) + (("in Fq6", "pure w") if level == 12 else ()):
                assert c(op, cls) >= 1, (op, cls)
            assert c(op, "special") >= 60 and c(op, "random") >= 60, op
    assert c("F2_MUL", "a0+a1=0") >= 16 and c("F2_MUL", "b=inverse") >= 8 and c("F2_MUL", "b=a") >= 8
    for cls in ("a0=0", "a1=0", "norm 1", "norm p-1", "zero"):
        assert c("F2_INV", cls) >= 1, cls
    assert c("F2_MUL_XI", "p-1 in c0") >= 9 and c("F2_MUL_XI", "p-1 in c1") >= 9
    for cls in ("c0+c1=0", "c1+c2=0", "c0+c2=0"):
        assert c("F6_MUL", cls) >= 8 and c("F6_MUL_01", cls) >= 6, cls
    assert c("F6_MUL_01", "b0+b1=0") >= 8 and c("F6_MUL", "b=inverse") >= 8 and c("F6_MUL", "b=a") >= 8 and c("F6_INV", "zero") >= 1
    for cls in ("c0+c1=0", "c0+v*c1=0"):
        assert c("F12_MUL", cls) >= 8 and c("F12_SQR", cls) >= 6, cls
    assert c("F12_MUL", "b=inverse") >= 8 and c("F12_MUL", "b=a") >= 8 and c("F12_SQR", "b=a of F12_MUL") >= 8
    assert c("F12_MUL", "b=conj(a), a cyclotomic") >= 8 and c("F12_INV", "zero") >= 1
    assert c("F12_IS_ONE", "one") == 1 and all(c("F12_IS_ONE", "off by one at %d" % k) == 1 for k in range(12))
    for cls in ("p-1", "p", "p+1", "2^256-1", "zero", "top word below", "top word above", "bottom word below", "bottom word above"):
        assert c("FQ_CANON", cls) == 1, cls
    for cls in ("first step", "doubling before an addition", "addition after a doubling", "last loop step", "Frobenius step 1", "Frobenius step 2"):
        assert c("F12_MUL_LINE", cls) >= 40, cls
    assert c("F12_MUL_LINE", "f one") >= 24 and c("F12_MUL_LINE", "f sparse") >= 100 and c("F12_MUL_LINE", "f random") >= 90
    line = recs[recs[:, 0] == F12_MUL_LINE]
    assert {(int(r[2]), int(r[1]) >> 8) for r in line} == {(0, 0), (0, 1), (1, 0), (1, 1)}  # both walks of two tables
    for cls in ("one", "minus one", "random", "cyclotomic"):
        assert c("F12_POW_U", cls) >= 1, cls
    for cls in ("holding pair", "non-holding pair", "table with an identity", "p0 identity", "p1 identity", "both identities", "x=1", "x=r-1"):
        assert c("MILLER", cls) >= 5, cls
    assert {int(r[2]) for r in recs[recs[:, 0] == MILLER]} == set(range(5))
    for cls in ("Miller value of a holding pair", "Miller value of a non-holding pair", "random", "c1=0", "one"):
        assert c("FEXP", cls) >= 1, cls
    assert c("FEXP", "Miller value of a holding pair") >= 12 and c("FEXP", "random") >= 16 and c("FEXP", "c1=0") >= 8
    for reason in range(4):
        assert c("CHECK", "reason %d" % reason) >= 20, reason
    for cls in ("RANGE before OFF_CURVE", "both identities", "a identity", "b identity", "b=a", "a.x = p", "b.y + p", "a off the curve", "b off the curve"):
        assert c("CHECK", cls) >= 1, cls
    # the first pass: sorted by op.  The second: a permutation in which no case keeps its place, consecutive lanes of a wave carry
    # different ops, and every wave has an early-returning CHECK lane and a VALID one
    n = recs.shape[0]
    ops = recs[:, 0].astype(np.int64)
    assert np.all(np.diff(ops) >= 0)
    assert sorted(order.tolist()) == list(range(n)) and not np.any(order == np.arange(n))
    for w in range(0, n, WAVE):
        lanes = order[w:w + WAVE]
        assert np.all(np.diff(ops[lanes]) != 0), w
        ks = {kinds[int(i)] for i in lanes}
        assert "early" in ks and "valid" in ks, w
        assert len(set(ops[lanes].tolist())) >= 8, w
    return per_op


def check_results(got, label=""):
    """got: (n, OUT_WORDS) uint32, one result record per case of build().  Raises AssertionError naming the first mismatch."""
    s = build()
    recs, expect = s["recs"], s["expect"]
    assert got.shape == expect.shape, "%s: result shape %s" % (label, got.shape)
    done = got[:, OUT_WORDS - 1] == expect[:, OUT_WORDS - 1]
    bad = np.nonzero(np.any(got != expect, axis=1))[0]
    if bad.size:
        per_op = {}
        for j in bad:
            k = OP_NAMES[int(recs[j, 0])]
            per_op[k] = per_op.get(k, 0) + 1
        i = int(bad[0])
        hexs = lambda ws: " ".join("%08x" % int(w) for w in ws)
        words = np.nonzero(got[i] != expect[i])[0]
        raise AssertionError("%s: %d of %d cases differ (%d without a DONE marker), by op %s.  First: case %d op %s aux %#x table %d, words %s differ\n"
                             "  a    %s\n  b    %s\n  p0   %s\n  p1   %s\n  got  %s\n  want %s" % (
                                 label, bad.size, recs.shape[0], int(np.sum(~done)), per_op, i, OP_NAMES[int(recs[i, 0])], int(recs[i, 1]),
                                 int(recs[i, 2]), words.tolist()[:12], hexs(recs[i, OFF_A:OFF_B]), hexs(recs[i, OFF_B:OFF_P0]),
                                 hexs(recs[i, OFF_P0:OFF_P1]), hexs(recs[i, OFF_P1:]), hexs(got[i]), hexs(expect[i])))
