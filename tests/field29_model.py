"""Limb-exact model of csrc/field29.hip.h and csrc/ec29.hip.h in plain Python integers.

Every function restates its device twin limb for limb: the same columns, the same masks, the same order of the lazy
additions and subtractions.  Where the hardware would silently wrap, the model raises `Wrap`:
  * a 64-bit column accumulator reaching 2^64,
  * a 32-bit limb sum reaching 2^32 (add29, norm29, the doubled operand of sqr29, the sum in sub29),
  * a negative limb difference C[i] - b[i] in sub29,
  * a product's top limb reaching 2^32.
The modulus is a parameter (zkoracle.field.P and .R); the spread constants of sub29<K, E>, the limbs of p, -p^-1 mod 2^29
and the powers of two are all recomputed from it here, not copied from the header.

tests/test_field29_model.py anchors the model to big-integer arithmetic; tests/test_gpu_field_device.py compares the
device with the model limb for limb.
"""
from zkoracle import field as F

M29 = (1 << 29) - 1
W64 = 1 << 64
W32 = 1 << 32


class Wrap(Exception):
    """An intermediate left the range of the register that holds it on the device."""


def value(limbs):
    """The integer a (possibly non-normalised) limb vector stands for."""
    return sum(l << (29 * i) for i, l in enumerate(limbs))


def split29(v):
    """Normalised limbs of v (top limb takes the rest)."""
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def words8(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def from_words8(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


class Field29:
    def __init__(self, p):
        self.p = p
        self.P = split29(p)
        self.INV = (-pow(p, -1, 1 << 29)) % (1 << 29)
        self.R261 = (1 << 261) % p
        self.R256 = (1 << 256) % p

    # ---- constants -------------------------------------------------------------------------------------------------
    def kp_limb(self, K, i):
        return ((K * self.p) >> (29 * i)) & M29

    def spread(self, K, E):
        """Spread29<PRM, K, E>::C: K p with 2^E lent to every limb but the top by the limb above it."""
        borrow = 1 << (E - 29)
        c = []
        for i in range(9):
            d = self.kp_limb(K, i)
            if i == 0:
                c.append(d + (1 << E))
            elif i < 8:
                c.append(d + (1 << E) - borrow)
            else:
                c.append(d - borrow)
        return c

    def pow2(self, e):
        """const_pow2_29<e>: the limbs of 2^e mod p."""
        return self.to29(pow(2, e, self.p))

    # ---- conversions -----------------------------------------------------------------------------------------------
    def to29(self, v):
        assert 0 <= v < (1 << 256)
        return [(v >> (29 * i)) & M29 for i in range(9)]

    def to29_x32(self, v):
        assert 0 <= v < (1 << 256)
        return [(v << 5) & M29] + [(v >> (29 * i - 5)) & M29 for i in range(1, 9)]

    def from29(self, a):
        w = []
        for k in range(8):
            i = (32 * k) // 29
            o = 32 * k - 29 * i
            v = a[i] >> o
            v |= a[i + 1] << (29 - o)
            if i + 2 < 9:
                v |= a[i + 2] << (58 - o)
            w.append(v & 0xFFFFFFFF)
        return from_words8(w)

    def reduce_once(self, v):
        return v - self.p if v >= self.p else v

    # ---- products --------------------------------------------------------------------------------------------------
    def _montgomery(self, pairs):
        """sum over (a, b) in pairs of a * b, times 2^-261, by product scanning with one reduction."""
        P, INV = self.P, self.INV
        m = [0] * 9
        r = [0] * 9
        acc = 0
        for k in range(17):
            lo, hi = (k - 8 if k > 8 else 0), (k if k < 9 else 8)
            for a, b in pairs:
                for i in range(lo, hi + 1):
                    acc += a[i] * b[k - i]
            if k < 9:
                for i in range(k):
                    acc += m[i] * P[k - i]
                if acc >= W64:
                    raise Wrap("column %d: 2^%.3f before the reduction digit" % (k, _log2(acc)))
                m[k] = ((acc & 0xFFFFFFFF) * INV) & M29
                acc += m[k] * P[0]
            else:
                for i in range(k - 8, 9):
                    acc += m[i] * P[k - i]
            if acc >= W64:
                raise Wrap("column %d: 2^%.3f" % (k, _log2(acc)))
            if k >= 9:
                r[k - 9] = acc & M29
            acc >>= 29
        if acc >= W32:
            raise Wrap("top limb 2^%.3f" % _log2(acc))
        r[8] = acc
        return r

    def worst_column(self, pairs):
        """log2 of the largest column accumulator of the product (for the docstrings' margins); no wrap check."""
        P, INV = self.P, self.INV
        m = [0] * 9
        acc = 0
        worst = 0
        for k in range(17):
            lo, hi = (k - 8 if k > 8 else 0), (k if k < 9 else 8)
            for a, b in pairs:
                for i in range(lo, hi + 1):
                    acc += a[i] * b[k - i]
            if k < 9:
                for i in range(k):
                    acc += m[i] * P[k - i]
                m[k] = ((acc & 0xFFFFFFFF) * INV) & M29
                acc += m[k] * P[0]
            else:
                for i in range(k - 8, 9):
                    acc += m[i] * P[k - i]
            worst = max(worst, acc)
            acc >>= 29
        return _log2(worst)

    def mul29(self, a, b):
        _limbs32(a), _limbs32(b)
        return self._montgomery([(a, b)])

    def sqr29(self, a):
        # the device takes the cross products against the doubled operand: 2 a_i must fit a word; the column sums are
        # those of a * a
        _limbs32(a)
        for l in a:
            if (l << 1) >= W32:
                raise Wrap("sqr29: doubled limb 2^%.3f" % _log2(l << 1))
        return self._montgomery([(a, a)])

    def mul2add29(self, a, b, c, d):
        _limbs32(a), _limbs32(b), _limbs32(c), _limbs32(d)
        return self._montgomery([(a, b), (c, d)])

    def mulKadd29(self, a, b):
        assert 1 <= len(a) == len(b) <= 5
        for x in list(a) + list(b):
            _limbs32(x)
        return self._montgomery(list(zip(a, b)))

    # ---- additions -------------------------------------------------------------------------------------------------
    def add29(self, a, b):
        r = [x + y for x, y in zip(a, b)]
        for i, l in enumerate(r):
            if l >= W32:
                raise Wrap("add29: limb %d = 2^%.3f" % (i, _log2(l)))
        return r

    def sub29(self, K, E, a, b):
        C = self.spread(K, E)
        r = []
        for i in range(9):
            d = C[i] - b[i]
            if d < 0:
                raise Wrap("sub29<%d, %d>: limb %d of b exceeds the spread constant by %d" % (K, E, i, -d))
            s = a[i] + d
            if s >= W32:
                raise Wrap("sub29<%d, %d>: limb %d = 2^%.3f" % (K, E, i, _log2(s)))
            r.append(s)
        return r

    def norm29(self, a):
        r = []
        c = 0
        for i in range(8):
            t = a[i] + c
            if t >= W32:
                raise Wrap("norm29: limb %d" % i)
            r.append(t & M29)
            c = t >> 29
        t = a[8] + c
        if t >= W32:
            raise Wrap("norm29: top limb")
        r.append(t)
        return r

    def is_zero29(self, a):
        return all(l == 0 for l in a) or all(l == q for l, q in zip(a, self.P))

    def std_to_internal(self, v):
        return self.mul29(self.to29(v), self.pow2(266))

    def internal_to_std(self, a):
        return self.reduce_once(self.from29(self.mul29(a, self.pow2(256))))


def _log2(v):
    import math

    return math.log2(v) if v > 0 else float("-inf")


def _limbs32(a):
    assert len(a) == 9
    for l in a:
        if not 0 <= l < W32:
            raise Wrap("operand limb outside a 32-bit word")


FR = Field29(F.R)
FQ = Field29(F.P)


# ---- ec29.hip.h ------------------------------------------------------------------------------------------------------
class G1X29:
    """An XYZZ accumulator in internal form; `inf` marks the identity (the limbs are then don't-cares)."""

    __slots__ = ("x", "y", "zz", "zzz", "inf")

    def __init__(self, x=None, y=None, zz=None, zzz=None, inf=False):
        z = [0] * 9
        self.x, self.y, self.zz, self.zzz, self.inf = list(x or z), list(y or z), list(zz or z), list(zzz or z), inf

    def copy(self):
        return G1X29(self.x, self.y, self.zz, self.zzz, self.inf)

    def key(self):
        return (tuple(self.x), tuple(self.y), tuple(self.zz), tuple(self.zzz), self.inf)


def g1x29_identity():
    return G1X29(inf=True)


def g1x29_load(w):
    """The 36-word stored form -> accumulator; all-zero ZZ is the identity."""
    assert len(w) == 36
    return G1X29(w[0:9], w[9:18], w[18:27], w[27:36], inf=not any(w[18:27]))


def g1x29_store(a):
    return [0] * 36 if a.inf else list(a.x) + list(a.y) + list(a.zz) + list(a.zzz)


def g1x29_from_std(x, y, zz, zzz):
    """Four canonical standard-Montgomery words (as integers) -> internal form."""
    f = FQ
    return G1X29(f.std_to_internal(x), f.std_to_internal(y), f.std_to_internal(zz), f.std_to_internal(zzz), inf=zz == 0)


def g1x29_to_std(a):
    """-> (x, y, zz, zzz) canonical standard-Montgomery integers; the identity is (R, R, 0, 0) as G1X::identity()."""
    f = FQ
    if a.inf:
        return (f.R256, f.R256, 0, 0)
    return tuple(f.internal_to_std(c) for c in (a.x, a.y, a.zz, a.zzz))


def g1x29_add_affine(acc, x, y, check=True, internal=False, sqr=True, fuse=True):
    """acc += (x, y) in place; returns what the device returns.  x, y: canonical words as integers (standard Montgomery
    form, or with `internal` the internal form); sqr / fuse are ZK_EC29_SQR / ZK_EC29_FUSE."""
    f = FQ
    if acc.inf:
        acc.x = f.to29(x) if internal else f.std_to_internal(x)
        acc.y = f.to29(y) if internal else f.std_to_internal(y)
        acc.zz = f.pow2(261)
        acc.zzz = list(acc.zz)
        acc.inf = False
        return True
    x2 = f.to29(x) if internal else f.to29_x32(x)
    y2 = f.to29(y) if internal else f.to29_x32(y)
    u2 = f.mul29(x2, acc.zz)
    s2 = f.mul29(y2, acc.zzz)
    p = f.norm29(f.sub29(10, 29, u2, acc.x))
    r = f.norm29(f.sub29(6, 29, s2, acc.y))
    pp = f.sqr29(p) if sqr else f.mul29(p, p)
    if check and f.is_zero29(pp):
        return False
    ppp = f.mul29(p, pp)
    q = f.mul29(acc.x, pp)
    rr = f.sqr29(r) if sqr else f.mul29(r, r)
    t = f.add29(ppp, f.add29(q, q))
    x3 = f.norm29(f.sub29(7, 31, rr, t))
    v = f.sub29(10, 29, q, x3)
    if fuse:
        y3 = f.mul2add29(r, v, acc.y, f.sub29(3, 29, [0] * 9, ppp))
    else:
        t1 = f.mul29(r, v)
        t2 = f.mul29(acc.y, ppp)
        y3 = f.norm29(f.sub29(3, 29, t1, t2))
    acc.x = x3
    acc.y = y3
    acc.zz = f.mul29(acc.zz, pp)
    acc.zzz = f.mul29(acc.zzz, ppp)
    return True


def g1x29_dbl_rare(p):
    f = FQ
    if p.inf:
        return
    u = f.add29(p.y, p.y)
    v = f.mul29(u, u)
    w = f.mul29(u, v)
    s = f.mul29(p.x, v)
    xx = f.mul29(p.x, p.x)
    m = f.norm29(f.add29(xx, f.add29(xx, xx)))
    mm = f.mul29(m, m)
    x3 = f.norm29(f.sub29(5, 30, mm, f.add29(s, s)))
    t1 = f.mul29(m, f.sub29(8, 29, s, x3))
    t2 = f.mul29(w, p.y)
    p.zz = f.mul29(v, p.zz)
    p.zzz = f.mul29(w, p.zzz)
    p.x = x3
    p.y = f.norm29(f.sub29(3, 29, t1, t2))


def g1x29_add(acc, b):
    """acc += b in place; returns the branch taken: 'b_inf', 'acc_inf', 'dbl', 'cancel' or 'add'."""
    f = FQ
    if b.inf:
        return "b_inf"
    if acc.inf:
        acc.x, acc.y, acc.zz, acc.zzz, acc.inf = list(b.x), list(b.y), list(b.zz), list(b.zzz), False
        return "acc_inf"
    u1 = f.mul29(acc.x, b.zz)
    u2 = f.mul29(b.x, acc.zz)
    s1 = f.mul29(acc.y, b.zzz)
    s2 = f.mul29(b.y, acc.zzz)
    p = f.norm29(f.sub29(3, 29, u2, u1))
    r = f.norm29(f.sub29(3, 29, s2, s1))
    pp = f.sqr29(p)
    rr = f.sqr29(r)
    if f.is_zero29(pp):
        if f.is_zero29(rr):
            g1x29_dbl_rare(acc)
            return "dbl"
        i = g1x29_identity()
        acc.x, acc.y, acc.zz, acc.zzz, acc.inf = i.x, i.y, i.zz, i.zzz, True
        return "cancel"
    ppp = f.mul29(p, pp)
    q = f.mul29(u1, pp)
    t = f.add29(ppp, f.add29(q, q))
    x3 = f.norm29(f.sub29(7, 31, rr, t))
    v = f.sub29(10, 29, q, x3)
    acc.y = f.mul2add29(r, v, s1, f.sub29(3, 29, [0] * 9, ppp))
    acc.x = x3
    acc.zz = f.mul29(f.mul29(acc.zz, b.zz), pp)
    acc.zzz = f.mul29(f.mul29(acc.zzz, b.zzz), ppp)
    return "add"


# ---- helpers shared by the two test modules --------------------------------------------------------------------------
def affine_of(a):
    """The affine point (plain integers, as zkoracle.curve) an accumulator stands for; None for the identity."""
    p = F.P
    if a.inf:
        return None
    ri = pow(1 << 261, -1, p)
    X, Y, ZZ, ZZZ = (value(c) * ri % p for c in (a.x, a.y, a.zz, a.zzz))
    assert ZZ != 0 and ZZZ != 0 and pow(ZZ, 3, p) == ZZZ * ZZZ % p, "not an XYZZ point"
    return (X * pow(ZZ, -1, p) % p, Y * pow(ZZZ, -1, p) % p)


def lifted(pt, z, i=0, j=0, kz=0, kzz=0):
    """The accumulator for affine `pt` with ZZ = z^2, ZZZ = z^3 and the representatives X + i p, Y + j p, ZZ + kz p,
    ZZZ + kzz p (normalised limbs)."""
    p = F.P
    s = (1 << 261) % p
    zz, zzz = z * z % p, z * z * z % p
    X, Y = pt[0] * zz % p, pt[1] * zzz % p
    return G1X29(split29(X * s % p + i * p), split29(Y * s % p + j * p), split29(zz * s % p + kz * p),
                 split29(zzz * s % p + kzz * p))


def extreme(bits, k, p):
    """The contract-extreme operand: the eight lower limbs at floor(2^bits) - 1 (bits may be fractional), the top limb
    the largest that keeps the value below k p."""
    lo = int(2.0 ** bits) - 1 if bits != int(bits) else (1 << int(bits)) - 1
    low = sum(lo << (29 * i) for i in range(8))
    top = (k * p - 1 - low) >> 232
    assert 0 <= top < W32
    a = [lo] * 8 + [top]
    assert value(a) < k * p
    return a
