"""An independent BN254 optimal-ate pairing over Python integers: the reference of the device pairing's value-level tests
(tests/pairing_device_cases.py).  Written from the mathematics in the comments of csrc/pairing.h, not from its code, and it imports
nothing compiled from csrc/.  tests/test_pairing_ref.py anchors it on facts that do not involve the code under test (Frobenius is
the p-th power, a a^-1 = 1, bilinearity, the order of e(G1, G2)); that file runs in about 3 s.

Tower: Fq2 = Fq[u] / (u^2 + 1), Fq6 = Fq2[v] / (v^3 - xi), Fq12 = Fq6[w] / (w^2 - v), xi = 9 + u.
  Fq2   (a0, a1)                          a0 + a1 u
  Fq6   (c0, c1, c2) of Fq2               c0 + c1 v + c2 v^2
  Fq12  (d0, .., d5) of Fq2               sum d_i w^i, w^6 = xi  (so w^2 = v: the tower's c0 = (d0, d2, d4), c1 = (d1, d3, d5))
Products are schoolbook by the defining relations.  Inverses go down by norms; the inverse of zero is zero.
G2 is the twist y^2 = x^3 + 3 / xi over Fq2, untwisted by (x, y) -> (x w^2, y w^3).

Limb images: an Fq value v travels as the 8 little-endian 32-bit words of v 2^256 mod p (its Montgomery image); an Fq12 as the 96
words of c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2, i.e. d0, d2, d4, d1, d3, d5.  A G1 point is 16 words (x, y), the identity all
zero: the same rows as tests/pairing_cases.py's g1_words, seen as 32-bit words.
"""
from zkoracle import field as F

P, R = F.P, F.R
U = 4965661367192848881
SIX_U_PLUS_2 = 6 * U + 2
STEPS = 102
W256 = 1 << 256
RINV = pow(W256, -1, P)
VALID, RANGE, OFF_CURVE, MISMATCH = 0, 1, 2, 3
HARD = (P**4 - P**2 + 1) // R
assert (P**4 - P**2 + 1) % R == 0 and SIX_U_PLUS_2.bit_length() == 65

# ---- Fq2 ---------------------------------------------------------------------------------------------------------------------
F2_ZERO, F2_ONE, XI = (0, 0), (1, 0), (9, 1)


def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_neg(a):
    return (-a[0] % P, -a[1] % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_mul_fq(a, s):
    return (a[0] * s % P, a[1] * s % P)


def f2_conj(a):
    return (a[0], -a[1] % P)


def f2_norm(a):
    return (a[0] * a[0] + a[1] * a[1]) % P


def f2_inv(a):
    n = f2_norm(a)
    d = pow(n, -1, P) if n else 0
    return (a[0] * d % P, -a[1] * d % P)


def f2_pow(a, e):
    acc = F2_ONE
    for bit in bin(e)[2:]:
        acc = f2_mul(acc, acc)
        if bit == "1":
            acc = f2_mul(acc, a)
    return acc


def f2_mul_xi(a):
    return f2_mul(a, XI)


# ---- Fq6 ---------------------------------------------------------------------------------------------------------------------
F6_ZERO, F6_ONE = (F2_ZERO,) * 3, (F2_ONE, F2_ZERO, F2_ZERO)


def f6_add(a, b):
    return tuple(f2_add(x, y) for x, y in zip(a, b))


def f6_sub(a, b):
    return tuple(f2_sub(x, y) for x, y in zip(a, b))


def f6_neg(a):
    return tuple(f2_neg(x) for x in a)


def f6_mul(a, b):
    d = [F2_ZERO] * 5
    for i in range(3):
        for j in range(3):
            d[i + j] = f2_add(d[i + j], f2_mul(a[i], b[j]))
    return (f2_add(d[0], f2_mul(XI, d[3])), f2_add(d[1], f2_mul(XI, d[4])), d[2])  # v^3 = xi, v^4 = xi v


def f6_mul_v(a):
    return f6_mul(a, (F2_ZERO, F2_ONE, F2_ZERO))


def f6_inv(a):
    """by the norm to Fq2: with t = the adjugate of a (a t lies in Fq2), a^-1 = t / (a t)"""
    c0, c1, c2 = a
    t = (f2_sub(f2_mul(c0, c0), f2_mul(XI, f2_mul(c1, c2))), f2_sub(f2_mul(XI, f2_mul(c2, c2)), f2_mul(c0, c1)),
         f2_sub(f2_mul(c1, c1), f2_mul(c0, c2)))
    n = f6_mul(a, t)
    assert n[1] == F2_ZERO and n[2] == F2_ZERO
    ni = f2_inv(n[0])
    return tuple(f2_mul(x, ni) for x in t)


# ---- Fq12 --------------------------------------------------------------------------------------------------------------------
F12_ZERO = (F2_ZERO,) * 6
F12_ONE = (F2_ONE,) + (F2_ZERO,) * 5


def f12_add(a, b):
    return tuple(f2_add(x, y) for x, y in zip(a, b))


def f12_neg(a):
    return tuple(f2_neg(x) for x in a)


def f12_mul(a, b):
    r0, r1 = [0] * 11, [0] * 11  # unreduced Fq2 coefficients of w^0 .. w^10
    for i in range(6):
        x0, x1 = a[i]
        if x0 == 0 and x1 == 0:
            continue
        for j in range(6):
            y0, y1 = b[j]
            r0[i + j] += x0 * y0 - x1 * y1
            r1[i + j] += x0 * y1 + x1 * y0
    out = []
    for k in range(6):
        h0, h1 = (r0[k + 6], r1[k + 6]) if k < 5 else (0, 0)  # w^(k+6) = xi w^k
        out.append(((r0[k] + 9 * h0 - h1) % P, (r1[k] + h0 + 9 * h1) % P))
    return tuple(out)


def f12_sqr(a):
    return f12_mul(a, a)


def f12_conj(a):
    """the conjugate over Fq6: w -> -w"""
    return tuple(f2_neg(c) if i & 1 else c for i, c in enumerate(a))


def f12_c0(a):
    return (a[0], a[2], a[4])


def f12_c1(a):
    return (a[1], a[3], a[5])


def f12_of_halves(c0, c1):
    return (c0[0], c1[0], c0[1], c1[1], c0[2], c1[2])


def f12_inv(a):
    """by the norm to Fq6: a conj(a) = c0^2 - v c1^2"""
    n = f12_mul(a, f12_conj(a))
    assert f12_c1(n) == F6_ZERO
    ni = f6_inv(f12_c0(n))
    return f12_mul(f12_conj(a), f12_of_halves(ni, F6_ZERO))


def f12_pow(a, e):
    acc = F12_ONE
    for bit in bin(e)[2:]:
        acc = f12_mul(acc, acc)
        if bit == "1":
            acc = f12_mul(acc, a)
    return acc


GAMMA = tuple(f2_pow(XI, i * (P - 1) // 6) for i in range(6))
assert (P - 1) % 6 == 0


def frobenius(a):
    """a^p = sum conj(c_i) gamma_i w^i"""
    return tuple(f2_mul(f2_conj(c), GAMMA[i]) for i, c in enumerate(a))


# ---- G2 walk -----------------------------------------------------------------------------------------------------------------
def _step(T, Q):
    """the line through T and Q (the tangent when Q is T) as (lambda, lambda xT - yT), and T + Q"""
    (xt, yt), (xq, yq) = T, Q
    if T == Q:
        lam = f2_mul(f2_mul_fq(f2_mul(xt, xt), 3), f2_inv(f2_add(yt, yt)))
    else:
        assert xt != xq
        lam = f2_mul(f2_sub(yq, yt), f2_inv(f2_sub(xq, xt)))
    x3 = f2_sub(f2_sub(f2_mul(lam, lam), xt), xq)
    return (lam, f2_sub(f2_mul(lam, xt), yt)), (x3, f2_sub(f2_mul(lam, f2_sub(xt, x3)), yt))


def g2_frobenius(Q):
    """pi(Q) on the twist: (conj(x) xi^((p-1)/3), conj(y) xi^((p-1)/2))"""
    return (f2_mul(f2_conj(Q[0]), GAMMA[2]), f2_mul(f2_conj(Q[1]), GAMMA[3]))


def g2_neg(Q):
    return (Q[0], f2_neg(Q[1]))


def prepared_walk(Q, with_t=False):
    """the 102 (lambda, c) of Q's walk: 64 doublings, an addition per set bit of the low 64 bits of 6u + 2 (T starts at Q for the
    top bit), then the lines to pi(Q) and -pi^2(Q).  with_t: also T before the two Frobenius steps and after each of them."""
    T, out = Q, []
    for b in range(63, -1, -1):
        line, T = _step(T, T)
        out.append(line)
        if (SIX_U_PLUS_2 >> b) & 1:
            line, T = _step(T, Q)
            out.append(line)
    q1 = g2_frobenius(Q)
    nq2 = g2_neg(g2_frobenius(q1))
    line, T1 = _step(T, q1)
    out.append(line)
    line, T2 = _step(T1, nq2)
    out.append(line)
    assert len(out) == STEPS
    return (out, (T, T1, T2)) if with_t else out


def line_value(line, Pt):
    """yP - lambda xP w + c w^3"""
    lam, c = line
    return ((Pt[1], 0), f2_neg(f2_mul_fq(lam, Pt[0])), F2_ZERO, c, F2_ZERO, F2_ZERO)


def make_table(g2, s_g2):
    """what a check against (g2, s_g2) reads: walk 0 is s_g2's, walk 1 is g2's; None for an identity"""
    return {"walks": (None if s_g2 is None else prepared_walk(s_g2), None if g2 is None else prepared_walk(g2))}


def miller(P0, P1, walk0, walk1):
    """ML(P0, Q0) ML(P1, Q1) over the two walks; a pair with an identity on either side (point or walk None) is left out"""
    pairs = [(Pt, wk) for Pt, wk in ((P0, walk0), (P1, walk1)) if Pt is not None and wk is not None]
    f, n = F12_ONE, 0
    for b in range(63, -3, -1):
        if b >= 0:
            f = f12_sqr(f)
        for _ in range(2 if b >= 0 and (SIX_U_PLUS_2 >> b) & 1 else 1):
            for Pt, wk in pairs:
                f = f12_mul(f, line_value(wk[n], Pt))
            n += 1
    assert n == STEPS
    return f


def final_exponentiation(f):
    """f^((p^12 - 1) / r): (p^6 - 1) by conjugate over inverse, (p^2 + 1) by two Frobenius maps, the rest a plain power"""
    t = f12_mul(f12_conj(f), f12_inv(f))
    t = f12_mul(frobenius(frobenius(t)), t)
    return f12_pow(t, HARD)


def pairing(Pt, Q):
    return final_exponentiation(miller(Pt, None, prepared_walk(Q), None))


# ---- limb images -------------------------------------------------------------------------------------------------------------
def to_words(v):
    """the 8 words of an integer below 2^256, as it is"""
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def from_words(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def mont(v):
    return v * W256 % P


def unmont(m):
    return m * RINV % P


def fq_words(v):
    return to_words(mont(v))


def f2_words(a):
    return fq_words(a[0]) + fq_words(a[1])


def f6_words(a):
    return [w for c in a for w in f2_words(c)]


F12_ORDER = (0, 2, 4, 1, 3, 5)  # memory order of the w-powers


def f12_words(a):
    return [w for i in F12_ORDER for w in f2_words(a[i])]


def f2_from_words(ws):
    return (unmont(from_words(ws[:8])), unmont(from_words(ws[8:16])))


def f12_from_words(ws):
    c = [f2_from_words(ws[16 * k:16 * k + 16]) for k in range(6)]
    return tuple(c[F12_ORDER.index(i)] for i in range(6))


def g1_words(Pt):
    return [0] * 16 if Pt is None else fq_words(Pt[0]) + fq_words(Pt[1])


def g1_row_to_words(row):
    """an 8 x uint64 row of pairing_cases.g1_words -> 16 32-bit words"""
    out = []
    for q in row:
        out += [int(q) & 0xFFFFFFFF, int(q) >> 32]
    return out


def g1_neg(Pt):
    return None if Pt is None else (Pt[0], -Pt[1] % P)


def check(a, b, table):
    """the ZK_PAIRING_* reason of e(a, s_g2) e(-b, g2) = 1 for a, b given as 16-word rows (any words at all)"""
    img = [from_words(a[:8]), from_words(a[8:]), from_words(b[:8]), from_words(b[8:])]
    if any(m >= P for m in img):
        return RANGE
    ax, ay, bx, by = (unmont(m) for m in img)
    pts = []
    for x, y in ((ax, ay), (bx, by)):
        if x == 0 and y == 0:
            pts.append(None)
        elif (y * y - x * x * x - 3) % P:
            return OFF_CURVE
        else:
            pts.append((x, y))
    f = final_exponentiation(miller(pts[0], g1_neg(pts[1]), table["walks"][0], table["walks"][1]))
    return VALID if f == F12_ONE else MISMATCH
