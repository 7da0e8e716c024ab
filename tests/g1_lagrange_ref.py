"""A pure-Python restatement of halo2's `g_to_lagrange` (arithmetic.rs [RECALLED]) on zkoracle.curve: the inverse FFT of a vector
of G1 points followed by a scale by 1/n,  out[i] = [1/n] sum_j [w^-ij] g[j],  w = the domain generator of k.  Slow (one
scalar multiplication per butterfly, in Python): small k only.  Points are affine int tuples, identity None."""
from zkoracle import curve, field as F

_ID = (1, 1, 0)


def _jmul(p, s):
    acc, base = _ID, p
    while s:
        if s & 1:
            acc = curve._jadd(acc, base)
        base = curve._jdbl(base)
        s >>= 1
    return acc


def _jneg(p):
    return (p[0], (-p[1]) % F.P, p[2])


def g_to_lagrange(points, k):
    n = 1 << k
    if len(points) != n:
        raise ValueError("need 2^k points")
    w_inv = F.inv(F.omega(k), F.R)
    a = [curve.to_jac(points[int(format(i, "0%db" % k)[::-1], 2)]) for i in range(n)]
    h = 1
    while h < n:
        wm = pow(w_inv, n // (2 * h), F.R)
        for start in range(0, n, 2 * h):
            t = 1
            for j in range(h):
                u, v = a[start + j], _jmul(a[start + j + h], t)
                a[start + j], a[start + j + h] = curve._jadd(u, v), curve._jadd(u, _jneg(v))
                t = t * wm % F.R
        h *= 2
    ninv = F.inv(n, F.R)
    return [curve.to_affine(_jmul(p, ninv)) for p in a]


def to_mont_limbs(points):
    """affine int tuples (None = identity) -> the engine's (n, 8) uint64 affine Montgomery image"""
    import numpy as np

    words = []
    for pt in points:
        for c in ((0, 0) if pt is None else (pt[0] * (1 << 256) % F.P, pt[1] * (1 << 256) % F.P)):
            words += [(c >> (64 * q)) & 0xFFFFFFFFFFFFFFFF for q in range(4)]
    return np.array(words, dtype=np.uint64).reshape(-1, 8)


def from_mont_limbs(arr):
    """the inverse of to_mont_limbs"""
    rinv = F.inv(1 << 256, F.P)
    out = []
    for row in arr.reshape(-1, 8):
        x = sum(int(row[q]) << (64 * q) for q in range(4))
        y = sum(int(row[4 + q]) << (64 * q) for q in range(4))
        out.append(None if x == 0 and y == 0 else (x * rinv % F.P, y * rinv % F.P))
    return out
