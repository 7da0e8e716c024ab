"""ES256 (ECDSA over secp256r1 with SHA-256 digests) verification on Python integers, written from the standards (SEC 1 v2
section 4.1.4, FIPS 186-4 D.1.2.3 for the curve) and independent of webauthn-halo2_amd/ecdsa_p256.py: projective arithmetic with
the complete addition formulas of Renes, Costello and Batina (2016, algorithm 1 specialised to a general a), one inversion per
verification.  It is the reference of zk_es256_verify and of csrc/p256.hip.h, and returns the REASON code, the first failing
test: the codes of include/zkmi355.h.
"""
VALID, RANGE, OFF_CURVE, MISMATCH = 0, 1, 2, 3
REASON_NAMES = {VALID: "VALID", RANGE: "RANGE", OFF_CURVE: "OFF_CURVE", MISMATCH: "MISMATCH"}

P = 2**256 - 2**224 + 2**192 + 2**96 - 1
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
A = P - 3
B = 0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B
GX = 0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296
GY = 0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5
G = (GX, GY)
B3 = 3 * B % P
IDENTITY = (0, 1, 0)  # homogeneous projective (X : Y : Z)


def on_curve(x, y):
    return (y * y - (x * x * x + A * x + B)) % P == 0


def padd(p, q):
    """Complete addition on y^2 z = x^3 + a x z^2 + b z^3 (Renes-Costello-Batina, algorithm 1): no exceptional case."""
    x1, y1, z1 = p
    x2, y2, z2 = q
    t0, t1, t2 = x1 * x2 % P, y1 * y2 % P, z1 * z2 % P
    t3 = ((x1 + y1) * (x2 + y2) - t0 - t1) % P
    t4 = ((x1 + z1) * (x2 + z2) - t0 - t2) % P
    t5 = ((y1 + z1) * (y2 + z2) - t1 - t2) % P
    z3 = (A * t4 + B3 * t2) % P
    x3 = (t1 - z3) % P
    z3 = (t1 + z3) % P
    y3 = x3 * z3 % P
    t1 = (3 * t0 + A * t2) % P
    t4 = (B3 * t4 + A * (t0 - A * t2)) % P
    y3 = (y3 + t1 * t4) % P
    x3 = (t3 * x3 - t5 * t4) % P
    z3 = (t5 * z3 + t3 * t1) % P
    return x3, y3, z3


def pmul(k, pt):
    """k (x, y) for an affine point, as a projective triple."""
    acc, run = IDENTITY, (pt[0], pt[1], 1)
    while k:
        if k & 1:
            acc = padd(acc, run)
        run = padd(run, run)
        k >>= 1
    return acc


def to_affine(p):
    """(x, y), or None for the identity."""
    if p[2] % P == 0:
        return None
    zi = pow(p[2], -1, P)
    return p[0] * zi % P, p[1] * zi % P


def affine_add(a, b):
    """a + b of affine points (None: the identity), through the complete formulas."""
    pa = IDENTITY if a is None else (a[0], a[1], 1)
    pb = IDENTITY if b is None else (b[0], b[1], 1)
    return to_affine(padd(pa, pb))


def affine_mul(k, pt):
    return None if pt is None else to_affine(pmul(k % N, pt))


def scalars(r, s, z):
    """(u1, u2) of a signature in range."""
    w = pow(s, -1, N)
    return z * w % N, r * w % N


def verify_ints(x, y, r, s, z):
    if x >= P or y >= P or z >= N or not 0 < r < N or not 0 < s < N:
        return RANGE
    if not on_curve(x, y):
        return OFF_CURVE
    u1, u2 = scalars(r, s, z)
    pt = to_affine(padd(pmul(u1, G), pmul(u2, (x, y))))
    if pt is None or pt[0] % N != r:
        return MISMATCH
    return VALID


def verify_record(rec):
    """rec: 160 bytes, pubkey_x || pubkey_y || r || s || msghash, each 32 little-endian bytes."""
    assert len(rec) == 160
    return verify_ints(*(int.from_bytes(rec[32 * i:32 * i + 32], "little") for i in range(5)))


def record(x, y, r, s, z):
    return b"".join(int(v).to_bytes(32, "little") for v in (x, y, r, s, z))


def sign(d, z, k):
    """(r, s) of the digest z under the key d with the nonce k (no retry: the caller picks k with r, s != 0)."""
    r = affine_mul(k, G)[0] % N
    s = pow(k, -1, N) * (z + r * d) % N
    return r, s
