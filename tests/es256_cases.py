"""The signature set of the ES256 tests: about 400 records of 160 bytes (pubkey_x || pubkey_y || r || s || msghash, each 32
little-endian bytes), deterministic, with the reason code tests/es256_ref.py gives each.  build() costs a few seconds of CPU and is
cached for the session (every test file that needs the set imports this module and calls it).

What is in it, by name prefix:
  valid/      300 random signatures (random key, digest and nonce)
  kat/        RFC 6979 A.2.5, "sample" with SHA-256: d G is the published key and the published (r, s) verifies
  spoil/      valid signatures with one field spoiled: one bit of r, s, z, x flipped; s + 1; y -> p - y
  range/      every boundary of the range test: x = p, y = p, z = n, z = n - 1 (in range), r = 0, r = n, s = 0, s = n, all-ones fields
  curve/      the key (0, 0) and a key off the curve
  key/        d = 1, d = n - 1, d = 2: Q = G, Q = -G, Q = 2 G
  z0/         z = 0: u1 = 0, the G accumulator stays the identity
  meet/       u1 G = u2 Q (the last addition is a doubling; valid) and u1 G = -u2 Q (the sum is the identity; invalid)

The module asserts, on the CPU, the outcome each construction is built for, and that over the VALID records every 4-bit digit
value occurs at every one of the 64 digit positions of both u1 and u2: a wrong entry of the comb table of G, or of the table of
Q's multiples, then turns some valid record invalid.  (With 300 random records a (position, digit) pair is missed with probability
(15/16)^300, about 4e-9; if the assertion ever trips after a change of the seeds, add records.)
"""
import functools
import hashlib
import random

import es256_ref as R

SEED = 0x45533235362D31  # "ES256-1"
N_RANDOM = 300
N_SPOILED = 12  # valid records that are spoiled, six ways each

KAT_D = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721
KAT_UX = 0x60FED4BA255A9D31C961EB74C6356D68C049B8923B61FA6CE669622E60F29FB6
KAT_UY = 0x7903FE1008B8BC99A41AE9E95628BC64F2F1B20C2D7E9F5177A3C294D4462299
KAT_R = 0xEFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716
KAT_S = 0xF7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8
KAT_Z = int.from_bytes(hashlib.sha256(b"sample").digest(), "big")

ONES = 2**256 - 1


class CaseSet:
    def __init__(self, names, fields, reasons):
        self.names, self.fields, self.reasons = names, fields, reasons  # fields: (x, y, r, s, z) integers per record
        self.records = [R.record(*f) for f in fields]
        self.blob = b"".join(self.records)

    def __len__(self):
        return len(self.names)

    def index(self, name):
        return self.names.index(name)

    def valid_indices(self):
        return [i for i, v in enumerate(self.reasons) if v == R.VALID]

    def invalid_indices(self):
        return [i for i, v in enumerate(self.reasons) if v != R.VALID]


def _signed(rng, d=None, z=None):
    d = rng.randrange(1, R.N) if d is None else d
    z = rng.randrange(R.N) if z is None else z
    while True:
        k = rng.randrange(1, R.N)
        r, s = R.sign(d, z, k)
        if r and s:
            break
    q = R.affine_mul(d, R.G)
    return (q[0], q[1], r, s, z)


@functools.lru_cache(maxsize=None)
def build():
    rng = random.Random(SEED)
    cases = []  # (name, fields, the outcome the construction is built for or None)
    for i in range(N_RANDOM):
        cases.append(("valid/%d" % i, _signed(rng), R.VALID))
    assert R.affine_mul(KAT_D, R.G) == (KAT_UX, KAT_UY), "RFC 6979 A.2.5: d G is not the published key"
    cases.append(("kat/rfc6979-a.2.5-sample-sha256", (KAT_UX, KAT_UY, KAT_R, KAT_S, KAT_Z), R.VALID))
    for i in range(N_SPOILED):
        x, y, r, s, z = cases[i][1]
        bit = 1 << rng.randrange(256)
        cases.append(("spoil/%d/r-bit" % i, (x, y, r ^ bit, s, z), None))  # (may leave the range: the reference says which)
        cases.append(("spoil/%d/s-bit" % i, (x, y, r, s ^ bit, z), None))
        cases.append(("spoil/%d/z-bit" % i, (x, y, r, s, z ^ bit), None))
        cases.append(("spoil/%d/x-bit" % i, (x ^ bit, y, r, s, z), None))
        cases.append(("spoil/%d/s+1" % i, (x, y, r, (s + 1) % 2**256, z), None))
        cases.append(("spoil/%d/y-negated" % i, (x, R.P - y, r, s, z), R.MISMATCH))
    x, y, r, s, z = cases[N_SPOILED][1]
    for name, f, want in (("x=p", (R.P, y, r, s, z), R.RANGE), ("y=p", (x, R.P, r, s, z), R.RANGE), ("z=n", (x, y, r, s, R.N), R.RANGE),
                          ("z=n-1", (x, y, r, s, R.N - 1), R.MISMATCH), ("r=0", (x, y, 0, s, z), R.RANGE), ("r=n", (x, y, R.N, s, z), R.RANGE),
                          ("s=0", (x, y, r, 0, z), R.RANGE), ("s=n", (x, y, r, R.N, z), R.RANGE), ("x=ones", (ONES, y, r, s, z), R.RANGE),
                          ("y=ones", (x, ONES, r, s, z), R.RANGE), ("r=ones", (x, y, ONES, s, z), R.RANGE),
                          ("s=ones", (x, y, r, ONES, z), R.RANGE), ("z=ones", (x, y, r, s, ONES), R.RANGE),
                          ("all=ones", (ONES,) * 5, R.RANGE), ("all=zero", (0,) * 5, R.RANGE)):
        cases.append(("range/" + name, f, want))
    cases.append(("curve/(0,0)", (0, 0, r, s, z), R.OFF_CURVE))
    cases.append(("curve/y+1", (x, (y + 1) % R.P, r, s, z), R.OFF_CURVE))
    cases.append(("curve/x=p-1", (R.P - 1, y, r, s, z), R.OFF_CURVE))
    for name, d in (("d=1", 1), ("d=n-1", R.N - 1), ("d=2", 2)):
        for j in range(4):
            cases.append(("key/%s/%d" % (name, j), _signed(rng, d=d), R.VALID))
        f = _signed(rng, d=d)
        cases.append(("key/%s/wrong-z" % name, f[:4] + ((f[4] + 1) % R.N,), R.MISMATCH))
    for j in range(4):
        cases.append(("z0/%d" % j, _signed(rng, z=0), R.VALID))
    f = _signed(rng, z=0)
    cases.append(("z0/wrong-r", (f[0], f[1], f[2] ^ 1 or 2, f[3], 0), None))
    for j in range(6):
        # u1 G = u2 Q: r = x(k G) mod n, z = r d, s = 2 z / k  ->  u1 = k / 2, u2 d = k / 2, the sum is k G
        k, d = rng.randrange(1, R.N), rng.randrange(1, R.N)
        q = R.affine_mul(d, R.G)
        r = R.affine_mul(k, R.G)[0] % R.N
        z = r * d % R.N
        cases.append(("meet/equal/%d" % j, (q[0], q[1], r, pow(k, -1, R.N) * 2 * z % R.N, z), R.VALID))
        # u1 G = -u2 Q: z = -r d, any s  ->  u1 + u2 d = 0, the sum is the identity
        cases.append(("meet/opposite/%d" % j, (q[0], q[1], r, rng.randrange(1, R.N), (-r * d) % R.N), R.MISMATCH))
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    fields = [c[1] for c in cases]
    reasons = [R.verify_ints(*f) for f in fields]
    for (name, f, want), got in zip(cases, reasons):
        assert want is None or want == got, "%s: built for %s, the reference says %s" % (name, R.REASON_NAMES[want], R.REASON_NAMES[got])
    for name, got in zip(names, reasons):
        if name.startswith("spoil/"):
            assert got != R.VALID, name
    # the meeting cases really meet
    for (name, f, _) in cases:
        if name.startswith("meet/"):
            u1, u2 = R.scalars(f[2], f[3], f[4])
            a, b = R.affine_mul(u1, R.G), R.affine_mul(u2, (f[0], f[1]))
            assert a[0] == b[0] and (a[1] == b[1]) == name.startswith("meet/equal"), name
    cs = CaseSet(names, fields, reasons)
    assert_digit_coverage(cs)
    return cs


def digit_coverage(cs):
    """seen[which][position] = the set of 4-bit digit values u1 (which = 0) / u2 (1) take there over the valid records."""
    seen = [[set() for _ in range(64)] for _ in range(2)]
    for i in cs.valid_indices():
        _, _, r, s, z = cs.fields[i]
        for which, u in enumerate(R.scalars(r, s, z)):
            for pos in range(64):
                seen[which][pos].add((u >> (4 * pos)) & 15)
    return seen


def assert_digit_coverage(cs):
    for which, per_pos in enumerate(digit_coverage(cs)):
        for pos, digits in enumerate(per_pos):
            assert len(digits) == 16, "u%d: digit position %d never takes the values %s over the valid records: add seeds" % (
                which + 1, pos, sorted(set(range(16)) - digits))
