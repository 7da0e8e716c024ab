"""The cases of tests/test_gpu_msm_wide_device.py: per geometry (window bits, table stride) of the wide MSM path a sequence of
passes on ONE workspace, as plain data.  tests/test_msm_wide_cases.py asserts, from the model alone (tests/msm_wide_model.py),
that the designed columns meet the conditions they are designed for, and writes nothing to a GPU.

A column is a list of n scalars (integers mod r) over the first n points of a basis; the bases are [a_i] G with the a_i below."""
import functools
import random

import numpy as np

from zkoracle import cops, field as F

import msm_cases as MC
import msm_wide_model as W

R = F.R
GEOMETRIES = ((15, 1 << 12), (15, 1 << 20), (15, 1 << 21), (16, 1 << 12), (16, 1 << 21), (17, 1 << 12))
# (c, S) -> (ib, fb, bins, esc): the six entry layouts of the wide shape
LAYOUTS = {(15, 1 << 12): (24, 7, 128, 63), (15, 1 << 20): (25, 6, 256, 31), (15, 1 << 21): (26, 5, 512, 15),
           (16, 1 << 12): (24, 7, 256, 63), (16, 1 << 21): (25, 6, 512, 31), (17, 1 << 12): (24, 7, 512, 63)}
MAX_BATCH = 3
RANDOM_LENGTHS = (1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025)
SEAM_SLOTS = (23, 24, 25, 26)  # ZK_T1B_LMAX = 24 from both sides
IDENTITY_AT = (0, 5, 17, 127)


@functools.lru_cache(maxsize=None)
def bases():
    """0: 4096 distinct points; 1: a[1] = a[0] (equal points), a[3] = -a[2] (opposite points), no identity; 2: with identity points"""
    rng = random.Random(0xBA5E5)
    draw = lambda m: [rng.randrange(1, R) for _ in range(m)]
    b0, b1, b2 = draw(4096), draw(1024), draw(1024)
    assert len(set(b0)) == 4096
    b1[1], b1[3] = b1[0], R - b1[2]
    for i in IDENTITY_AT:
        b2[i] = 0
    return (b0, b1, b2)


def one_bucket_scalar(c):
    """digit 1 in every window, the top one included"""
    return sum(1 << (c * w) for w in range(254 // c + 1))


def one_bucket_n(c):
    """the column length whose one-bucket column has SUB = 4096 entries, or the nearest count"""
    return round(W.SUB / (254 // c + 1))


def ladder_buckets(g):
    """The gap ladder: local bucket numbers per coarse bin.  esc = keys / 2 - 1, so a bin holds one long gap at most."""
    mid, e = g.bins // 2, g.esc
    bins = {0: [5], g.bins - 1: [g.keys - 1]}
    for base, o in ((g.bins // 4, 1), (mid, 0)):  # gaps 0 and esc - 1 | esc | esc + 1, twice
        bins.update({base: [o, o + 1, o + e + 1], base + 1: [o + 2, o + e + 3], base + 2: [o + 3, o + e + 5]})
    if g.keys == 128:
        bins[mid + 3] = [62, 63, 64, 65]  # the seam between the two waves of the bin-local scan
    return [bn * g.keys + l for bn in sorted(bins) for l in bins[bn]]


def ladder(g):
    """two entries per bucket, one to three non-zero digits per scalar"""
    want, out, j = [b for b in ladder_buckets(g) for _ in range(2)], [], 0
    while want:
        k = (1, 1, 2, 1, 1, 3)[j % 6]
        take, want = want[:k], want[k:]
        w0 = (5 * j) % (g.nwin - 4)
        out.append(W.scalar_from_digits([0] * w0 + sum((_digit(g, b) for b in take), []), g.c))
        j += 1
    return out


def _digit(g, b):
    """the digits that put one entry into bucket b: b + 1, or for bucket nb - 1 the digit -2^(c-1) and its carry (bucket 0)"""
    return [b + 1] if b + 1 < g.nb else [-g.nb, 1]


def seam_counts(targets=SEAM_SLOTS):
    """entries per bucket so that consecutive buckets from position 0 have `targets` slots"""
    s, out = 0, []
    for t in targets:
        cnt = next(k for k in range(1, 16 * t + 2) if W.slot_count(s, k) == t)
        out.append(cnt + 3)  # (not the least count: the slot count holds for a few more)
        assert W.slot_count(s, out[-1]) == t
        s += out[-1]
    return out


SEAM_BUCKETS = (1000, 1001, 3000, 3001)


def seam(g):
    out = []
    for b, cnt in zip(SEAM_BUCKETS, seam_counts()):
        per = g.nwin - 1
        while cnt:
            k = min(per, cnt)
            out.append(W.scalar_from_digits([b + 1] * k, g.c))
            cnt -= k
    return out


def edge_buckets(g):
    return sorted(set([0, 255, 256, 257, g.nb - 256, g.nb - 1] + [256 * h + 255 for h in range(g.rows)]))


def edges(g):
    """one entry per bucket, every one over a base of its own; bucket nb - 1 is the digit -2^(c-1) (its carry: one more entry in bucket 0)"""
    out = []
    for j, b in enumerate(edge_buckets(g)):
        w = j % (g.nwin - 2)
        out.append(W.scalar_from_digits([0] * w + ([b + 1] if b + 1 < g.nb else [-g.nb, 1]), g.c))
    return out


def _pad(col, n):
    return list(col) + [0] * (n - len(col))


def _adjacent_pair(g, a, i, others, what):
    """A column whose scalars i and i + 1 are one equal single digit — two entries alone in their bucket, in ONE lane — over
    random scalars elsewhere; the digit is searched for (the bucket must not start on a lane's last entry)."""
    for d in range(777, 900):
        col = list(others)
        col[i] = col[i + 1] = W.scalar_from_digits([0, 0, d], g.c)
        m = W.Column(g, a, col)
        if m.totals[d - 1] == 2 and m.bstart[d - 1] % W.WL != W.WL - 1:
            return col
    raise AssertionError("no digit for the %s column" % what)


def _pass(basis, ident, t1, kinds, cols):
    n = len(cols[0])
    assert all(len(c) == n for c in cols) and len(cols) == len(kinds) <= MAX_BATCH
    may = ident == 1 or (ident == 2 and 0 in bases()[basis][:])
    return W.Dump(basis=basis, n=n, ident=ident, t1=t1, may=may, kinds=tuple(kinds), cols=[list(c) for c in cols])


@functools.lru_cache(maxsize=None)
def passes(c, S):
    """The sequence of passes of geometry (c, S).  Pass widths in order: 3 1 3 | 1 2 1 1 3 | 2 empty 2 | ..."""
    g, rng = W.Geo(c, S), random.Random(1000 * c + S.bit_length())
    rand = lambda n: [rng.randrange(R) for _ in range(n)]
    mc = {name: cops.fr_ints(arr[:1100]) for name, arr in MC.columns(c, 11) if name in ("mix", "bool", "top", "sparse")}
    ob, hv, n1 = one_bucket_scalar(c), MC.halves_scalar(c), one_bucket_n(c)
    lad, sm, ed = ladder(g), seam(g), edges(g)
    nd = max(len(lad), len(sm), len(ed))
    b1, b2 = bases()[1], bases()[2]
    others = [0] * 4 + rand(28)
    t = rng.randrange(1, R)
    degenerate = [_adjacent_pair(g, b1, 0, others, "equal"), _adjacent_pair(g, b1, 2, others, "opposite"), _pad([t, R - t], 32)]
    dk = ("equal points", "opposite points", "identity sum")
    out = [
        _pass(0, 0, 0, ("random", "mix", "bool"), [rand(1100), mc["mix"], mc["bool"]]),          # 3: a long pass ...
        _pass(0, 0, 0, ("random",), [rand(17)]),                                                  # 1: ... followed by n = 17
        _pass(0, 0, 1, ("top", "sparse", "zero"), [mc["top"], mc["sparse"], [0] * 1100]),         # 3
        _pass(0, 0, 0, ("random",), [rand(1)]),                                                   # 1
        _pass(0, 0, 0, ("random", "zero"), [rand(15), [0] * 15]),                                 # 2
        _pass(0, 0, 1, ("random",), [rand(16)]),                                                  # 1
        _pass(0, 0, 0, ("random",), [rand(255)]),                                                 # 1
        _pass(0, 0, 0, ("one bucket", "halves", "zero"), [[ob] * n1, [hv] * n1, [0] * n1]),       # 3
        _pass(0, 0, 0, ("one bucket", "halves"), [[ob] * (n1 + 1), [hv] * (n1 + 1)]),             # 2
        _pass(0, 0, 0, ("empty", "empty"), [[], []]),                                             # empty
        _pass(0, 0, 0, ("random", "zero"), [rand(257), [0] * 257]),                               # 2
        _pass(0, 0, 0, ("random",), [rand(256)]),
        _pass(0, 0, 1, ("one bucket", "halves"), [[ob] * 640, [hv] * 640]),
        _pass(0, 0, 0, ("one bucket",), [[ob] * 640]),
        _pass(0, 0, 0, ("random",), [rand(1023)]),
        _pass(0, 0, 1, ("random",), [rand(1024)]),
        _pass(0, 0, 0, ("random",), [rand(1025)]),
        _pass(0, 0, 1, ("ladder", "seam", "edges"), [_pad(lad, nd), _pad(sm, nd), _pad(ed, nd)]),
        _pass(0, 1, 0, ("ladder", "seam", "edges"), [_pad(lad, nd), _pad(sm, nd), _pad(ed, nd)]),
        _pass(0, 0, 0, ("ladder",), [lad]),
        _pass(1, 0, 0, dk, degenerate),   # unchecked: the lanes with the equal / opposite pair are listed and redone
        _pass(1, 1, 0, dk, degenerate),   # checked
        _pass(1, 2, 1, dk, degenerate),   # as msm_bases_have_identity says: unchecked, per-bucket T1, redone by parts
        _pass(1, 0, 0, ("random",), [rand(32)]),
        _pass(2, 2, 0, ("random", "ladder"), [rand(128), _pad(lad, 128)]),  # a basis with identity points: checked
        _pass(2, 1, 1, ("random",), [rand(128)]),
        _pass(0, 0, 0, ("empty",), [[]]),
    ]
    if S == 1 << 12:
        out += [_pass(0, 0, 0, ("random",), [rand(4096)]), _pass(0, 0, 0, ("random",), [rand(17)])]  # full length, then short
    return tuple(out)


@functools.lru_cache(maxsize=None)
def basis_points(basis):
    """the affine Montgomery image of [a_i] G for a basis of bases(); the identity is (0, 0)"""
    a = bases()[basis]
    pts = cops.fixed_base_g1(cops.fr_mont(a))
    pts[[i for i, k in enumerate(a) if k == 0]] = 0
    return pts


def write_case_file(path, geometries=GEOMETRIES):
    words = [np.array([W.MAGIC_IN, len(bases()), len(geometries)], dtype=np.uint32)]
    for b, a in enumerate(bases()):
        words += [np.array([len(a)], dtype=np.uint32), np.ascontiguousarray(basis_points(b)).view(np.uint32).reshape(-1)]
    for c, S in geometries:
        ps = passes(c, S)
        words.append(np.array([c, S, MAX_BATCH, len(ps)], dtype=np.uint32))
        for p in ps:
            words.append(np.array([p.basis, p.n, len(p.cols), p.ident, p.t1], dtype=np.uint32))
            if p.n:
                words.append(cops.fr_mont([s for col in p.cols for s in col]).view(np.uint32).reshape(-1))
    np.concatenate(words).tofile(path)


def simulate(c, S, order_seed, only=None):
    """every pass (or the passes `only`) of a geometry through the model's pipeline -> the parsed dump of geometry 0"""
    g, rec, late, par, enc = W.Geo(c, S), [], [], 0, W.Encoder(order_seed)
    for pi, p in enumerate(passes(c, S)):
        if only is not None and pi not in only:
            continue
        r, l, par = W.simulate_pass(g, bases()[p.basis], p, 0, pi, order_seed + pi, par, enc)
        rec += r
        late += l
    enc.resolve()
    return W.parse_results(W.records_to_array(rec + W.finish_pass(enc, late)))[0]
