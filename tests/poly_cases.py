"""The case set of the polynomial entry points (zk_eval, zk_eval_batch, zk_kate_division) and its references.  No GPU.

  geometry    a Python restatement of csrc/poly_plan.h: tests/test_poly_cases.py compares it line by line with what
              tests/poly_plan_check.cpp prints from the header, so a drift in either one is caught
  lengths     lengths_eval() and lengths_kd(): every length with the tag of the class it opens; classes_eval(n) and classes_kd(n)
              say, from the restatement alone, which classes a length reaches
  points      0, 1, r - 1, 2, roots of unity of order 8, 256 and 2048 (the Horner multipliers z^8, x^256, (z^8)^256 become one), a
              root whose order is the largest power of two dividing zk_eval's stride for that length, and three seeded random points
  vectors     random, max (every coefficient r - 1), zero, sparse (ones at both sides of every seam of the restatement: the value
              of a sparse polynomial is sum x^i by pow - a formula that shares nothing with any Horner chain)
  references  plain Python (zkoracle.prover) up to 2^13 coefficients, the C oracle (zkoracle.fastprover) above; the division
              identity p(x) = q(x) (x - z) + p(z)

Vectors are (n, 4) uint64 arrays of Montgomery words, as the engine stores them."""
import random

import numpy as np

from zkoracle import cops, fastprover as fp, prover
from zkoracle.field import R, omega

# ------------------------------------------------------------------------------------------- geometry (csrc/poly_plan.h) ---
EVAL_LANES, EVAL_PER_LANE, EVAL_MAX_BLOCKS, EVAL_SMALL_ELEMS = 256, 16, 1024, 2048 + 8
KD_L_MIN, KD_BLK, KD_TOP = 8, 256, 1024
KD_MAX_N = 1 << 26          # the longest division zk_kate_division accepts
EVAL_BATCH_PAIRS = 64       # pairs per launch of zk_eval_batch
EVAL_TABLE = 16             # distinct points whose powers one launch remembers
PLAIN_MAX = 1 << 13         # the plain-Python references serve up to here


def ceil_div(a, b):
    return -(-a // b)


def eval_blocks(n):
    return min(EVAL_MAX_BLOCKS, max(1, ceil_div(n, EVAL_LANES * EVAL_PER_LANE)))


def eval_stride(n):
    return eval_blocks(n) * EVAL_LANES


def eval_batch_per_lane(n):
    return ceil_div(n, eval_blocks(n) * EVAL_LANES)


def eval_batch_live(n, M, b):
    return min(EVAL_LANES, n - min(n, b * EVAL_LANES * M))


def eval_batch_workgroups(n):
    """(workgroups that hold a coefficient, live lanes of the last of them)"""
    M = eval_batch_per_lane(n)
    wg = ceil_div(n, EVAL_LANES * M)
    return wg, eval_batch_live(n, M, wg - 1)


def kd_len(n):
    L = KD_L_MIN
    while ceil_div(ceil_div(n, L), KD_BLK) > KD_TOP:
        L *= 2
    return L


def kd_shape(n):
    """(KD_L, chunks, blocks, scratch elements) of an n-coefficient division"""
    L = kd_len(n)
    m = ceil_div(n, L)
    nblk = ceil_div(m, KD_BLK)
    return L, m, nblk, 2 * m + 2 * nblk + KD_BLK


def plan_line(n):
    """the line tests/poly_plan_check.cpp prints for n"""
    wg, live = eval_batch_workgroups(n)
    L, m, nblk, scratch = kd_shape(n)
    return (f"n={n} blocks={eval_blocks(n)} S={eval_stride(n)} M={eval_batch_per_lane(n)} wg={wg} live={live} "
            f"L={L} m={m} nblk={nblk} scratch={scratch}")


# ------------------------------------------------------------------------------------------------------- the lengths ---
EVAL_CLASSES = ("one_workgroup", "several_workgroups", "M1", "M9", "M17", "ragged_live", "unequal_chains", "over_256_partials",
                "block_cap", "empty_workgroups", "over_18_blocks")
KD_CLASSES = ("single_chunk", "short_last_chunk", "m256", "m257", "single_chunk_last_block", "nblk2", "nblk256", "nblk257", "nblk1024",
              "L8_longest", "L16", "L32")


def classes_eval(n):
    """the classes an n-coefficient evaluation reaches, by the restatement"""
    blocks, M = eval_blocks(n), eval_batch_per_lane(n)
    wg, live = eval_batch_workgroups(n)
    span = n - (wg - 1) * EVAL_LANES * M  # coefficients of the last non-empty workgroup
    c = {"one_workgroup" if blocks == 1 else "several_workgroups"}
    if M in (1, 9, 17):
        c.add("M%d" % M)
    if live & (live - 1):
        c.add("ragged_live")  # the fold skips the levels s >= live: live is no power of two
    if span > EVAL_LANES and span % EVAL_LANES:
        c.add("unequal_chains")  # lanes of one workgroup with chains of different length
    if blocks > 256:
        c.add("over_256_partials")  # a second trip of the Horner loop of poly_sum_batch_kernel / of poly_sum_kernel's lanes
    if blocks == EVAL_MAX_BLOCKS:
        c.add("block_cap")
    if wg < blocks:
        c.add("empty_workgroups")
    if blocks > 18:
        c.add("over_18_blocks")  # (what zk_eval's older seven lengths stop short of)
    return c


def classes_kd(n):
    L, m, nblk, _ = kd_shape(n)
    c = set()
    if m == 1:
        c.add("single_chunk")
    if n % L:
        c.add("short_last_chunk")
    if m in (256, 257):
        c.add("m%d" % m)
    if nblk > 1 and m % KD_BLK == 1:
        c.add("single_chunk_last_block")
    if nblk in (2, 256, 257, 1024):
        c.add("nblk%d" % nblk)  # 257: a second table workgroup for tpow and a second trip of the G loop
    if L == 8 and n == 1 << 21:
        c.add("L8_longest")  # every bit of the tw.top exponents used
    if L in (16, 32):
        c.add("L%d" % L)
    return c


def lengths_eval():
    """(n, the class it opens) - every tag is among classes_eval(n) (tests/test_poly_cases.py)"""
    return [(1, "one_workgroup"), (2, "M1"), (100, "ragged_live"), (129, "ragged_live"), (255, "ragged_live"), (256, "M1"),
            (257, "unequal_chains"), (4095, "unequal_chains"), (4096, "one_workgroup"), (4097, "M9"), (4096 + 100, "several_workgroups"),
            (8193, "unequal_chains"), ((1 << 20) + 4097, "over_256_partials"), ((1 << 22) - 1, "block_cap"), (1 << 22, "block_cap"),
            ((1 << 22) + 1, "empty_workgroups")]


def lengths_kd():
    return [(1, "single_chunk"), (2, "single_chunk"), (7, "short_last_chunk"), (8, "single_chunk"), (9, "short_last_chunk"),
            (2041, "m256"), (2047, "short_last_chunk"), (2048, "m256"), (2049, "m257"), (4104, "single_chunk_last_block"),
            ((1 << 19) - 1, "nblk256"), ((1 << 19) + 1, "nblk257"), ((1 << 21) - 7, "nblk1024"), (1 << 21, "L8_longest"),
            ((1 << 21) + 1, "L16"), ((1 << 21) + 8, "short_last_chunk"), ((1 << 22) + 1, "L32")]


EVAL_SMALL = [n for n, _ in lengths_eval() if n <= 8193]
EVAL_LARGE = [n for n, _ in lengths_eval() if n > 8193]          # the four lengths from 2^20 up
KD_ALL_Z = [n for n, _ in lengths_kd() if n <= (1 << 19) + 1]    # z over every class
KD_FEW_Z = [n for n, _ in lengths_kd() if n > (1 << 19) + 1]     # z over {0, 1, w8, w2048, one random point}
# the runs under the stream audit: together they reach every class (tests/test_poly_cases.py)
AUDIT_EVAL = [100, 257, 4097, (1 << 20) + 4097, (1 << 22) + 1]
AUDIT_KD = [8, 9, 2048, 2049, (1 << 19) - 1, (1 << 19) + 1, 1 << 21, (1 << 21) + 1, (1 << 22) + 1]


# -------------------------------------------------------------------------------------------------------- the points ---
def stride_root(n):
    """a root of unity whose order is the largest power of two that divides zk_eval's stride S: its Horner multiplier x^S is one"""
    S = eval_stride(n)
    return omega((S & -S).bit_length() - 1)


def points(n, seed=0):
    """[(name, x)]: every class of point for an n-coefficient vector"""
    rng = random.Random(0x9017 + 31 * n + seed)
    return [("zero", 0), ("one", 1), ("minus_one", R - 1), ("two", 2), ("w8", omega(3)), ("w256", omega(8)), ("w2048", omega(11)),
            ("w_stride", stride_root(n))] + [("random%d" % i, rng.randrange(2, R - 1)) for i in range(3)]


def points_few_eval(n, seed=0):
    """the points of the four large evaluation lengths"""
    p = dict(points(n, seed))
    return [(k, p[k]) for k in ("zero", "one", "w_stride", "random0")]


def points_few_kd(n, seed=0):
    """the points of the long divisions"""
    p = dict(points(n, seed))
    return [(k, p[k]) for k in ("zero", "one", "w8", "w2048", "random0")]


def mont1(x):
    return cops.fr_mont([x % R])[0]


def mont_points(xs):
    return cops.fr_mont([x % R for x in xs])


# ------------------------------------------------------------------------------------------------------- the vectors ---
KINDS = ("random", "max", "zero", "sparse")


def random_rows(rng, n):
    """n stored words below 2^252 (< r: valid Montgomery residues of uniformly distributed values)"""
    a = np.frombuffer(rng.bytes(n * 32), dtype=np.uint64).reshape(n, 4).copy()
    a[:, 3] &= 0x0FFFFFFFFFFFFFFF
    return a


def seams(n):
    """The indexes of a sparse vector: 0, n - 1 and both sides of every seam of the restatement that lies inside [0, n)."""
    idx = {0, n - 1}

    def seam(i):  # i - 1 | i
        idx.update((i - 1, i))

    # zk_eval_batch: lane 255 | lane 0 of the next chain step in the first, a middle and the last non-empty workgroup; the first
    # and the last index of the last non-empty workgroup
    M = eval_batch_per_lane(n)
    per = EVAL_LANES * M
    wg, _ = eval_batch_workgroups(n)
    for b in sorted({0, wg // 2, wg - 1}):
        seam(b * per)
        seam(b * per + EVAL_LANES)
    # zk_eval: the first wrap of the stride, and the workgroup seam inside it
    seam(eval_stride(n))
    seam(EVAL_LANES)
    # the division: chunk seams of the first, a middle and the last chunk, block seams of the first, a middle and the last block
    L, m, nblk, _ = kd_shape(n)
    for t in sorted({1, m // 2, m - 1}):
        seam(t * L)
    for B in sorted({1, nblk // 2, nblk - 1}):
        seam(B * KD_BLK * L)
    return sorted(i for i in idx if 0 <= i < n)


def coefficients(n, kind, rng=None, base=None):
    """An n-coefficient vector of `kind`.  random: from `base` (rows of random words made once, at least n of them) when given,
    else from `rng` (a numpy generator; default: seeded by n)."""
    if kind == "random":
        if base is not None:
            return base[:n]
        return random_rows(rng if rng is not None else np.random.default_rng(0xC0EF + n), n)
    if kind == "max":
        return np.tile(mont1(R - 1), (n, 1))
    a = np.zeros((n, 4), dtype=np.uint64)
    if kind == "sparse":
        a[seams(n)] = mont1(1)
    elif kind != "zero":
        raise ValueError(kind)
    return a


def sparse_value(n, x):
    """the value at x of the sparse vector of length n: sum x^i, by pow"""
    return sum(pow(x, i, R) for i in seams(n)) % R


# ---------------------------------------------------------------------------------------------------- the references ---
def eval_ref(a, x):
    """a(x) as an integer: plain Python up to 2^13 coefficients, the C oracle above"""
    if a.shape[0] <= PLAIN_MAX:
        return prover.eval_poly(cops.fr_ints(a), x % R)
    return fp.eval_poly(np.ascontiguousarray(a), x % R)


def kd_ref(a, z):
    """(a - a(z)) / (X - z) as n stored words, the last one zero"""
    n = a.shape[0]
    if n <= PLAIN_MAX:
        q = prover.kate_division(cops.fr_ints(a), z % R) + [0]
        return cops.fr_mont(q) if n > 1 else np.zeros((1, 4), dtype=np.uint64)
    return fp.kate_division(np.ascontiguousarray(a), z % R)


def division_identity_holds(a, q, z, xs):
    """a(x) = q(x) (x - z) + a(z) at every x of xs, through the C oracle's evaluation"""
    a, q = np.ascontiguousarray(a), np.ascontiguousarray(q)
    az = fp.eval_poly(a, z % R)
    return all(fp.eval_poly(a, x) == (fp.eval_poly(q, x) * (x - z) + az) % R for x in xs)


# ---------------------------------------------------------------------------------------- pairs of one zk_eval_batch ---
def mixed_pairs(n_polys, pts):
    """[(polynomial index, point)]: every point with every polynomial, the polynomials rotating so that neighbours differ"""
    return [((i + j) % n_polys, x) for i, x in enumerate(pts) for j in range(n_polys)]


TABLE_COUNTS = (1, 16, 17, 18, 64, 65, 129, 130)


def table_points(seed):
    rng = random.Random(0x7AB1E + seed)
    return [rng.randrange(2, R - 1) for _ in range(20)]


def table_order():
    """40 uses of 20 distinct points (as indexes): the first 16 fill the launch's table of distinct points; points 16 .. 19 overflow
    it, each followed by the second use of a point that is in it (a hit behind a full table); then the other hits, then the second
    uses of the four that never got in (computed again)."""
    order = list(range(16))
    for k in range(4):
        order += [16 + k, k]
    return order + list(range(4, 16)) + list(range(16, 20))


def table_pairs(count, n_polys, pts):
    """`count` pairs over the 20 points of `pts`, walking table_order() from an offset that depends on the count, so that a slot of
    the staging never holds the same point in two calls of the matrix (a stale slot cannot stand in for a missing copy)."""
    order = table_order()
    return [((3 * i + count) % n_polys, pts[(order[i % len(order)] + count) % len(pts)]) for i in range(count)]
