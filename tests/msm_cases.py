"""The MSM case set, shared by tests/test_gpu_msm_wide.py, tests/test_gpu_msm_plans.py and their CPU-side checks
(tests/test_msm_cases.py, tests/test_msm_plan.py):

  * the column builders: the scalar distributions at which bucket methods go wrong, parametrised by the window bits;
  * a plain restatement of the plan rules of csrc/msm_plan.h (which window, which path, which sort, how the bit sums are split,
    how wide a pass may be) — written from the rules' description, compared line for line with the header's own answers by
    tests/msm_plan_check.cpp;
  * the grid of tests/test_gpu_msm_plans.py as data, and the branch classes each of its cases reaches.

No GPU, no engine: numpy and the oracle only."""
import random

import numpy as np

from zkoracle import cops, field as F, srs

# --------------------------------------------------------------------------- columns ---


def rand_col(rng, n):
    """n stored words below 2^252 (< r: valid Montgomery residues of uniformly distributed scalars)."""
    a = np.frombuffer(rng.bytes(n * 32), dtype=np.uint64).reshape(n, 4).copy()
    a[:, 3] &= 0x0FFFFFFFFFFFFFFF
    return a


def tau_commit(a):
    """[sum a_i tau^i] G1 of the seed-generated SRS (the tau-oracle), for a column of stored words."""
    return srs.g1_of_scalar(srs.commit_scalar_monomial(cops.fr_ints(a)))


def constant_tau_commit(s, n):
    """the tau-oracle of the column [s] * n in closed form: s (tau^n - 1) / (tau - 1)"""
    return srs.g1_of_scalar(s * (pow(srs.TAU, n, F.R) - 1) % F.R * F.inv((srs.TAU - 1) % F.R, F.R) % F.R)


def ones_scalar(bits):
    """every digit of the scalar 1: ALL entries of a column of it fall in one bucket"""
    return sum(1 << (bits * w) for w in range(250 // bits))


def halves_scalar(bits):
    """every raw digit 2^(bits - 1): the recoded digit is -2^(bits - 1) with a carry into every window"""
    return sum((1 << (bits - 1)) << (bits * w) for w in range(250 // bits))


SPARSE_VALUES = [1, 40000, (3 << 16) | 7, (12345 << 32) | (65535 << 16) | 200, (1 << 253) | (9 << 128), F.R - 2]
LAST_POINT_WORD = (1 << 252) - 1  # the stored word; as a scalar (word / 2^256 mod r) its digit is non-zero in every window of 9 .. 17 bits
LAST_POINTS = 5
COLUMN_NAMES = ("random", "zero", "hot16", "mix", "bool", "top", "sparse", "ones", "halves")


def columns(bits, k, np_seed=None, py_seed=None):
    """The nine columns of test_wide_commit_matches_tau_oracle, in its order, as (name, stored words) pairs; the generators are
    seeded and drawn from exactly as that test always did (1000 bits + k and k), so the values are the ones it always used."""
    n = 1 << k
    rng = np.random.default_rng(1000 * bits + k if np_seed is None else np_seed)
    cols = [rand_col(rng, n) for _ in range(5)]
    cols[1][:] = 0                                   # the zero column: the identity
    cols[2][:, 1:] = 0                               # 16-bit values: one window, a few hot buckets
    cols[2][:, 0] &= 0xFFFF
    cols[2][::3] = 0
    pr = random.Random(k if py_seed is None else py_seed)
    mix = []                                         # the advice-column mix of SURVEY.md 8d
    for _ in range(n):
        u = pr.random()
        mix.append(pr.randrange(1 << 18) if u < 0.4 else pr.randrange(1 << 88) if u < 0.75 else pr.randrange(F.R) if u < 0.9 else 0)
    mixm = cops.fr_mont(mix)
    boolc = cops.fr_mont([pr.randrange(2) for _ in range(n)])   # one giant bucket
    top = cops.fr_mont([F.R - 1 - pr.randrange(3) for _ in range(n)])  # largest scalars: every window's top digits, carries
    # a handful of distinct digits: non-empty buckets hundreds apart and whole coarse bins empty — every first-of-bucket entry
    # takes the escape of the lanes' bucket tracking (distance field saturated / first bucket of a bin)
    vals = SPARSE_VALUES
    sparse = cops.fr_mont([vals[pr.randrange(len(vals))] if pr.random() < 0.7 else 0 for _ in range(n)])
    # every digit of every scalar the same: ALL nwin n entries of the column in one bucket (one bin, one bucket, every
    # accumulation lane a slot of it, thousands of parts); and the digit 2^(bits - 1) throughout (with a carry into every window)
    ones = cops.fr_mont([ones_scalar(bits)] * n)
    halves = cops.fr_mont([halves_scalar(bits)] * n)
    return list(zip(COLUMN_NAMES, cols[:3] + [mixm, boolc, top, sparse, ones, halves]))


def last_points(n, seed):
    """Random, with the last five stored words 2^252 - 1, as test_wide_commit_at_the_24_bit_index_boundary has them (every digit of
    every window non-zero, tests/test_msm_cases.py): the highest table indexes w * stride + n - 1 .. of every window are entries."""
    a = rand_col(np.random.default_rng(seed), n)
    m = min(LAST_POINTS, n)
    a[n - m:] = cops.ints_to_arr([LAST_POINT_WORD])[0]
    return a


def small18(n, seed):
    """lookup-table-like: 18-bit values (two windows at most, hot low buckets)"""
    a = rand_col(np.random.default_rng(seed), n)
    a[:, 1:] = 0
    a[:, 0] &= 0x3FFFF
    return a


EDGE_SCALARS = [0, 1, F.R - 1, 2, (1 << 128) - 1, 1 << 253]


def edge_head(a):
    """rows 0 .. 5 of `a` replaced by the edge scalars of test_msm_matches_oracle"""
    a = a.copy()
    a[:len(EDGE_SCALARS)] = cops.fr_mont(EDGE_SCALARS)
    return a


# ---------------------------------------------------------------- the plan, restated ---
# From the description of the rules (include/zkmi355.h), not from the header's code.

MAX_BATCH = 256
LDS_BUCKETS = 8192
COARSE_BINS_MAX = 256
SPLIT_MAX = 4
WS_MIN = 1024
SORT2_MIN_N = 1 << 18
PLAN_LOG_N = range(0, 27)
PLAN_OVERRIDES = (0,) + tuple(range(9, 18))
PLAN_WIDTHS = (0, 1, 3, 256)


def windows(c):
    """windows of c bits that cover a 254-bit scalar and the carry out of its top digit"""
    return 254 // c + 1


def is_wide(c, stride):
    """15 .. 17-bit windows whose table indexes fit 26 bits and whose coarse bins (buckets / 2^fine bits) number 512 at most"""
    if not 15 <= c <= 17 or stride == 0:
        return False
    ib = max(24, (windows(c) * stride - 1).bit_length())
    if ib > 26:
        return False
    fb = min(7, 31 - ib)
    return (1 << (c - 1)) >> fb <= 512


def fixed_window(n, override=0):
    lg = n.bit_length() - 1
    if override:
        c = override
    elif lg >= 22:
        c = 15
    elif lg >= 16:
        c = 16
    else:
        c = lg - 5
    c = min(max(c, 9), 17)
    while c > 15 and not is_wide(c, n):
        c -= 1
    if c >= 15 and n < WS_MIN:
        c = 14
    return c


def generic_window(n):
    lg = n.bit_length() - 1
    if lg >= 21:
        c = 15
    elif lg >= 19:
        c = min(lg - 6, 14)
    elif lg >= 16:
        c = 12
    else:
        c = lg - 5
    return max(c, 9)


def ws_len(n):
    return max(WS_MIN, 1 << max(n - 1, 0).bit_length())


def split_of(nb):
    return min(SPLIT_MAX, max(1, nb // 1024))


def plan(mode, n, override=0, width=0, length=None):
    """What the engine does with an MSM of `length` scalars (default n): mode "fixed" over a resident SRS of n points under
    ZK_OPT_MSM_WINDOW = override and ZK_OPT_MSM_BATCH = width, mode "generic" over n arbitrary bases."""
    length = n if length is None else length
    if mode == "generic":
        c = generic_window(ws_len(n))
        nb = 1 << (c - 1)
        return dict(c=c, nwin=windows(c), nb=nb, wide=False, fused=False, sort2=False, percol=False, split=split_of(nb),
                    sweeps=-(-nb // LDS_BUCKETS), pass_max=1, split_capped=nb // 1024 > SPLIT_MAX)
    c = fixed_window(n, override)
    nb, nwin = 1 << (c - 1), windows(c)
    wide = is_wide(c, n) and n == ws_len(n)
    fused = not wide and nb <= LDS_BUCKETS
    sort2 = fused and length >= SORT2_MIN_N and nwin * n <= 1 << 24 and 64 <= nb <= 64 * COARSE_BINS_MAX
    percol = fused and not sort2 and length >= 1 << 18
    asked = width if width else max(1, (1 << 20) // max(n, 1))
    asked = min(asked, MAX_BATCH)
    return dict(c=c, nwin=nwin, nb=nb, wide=wide, fused=fused, sort2=sort2, percol=percol, split=split_of(nb),
                sweeps=0 if wide or fused else -(-nb // LDS_BUCKETS), pass_max=asked if wide or fused else 1,
                split_capped=nb // 1024 > SPLIT_MAX)


def plan_line(mode, lg, override, width):
    p = plan(mode, 1 << lg, override, width)
    return (f"{mode} lg={lg} ov={override} req={width} c={p['c']} nwin={p['nwin']} nb={p['nb']} wide={int(p['wide'])} "
            f"fused={int(p['fused'])} sort2={int(p['sort2'])} percol={int(p['percol'])} split={p['split']} sweeps={p['sweeps']} "
            f"pass={p['pass_max']}")


def plan_lines():
    out = []
    for lg in PLAN_LOG_N:
        for ov in PLAN_OVERRIDES:
            for w in PLAN_WIDTHS:
                out.append(plan_line("fixed", lg, ov, w))
    for lg in PLAN_LOG_N:
        out.append(plan_line("generic", lg, 0, 0))
    return out


# -------------------------------------------------------------------------- the grid ---
# tests/test_gpu_msm_plans.py runs exactly these; tests/test_msm_cases.py checks that they reach every branch class.

A_BITS = (9, 10, 11, 12, 13, 14)
A_KS = (10, 13)
A_SINGLE_ORDER = ("random", "zero", "sparse", "ones", "zero", "random", "hot16", "mix", "bool", "top", "halves", "last")

# (k, bits): long columns on the standard plan; three columns each, ZK_OPT_MSM_BATCH = 3 where the default pass is narrower
B_CASES = ((18, 9), (18, 14), (19, 13), (19, 9), (20, 13))
B_COLUMNS = 3
B_SRS_LENGTHS = {(19, 13): ((1 << 18) - 1, 1 << 18, (1 << 18) + 1, (1 << 19) - 1)}

C_K = 10
C_COUNTS = (1, 255, 256, 257, 300)          # default window, default width
C_WIDTH_COLUMNS = 70
C_WIDTHS = (1, 3, 7)
C_WIDE = ((10, 15, 11, (1, 5)), (16, 0, 11, (1, 5)))  # (k, ZK_OPT_MSM_WINDOW, columns, widths)
C_WIDE_FULL = (10, 15, 257)                 # (k, bits, columns) at the default width
C_REGROW = (3, 16, 2)                       # widths in sequence on a FRESH context (k = 10): its lane's first workspace is 3 wide
C_REGROW_COLUMNS = 20                       # per call: at width 16 a full 16-column pass comes right after the 3-wide ones

D_K = 12
D_LENGTHS = (1, 2, 1000, (1 << 12) - 1)
D_BATCH = 4
D_WIDE = (16, (1 << 16) - 3)

E_BITS = (11, 14)
E_K = 10

F_LENGTHS = (1 << 16, 1 << 17, (1 << 16) + 1, (1 << 20) - 1, 1 << 20, 1 << 21)
F_HALVES_AT = 1 << 21


def b_width(k):
    """ZK_OPT_MSM_BATCH of a block-B case: 0 where the default pass takes the three columns"""
    return 0 if (1 << 20) >> k >= B_COLUMNS else B_COLUMNS


def grid():
    """Every case of the GPU grid as (block, mode, n, override, width, length, columns-per-call)."""
    g = []
    for bits in A_BITS:
        for k in A_KS:
            g.append(("A", "fixed", 1 << k, bits, 0, 1 << k, 1))
            g.append(("A", "fixed", 1 << k, bits, 0, 1 << k, 10))
    for k, bits in B_CASES:
        g.append(("B", "fixed", 1 << k, bits, b_width(k), 1 << k, 1))
        g.append(("B", "fixed", 1 << k, bits, b_width(k), 1 << k, B_COLUMNS))
        for m in B_SRS_LENGTHS.get((k, bits), ()):
            g.append(("B", "fixed", 1 << k, bits, b_width(k), m, 1))
    for cnt in C_COUNTS:
        g.append(("C", "fixed", 1 << C_K, 0, 0, 1 << C_K, cnt))
    for w in C_WIDTHS:
        g.append(("C", "fixed", 1 << C_K, 0, w, 1 << C_K, C_WIDTH_COLUMNS))
    for k, bits, cnt, widths in C_WIDE:
        for w in widths:
            g.append(("C", "fixed", 1 << k, bits, w, 1 << k, cnt))
    g.append(("C", "fixed", 1 << C_WIDE_FULL[0], C_WIDE_FULL[1], 0, 1 << C_WIDE_FULL[0], C_WIDE_FULL[2]))
    for w in C_REGROW:
        g.append(("C-regrow", "fixed", 1 << C_K, 0, w, 1 << C_K, C_REGROW_COLUMNS))
    for m in D_LENGTHS:
        g.append(("D", "fixed", 1 << D_K, 0, 0, m, 1))
        g.append(("D", "fixed", 1 << D_K, 0, 0, m, D_BATCH))
    g.append(("D", "fixed", 1 << D_WIDE[0], 0, 0, D_WIDE[1], 1))
    for bits in E_BITS:
        g.append(("E", "fixed", 1 << E_K, bits, 0, 1 << E_K, 1))
        g.append(("E", "fixed", 1 << E_K, bits, 0, 1 << E_K, 2))
    for n in F_LENGTHS:
        g.append(("F", "generic", n, 0, 0, n, 1))
    return g


BRANCH_CLASSES = (
    tuple(f"fixed window {b}" for b in A_BITS)
    + ("split 1", "split 2", "split 4", "split capped at 4", "sort2 on, n >= 2^18", "sort2 off, n >= 2^18", "per-column scatter",
       "n < stride", "n = stride", "one pass", "several passes", "a 256-column pass", "generic window 12", "generic window 14",
       "generic window 15, two sweeps", "generic n below its workspace", "workspace regrown", "wide pass"))


def lane_events(cases, min_cols=0, slot=None):
    """What the lane's fixed-base workspace does for each MSM of `cases` in turn, restating get_msm_ws: the workspace is keyed by
    (length, window) and holds max(pass width asked for, min_cols) columns, capped by the plan; a call that needs more columns than
    the slot has destroys it and makes a wider one ("regrown"), one that needs fewer keeps it.  `slot` is the (length, window,
    columns) the lane holds before the first case: None on a fresh context — on a used one it is whatever the widest earlier
    MSM left, 256 columns after a single default-width commit at k = 10, and nothing regrows."""
    out = []
    for block, mode, n, override, width, length, cols in cases:
        p = plan(mode, n, override, max(width if width else max(1, (1 << 20) // n), min_cols))
        need = (ws_len(n), p["c"], p["pass_max"])
        if slot is None:
            out.append("created")
        elif slot[:2] != need[:2]:
            out.append("replaced")
        elif slot[2] < need[2]:
            out.append("regrown")
        else:
            out.append("kept")
            need = slot
        slot = need
    return out


def classes_of(case, lane_event=None):
    """the branch classes one grid case reaches, by the restated plan; `lane_event` is what lane_events says of the case"""
    block, mode, n, override, width, length, cols = case
    p = plan(mode, n, override, width, length)
    out = set()
    if mode == "generic":
        out.add(f"generic window {p['c']}" + (", two sweeps" if p["sweeps"] == 2 else ""))
        if n != ws_len(n):
            out.add("generic n below its workspace")
        return out
    if p["wide"]:
        out.add("wide pass")
    else:
        out.add(f"fixed window {p['c']}")
        out.add("split capped at 4" if p["split_capped"] else f"split {p['split']}")
        if p["split"] == 4:
            out.add("split 4")
        if length >= 1 << 18:
            out.add("sort2 on, n >= 2^18" if p["sort2"] else "sort2 off, n >= 2^18")
        if p["percol"] and cols > 1:
            out.add("per-column scatter")
    out.add("n < stride" if length < n else "n = stride")
    passes = -(-cols // p["pass_max"])
    out.add("one pass" if passes == 1 else "several passes")
    if cols >= MAX_BATCH and p["pass_max"] == MAX_BATCH:
        out.add("a 256-column pass")
    if lane_event == "regrown":
        out.add("workspace regrown")
    return out
