"""tests/msm_cases.py on the CPU: the column builders give what they say (and what test_gpu_msm_wide.py always used), the
references agree with each other, and the GPU grid of tests/test_gpu_msm_plans.py reaches every branch class of the standard
plan.  No GPU."""
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_cases as MC  # noqa: E402
from zkoracle import cops, field as F, srs  # noqa: E402


def digits(s, c):
    """signed c-bit digits of s, as the kernels recode them (a raw digit above 2^(c-1) borrows from the next window)"""
    out, carry = [], 0
    for w in range(MC.windows(c)):
        raw = ((s >> (w * c)) & ((1 << c) - 1)) + carry
        carry = 1 if raw > 1 << (c - 1) else 0
        out.append(raw - (carry << c))
    assert carry == 0 and sum(d << (c * w) for w, d in enumerate(out)) == s
    return out


def test_columns_are_the_wide_tests_columns():
    """Same seeds, same draws, same values as the builder that lived in test_wide_commit_matches_tau_oracle."""
    bits, k = 16, 10
    n = 1 << k
    cols = dict(MC.columns(bits, k))
    assert tuple(cols) == MC.COLUMN_NAMES
    rng = np.random.default_rng(1000 * bits + k)
    first = np.frombuffer(rng.bytes(n * 32), dtype=np.uint64).reshape(n, 4).copy()
    first[:, 3] &= 0x0FFFFFFFFFFFFFFF
    assert np.array_equal(cols["random"], first)
    assert not cols["zero"].any()
    assert not cols["hot16"][:, 1:].any() and cols["hot16"][:, 0].max() <= 0xFFFF and not cols["hot16"][::3].any()
    pr = random.Random(k)
    mix = []
    for _ in range(n):
        u = pr.random()
        mix.append(pr.randrange(1 << 18) if u < 0.4 else pr.randrange(1 << 88) if u < 0.75 else pr.randrange(F.R) if u < 0.9 else 0)
    assert cops.fr_ints(cols["mix"]) == mix
    assert cops.fr_ints(cols["bool"]) == [pr.randrange(2) for _ in range(n)]
    assert cops.fr_ints(cols["top"]) == [F.R - 1 - pr.randrange(3) for _ in range(n)]
    assert set(cops.fr_ints(cols["sparse"])) <= set(MC.SPARSE_VALUES) | {0}
    assert cops.fr_ints(cols["ones"]) == [sum(1 << (16 * w) for w in range(15))] * n
    assert cops.fr_ints(cols["halves"]) == [sum(0x8000 << (16 * w) for w in range(15))] * n


def test_ones_and_halves_put_every_digit_in_one_bucket():
    for bits in range(9, 18):
        d = digits(MC.ones_scalar(bits), bits)
        assert set(d[:250 // bits]) == {1} and set(d[250 // bits:]) <= {0}
        h = digits(MC.halves_scalar(bits), bits)
        # raw 2^(bits-1) stays (it is not ABOVE the half), the bucket is the top one: |digit| = 2^(bits-1), the int16 edge at 15 / 16
        assert {abs(x) for x in h[:250 // bits]} == {1 << (bits - 1)}


def test_last_points_fill_every_window():
    a = MC.last_points(64, 5)
    v = cops.fr_ints(a)
    w = cops.arr_to_ints(a)
    assert w[-MC.LAST_POINTS:] == [MC.LAST_POINT_WORD] * MC.LAST_POINTS and w[-MC.LAST_POINTS - 1] != MC.LAST_POINT_WORD
    for bits in range(9, 18):
        assert all(d != 0 for d in digits(v[-1], bits)), bits
    assert cops.arr_to_ints(MC.last_points(3, 5)) == [MC.LAST_POINT_WORD] * 3
    e = cops.fr_ints(MC.edge_head(a))
    assert e[:6] == MC.EDGE_SCALARS and e[6:] == v[6:] and cops.fr_ints(a) == v
    s = MC.small18(100, 3)
    assert max(cops.arr_to_ints(s)) < 1 << 18


def test_tau_oracle_agrees_with_the_c_pippenger():
    """the two references of the GPU grid against each other, at a size both finish at once"""
    n = 64
    a = MC.edge_head(MC.last_points(n, 9))
    g = cops.fixed_base_g1(cops.fr_powers(srs.TAU, n))
    assert cops.jac_to_affine_ints(cops.msm(a, g)) == MC.tau_commit(a)
    assert MC.tau_commit(np.zeros((n, 4), dtype=np.uint64)) is None
    h = MC.halves_scalar(15)
    assert MC.constant_tau_commit(h, n) == MC.tau_commit(np.tile(cops.fr_mont([h]), (n, 1)))


def test_restated_plan_at_the_documented_points():
    assert [MC.fixed_window(1 << k) for k in (10, 14, 15, 16, 19, 21, 22, 24)] == [9, 9, 10, 16, 16, 16, 15, 15]
    assert [MC.generic_window(MC.ws_len(n)) for n in MC.F_LENGTHS] == [12, 12, 12, 14, 14, 15]
    assert MC.fixed_window(1 << 9, 16) == 14 and MC.fixed_window(1 << 10, 17) == 17
    assert MC.plan("fixed", 1 << 22, 0, 8)["pass_max"] == 1 and MC.plan("fixed", 1 << 19, 0, 8)["pass_max"] == 8
    assert MC.plan("fixed", 1 << 19, 13)["sort2"] and not MC.plan("fixed", 1 << 19, 13, length=(1 << 18) - 1)["sort2"]
    p = MC.plan("fixed", 1 << 20, 13)
    assert (p["nwin"], p["sort2"], p["percol"], p["split"]) == (20, False, True, 4)
    assert MC.plan("fixed", 1 << 19, 9)["nwin"] * (1 << 19) == 15204352 < 1 << 24


def test_grid_covers_every_branch_class():
    hit = {}
    # the regrow sequence runs on a context of its own, whose lane holds nothing before it
    regrow = [c for c in MC.grid() if c[0] == "C-regrow"]
    events = dict(zip(regrow, MC.lane_events(regrow)))
    assert list(events.values()) == ["created", "regrown", "kept"]
    for case in MC.grid():
        for cl in MC.classes_of(case, events.get(case)):
            hit.setdefault(cl, []).append(case)
    missing = [cl for cl in MC.BRANCH_CLASSES if cl not in hit]
    assert not missing, missing
    # and the particular cases the grid was built around
    assert ("B", "fixed", 1 << 18, 9, 0, 1 << 18, 3) in hit["sort2 on, n >= 2^18"]
    assert ("B", "fixed", 1 << 20, 13, 3, 1 << 20, 3) in hit["per-column scatter"]
    assert ("B", "fixed", 1 << 18, 14, 0, 1 << 18, 3) in hit["split capped at 4"]
    assert ("B", "fixed", 1 << 19, 13, 3, (1 << 18) - 1, 1) in hit["n < stride"]
    assert hit["workspace regrown"] == [("C-regrow", "fixed", 1 << 10, 0, 16, 1 << 10, 20)]
    # the same sequence behind one default-width commit (a shared context): the lane is 256 wide already and never regrows
    first = ("C", "fixed", 1 << 10, 0, 0, 1 << 10, 1)
    assert MC.lane_events([first] + regrow) == ["created", "kept", "kept", "kept"]
    assert MC.lane_events(regrow, min_cols=16) == ["created", "kept", "kept"]
    assert ("C", "fixed", 1 << 10, 0, 0, 1 << 10, 256) in hit["a 256-column pass"]
    assert ("C", "fixed", 1 << 10, 0, 7, 1 << 10, 70) in hit["several passes"]
    assert ("F", "generic", (1 << 16) + 1, 0, 0, (1 << 16) + 1, 1) in hit["generic n below its workspace"]
    assert ("F", "generic", 1 << 21, 0, 0, 1 << 21, 1) in hit["generic window 15, two sweeps"]
    # every standard-plan window of block A is reached at both SRS sizes, alone and batched
    for bits in MC.A_BITS:
        assert {(c[2], c[6]) for c in hit[f"fixed window {bits}"] if c[0] == "A"} == {(1 << k, m) for k in MC.A_KS for m in (1, 10)}
