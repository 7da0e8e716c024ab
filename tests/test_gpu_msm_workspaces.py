"""GPU parity for MSM workspaces of DIFFERENT plans succeeding each other on one context's lanes.  A workspace is made for one
plan and holds that plan's buffers only (csrc/msm_plan.h msm_ws_layout; bounds proven on the host by tests/msm_plan_check.cpp):
wide over the resident SRS, standard fixed-base, standard for arbitrary bases.  One engine goes through wide (15 bits), a wider
wide workspace, arbitrary bases beside it, the SRS again, standard fused (13 bits), wide (16 bits: 32 768 buckets, 256 coarse
bins) and the defaults at 2^10.  Every result is compared with the tau-oracle after affine normalisation, and every step asserts
the plan it claims through zk_srs_msm_plan and the pass / column / wide-tail counters, as tests/test_gpu_msm_plans.py does."""
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_cases as MC  # noqa: E402
from zkoracle import cops  # noqa: E402

pytestmark = pytest.mark.gpu

K = 12
GENERIC_N = 1500  # a generic workspace of 2048


@contextmanager
def counted(eng, passes, columns, wide):
    """the MSM passes and columns the block runs, and how many of the passes took the wide path (ZK_T_MSM_TAIL counts those only)"""
    from webauthn_halo2_amd import engine as E

    which = (E.ZK_T_MSM, E.ZK_T_MSM_COLUMNS, E.ZK_T_MSM_TAIL)
    before = [eng.timer_stats(w)[1] for w in which]
    yield
    after = [eng.timer_stats(w)[1] for w in which]
    assert [a - b for a, b in zip(after, before)] == [passes, columns, wide]


def affine(row):
    return cops.affine_arr_to_ints(np.asarray(row).reshape(1, 8))[0]


@pytest.fixture(scope="module")
def cases():
    """eight columns of 2^12 (random, zero, last points, 18-bit values, random ...) and three of 2^10, with their tau-oracles"""
    def make(k, count, seed):
        n = 1 << k
        rng = np.random.default_rng(seed)
        cols = [MC.rand_col(rng, n) for _ in range(count)]
        cols[1][:] = 0
        cols[2] = MC.last_points(n, seed + 1)
        if count > 3:
            cols[3] = MC.small18(n, seed + 2)
        return cols, [MC.tau_commit(d) for d in cols]

    generic = MC.edge_head(MC.last_points(GENERIC_N, 0xAB))
    return {"k12": make(K, 8, 0x5712), "k10": make(10, 3, 0x5710), "generic": (generic, MC.tau_commit(generic))}


def single_and_batched(eng, data, want, wide, tag):
    """every column alone, then the first three in one pass on both bases"""
    n = len(data[0])
    polys = [eng.poly(n, d) for d in data[:3]]
    w = 1 if wide else 0
    with counted(eng, 3, 3, 3 * w):
        for j, p in enumerate(polys):
            assert affine(eng.commit(p, 0)) == want[j], (tag, j)
    with counted(eng, 1, 3, w):
        got = eng.commit_batch(polys, 0)
    for j in range(3):
        assert affine(got[j]) == want[j], (tag, "batch", j)
    with counted(eng, 1, 3, w):
        gl = eng.commit_batch(polys, 1)
    with counted(eng, 3, 3, 3 * w):
        for j, p in enumerate(polys):
            assert (gl[j] == eng.commit(p, 1)).all(), (tag, "lagrange", j)
    # commit_lagrange(v) == commit(iNTT(v))
    eng.lagrange_to_coeff(polys[0])
    assert (eng.commit(polys[0], 0) == gl[0]).all(), (tag, "intt")
    for p in polys:
        p.free()


def test_workspaces_of_different_plans_succeed_each_other(engine, cases):
    from webauthn_halo2_amd import engine as E

    eng = engine
    data, want = cases["k12"]
    n = 1 << K
    try:
        # 1. wide at 2^12 (15-bit windows), passes of three columns
        eng.set_option(E.ZK_OPT_MSM_WINDOW, 15)
        eng.set_option(E.ZK_OPT_MSM_BATCH, 3)
        eng.srs_setup(K)
        assert eng.srs_msm_plan() == (15, 17) and MC.plan("fixed", n, 15, 3)["wide"]
        single_and_batched(eng, data, want, True, "wide 15")
        # ... a wider pass: the lane's wide workspace is made again for eight columns and used at once
        eng.set_option(E.ZK_OPT_MSM_BATCH, 8)
        polys = [eng.poly(n, d) for d in data]
        with counted(eng, 1, 8, 1):
            got = eng.commit_batch(polys, 0)
        for j in range(8):
            assert affine(got[j]) == want[j], ("wide 15, eight columns", j)
        # 2. arbitrary bases: a generic workspace of 2048 beside the wide one
        bases = eng.srs_export(0, 0, n)
        a, want_a = cases["generic"]
        assert MC.plan("generic", GENERIC_N)["c"] == 9 and not MC.plan("generic", GENERIC_N)["wide"]
        with counted(eng, 1, 1, 0):
            assert cops.jac_to_affine_ints(eng.msm(a, bases[:GENERIC_N])) == want_a
        # 3. the SRS again: the wide workspace is still the lane's
        with counted(eng, 2, 9, 2):
            assert affine(eng.commit(polys[4], 0)) == want[4]
            again = eng.commit_batch(polys[::-1], 0)
        for j in range(8):
            assert affine(again[7 - j]) == want[j], ("wide 15 after arbitrary bases", j)
        with counted(eng, 1, 1, 0):
            assert cops.jac_to_affine_ints(eng.msm(a, bases[:GENERIC_N])) == want_a
        for p in polys:
            p.free()
        # 4. standard fused (13 bits): the lanes' workspaces are made again for another plan
        eng.set_option(E.ZK_OPT_MSM_WINDOW, 13)
        eng.srs_setup(K)
        p13 = MC.plan("fixed", n, 13, 8)
        assert eng.srs_msm_plan() == (13, 20) and p13["fused"] and not p13["wide"]
        single_and_batched(eng, data, want, False, "fused 13")
        # 5. wide again, 16 bits: 32 768 buckets, 256 coarse bins
        eng.set_option(E.ZK_OPT_MSM_WINDOW, 16)
        eng.srs_setup(K)
        assert eng.srs_msm_plan() == (16, 16) and MC.plan("fixed", n, 16, 8)["wide"]
        single_and_batched(eng, data, want, True, "wide 16")
        # 6. the defaults at 2^10: standard, 9 bits, tables of 2^10
        eng.set_option(E.ZK_OPT_MSM_WINDOW, 0)
        eng.set_option(E.ZK_OPT_MSM_BATCH, 0)
        eng.srs_setup(10)
        assert eng.srs_msm_plan() == (9, 29) and not MC.plan("fixed", 1 << 10)["wide"]
        single_and_batched(eng, *cases["k10"], False, "defaults at 2^10")
    finally:
        eng.set_option(E.ZK_OPT_MSM_WINDOW, 0)
        eng.set_option(E.ZK_OPT_MSM_BATCH, 0)
        eng.srs_setup(10)
