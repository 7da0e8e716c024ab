"""zk_pairing_check_batch on an MI355X: one KZG pairing check per lane (csrc/pairing.hip) against verdicts known from scalars
(tests/pairing_cases.py: e([x] G1, [t] G2) = e([y] G1, G2) exactly when x t = y mod r).  Counts around the wave size with holding
and non-holding pairs in every wave; one holding pair at lanes 0, 63 and 64; the reasons of improper G1 points and the identity
cases; reasons = NULL; every argument error with untouched outputs; the resident SRS's pair and its cached table across
zk_srs_update and zk_srs_downsize; one call under ZK_OPT_STREAM_AUDIT; one call of ZK_PAIRING_BATCH_MAX pairs (every other launch
is 130 pairs at the most); contexts that share an SRS, across zk_srs_set_g2 and the parent's end.  The values behind the verdicts
are tests/test_gpu_pairing_device.py's.
"""
import ctypes
import random

import numpy as np
import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
import pairing_cases as pc
from zkoracle import curve, field as F

pytestmark = pytest.mark.gpu

T = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % F.R  # x t wraps mod r for almost every x
G2W = pc.g2_to_words(curve.G2_GEN)


@pytest.fixture(scope="module")
def eng():
    e = zk.Engine(0)  # (no SRS, no key)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pool():
    """130 (x, y) pairs against s_g2 = [T] G2 with their limb rows and expected verdicts, made once"""
    xy = pc.mixed_pairs(130, T, 41)
    return {"a": pc.g1_words([pc.g1(x) for x, _ in xy]), "b": pc.g1_words([pc.g1(y) for _, y in xy]), "want": [pc.holds(x, y, T) for x, y in xy],
            "s_g2": pc.g2_to_words(pc.g2(T))}


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_counts_around_the_wave(eng, pool, count):
    want = pool["want"][:count]
    if count > 1:
        assert set(want[:64]) == {True, False}
    if count == 130:
        assert set(want[64:128]) == {True, False} and set(want[128:]) == {True, False}  # (the third wave holds two pairs)
    verdicts, reasons = eng.pairing_check_batch(pool["a"][:count], pool["b"][:count], G2W, pool["s_g2"])
    assert verdicts == want
    assert reasons == [pc.VALID if w else pc.MISMATCH for w in want]


@pytest.mark.parametrize("lane", [0, 63, 64])
def test_one_holding_pair_among_others(eng, pool, lane):
    bad = [i for i, w in enumerate(pool["want"]) if not w]
    good = pool["want"].index(True, 3)
    idx = [bad[j % len(bad)] for j in range(65)]
    idx[lane] = good
    verdicts, _ = eng.pairing_check_batch(pool["a"][idx], pool["b"][idx], G2W, pool["s_g2"])
    assert verdicts == [j == lane for j in range(65)]


def test_s_g2_equal_to_g2(eng):
    rnd = random.Random(5)
    xs = [1, F.R - 1, rnd.randrange(2, F.R)]
    a = pc.g1_words([pc.g1(x) for x in xs] + [pc.g1(xs[2])])
    b = pc.g1_words([pc.g1(x) for x in xs] + [curve.neg(pc.g1(xs[2]))])
    assert eng.pairing_check_batch(a, b, G2W, G2W)[0] == [True, True, True, False]


def test_another_g2_base(eng):
    """g2 need not be the generator: e([x] G, [t v] G2) = e([x t] G, [v] G2)"""
    v, t, x = 0xABCDEF123456789, F.R - 3, 0x1234567
    a = pc.g1_words([pc.g1(x), pc.g1(x)])
    b = pc.g1_words([pc.g1(x * t), pc.g1(x * t + 1)])
    assert eng.pairing_check_batch(a, b, pc.g2_to_words(pc.g2(v)), pc.g2_to_words(pc.g2(t * v)))[0] == [True, False]


def test_reasons(eng, pool):
    s_g2 = pc.g2_to_words(pc.g2(7))
    ga, gb = pc.g1_words([pc.g1(3)])[0], pc.g1_words([pc.g1(21)])[0]
    zero = np.zeros(8, dtype=np.uint64)
    p_x = ga.copy()
    p_x[:4] = pc.p_words()  # a coordinate EQUAL to p
    one_one = pc.g1_words([(1, 1)])[0]
    cases = [(ga, gb, pc.VALID), (p_x, gb, pc.RANGE), (ga, pc.with_p_added(gb, 4), pc.RANGE), (one_one, gb, pc.OFF_CURVE), (ga, one_one, pc.OFF_CURVE),
             (one_one, pc.with_p_added(gb, 0), pc.RANGE),  # RANGE is reported before OFF_CURVE
             (zero, zero, pc.VALID), (zero, gb, pc.MISMATCH), (ga, zero, pc.MISMATCH), (ga, ga, pc.MISMATCH)]
    verdicts, reasons = eng.pairing_check_batch(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), G2W, s_g2)
    assert reasons == [c[2] for c in cases]
    assert verdicts == [c[2] == pc.VALID for c in cases]


def raw_call(eng, count, a, b, g2, s_g2, verdicts, reasons):
    u64p = ctypes.POINTER(ctypes.c_uint64)
    ptr = lambda v: ctypes.cast(None, u64p) if v is None else v.ctypes.data_as(u64p)
    return eng.L.zk_pairing_check_batch(eng.ctx, count, ptr(a), ptr(b), ptr(g2), ptr(s_g2), verdicts, reasons)


def test_reasons_may_be_null(eng, pool):
    verdicts = (ctypes.c_uint8 * 70)(*([7] * 70))
    a, b = np.ascontiguousarray(pool["a"][:70]), np.ascontiguousarray(pool["b"][:70])
    assert raw_call(eng, 70, a, b, G2W, pool["s_g2"], verdicts, None) == 0
    assert list(verdicts) == [int(w) for w in pool["want"][:70]]


def test_bad_arguments_leave_the_outputs_untouched(eng, pool):
    a, b, s_g2 = np.ascontiguousarray(pool["a"][:2]), np.ascontiguousarray(pool["b"][:2]), pool["s_g2"]
    verdicts, reasons = (ctypes.c_uint8 * 4)(*([0xA5] * 4)), (ctypes.c_uint8 * 4)(*([0x5A] * 4))
    u8p = ctypes.POINTER(ctypes.c_uint8)
    assert raw_call(eng, 0, a, b, G2W, s_g2, verdicts, reasons) == -1
    assert raw_call(eng, E.ZK_PAIRING_BATCH_MAX + 1, a, b, G2W, s_g2, verdicts, reasons) == -1  # (refused before a pair is read)
    assert raw_call(eng, 2, None, b, G2W, s_g2, verdicts, reasons) == -1
    assert raw_call(eng, 2, a, None, G2W, s_g2, verdicts, reasons) == -1
    assert raw_call(eng, 2, a, b, G2W, s_g2, ctypes.cast(None, u8p), reasons) == -1
    assert eng.L.zk_pairing_check_batch(None, 2, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), b.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                        None, None, verdicts, reasons) == -1
    assert raw_call(eng, 2, a, b, G2W, None, verdicts, reasons) == -1  # exactly one of the two
    assert raw_call(eng, 2, a, b, None, s_g2, verdicts, reasons) == -1
    # improper G2 points, in either place: a coordinate not below p, off the twist, outside the subgroup, the identity
    over = s_g2.copy()
    v = sum(int(over[q]) << (64 * q) for q in range(4)) + F.P
    over[:4] = [(v >> (64 * q)) & 0xFFFFFFFFFFFFFFFF for q in range(4)]
    off = s_g2.copy()
    off[0] ^= np.uint64(1)
    outside = pc.g2_to_words(pc.twist_point_outside_g2())
    for bad in (over, off, outside, np.zeros(16, dtype=np.uint64)):
        assert raw_call(eng, 2, a, b, G2W, bad, verdicts, reasons) == -1
        assert raw_call(eng, 2, a, b, bad, s_g2, verdicts, reasons) == -1
    assert raw_call(eng, 2, a, b, None, None, verdicts, reasons) == -5  # no SRS on this context
    assert list(verdicts) == [0xA5] * 4 and list(reasons) == [0x5A] * 4
    assert raw_call(eng, 2, a, b, G2W, s_g2, verdicts, reasons) == 0  # (the context works on)
    assert list(verdicts)[:2] == [int(w) for w in pool["want"][:2]] and list(verdicts)[2:] == [0xA5] * 2 and list(reasons)[2:] == [0x5A] * 2


def test_state_error_without_a_g2_half(pool):
    src, e = zk.Engine(0), zk.Engine(0)
    try:
        src.srs_setup(4, b"\x07" * 32)
        e.srs_load(4, src.srs_export(0, 0, 16), src.srs_export(1, 0, 16))  # an SRS without its G2 half
        verdicts, reasons = (ctypes.c_uint8 * 2)(*([0xA5] * 2)), (ctypes.c_uint8 * 2)(*([0x5A] * 2))
        a, b = np.ascontiguousarray(pool["a"][:2]), np.ascontiguousarray(pool["b"][:2])
        assert raw_call(e, 2, a, b, None, None, verdicts, reasons) == -5
        assert list(verdicts) == [0xA5] * 2 and list(reasons) == [0x5A] * 2
    finally:
        src.close()
        e.close()


def test_resident_pair_and_its_table_across_update_and_downsize():
    e = zk.Engine(0)
    try:
        e.srs_setup(5, b"\x11" * 32)
        g = e.srs_export(0, 0, 2)
        a, b = np.stack([g[0], g[0], g[1]]), np.stack([g[1], g[0], g[0]])  # e(g0, s_g2) = e(g1, g2) alone holds (tau is not 1 or -1)
        assert e.pairing_check_batch(a, b)[0] == [True, False, False]
        assert e.pairing_check_batch(a, b)[0] == [True, False, False]  # (the cached table)
        e.srs_update(b"\x22" * 32)
        g_new = e.srs_export(0, 0, 2)
        assert np.array_equal(g_new[0], g[0]) and not np.array_equal(g_new[1], g[1])
        # the old g[1] no longer holds and the new one does: the table of the old pair was dropped
        assert e.pairing_check_batch(np.stack([g[0], g_new[0]]), np.stack([g[1], g_new[1]]))[0] == [False, True]
        e.srs_downsize(4)
        assert np.array_equal(e.srs_export(0, 0, 2), g_new)
        assert e.pairing_check_batch(np.stack([g[0], g_new[0]]), np.stack([g[1], g_new[1]]))[0] == [False, True]
        e.srs_update(b"\x33" * 32)
        g_3 = e.srs_export(0, 0, 2)
        assert e.pairing_check_batch(np.stack([g_new[0], g_3[0]]), np.stack([g_new[1], g_3[1]]))[0] == [False, True]
        # zk_srs_set_g2 with the pair of another secret: g[1] of the resident basis stops holding, [t] G1 holds
        e.srs_set_g2(G2W, pc.g2_to_words(pc.g2(T)))
        assert e.pairing_check_batch(np.stack([g_3[0], g_3[0]]), np.stack([g_3[1], pc.g1_words([pc.g1(T)])[0]]))[0] == [False, True]
    finally:
        e.close()


def test_under_the_stream_audit(pool):
    e = zk.Engine(0)
    try:
        e.set_option(E.ZK_OPT_STREAM_AUDIT, 1)
        assert e.pairing_check_batch(pool["a"][:65], pool["b"][:65], G2W, pool["s_g2"])[0] == pool["want"][:65]
        checks, violations, msg = e.audit_report()
        assert checks > 0 and violations == 0, msg
    finally:
        e.close()


def test_one_call_at_the_batch_maximum(eng, pool):
    """ZK_PAIRING_BATCH_MAX pairs in one call: 64 one-wave workgroups and their scratch, which no smaller launch reaches.  The pool
    tiled by a stride coprime to its length, so the points cost nothing new and every wave holds both verdicts; then one pair on
    the same engine, through the staging buffers the large call left behind."""
    n, stride = E.ZK_PAIRING_BATCH_MAX, 37
    assert n == 4096 and np.gcd(stride, 130) == 1
    idx = [(5 + stride * i) % 130 for i in range(n)]
    assert len(set(idx[:130])) == 130
    want = [pool["want"][j] for j in idx]
    assert all(set(want[w:w + 64]) == {True, False} for w in range(0, n, 64))
    verdicts, reasons = eng.pairing_check_batch(pool["a"][idx], pool["b"][idx], G2W, pool["s_g2"])
    assert verdicts == want
    assert reasons == [pc.VALID if w else pc.MISMATCH for w in want]
    for j in (idx[0], pool["want"].index(False)):
        verdicts, reasons = eng.pairing_check_batch(pool["a"][j:j + 1], pool["b"][j:j + 1], G2W, pool["s_g2"])
        assert verdicts == [pool["want"][j]] and reasons == [pc.VALID if pool["want"][j] else pc.MISMATCH]


def test_contexts_that_share_an_srs():
    """Engine(0, share_with=parent): a child made after the parent's first resident-pair check gets the parent's table with the
    view and keeps it when the parent is closed; one made before makes its own; zk_srs_set_g2 on the parent moves the parent
    alone."""
    parent = zk.Engine(0)
    early = late = None
    try:
        parent.srs_setup(5, b"\x44" * 32)
        g = parent.srs_export(0, 0, 2)
        a, b, want = np.stack([g[0], g[0], g[1]]), np.stack([g[1], g[0], g[0]]), [True, False, False]  # e(g0, s_g2) = e(g1, g2) alone holds
        early = zk.Engine(0, share_with=parent)  # (the parent has no table yet)
        assert parent.pairing_check_batch(a, b) == (want, [pc.VALID, pc.MISMATCH, pc.MISMATCH])
        late = zk.Engine(0, share_with=parent)
        assert late.pairing_check_batch(a, b)[0] == want
        assert early.pairing_check_batch(a, b)[0] == want
        assert early.pairing_check_batch(a, b)[0] == want  # (its own cached table)
        # the parent moves to the pair of another secret: [T] G1 holds there, the resident g[1] stops holding; the children stay
        parent.srs_set_g2(G2W, pc.g2_to_words(pc.g2(T)))
        a2, b2 = np.stack([g[0], g[0]]), np.stack([g[1], pc.g1_words([pc.g1(T)])[0]])
        assert parent.pairing_check_batch(a2, b2)[0] == [False, True]
        assert late.pairing_check_batch(a2, b2)[0] == [True, False]
        assert early.pairing_check_batch(a2, b2)[0] == [True, False]
        assert parent.pairing_check_batch(a, b)[0] == [False, False, False]
        parent.close()
        assert late.pairing_check_batch(a, b)[0] == want  # the table lives on with the view that holds it
        assert late.pairing_check_batch(a2, b2)[0] == [True, False]
        assert early.pairing_check_batch(a, b)[0] == want
    finally:
        for e in (late, early, parent):
            if e is not None:
                e.close()
