"""zk_pairing_check_each on an MI355X: e(a_i, q_i) = e(b_i, g2) with a G2 point per lane, which the lane tests and walks through the
Miller loop itself (csrc/pairing.h miller_loop_walk, csrc/pairing.hip pairing_check_each_kernel).  130 lanes with a different
q_i = [t_i] G2 each, holding in about half of them, with one lane of every reason — an improper q_i of each kind among them — at
the edges of the waves; verdicts and reasons against the Python pairing of tests/pairing_ref.py (one reference run for the module,
a few seconds of integer arithmetic) and against the scalars; one q for all lanes against zk_pairing_check_batch; the caller's g2 and
the resident one; every argument error with untouched outputs; one call under ZK_OPT_STREAM_AUDIT.
"""
import ctypes
import random

import numpy as np
import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
import pairing_cases as pc
import pairing_ref as ref
from zkoracle import curve, field as F

pytestmark = pytest.mark.gpu

G2 = 4  # ZK_PAIRING_G2
G2W = pc.g2_to_words(curve.G2_GEN)
LANES = 130


def g2_with_p_added(words, col):
    w = np.array(words, dtype=np.uint64).copy()
    v = sum(int(w[col + q]) << (64 * q) for q in range(4)) + F.P
    w[col:col + 4] = [(v >> (64 * q)) & 0xFFFFFFFFFFFFFFFF for q in range(4)]
    return w


@pytest.fixture(scope="module")
def eng():
    e = zk.Engine(0)  # (no SRS, no key)
    yield e
    e.close()


@pytest.fixture(scope="module")
def lanes():
    """130 lanes (a, b, q) as limb rows with the reason each owes.  Ordinary lanes follow pairing_cases.mixed_pairs with a t of
    their own: two holding ones to every non-holding one.  The special lanes sit in the first and last places of the waves."""
    rnd = random.Random(1234)
    a, b, q, want, ts = [], [], [], [], []
    for i in range(LANES):
        t = rnd.randrange(2, F.R)
        x = rnd.randrange(1, F.R)
        if i == 1:
            x = F.R - 1
        if i == 2:
            t = 1  # q = G2 itself
        if i == 3:
            t = F.R - 1  # q = -G2
        y = x * t % F.R
        if i % 3 == 2:
            y = (F.R - y) % F.R if i % 2 else rnd.randrange(1, F.R)
        a.append(pc.g1_words([pc.g1(x)])[0])
        b.append(pc.g1_words([pc.g1(y)])[0])
        q.append(pc.g2_to_words(pc.g2(t)))
        want.append(pc.VALID if pc.holds(x, y, t) else pc.MISMATCH)
        ts.append(t)
    assert len(set(ts)) == LANES
    one_one = pc.g1_words([(1, 1)])[0]
    zero = np.zeros(8, dtype=np.uint64)
    outside = pc.g2_to_words(pc.twist_point_outside_g2())
    off = q[0].copy()
    off[0] ^= np.uint64(1)
    special = {0: ("q", off, G2), 63: ("q", outside, G2), 64: ("q", np.zeros(16, dtype=np.uint64), G2), 65: ("q", g2_with_p_added(q[65], 8), G2),
               127: ("a", pc.with_p_added(a[127], 0), pc.RANGE), 128: ("b", one_one, pc.OFF_CURVE), 129: ("q", g2_with_p_added(q[129], 4), G2),
               62: ("a", one_one, pc.OFF_CURVE), 66: ("b", pc.with_p_added(b[66], 4), pc.RANGE)}
    for i, (side, words, reason) in special.items():
        {"a": a, "b": b, "q": q}[side][i] = words
        want[i] = reason
    # the order of the tests: a G1 coordinate out of range beside an improper q is RANGE; an off-curve a is OFF_CURVE
    a[126], q[126], want[126] = pc.with_p_added(a[126], 4), outside, pc.RANGE
    a[61], q[61], want[61] = one_one, off, pc.OFF_CURVE
    # the identity on the G1 side: (O, O) holds, (O, b) and (a, O) do not
    a[10], b[10], want[10] = zero, zero, pc.VALID
    a[11], want[11] = zero, pc.MISMATCH
    b[12], want[12] = zero, pc.MISMATCH
    for w in (slice(0, 64), slice(64, 128)):
        assert {pc.VALID, pc.MISMATCH, G2} <= set(want[w])
    assert set(want) == {pc.VALID, pc.RANGE, pc.OFF_CURVE, pc.MISMATCH, G2}
    assert 50 <= want.count(pc.VALID) <= 90
    return {"a": np.stack(a), "b": np.stack(b), "q": np.stack(q), "want": want}


@pytest.fixture(scope="module")
def ref_reasons(lanes):
    """the reason of every lane by tests/pairing_ref.py: its own walk of q_i and of G2, its own Miller loop and final
    exponentiation.  The reference has no G2 tests: a lane whose q_i is improper by construction is ZK_PAIRING_G2 when the
    reference's G1 tests pass."""
    from srs_update_ref import g2_from_words

    walk_g2 = ref.prepared_walk(curve.G2_GEN)
    out = []
    for i in range(LANES):
        ar, br = ref.g1_row_to_words(lanes["a"][i]), ref.g1_row_to_words(lanes["b"][i])
        if lanes["want"][i] == G2 or i in (126, 61):  # improper q_i: the G1 reasons alone, against any proper walk
            r = ref.check(ar, br, {"walks": (walk_g2, walk_g2)})
            out.append(r if r in (pc.RANGE, pc.OFF_CURVE) else G2)
        else:
            out.append(ref.check(ar, br, {"walks": (ref.prepared_walk(g2_from_words(lanes["q"][i])), walk_g2)}))
    return out


def test_the_reference_agrees_with_the_scalars(lanes, ref_reasons):
    assert ref_reasons == lanes["want"]


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_a_g2_point_per_lane(eng, lanes, ref_reasons, count):
    verdicts, reasons = eng.pairing_check_each(lanes["a"][:count], lanes["b"][:count], lanes["q"][:count], G2W)
    assert reasons == ref_reasons[:count]
    assert verdicts == [r == pc.VALID for r in ref_reasons[:count]]


def test_the_resident_g2(lanes, ref_reasons):
    e = zk.Engine(0)
    try:
        e.srs_setup(4, b"\x07" * 32)  # (its g2 is the generator)
        verdicts, reasons = e.pairing_check_each(lanes["a"], lanes["b"], lanes["q"])
        assert reasons == ref_reasons and verdicts == [r == pc.VALID for r in ref_reasons]
        assert e.pairing_check_each(lanes["a"][:3], lanes["b"][:3], lanes["q"][:3])[1] == ref_reasons[:3]  # (the cached table)
    finally:
        e.close()


def test_one_q_for_all_lanes_equals_the_batch_check(eng):
    t = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % F.R
    xy = pc.mixed_pairs(LANES, t, 41)
    a, b = pc.g1_words([pc.g1(x) for x, _ in xy]), pc.g1_words([pc.g1(y) for _, y in xy])
    s_g2 = pc.g2_to_words(pc.g2(t))
    want = [pc.VALID if pc.holds(x, y, t) else pc.MISMATCH for x, y in xy]
    assert set(want[:64]) == set(want[64:128]) == {pc.VALID, pc.MISMATCH}
    each = eng.pairing_check_each(a, b, np.tile(s_g2, (LANES, 1)), G2W)
    assert each[1] == want
    assert each == eng.pairing_check_batch(a, b, G2W, s_g2)


def test_another_g2_base(eng):
    """g2 need not be the generator: e([x] G, [t v] G2) = e([x t] G, [v] G2)"""
    v, t, x = 0xABCDEF123456789, F.R - 3, 0x1234567
    a = pc.g1_words([pc.g1(x), pc.g1(x)])
    b = pc.g1_words([pc.g1(x * t), pc.g1(x * t + 1)])
    q = np.stack([pc.g2_to_words(pc.g2(t * v))] * 2)
    assert eng.pairing_check_each(a, b, q, pc.g2_to_words(pc.g2(v)))[0] == [True, False]


def raw_call(eng, count, a, b, q, g2, verdicts, reasons):
    u64p = ctypes.POINTER(ctypes.c_uint64)
    ptr = lambda v: ctypes.cast(None, u64p) if v is None else v.ctypes.data_as(u64p)
    return eng.L.zk_pairing_check_each(eng.ctx, count, ptr(a), ptr(b), ptr(q), ptr(g2), verdicts, reasons)


def test_reasons_may_be_null(eng, lanes):
    verdicts = (ctypes.c_uint8 * 70)(*([7] * 70))
    a, b, q = (np.ascontiguousarray(lanes[f][:70]) for f in "abq")
    assert raw_call(eng, 70, a, b, q, G2W, verdicts, None) == 0
    assert list(verdicts) == [int(w == pc.VALID) for w in lanes["want"][:70]]


def test_bad_arguments_leave_the_outputs_untouched(eng, lanes):
    a, b, q = (np.ascontiguousarray(lanes[f][1:3]) for f in "abq")
    verdicts, reasons = (ctypes.c_uint8 * 4)(*([0xA5] * 4)), (ctypes.c_uint8 * 4)(*([0x5A] * 4))
    u8p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    assert raw_call(eng, 0, a, b, q, G2W, verdicts, reasons) == -1
    assert raw_call(eng, E.ZK_PAIRING_BATCH_MAX + 1, a, b, q, G2W, verdicts, reasons) == -1  # (refused before an item is read)
    assert raw_call(eng, 2, None, b, q, G2W, verdicts, reasons) == -1
    assert raw_call(eng, 2, a, None, q, G2W, verdicts, reasons) == -1
    assert raw_call(eng, 2, a, b, None, G2W, verdicts, reasons) == -1
    assert raw_call(eng, 2, a, b, q, G2W, ctypes.cast(None, u8p), reasons) == -1
    assert eng.L.zk_pairing_check_each(None, 2, a.ctypes.data_as(u64p), b.ctypes.data_as(u64p), q.ctypes.data_as(u64p), G2W.ctypes.data_as(u64p),
                                       verdicts, reasons) == -1
    # a caller's g2 that is not proper: a coordinate not below p, off the twist, outside the subgroup, the identity
    off = G2W.copy()
    off[0] ^= np.uint64(1)
    for bad in (g2_with_p_added(G2W, 0), off, pc.g2_to_words(pc.twist_point_outside_g2()), np.zeros(16, dtype=np.uint64)):
        assert raw_call(eng, 2, a, b, q, bad, verdicts, reasons) == -1
    assert raw_call(eng, 2, a, b, q, None, verdicts, reasons) == -5  # no SRS on this context
    assert list(verdicts) == [0xA5] * 4 and list(reasons) == [0x5A] * 4
    assert raw_call(eng, 2, a, b, q, G2W, verdicts, reasons) == 0  # (the context works on)
    assert list(reasons)[:2] == lanes["want"][1:3] and list(verdicts)[2:] == [0xA5] * 2 and list(reasons)[2:] == [0x5A] * 2


def test_state_error_without_a_g2_half(lanes):
    src, e = zk.Engine(0), zk.Engine(0)
    try:
        src.srs_setup(4, b"\x07" * 32)
        e.srs_load(4, src.srs_export(0, 0, 16), src.srs_export(1, 0, 16))  # an SRS without its G2 half
        verdicts, reasons = (ctypes.c_uint8 * 2)(*([0xA5] * 2)), (ctypes.c_uint8 * 2)(*([0x5A] * 2))
        a, b, q = (np.ascontiguousarray(lanes[f][1:3]) for f in "abq")
        assert raw_call(e, 2, a, b, q, None, verdicts, reasons) == -5
        assert list(verdicts) == [0xA5] * 2 and list(reasons) == [0x5A] * 2
        assert raw_call(e, 2, a, b, q, G2W, verdicts, reasons) == 0  # (its own g2 needs no SRS half)
        assert list(reasons) == lanes["want"][1:3]
    finally:
        src.close()
        e.close()


def test_under_the_stream_audit(lanes):
    e = zk.Engine(0)
    try:
        e.set_option(E.ZK_OPT_STREAM_AUDIT, 1)
        assert e.pairing_check_each(lanes["a"][:66], lanes["b"][:66], lanes["q"][:66], G2W)[1] == lanes["want"][:66]
        checks, violations, msg = e.audit_report()
        assert checks > 0 and violations == 0, msg
    finally:
        e.close()
