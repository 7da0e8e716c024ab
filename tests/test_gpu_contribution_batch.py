"""zk_srs_contribution_check_batch on an MI355X: a chain of ceremony receipts in one launch, one receipt per lane, each lane testing
its four points and walking its own s_g2 once for both pairing equations (csrc/pairing.h contribution_check_lanes, csrc/pairing.hip
contribution_check_kernel).  Every kind of receipt (tests/contribution_cases.py) with the flag word its scalars owe
(srs_update_ref.expected_flags: no pairing) and the word zk_srs_contribution_check gives; counts around the wave size, all honest
and with the kinds interleaved so that lanes which return early sit beside lanes that walk; the CHAINED and RESIDENT bits; the
argument errors; the stream audit; and ecdsa_p256.check_contributions under both settings.
"""
import ctypes

import numpy as np
import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import ecdsa_p256 as api, engine as E
import contribution_cases as cc
import srs_update_ref as ref
from zkoracle import curve, field as F

pytestmark = pytest.mark.gpu

CHAINED = 16
COUNTS = [1, 63, 64, 65, 129]


@pytest.fixture(scope="module")
def eng():
    e = zk.Engine(0)  # (no SRS: RESIDENT is clear everywhere)
    yield e
    e.close()


@pytest.fixture(scope="module")
def single_words(eng):
    """zk_srs_contribution_check's word for every receipt of the pools, once (the host route: two pairing checks each)"""
    out = {}
    for _, rec, _ in cc.kinds():
        out[id(rec)] = eng.srs_contribution_check(rec)
    for rec, _ in cc.honest_pool():
        out[id(rec)] = eng.srs_contribution_check(rec)
    return out


def test_kinds_cover_the_rule():
    names = [n for n, _, _ in cc.kinds()]
    assert len(names) == len(set(names)) == 22
    for count in COUNTS[1:]:
        got = {id(r) for r, _ in cc.mixed_batch(count)}
        assert {id(r) for _, r, _ in cc.kinds()} <= got, count
    batch = cc.mixed_batch(129)
    for lane in (0, 63, 64, 127, 128):
        assert batch[lane][1] == 0
    assert any(batch[i][1] == 7 and batch[i + 1][1] == 0 for i in range(128))


def chained_only(words):
    """the words without CHAINED: unrelated receipts are chained at place 0 alone"""
    assert words[0] & CHAINED and not any(w & CHAINED for w in words[1:])
    return [w & ~CHAINED for w in words]


@pytest.mark.parametrize("count", COUNTS)
def test_honest_receipts(eng, single_words, count):
    batch = cc.honest_batch(count)
    got = eng.srs_contribution_check_batch([r for r, _ in batch])
    assert got[0] == 7 | CHAINED
    # the pool's receipts repeat: a receipt whose before_g1 is not the one before's after_g1 is not CHAINED
    assert [w & ~CHAINED for w in got] == [7] * count == [single_words[id(r)] for r, _ in batch]
    assert not any(w & CHAINED for w in got[1:])


@pytest.mark.parametrize("count", COUNTS)
def test_kinds_interleaved_in_every_wave(eng, single_words, count):
    batch = cc.mixed_batch(count)
    got = chained_only(eng.srs_contribution_check_batch([r for r, _ in batch]))
    assert got == [w for _, w in batch]
    assert got == [single_words[id(r)] for r, _ in batch]


def test_every_kind_alone(eng, single_words):
    for name, rec, want in cc.kinds():
        assert eng.srs_contribution_check_batch([rec]) == [want | CHAINED], name
        assert single_words[id(rec)] == want, name


SETUP_SEED = b"\x05" * 32
SEEDS = [bytes([0x20 + i]) * 32 for i in range(5)]
SECRETS = [ref.secret_of_seed(s) for s in SEEDS]


@pytest.fixture(scope="module")
def chain():
    """five receipts by srs_update_ref.contribution, each from the after_g1 of the one before, starting at g[1] = [tau] G1 of the
    setup from SETUP_SEED"""
    g1, out = curve.mul(curve.G1_GEN, ref.secret_of_seed(SETUP_SEED)), []
    for s in SECRETS:
        c = ref.contribution(g1, s)
        out.append(ref.contribution_to_limbs(c))
        g1 = c["after_g1"]
    return out


def test_chain_bits(eng, chain):
    assert eng.srs_contribution_check_batch(chain) == [7 | CHAINED] * 5
    other = ref.contribution_to_limbs(ref.contribution(curve.mul(curve.G1_GEN, 99), SECRETS[2]))
    broken = list(chain)
    broken[2] = dict(chain[2], before_g1=other["before_g1"])  # (LINKS goes with it: after_g1 is no longer [s] before_g1)
    got = eng.srs_contribution_check_batch(broken)
    assert [bool(w & CHAINED) for w in got] == [True, True, False, True, True]
    assert [w & 7 for w in got] == [7, 7, 5, 7, 7]
    whole = dict(other)  # an honest receipt that does not continue the chain: every bit but CHAINED
    broken[2] = whole
    got = eng.srs_contribution_check_batch(broken)
    assert got == [7 | CHAINED, 7 | CHAINED, 7, 7, 7 | CHAINED]  # receipt 3 no longer follows receipt 2 either


def test_resident_bit_after_the_same_five_updates_on_the_device(chain):
    e = zk.Engine(0)
    try:
        e.srs_setup(4, SETUP_SEED)
        recs = [e.srs_update(s) for s in SEEDS]
        for mine, theirs in zip(chain, recs):
            assert all(np.array_equal(np.asarray(mine[f], dtype=np.uint64).reshape(-1), theirs[f]) for f in ref.FIELDS)
        assert e.srs_contribution_check_batch(chain) == [7 | CHAINED] * 4 + [15 | CHAINED]
        assert [e.srs_contribution_check(r) for r in chain] == [7] * 4 + [15]
    finally:
        e.close()


def raw_call(eng, count, recs, flags):
    return eng.L.zk_srs_contribution_check_batch(eng.ctx, count, recs, flags)


def test_bad_arguments_leave_the_flags_untouched(eng, chain):
    cs = (E.SrsContributionC * 2)()
    for c, rec in zip(cs, chain):
        for f in ref.FIELDS:
            a = np.ascontiguousarray(rec[f], dtype=np.uint64)
            ctypes.memmove(getattr(c, f), a.ctypes.data, a.nbytes)
    flags = (ctypes.c_uint32 * 3)(*([0xDEADBEEF] * 3))
    assert raw_call(eng, 0, cs, flags) == -1
    assert raw_call(eng, E.ZK_SRS_CONTRIB_BATCH_MAX + 1, cs, flags) == -1  # (refused before a receipt is read)
    assert raw_call(eng, 2, None, flags) == -1
    assert raw_call(eng, 2, cs, None) == -1
    assert eng.L.zk_srs_contribution_check_batch(None, 2, cs, flags) == -1
    assert list(flags) == [0xDEADBEEF] * 3
    assert raw_call(eng, 2, cs, flags) == 0
    assert list(flags) == [7 | CHAINED, 7 | CHAINED, 0xDEADBEEF]


def test_under_the_stream_audit():
    e = zk.Engine(0)
    try:
        e.set_option(E.ZK_OPT_STREAM_AUDIT, 1)
        batch = cc.mixed_batch(65)
        assert chained_only(e.srs_contribution_check_batch([r for r, _ in batch])) == [w for _, w in batch]
        checks, violations, msg = e.audit_report()
        assert checks > 0 and violations == 0, msg
    finally:
        e.close()


def test_check_contributions_on_the_host_and_on_the_device(tmp_path):
    files = [str(tmp_path / ("kzg_bn254_4_%d.srs" % i)) for i in range(3)]
    receipts = [api.contribute_params(None, files[0], b"\x31" * 32, degree=4)]
    for i in (1, 2):
        receipts.append(api.contribute_params(files[i - 1], files[i], bytes([0x31 + i]) * 32))
    stranger = api.contribute_params(None, str(tmp_path / "other.srs"), b"\x77" * 32, degree=4)
    forged = [receipts[0], dict(receipts[1], s_g1=stranger["s_g1"]), receipts[2]]
    swapped = [receipts[1], receipts[0], receipts[2]]
    try:
        for mode in ("host", "device"):
            api.set_contribution_check(mode)
            assert api.check_contributions(files[2], receipts), mode
            assert not api.check_contributions(files[2], forged), mode
            assert not api.check_contributions(files[2], swapped), mode
    finally:
        api.set_contribution_check("auto")
