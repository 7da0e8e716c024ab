"""zk_es256_verify on the device against tests/es256_ref.py over the signature set of tests/es256_cases.py (about 400 records,
the largest launch of this file): verdicts and reasons of the whole set in one call; counts around the wave size with valid and
invalid records mixed within a wave; one valid record at lanes 0, 63 and 64 among invalid ones; the first call of a fresh context
(which builds the comb table of G) against its second; reasons = NULL; the argument errors with untouched outputs; one call
under ZK_OPT_STREAM_AUDIT.
"""
import ctypes

import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
import es256_cases
import es256_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cs():
    return es256_cases.build()


@pytest.fixture(scope="module")
def eng():
    e = zk.Engine(0)  # (no SRS, no key)
    yield e
    e.close()


def mixed(cs, count):
    """`count` record indices drawn from the set, valid and invalid alternating two to one (so every wave holds both)."""
    v, b = cs.valid_indices(), cs.invalid_indices()
    return [b[(j // 3) % len(b)] if j % 3 == 2 else v[(j - j // 3) % len(v)] for j in range(count)]


def check(eng, cs, idx):
    verdicts, reasons = eng.es256_verify(b"".join(cs.records[i] for i in idx))
    want = [cs.reasons[i] for i in idx]
    bad = [(cs.names[i], g, w) for i, g, w in zip(idx, reasons, want) if g != w]
    assert not bad, "%d of %d reasons differ from the reference, first (name, got, want): %s" % (len(bad), len(idx), bad[:5])
    assert verdicts == [w == R.VALID for w in want]


def test_whole_set_in_one_call(eng, cs):
    check(eng, cs, list(range(len(cs))))


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_counts_around_the_wave(eng, cs, count):
    idx = mixed(cs, count)
    if count > 1:
        assert {cs.reasons[i] == R.VALID for i in idx[:min(count, 64)]} == {True, False}
    check(eng, cs, idx)


@pytest.mark.parametrize("lane", [0, 63, 64])
def test_one_valid_record_among_invalid_ones(eng, cs, lane):
    bad = cs.invalid_indices()
    idx = [bad[j % len(bad)] for j in range(65)]
    idx[lane] = cs.index("kat/rfc6979-a.2.5-sample-sha256")
    verdicts, reasons = eng.es256_verify(b"".join(cs.records[i] for i in idx))
    assert verdicts == [j == lane for j in range(65)]
    assert reasons == [cs.reasons[i] for i in idx]


def test_first_call_of_a_fresh_context_equals_the_second(cs):
    e = zk.Engine(0)
    try:
        blob = b"".join(cs.records[i] for i in mixed(cs, 96))
        first = e.es256_verify(blob)   # builds the table
        second = e.es256_verify(blob)  # finds it
        assert first == second
        assert first[1] == [cs.reasons[i] for i in mixed(cs, 96)]
    finally:
        e.close()


def raw_call(eng, count, sigs, verdicts, reasons):
    return eng.L.zk_es256_verify(eng.ctx, count, sigs, verdicts, reasons)


def test_reasons_may_be_null(eng, cs):
    idx = mixed(cs, 70)
    verdicts = (ctypes.c_uint8 * 70)(*([7] * 70))
    assert raw_call(eng, 70, b"".join(cs.records[i] for i in idx), verdicts, None) == 0
    assert list(verdicts) == [int(cs.reasons[i] == R.VALID) for i in idx]


def test_bad_arguments_leave_the_outputs_untouched(eng, cs):
    blob = cs.records[0] * 2
    verdicts, reasons = (ctypes.c_uint8 * 4)(*([0xA5] * 4)), (ctypes.c_uint8 * 4)(*([0x5A] * 4))
    u8p = ctypes.POINTER(ctypes.c_uint8)
    assert raw_call(eng, 0, blob, verdicts, reasons) == -1
    assert raw_call(eng, E.ZK_ES256_BATCH_MAX + 1, blob, verdicts, reasons) == -1  # (refused before a record is read)
    assert raw_call(eng, 2, None, verdicts, reasons) == -1
    assert raw_call(eng, 2, blob, ctypes.cast(None, u8p), reasons) == -1
    assert eng.L.zk_es256_verify(None, 2, blob, verdicts, reasons) == -1
    assert list(verdicts) == [0xA5] * 4 and list(reasons) == [0x5A] * 4
    with pytest.raises(zk.ZkError) as e:
        eng.es256_verify(b"")
    assert e.value.code == -1
    with pytest.raises(ValueError):
        eng.es256_verify(bytes(161))
    assert raw_call(eng, 2, blob, verdicts, reasons) == 0  # (the context works on)
    assert list(verdicts)[:2] == [1, 1] and list(reasons)[:2] == [0, 0] and list(verdicts)[2:] == [0xA5] * 2


def test_under_the_stream_audit(cs):
    e = zk.Engine(0)
    try:
        e.set_option(E.ZK_OPT_STREAM_AUDIT, 1)
        idx = mixed(cs, 65)
        assert e.es256_verify(b"".join(cs.records[i] for i in idx))[1] == [cs.reasons[i] for i in idx]
        checks, violations, msg = e.audit_report()
        assert checks > 0 and violations == 0, msg
    finally:
        e.close()
