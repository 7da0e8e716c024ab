"""zk_webauthn_verify on the device against tests/webauthn_ref.py over the assertion set of tests/webauthn_cases.py (about 220
assertions, the largest launch of this file): verdicts, reasons, records and counters of the whole set in one call; counts around
the wave and workgroup sizes with valid and invalid requests and short and long messages mixed inside every wave; one valid request
at lanes 0, 63, 64, 255 and 256 among invalid ones; the first call of a fresh context (which builds the comb table of G) against
its second; each optional output NULL in turn; the argument errors with untouched outputs; the records fed to zk_es256_verify; one
call under ZK_OPT_STREAM_AUDIT; zk_es256_verify on the same context before and after (the two share the table and the staging).
"""
import ctypes

import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
import es256_cases
import webauthn_cases as C
import webauthn_ref as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cs():
    return C.build()


@pytest.fixture(scope="module")
def eng():
    e = zk.Engine(0)  # (no SRS, no key)
    yield e
    e.close()


def as_dict(a):
    return {"authenticator_data": a.authenticator_data, "client_data_json": a.client_data_json, "signature": a.signature,
            "pubkey_x": a.x.to_bytes(32, "big"), "pubkey_y": a.y.to_bytes(32, "big"), "challenge": a.challenge, "origin": a.origin,
            "rp_id_hash": a.rp_id_hash, "flags_required": a.flags_required, "allow_cross_origin": a.allow_cross_origin}


def check(eng, cs, idx):
    verdicts, reasons, records, counts = eng.webauthn_verify([as_dict(cs.assertions[i]) for i in idx])
    want = [cs.reasons[i] for i in idx]
    bad = [(cs.names[i], W.REASON_NAMES.get(g, g), W.REASON_NAMES[w]) for i, g, w in zip(idx, reasons, want) if g != w]
    assert not bad, "%d of %d reasons differ from the reference, first (name, got, want): %s" % (len(bad), len(idx), bad[:5])
    assert verdicts == [w == W.VALID for w in want]
    bad = [cs.names[i] for i, g in zip(idx, records) if g != cs.records[i]]
    assert not bad, "%d of %d records differ from the reference, first: %s" % (len(bad), len(idx), bad[:5])
    bad = [(cs.names[i], g, cs.counts[i]) for i, g in zip(idx, counts) if g != cs.counts[i]]
    assert not bad, "%d of %d counters differ from the reference, first (name, got, want): %s" % (len(bad), len(idx), bad[:5])


def mixed(cs, count):
    """`count` case indices: valid and invalid alternating two to one, and among the valid ones every fourth with long messages
    (clientDataJSON at its cap, or authenticatorData at its cap), so that every wave holds all of these."""
    long_ones = [cs.index(n) for n in ("cdlen/4096", "adlen/1024", "cdlen/4095", "adlen/1024+cdlen/4096")]
    v = [i for i in cs.valid_indices() if i not in long_ones]
    b = cs.invalid_indices()
    out = []
    for j in range(count):
        if j % 3 == 2:
            out.append(b[(j // 3) % len(b)])
        elif j % 12 == 4:
            out.append(long_ones[(j // 12) % len(long_ones)])
        else:
            out.append(v[(j - j // 3) % len(v)])
    return out


def test_whole_set_in_one_call(eng, cs):
    check(eng, cs, list(range(len(cs))))


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_counts_around_the_wave(eng, cs, count):
    idx = mixed(cs, count)
    if count > 1:
        for lo in range(0, count - 62, 64):
            wave = idx[lo:lo + 64]
            assert {cs.reasons[i] == W.VALID for i in wave} == {True, False}
            lens = [len(cs.assertions[i].client_data_json) for i in wave if cs.reasons[i] == W.VALID]
            assert min(lens) < 200 and max(lens) >= 4095
    check(eng, cs, idx)


@pytest.mark.parametrize("lane", [0, 63, 64, 255, 256])
def test_one_valid_request_among_invalid_ones(eng, cs, lane):
    bad = cs.invalid_indices()
    idx = [bad[j % len(bad)] for j in range(257)]
    idx[lane] = cs.index("der/r=33-bytes")
    verdicts = eng.webauthn_verify([as_dict(cs.assertions[i]) for i in idx])[0]
    assert verdicts == [j == lane for j in range(257)]
    check(eng, cs, idx)


def test_first_call_of_a_fresh_context_equals_the_second(cs):
    e = zk.Engine(0)
    try:
        idx = mixed(cs, 96)
        first = e.webauthn_verify([as_dict(cs.assertions[i]) for i in idx])   # builds the table
        second = e.webauthn_verify([as_dict(cs.assertions[i]) for i in idx])  # finds it
        assert first == second
        check(e, cs, idx)
    finally:
        e.close()


def raw_args(cs, idx):
    """(count, the C array, the four output arrays filled with marks) for a direct call."""
    n = len(idx)
    arr = (E.WebauthnAssertionC * n)()
    for c, i in zip(arr, idx):
        q = as_dict(cs.assertions[i])
        for name in ("authenticator_data", "client_data_json", "signature", "challenge"):
            setattr(c, name, q[name])
            setattr(c, name + "_len", len(q[name]))
        c.origin, c.origin_len = q["origin"].encode(), len(q["origin"].encode())
        for name in ("pubkey_x", "pubkey_y", "rp_id_hash"):
            getattr(c, name)[:] = q[name]
        c.flags_required, c.allow_cross_origin = q["flags_required"], int(q["allow_cross_origin"])
    return (n, arr, (ctypes.c_uint8 * n)(*([0xA5] * n)), (ctypes.c_uint8 * n)(*([0x5A] * n)), (ctypes.c_uint8 * (160 * n))(*([0xC3] * (160 * n))),
            (ctypes.c_uint32 * n)(*([0x3C3C3C3C] * n)))


def test_each_optional_output_may_be_null(eng, cs):
    idx = mixed(cs, 70) + [cs.index("cap/authdata=1025"), cs.index("cap/authdata=36")]
    for skip in (None, 1, 2, 3):
        n, arr, verdicts, reasons, records, counts = raw_args(cs, idx)
        outs = [verdicts, reasons, records, counts]
        if skip is not None:
            outs[skip] = None
        assert eng.L.zk_webauthn_verify(eng.ctx, n, arr, *outs) == 0
        assert list(verdicts) == [int(cs.reasons[i] == W.VALID) for i in idx]
        if skip != 1:
            assert list(reasons) == [cs.reasons[i] for i in idx]
        if skip != 2:
            assert bytes(records) == b"".join(cs.records[i] for i in idx)
        if skip != 3:
            assert list(counts) == [cs.counts[i] for i in idx]
    n, arr, verdicts, reasons, records, counts = raw_args(cs, idx)
    assert eng.L.zk_webauthn_verify(eng.ctx, n, arr, verdicts, None, None, None) == 0
    assert list(verdicts) == [int(cs.reasons[i] == W.VALID) for i in idx]
    assert list(reasons) == [0x5A] * n and bytes(records) == b"\xC3" * (160 * n) and list(counts) == [0x3C3C3C3C] * n


def test_only_requests_outside_the_caps(eng, cs):
    """No request is uploaded and nothing is launched: every verdict is the host's."""
    idx = [cs.index(n) for n in ("cap/authdata=1025", "cap/clientdata=4097", "cap/challenge=65", "cap/challenge=0", "cap/origin=256",
                                 "cap/signature=73", "cap/signature=7")]
    check(eng, cs, idx)
    assert {cs.reasons[i] for i in idx} == {W.SIZE}


def test_bad_arguments_leave_the_outputs_untouched(eng, cs):
    idx = [cs.index("valid/0"), cs.index("valid/1")]
    n, arr, verdicts, reasons, records, counts = raw_args(cs, idx)
    call = eng.L.zk_webauthn_verify
    u8p = ctypes.POINTER(ctypes.c_uint8)
    assert call(eng.ctx, 0, arr, verdicts, reasons, records, counts) == -1
    assert call(eng.ctx, E.ZK_WEBAUTHN_BATCH_MAX + 1, arr, verdicts, reasons, records, counts) == -1  # (refused before a request is read)
    assert call(eng.ctx, 2, None, verdicts, reasons, records, counts) == -1
    assert call(eng.ctx, 2, arr, ctypes.cast(None, u8p), reasons, records, counts) == -1
    assert call(None, 2, arr, verdicts, reasons, records, counts) == -1
    for name in ("authenticator_data", "client_data_json", "signature", "challenge", "origin"):  # a NULL pointer with a length
        keep = as_dict(cs.assertions[idx[1]])[name]  # (reading the field back would stop at the first zero byte)
        setattr(arr[1], name, None)
        assert call(eng.ctx, 2, arr, verdicts, reasons, records, counts) == -1, name
        setattr(arr[1], name, keep.encode() if isinstance(keep, str) else keep)
    assert list(verdicts) == [0xA5] * 2 and list(reasons) == [0x5A] * 2 and bytes(records) == b"\xC3" * 320 and list(counts) == [0x3C3C3C3C] * 2
    with pytest.raises(zk.ZkError) as e:
        eng.webauthn_verify([])
    assert e.value.code == -1
    # a NULL pointer with length 0 is an empty string: a verdict
    arr[1].authenticator_data, arr[1].authenticator_data_len = None, 0
    assert call(eng.ctx, 2, arr, verdicts, reasons, records, counts) == 0  # (the context works on)
    assert list(verdicts) == [1, 0] and list(reasons) == [W.VALID, W.AUTHDATA] and list(counts) == [cs.counts[idx[0]], 0]
    assert bytes(records) == cs.records[idx[0]] + bytes(160)


def test_records_go_to_es256_verify(eng, cs):
    idx = list(range(len(cs)))
    verdicts, reasons, records, _ = eng.webauthn_verify([as_dict(cs.assertions[i]) for i in idx])
    es_verdicts, es_reasons = eng.es256_verify(b"".join(records))
    assert [r == E.ZK_ES256_VALID for r in es_reasons] == verdicts == es_verdicts
    # where the curve was reached the two calls give one reason; an all-zero record is out of range
    for name, r, er in zip(cs.names, reasons, es_reasons):
        assert er == (r if r <= W.MISMATCH else E.ZK_ES256_RANGE), name


def test_under_the_stream_audit(cs):
    e = zk.Engine(0)
    try:
        e.set_option(E.ZK_OPT_STREAM_AUDIT, 1)
        check(e, cs, mixed(cs, 65))
        checks, violations, msg = e.audit_report()
        assert checks > 0 and violations == 0, msg
    finally:
        e.close()


def test_es256_verify_before_and_after_on_one_context(cs):
    es = es256_cases.build()
    pick = (es.valid_indices()[:40] + es.invalid_indices()[:30])[::-1]
    blob = b"".join(es.records[i] for i in pick)
    want = [es.reasons[i] for i in pick]
    e = zk.Engine(0)
    try:
        before = e.es256_verify(blob)  # builds the table; its staging is 70 records
        check(e, cs, mixed(cs, 130))   # grows the staging
        after = e.es256_verify(blob)
        assert before == after and before[1] == want
        check(e, cs, mixed(cs, 5))
    finally:
        e.close()
