"""zk_webauthn_register on the device against tests/webauthn_register_ref.py over the registration set of
tests/webauthn_register_cases.py (about 290 registrations, the largest launch of this file): verdicts, reasons and every field of
the credentials of the whole set in one call; counts around the wave and workgroup sizes with accepted and refused, hashing and
non-hashing, short and capped requests mixed inside every wave; one accepted registration at lanes 0, 63, 64, 255 and 256 among
refused ones; the first call of a fresh context (which builds the comb table of G) against its second; each optional output NULL;
a call with only SIZE requests; the argument errors with untouched outputs; one call under ZK_OPT_STREAM_AUDIT; zk_es256_verify
and zk_webauthn_verify on the same context before and after (the three share the table and the staging); and the key of an
accepted registration put into an assertion for the same private key, which zk_webauthn_verify accepts.
"""
import ctypes

import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
import es256_cases
import webauthn_cases as A
import webauthn_ref as W
import webauthn_register_cases as C
import webauthn_register_ref as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cs():
    return C.build()


@pytest.fixture(scope="module")
def eng():
    e = zk.Engine(0)  # (no SRS, no key)
    yield e
    e.close()


def as_dict(g):
    return {"attestation_object": g.attestation_object, "client_data_json": g.client_data_json, "challenge": g.challenge, "origin": g.origin,
            "rp_id_hash": g.rp_id_hash, "flags_required": g.flags_required, "allow_cross_origin": g.allow_cross_origin,
            "attestation_policy": g.policy}


def check(eng, cs, idx):
    got = eng.webauthn_register([as_dict(cs.regs[i]) for i in idx])
    assert len(got) == len(idx)
    want = [cs.reasons[i] for i in idx]
    bad = [(cs.names[i], G.REASON_NAMES.get(g[1], g[1]), G.REASON_NAMES[w]) for i, g, w in zip(idx, got, want) if g[1] != w]
    assert not bad, "%d of %d reasons differ from the reference, first (name, got, want): %s" % (len(bad), len(idx), bad[:5])
    assert [g[0] for g in got] == [w == G.VALID for w in want]
    bad = []
    for i, (_, _, cred) in zip(idx, got):
        ref = cs.creds[i]
        if (cred is None) != (ref is None) or (ref and {k: cred[k] for k in ref} != ref):
            bad.append(cs.names[i])
        if ref:
            o = cs.regs[i].attestation_object
            assert cred["auth_data"] == o[ref["auth_data_off"]:] and cred["credential_id"] == C.cred_id(ref["credential_id_len"]), cs.names[i]
    assert not bad, "%d of %d credentials differ from the reference, first: %s" % (len(bad), len(idx), bad[:5])


def mixed(cs, count):
    """`count` case indices: accepted and refused alternating two to one; among the accepted every fourth a capped one (an object
    or a clientDataJSON at its cap, hashed), the others alternately self-attested (hashing) and not, so that every wave holds all."""
    long_ones = [cs.index(n) for n in ("cap/object=8192-self-attested", "cap/clientdata=4096", "head/id=1023", "cap/everything-at-its-cap")]
    v = [i for i in cs.valid_indices() if i not in long_ones]
    selfs = [i for i in v if cs.creds[i]["attestation"] == G.ATTESTED_SELF]
    plain = [i for i in v if cs.creds[i]["attestation"] != G.ATTESTED_SELF]
    b = cs.invalid_indices()
    out = []
    for j in range(count):
        if j % 3 == 2:
            out.append(b[(j // 3) % len(b)])
        elif j % 12 == 4:
            out.append(long_ones[(j // 12) % len(long_ones)])
        elif j % 2:
            out.append(selfs[(j // 2) % len(selfs)])
        else:
            out.append(plain[(j // 2) % len(plain)])
    return out


def test_whole_set_in_one_call(eng, cs):
    check(eng, cs, list(range(len(cs))))


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_counts_around_the_wave(eng, cs, count):
    idx = mixed(cs, count)
    if count > 1:
        for lo in range(0, count - 62, 64):
            wave = idx[lo:lo + 64]
            assert {cs.reasons[i] == G.VALID for i in wave} == {True, False}
            assert {cs.creds[i]["attestation"] for i in wave if cs.creds[i]} >= {G.ATTESTED_SELF, G.ATTESTED_NOT_JUDGED}
            lens = [len(cs.regs[i].attestation_object) for i in wave if cs.reasons[i] == G.VALID]
            assert min(lens) < 300 and max(lens) == 8192
    check(eng, cs, idx)


@pytest.mark.parametrize("lane", [0, 63, 64, 255, 256])
def test_one_accepted_registration_among_refused_ones(eng, cs, lane):
    bad = cs.invalid_indices()
    idx = [bad[j % len(bad)] for j in range(257)]
    idx[lane] = cs.index("valid/packed-self/policy=1")
    got = eng.webauthn_register([as_dict(cs.regs[i]) for i in idx])
    assert [g[0] for g in got] == [j == lane for j in range(257)]
    assert [g[2] is not None for g in got] == [j == lane for j in range(257)]
    check(eng, cs, idx)


def test_first_call_of_a_fresh_context_equals_the_second(cs):
    e = zk.Engine(0)
    try:
        idx = mixed(cs, 96)
        first = e.webauthn_register([as_dict(cs.regs[i]) for i in idx])   # builds the table
        second = e.webauthn_register([as_dict(cs.regs[i]) for i in idx])  # finds it
        assert first == second
        check(e, cs, idx)
    finally:
        e.close()


def raw_args(cs, idx):
    """(count, the C array, the three output arrays filled with marks) for a direct call."""
    arr = E.Engine.webauthn_register_pack([as_dict(cs.regs[i]) for i in idx])
    n = len(idx)
    creds = (E.WebauthnCredentialC * n)()
    ctypes.memset(creds, 0xC3, ctypes.sizeof(creds))
    return n, arr, (ctypes.c_uint8 * n)(*([0xA5] * n)), (ctypes.c_uint8 * n)(*([0x5A] * n)), creds


def creds_want(cs, idx):
    return b"".join(C.cred_bytes(cs.creds[i]) for i in idx)


def test_each_optional_output_may_be_null(eng, cs):
    idx = mixed(cs, 70) + [cs.index("cap/object=8193"), cs.index("ad/36-bytes")]
    for skip in (None, 1, 2):
        n, arr, verdicts, reasons, creds = raw_args(cs, idx)
        outs = [verdicts, reasons, creds]
        if skip is not None:
            outs[skip] = None
        assert eng.L.zk_webauthn_register(eng.ctx, n, arr, *outs) == 0
        assert list(verdicts) == [int(cs.reasons[i] == G.VALID) for i in idx]
        if skip != 1:
            assert list(reasons) == [cs.reasons[i] for i in idx]
        if skip != 2:
            assert bytes(creds) == creds_want(cs, idx)  # every byte: a refused registration's credential is all zero
    n, arr, verdicts, reasons, creds = raw_args(cs, idx)
    assert eng.L.zk_webauthn_register(eng.ctx, n, arr, verdicts, None, None) == 0
    assert list(verdicts) == [int(cs.reasons[i] == G.VALID) for i in idx]
    assert list(reasons) == [0x5A] * n and bytes(creds) == b"\xC3" * (104 * n)


def test_only_requests_outside_the_caps(eng, cs):
    """No request is uploaded and nothing is launched: every verdict is the host's."""
    idx = [cs.index(n) for n in ("cap/object=8193", "cap/object=0", "cap/clientdata=4097", "cap/challenge=65", "cap/challenge=0", "cap/origin=256",
                                 "cap/object=8193-self-attested", "order/size-before-cbor")]
    check(eng, cs, idx)
    assert {cs.reasons[i] for i in idx} == {G.SIZE}


def test_bad_arguments_leave_the_outputs_untouched(eng, cs):
    idx = [cs.index("valid/packed-self/policy=1"), cs.index("valid/none/policy=0")]
    n, arr, verdicts, reasons, creds = raw_args(cs, idx)
    call = eng.L.zk_webauthn_register
    u8p = ctypes.POINTER(ctypes.c_uint8)
    assert call(eng.ctx, 0, arr, verdicts, reasons, creds) == -1
    assert call(eng.ctx, E.ZK_WEBAUTHN_BATCH_MAX + 1, arr, verdicts, reasons, creds) == -1  # (refused before a request is read)
    assert call(eng.ctx, 2, None, verdicts, reasons, creds) == -1
    assert call(eng.ctx, 2, arr, ctypes.cast(None, u8p), reasons, creds) == -1
    assert call(None, 2, arr, verdicts, reasons, creds) == -1
    for name in ("attestation_object", "client_data_json", "challenge", "origin"):  # a NULL pointer with a length
        keep = as_dict(cs.regs[idx[1]])[name]  # (reading the field back would stop at the first zero byte)
        setattr(arr[1], name, None)
        assert call(eng.ctx, 2, arr, verdicts, reasons, creds) == -1, name
        setattr(arr[1], name, keep.encode() if isinstance(keep, str) else keep)
    arr[1].attestation_policy = 2  # no such policy
    assert call(eng.ctx, 2, arr, verdicts, reasons, creds) == -1
    arr[1].attestation_policy = 0
    assert list(verdicts) == [0xA5] * 2 and list(reasons) == [0x5A] * 2 and bytes(creds) == b"\xC3" * 208
    with pytest.raises(zk.ZkError) as e:
        eng.webauthn_register([])
    assert e.value.code == -1
    # a NULL pointer with length 0 is an empty string: a verdict
    arr[1].client_data_json, arr[1].client_data_json_len = None, 0
    assert call(eng.ctx, 2, arr, verdicts, reasons, creds) == 0  # (the context works on)
    assert list(verdicts) == [1, 0] and list(reasons) == [G.VALID, G.CLIENTDATA]
    assert bytes(creds) == C.cred_bytes(cs.creds[idx[0]]) + bytes(104)


def test_under_the_stream_audit(cs):
    e = zk.Engine(0)
    try:
        e.set_option(E.ZK_OPT_STREAM_AUDIT, 1)
        check(e, cs, mixed(cs, 65))
        checks, violations, msg = e.audit_report()
        assert checks > 0 and violations == 0, msg
    finally:
        e.close()


def assertion_dict(a):
    return {"authenticator_data": a.authenticator_data, "client_data_json": a.client_data_json, "signature": a.signature,
            "pubkey_x": a.x.to_bytes(32, "big"), "pubkey_y": a.y.to_bytes(32, "big"), "challenge": a.challenge, "origin": a.origin,
            "rp_id_hash": a.rp_id_hash, "flags_required": a.flags_required, "allow_cross_origin": a.allow_cross_origin}


def test_es256_and_webauthn_verify_before_and_after_on_one_context(cs):
    """The three calls share the comb table and the staging buffers: the neighbours give the bytes they gave."""
    es, ws = es256_cases.build(), A.build()
    pick = (es.valid_indices()[:40] + es.invalid_indices()[:30])[::-1]
    blob = b"".join(es.records[i] for i in pick)
    wpick = (ws.valid_indices()[:30] + ws.invalid_indices()[:40])[::2]
    assertions = [assertion_dict(ws.assertions[i]) for i in wpick]
    e = zk.Engine(0)
    try:
        before = (e.es256_verify(blob), e.webauthn_verify(assertions))  # builds the table; small staging
        check(e, cs, mixed(cs, 130))                                    # grows the staging
        after = (e.es256_verify(blob), e.webauthn_verify(assertions))
        assert before == after
        assert before[0][1] == [es.reasons[i] for i in pick]
        assert before[1][1] == [ws.reasons[i] for i in wpick] and before[1][2] == [ws.records[i] for i in wpick]
        check(e, cs, mixed(cs, 5))
    finally:
        e.close()


def test_a_registered_key_verifies_the_assertions_of_its_private_key(eng, cs):
    """What the call is for: the key it hands out is the one zk_webauthn_verify takes.  An assertion signed with D is accepted under
    the key registered for D and is a MISMATCH under the key of another registration."""
    other = A._key(A.D + 1)
    regs = [cs.regs[cs.index("valid/packed-self/policy=1")], C.reg(C.att_obj(C.auth_data(key=C.cose_key(other))), policy=G.ATT_NONE_OR_SELF)]
    got = eng.webauthn_register([as_dict(g) for g in regs])
    assert [g[:2] for g in got] == [(True, G.VALID)] * 2
    mine, theirs = got[0][2], got[1][2]
    assert (mine["attestation"], theirs["attestation"]) == (G.ATTESTED_SELF, G.ATTESTED_NONE)
    a = assertion_dict(A.make(ad=A.auth_data(counter=mine["sign_count"] + 1)))
    with_mine = dict(a, pubkey_x=mine["pubkey_x"], pubkey_y=mine["pubkey_y"])
    with_theirs = dict(a, pubkey_x=theirs["pubkey_x"], pubkey_y=theirs["pubkey_y"])
    verdicts, reasons, _, counts = eng.webauthn_verify([with_mine, with_theirs])
    assert verdicts == [True, False] and reasons == [W.VALID, W.MISMATCH] and counts == [mine["sign_count"] + 1] * 2
