"""zk_verify_batch_public and zk_verify_multi_public (csrc/verify.hip, csrc/verifier.h).

The batch form: 17 proofs of k17like with per-proof lists of 0, 1, 9 and `usable` values; its verdicts are zk_verify_public's one by
one; three planted proofs - a wrong list, a tampered byte, a wrong length - are exactly the zeros; the same under
zk_verify_instance_eval_mode 1 (host) and 2 (device); on a verifying-only key.  The multi form accepts zk_prove_multi_public's proofs
and rejects what tests/halo2_ref.py rejects.  An over-long list is an error for the whole call, not a verdict."""
import json
import os

import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
from multi_public_cases import engine_lanes, lanes, wrong_multi_lists
from public_cases import PAIRINGS, SEED, mont, params_of, shape_of, tampered, wrong_lists

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KIND = {"evm": E.ZK_TRANSCRIPT_EVM, "blake2b": E.ZK_TRANSCRIPT_BLAKE2B}
SCHEME = {"gwc": E.ZK_SCHEME_GWC, "shplonk": E.ZK_SCHEME_SHPLONK}


def m_or_none(vals):
    return mont(vals) if vals else None


@pytest.mark.parametrize("kind,scheme", PAIRINGS)
def test_batch_verdicts_are_zk_verify_public_s(kind, scheme):
    eng = zk.Engine(0)
    name, B = "k17like", 17
    usable = shape_of(name).usable_rows
    made = lanes(name, [[0, 1, 9, usable][j % 4] for j in range(B)])
    pk, sets, lists = engine_lanes(eng, name, made)
    vk = eng.vk_read(params_of(name), eng.vk_write(pk))
    t, s = KIND[kind], SCHEME[scheme]
    sd = [bytes([0x30 + j]) * 32 for j in range(B)]
    proofs = eng.prove_batch_public(pk, sets, lists, sd, t, s)
    vals = [v for _, v in made]
    # planted: a wrong list (every variant in turn), a tampered byte, a wrong length
    for what, wrong in wrong_lists(vals[6]):
        use = list(lists)
        use[6] = m_or_none(wrong)
        got = eng.verify_batch_public(pk, proofs, use, t, s)
        assert got == [j != 6 for j in range(B)], what
    bad_proofs, use = list(proofs), list(lists)
    use[2] = m_or_none(wrong_lists(vals[2])[0][1])
    bad_proofs[9] = tampered(proofs[9], shape_of(name), 1, kind, scheme)[0][1]
    bad_proofs[13] = proofs[13][:-32]
    want = [j not in (2, 9, 13) for j in range(B)]
    one_by_one = [eng.verify_public(pk, bad_proofs[j], use[j], t, s) for j in range(B)]
    assert one_by_one == want
    for key in (pk, vk):
        for mode in (0, 1, 2):
            eng.set_verify_instance_eval(mode)
            assert eng.verify_batch_public(key, bad_proofs, use, t, s) == want, mode
            assert eng.verify_batch_public(key, proofs, lists, t, s) == [True] * B, mode
    # an over-long list is an error for the whole call; the context verifies on
    use[4] = mont([0] * (usable + 1))
    with pytest.raises(zk.ZkError) as e:
        eng.verify_batch_public(pk, bad_proofs, use, t, s)
    assert e.value.code == -1
    with pytest.raises(zk.ZkError):
        eng.verify_batch(pk, proofs, t, s)  # (the form without instances still refuses the key)
    assert eng.verify_batch_public(pk, proofs[:1], lists[:1], t, s) == [True]
    eng.close()


@pytest.mark.parametrize("name,lengths", [("k19like", (9, 9)), ("k17like", (0, 9)), ("k17like", (1, 9, 2)), ("wide", (9, 1))])
def test_multi_verdicts(name, lengths):
    eng = zk.Engine(0)
    made = lanes(name, lengths)
    pk, sets, lists = engine_lanes(eng, name, made)
    vk = eng.vk_read(params_of(name), eng.vk_write(pk))
    vals = [v for _, v in made]
    usable = shape_of(name).usable_rows
    for kind, scheme in PAIRINGS:
        t, s = KIND[kind], SCHEME[scheme]
        proof = eng.prove_multi_public(pk, sets, lists, SEED, t, s)
        for mode in (1, 2):
            eng.set_verify_instance_eval(mode)
            for key in (pk, vk):
                assert eng.verify_multi_public(key, proof, lists, t, s), (kind, mode)
            for what, wrong in wrong_multi_lists(vals):
                assert not eng.verify_multi_public(pk, proof, [m_or_none(l) for l in wrong], t, s), (kind, mode, what)
            for place, bad in tampered(proof, shape_of(name), len(lengths), kind, scheme):
                assert not eng.verify_multi_public(pk, bad, lists, t, s), (kind, mode, place)
        with pytest.raises(zk.ZkError) as e:
            eng.verify_multi_public(pk, proof, [lists[0], mont([0] * (usable + 1))] + lists[2:], t, s)
        assert e.value.code == -1
        with pytest.raises(zk.ZkError):
            eng.verify_multi(pk, len(lists), proof, t, s)
    eng.close()


def test_the_fixture_proofs_and_one_circuit():
    with open(os.path.join(HERE, "golden", "multi_public_proofs.json")) as f:
        g = json.load(f)
    eng = zk.Engine(0)
    made = lanes(g["shape"], g["lengths"])
    pk, sets, lists = engine_lanes(eng, g["shape"], made)
    for kind, scheme in PAIRINGS:
        proof = bytes.fromhex(g["proofs"][kind + "/" + scheme])
        for mode in (1, 2):
            eng.set_verify_instance_eval(mode)
            assert eng.verify_multi_public(pk, proof, lists, KIND[kind])
            assert not eng.verify_multi_public(pk, proof, [lists[1], lists[0]], KIND[kind])
    # one circuit is zk_verify_public
    t = E.ZK_TRANSCRIPT_EVM
    one = eng.prove_public(pk, sets[0], lists[0], SEED, t)
    assert eng.verify_multi_public(pk, one, lists[:1], t) and eng.verify_public(pk, one, lists[0], t)
    assert not eng.verify_multi_public(pk, one, lists[1:], t)
    eng.close()
