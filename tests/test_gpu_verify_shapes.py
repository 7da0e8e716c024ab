"""zk_verify / zk_verify_batch at every shape the prover is tested at (csrc/verify.hip): device proofs of the prover's shape
families, of the random draw and of adversarial layouts in all four transcript x scheme combinations, with their tampered variants;
every full-size bench_ecdsa.config row (KZG term lists of hundreds to thousands of terms: several per lane of verify_msm_kernel);
a key with an identity commitment; batch sizes at the fold's 64-term segment edges and at ZK_VERIFY_BATCH_MAX; and, through the
stream audit's check count, that an all-valid batch settles with one fold."""
import random

import numpy as np
import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
from zkoracle import cops, plonk, prover
from zkoracle.hashes import ChaCha20Rng
from prover_shapes import BENCH_ROWS, DRAW_SEED, SHAPES, random_shapes
import adversarial_layout as adv
import test_gpu_prover as tp
import verify_cases as vc

pytestmark = pytest.mark.gpu
T = {"evm": E.ZK_TRANSCRIPT_EVM, "blake2b": E.ZK_TRANSCRIPT_BLAKE2B}
S = {"gwc": E.ZK_SCHEME_GWC, "shplonk": E.ZK_SCHEME_SHPLONK}
REFERENCE_PAIRINGS = (("blake2b", "shplonk"), ("evm", "gwc"))


def upload(engine, k, cols):
    hs = []
    for col in cols:
        h = engine.poly(1 << k)
        engine.upload_canonical(h, tp._limbs(col))
        hs.append(h)
    return hs


def label(case):
    return case if isinstance(case, str) else "A%dL%dF%dk%dlb%di%d" % case


# the prover's shape families (k19like / k17like are tests/test_gpu_verify.py's), the head of its random draw, two adversarial layouts
SHAPE_CASES = ([n for n in SHAPES if n not in ("k19like", "k17like")] + random_shapes(8, DRAW_SEED)
               + ["adversarial-8-1234", "adversarial-9-1234"])
ADVERSARIAL = {"adversarial-8-1234": ((8, 3, 2, 2, 5), 1234), "adversarial-9-1234": ((9, 4, 1, 1, 6), 1234)}


@pytest.mark.parametrize("case", SHAPE_CASES, ids=label)
def test_shape_families_same_verdicts_as_oracle(engine, case):
    if case in ADVERSARIAL:
        (k, A, L, F, lb), seed = ADVERSARIAL[case]
        sh = plonk.Shape(k, A, L, F, lb)
        fixed, copies, advice = adv.build(sh, seed)
        p = vc.params_of_shape((A, L, F, k, lb))
        engine.srs_setup(k)
        pk = engine.keygen(p, np.stack([tp._limbs(c) for c in fixed]), copies)
        polys = upload(engine, k, advice)
    else:
        A, L, F, k, lb, idle = (tuple(SHAPES[case] if isinstance(case, str) else case) + (0,))[:6]
        p, _, pk, polys = tp.setup(engine, A, L, F, k, lb, idle=idle)
        sh = plonk.Shape(k, A, L, F, lb, idle)
    ovk = tp.product_vk(engine, pk, sh)
    fc, pc, tr = engine.vk_export(pk)
    vko = engine.vk_from_parts(p, fc, pc, tr)
    try:
        for kind, scheme in vc.COMBOS:
            proof = engine.prove(pk, polys, bytes([k, sh.num_advice & 255, kind == "evm", scheme == "gwc"]) * 8, T[kind], S[scheme])
            cases = [("intact", proof)] + vc.variants(proof, sh, kind, scheme, seed=sum(map(ord, label(case) + kind + scheme)))
            want = [plonk.verify(ovk, c[1], kind, scheme) for c in cases]
            assert want[0] and not any(want[1:]), (kind, scheme)
            got = [engine.verify(pk, c[1], T[kind], S[scheme]) for c in cases]
            assert got == want, (kind, scheme, [c[0] for c, g, w in zip(cases, got, want) if g != w])
            assert engine.verify_batch(vko, [c[1] for c in cases], T[kind], S[scheme]) == want, (kind, scheme)
    finally:
        engine.pk_free(vko)
        engine.pk_free(pk)
        for h in polys:
            h.free()


# ---- every full-size bench row: one key per row (its own context, so that no other test's SRS replaces it while the row's tests run)
@pytest.fixture(scope="module", params=BENCH_ROWS, ids=lambda r: "k%d" % r[0])
def bench_row(request):
    k, A, L, F, lb, size, idle = request.param
    eng = zk.Engine(0)
    try:
        p, _, pk, polys = tp.setup(eng, A, L, F, k, lb, idle=idle)
        sh = plonk.Shape(k, A, L, F, lb, idle)
        row = {"eng": eng, "p": p, "pk": pk, "sh": sh, "ovk": tp.product_vk(eng, pk, sh), "proofs": {}}
        for kind, scheme in REFERENCE_PAIRINGS:
            row["proofs"][kind, scheme] = eng.prove(pk, polys, bytes([k, 3]) * 16, T[kind], S[scheme])
            assert len(row["proofs"][kind, scheme]) == eng.proof_size(pk, T[kind], S[scheme])
        for h in polys:
            h.free()
        yield row
        eng.pk_free(pk)
    finally:
        eng.close()


@pytest.mark.parametrize("kind,scheme", REFERENCE_PAIRINGS)
def test_bench_row_verdicts(bench_row, kind, scheme):
    eng, pk, sh, ovk = bench_row["eng"], bench_row["pk"], bench_row["sh"], bench_row["ovk"]
    proof = bench_row["proofs"][kind, scheme]
    bad = vc.variants(proof, sh, kind, scheme, seed=sh.k)
    assert eng.verify(pk, proof, T[kind], S[scheme])
    got = [eng.verify(pk, b, T[kind], S[scheme]) for _, b in bad]
    assert not any(got), [lb for (lb, _), g in zip(bad, got) if g]
    # the oracle on the intact proof and on a bit flip and a bad point (one oracle verification takes seconds at k = 11)
    assert plonk.verify(ovk, proof, kind, scheme)
    for lb, b in (bad[0], next(x for x in bad if x[0].startswith("h point"))):
        assert not plonk.verify(ovk, b, kind, scheme), lb
    assert eng.verify_batch(pk, [proof] + [b for _, b in bad] + [proof], T[kind], S[scheme]) == [True] + [False] * len(bad) + [True]


def test_bench_row_vk_file_round_trip(bench_row):
    """zk_vk_write -> zk_vk_read (the path of ecdsa_p256.verify and the server): the key read back verifies both pairings."""
    eng, p, pk, sh = bench_row["eng"], bench_row["p"], bench_row["pk"], bench_row["sh"]
    vkr = eng.vk_read(p, eng.vk_write(pk))
    try:
        assert eng.vk_export(vkr)[2].tolist() == eng.vk_export(pk)[2].tolist()
        for (kind, scheme), proof in bench_row["proofs"].items():
            bad = bytearray(proof)
            bad[len(bad) // 2] ^= 1
            assert eng.verify(vkr, proof, T[kind], S[scheme]) and not eng.verify(vkr, bytes(bad), T[kind], S[scheme])
            assert eng.verify_batch(vkr, [bytes(bad), proof, proof], T[kind], S[scheme]) == [False, True, True]
    finally:
        eng.pk_free(vkr)


# ---- a key with an identity commitment
def test_identity_commitment_key(engine):
    p, asg = vc.identity_assignment()
    k = p.degree
    sh = vc.oracle_shape(p)
    opk = prover.keygen(prover.Circuit(sh, asg.fixed, asg.copies, asg.advice))
    assert opk.vk.fixed_commitments.count(None) == 1
    engine.srs_setup(k)
    pk = engine.keygen(p, np.stack([tp._limbs(c) for c in asg.fixed]), asg.copies)
    polys = upload(engine, k, asg.advice)
    fc, pc, tr = engine.vk_export(pk)
    keys = [pk]
    try:
        assert [not fc[i].any() for i in range(len(fc))] == [c is None for c in opk.vk.fixed_commitments]  # (0, 0) where None
        assert cops.affine_arr_to_ints(fc) == opk.vk.fixed_commitments
        assert cops.affine_arr_to_ints(pc) == opk.vk.permutation_commitments
        assert cops.fr_ints(tr.reshape(1, 4))[0] == opk.vk.transcript_repr
        seed = b"\x29" * 32
        for kind, scheme in REFERENCE_PAIRINGS:
            assert engine.prove(pk, polys, seed, T[kind], S[scheme]) == prover.create_proof(opk, asg.advice, ChaCha20Rng(seed), kind, scheme)
        keys.append(engine.vk_from_parts(p, fc, pc, tr))
        keys.append(engine.vk_read(p, engine.vk_write(pk)))  # (its transcript_repr made again from the file's commitments)
        assert engine.vk_export(keys[2])[2].tolist() == tr.tolist()
        for kind, scheme in vc.COMBOS:
            proof = engine.prove(pk, polys, seed, T[kind], S[scheme])
            cases = [("intact", proof)] + vc.variants(proof, sh, kind, scheme, seed=sum(map(ord, kind + scheme)))
            want = [plonk.verify(opk.vk, c[1], kind, scheme) for c in cases]
            assert want[0] and not any(want[1:])
            for key in keys:
                assert [engine.verify(key, c[1], T[kind], S[scheme]) for c in cases] == want, (kind, scheme, key)
                assert engine.verify_batch(key, [c[1] for c in cases] + [proof], T[kind], S[scheme]) == want + [True]
    finally:
        for key in keys:
            engine.pk_free(key)
        for h in polys:
            h.free()


# ---- batches: sizes at the fold's segment edges, proofs that leave before the device sums
class Pool:
    """Proofs of one k19like key in one combination: valid ones, ones that reach the device sums and fail the pairing (an evaluation
    changed), and ones that leave the batch before the sums (wrong length, an undecodable point, a non-canonical scalar)."""

    def __init__(self, engine, kind, scheme):
        self.p, self.pk, self.adv, self.ovk, parts = k19like_key(engine)
        self.vko = engine.vk_from_parts(self.p, *parts)
        self.engine, self.kind, self.scheme = engine, kind, scheme
        self.good = [engine.prove(self.pk, self.adv, bytes([i + 1]) * 32, T[kind], S[scheme]) for i in range(8)]
        ev0 = self.ovk.shape.n_points_before_multiopen() * (64 if kind == "evm" else 32)
        low = ev0 + 31 if kind == "evm" else ev0  # the low byte of the first evaluation: a flip keeps it canonical
        self.late = []
        for i, g in enumerate(self.good[:4]):
            b = bytearray(g)
            b[low] ^= 1 << i
            self.late.append(bytes(b))
        want = {"truncated", "extended", "empty", "first point: off curve", "first point: zero", "scalar = r"}
        self.early = [b for g in self.good[:3] for lb, b in vc.variants(g, self.ovk.shape, kind, scheme) if lb in want]
        self.single = {}

    def verdict(self, x):
        if x not in self.single:
            self.single[x] = self.engine.verify(self.vko, x, T[self.kind], S[self.scheme])
        return self.single[x]

    def close(self):
        self.engine.pk_free(self.vko)
        self.engine.pk_free(self.pk)
        for h in self.adv:
            h.free()


def k19like_key(engine):
    p = vc.params_of("k19like")
    _, _, pk, polys = tp.setup(engine, p.num_advice, p.num_lookup_advice, p.num_fixed, p.degree, p.lookup_bits)
    fc, pc, tr = engine.vk_export(pk)
    return p, pk, polys, tp.product_vk(engine, pk, vc.oracle_shape(p)), (fc, pc, tr)


@pytest.mark.parametrize("kind,scheme", REFERENCE_PAIRINGS)
def test_batch_edges(engine, kind, scheme):
    pool = Pool(engine, kind, scheme)
    rnd = random.Random(sum(map(ord, kind + scheme)))
    try:
        assert all(pool.verdict(g) for g in pool.good)
        assert not any(pool.verdict(x) for x in pool.late + pool.early)
        for x in pool.late[:2] + pool.early[:6:2]:
            assert not plonk.verify(pool.ovk, x, kind, scheme)
        for B in (63, 64, 65, 127, 128, 129, E.ZK_VERIFY_BATCH_MAX):
            masks = [["good"] * B]
            m = ["good"] * B
            for at in (0, 64, B - 1):
                if at < B:
                    m[at] = "late"
            masks.append(m)
            masks.append([rnd.choice(["good", "good", "good", "late", "early"]) for _ in range(B)])
            masks.append(["early"] * B)
            m = ["early"] * B
            m[rnd.randrange(B)] = "good"  # one survivor: no fold
            masks.append(m)
            for m in masks:
                batch = [rnd.choice(getattr(pool, w)) for w in m]
                got = engine.verify_batch(pool.vko, batch, T[kind], S[scheme])
                assert got == [pool.verdict(x) for x in batch], (B, [w for w, g in zip(m, got) if g != (w == "good")][:5])
    finally:
        pool.close()


def test_valid_batch_settles_with_one_fold(engine):
    """The fold is used, not bypassed: a broken fold (each subset's pairing fails) still gives exact verdicts through bisection, so
    verdicts cannot show it.  The stream audit counts a fixed number of ordering checks per zk_verify_batch call and a fixed number
    per fold (its uploads, launch and download): 256 valid proofs must cost exactly what 2 do — one fold — and one bad proof among
    256 must cost more (about log2(256) levels of folds)."""
    pool = Pool(engine, "evm", "gwc")
    tr, sc = T["evm"], S["gwc"]
    engine.set_option(E.ZK_OPT_STREAM_AUDIT, 1)

    def checks(batch):
        c0 = engine.audit_report()[0]
        v = engine.verify_batch(pool.vko, batch, tr, sc)
        return v, engine.audit_report()[0] - c0

    try:
        checks(pool.good[:2])  # (the key's commitments go to the device once, on its first verify)
        # the per-call count does not depend on the batch size: one survivor among 2 and among 256 (no fold either way)
        v_a, d_a = checks([pool.good[0], pool.early[0]])
        v_b, d_b = checks([pool.good[0]] + [pool.early[i % len(pool.early)] for i in range(255)])
        assert v_a == [True, False] and v_b == [True] + [False] * 255 and d_a == d_b > 0
        v2, d2 = checks(pool.good[:2])
        v256, d256 = checks([pool.good[i % 8] for i in range(256)])
        assert v2 == [True] * 2 and v256 == [True] * 256
        assert d256 == d2 > d_a  # one fold, the same for 2 and 256 proofs
        batch = [pool.good[i % 8] for i in range(256)]
        batch[100] = pool.late[0]
        vbad, dbad = checks(batch)
        assert vbad == [i != 100 for i in range(256)]
        assert dbad > d256 + 6 * (d256 - d_a), (d_a, d256, dbad)  # at least 7 more folds
        _, violations, msg = engine.audit_report()
        assert violations == 0, msg
    finally:
        engine.set_option(E.ZK_OPT_STREAM_AUDIT, 0)
        pool.close()
