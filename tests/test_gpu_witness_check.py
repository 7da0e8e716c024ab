"""zk_witness_check on the device — MockProver::verify of resident advice against a resident key — compared with the plain-Python
reference (tests/witness_ref.py): clean witnesses of every shape, exact ordered failure lists for planted corruptions at small k,
the blinded-gate and compressed-selector rules, equivalence with zk_prove's ZK_EWITNESS, file-read keys, the full-size k = 17 and
k = 19 rows, no side effect on proofs, error codes, and the Python layer."""
import ctypes

import numpy as np
import pytest

import webauthn_halo2_amd as zk
import witness_cases as C
import witness_ref as W
from prover_shapes import DRAW_SEED, SHAPES, random_shapes
from webauthn_halo2_amd import engine as E
from zkoracle import cops, prover
from zkoracle.field import R

pytestmark = pytest.mark.gpu

SMALL = [name for name, t in SHAPES.items() if t[3] <= 8]
ADV_SHAPES = {"k19like": SHAPES["k19like"], "k17like": SHAPES["k17like"], "wide": SHAPES["wide"]}


class Case:
    """A key and one set of resident advice columns on `eng` (SRS of the shape's k set up first)."""

    def __init__(self, eng, t, fixed, copies, advice, setup=True):
        self.eng, self.t, self.p = eng, t, C.params_of(t)
        self.n = 1 << self.p.degree
        if setup:
            eng.srs_setup(self.p.degree)
        self.pk = eng.keygen(self.p, np.stack([C.limbs(c) for c in fixed]), copies)
        self.polys = [eng.poly(self.n) for _ in advice]
        self.load(advice)

    def load(self, advice):
        for h, col in zip(self.polys, advice):
            self.eng.upload_canonical(h, col if isinstance(col, np.ndarray) else C.limbs(col))

    def check(self, cap=64, pk=None):
        return self.eng.witness_check(self.pk if pk is None else pk, self.polys, cap)

    def close(self):
        for h in self.polys:
            h.free()
        self.eng.pk_free(self.pk)


def assert_clean(case):
    counts, failures = case.check()
    assert counts == [0, 0, 0, 0, 0] and failures == []


# ---- 1. clean witnesses ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_clean_witness_of_every_shape(engine, name):
    sh, fixed, copies, advice = C.synth_case(SHAPES[name])
    case = Case(engine, SHAPES[name], fixed, copies, advice)
    assert_clean(case)
    case.close()


@pytest.mark.parametrize("t", random_shapes(20, DRAW_SEED), ids=lambda t: "A%dL%dF%dk%dlb%di%d" % t)
def test_clean_witness_of_random_shapes(engine, t):
    sh, fixed, copies, advice = C.synth_case(t, 0x5EED0019 + 5)
    case = Case(engine, t, fixed, copies, advice)
    assert_clean(case)
    case.close()


@pytest.mark.parametrize("name", list(ADV_SHAPES))
@pytest.mark.parametrize("seed", [7, 1234, 99])
def test_clean_adversarial_layouts(engine, name, seed):
    sh, fixed, copies, advice = C.adv_case(ADV_SHAPES[name], seed)
    case = Case(engine, ADV_SHAPES[name], fixed, copies, advice)
    assert_clean(case)
    case.close()


# ---- 2. exact lists at small k -------------------------------------------------------------------------------------------------
def exact_lists(engine, t, fixed, copies, advice, seed):
    sh = W.shape_of(t)
    bad, cells = C.plant(sh, fixed, copies, advice, seed)
    want = W.check(sh, fixed, copies, bad)
    assert want, "the planted cells must violate something"
    case = Case(engine, t, fixed, copies, bad)
    try:
        counts, got = case.check(cap=len(want) + 7)
        print("shape", t, "seed", seed, "cells", cells, "counts", counts)
        assert counts == W.counts(want)
        assert got == want
        for cap in sorted({0, 1, len(want) - 1}):
            c2, g2 = case.check(cap=cap)
            assert c2 == counts and g2 == want[:cap], cap
        case.load(advice)  # the satisfying witness on the same key, after failing checks
        assert_clean(case)
    finally:
        case.close()


@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_exact_failure_lists(engine, name, seed):
    sh, fixed, copies, advice = C.synth_case(SHAPES[name], 0x5EED0019 + seed)
    exact_lists(engine, SHAPES[name], fixed, copies, advice, 100 * seed + 17)


@pytest.mark.parametrize("name", list(ADV_SHAPES))
@pytest.mark.parametrize("seed", [7, 1234, 99])
def test_exact_failure_lists_adversarial(engine, name, seed):
    sh, fixed, copies, advice = C.adv_case(ADV_SHAPES[name], seed)
    exact_lists(engine, ADV_SHAPES[name], fixed, copies, advice, seed + 1)


# ---- 3. ZK_FAIL_GATE_BLINDED -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k19like", "k17like"])
def test_gate_selector_on_a_blinded_window(engine, name):
    sh, fixed, copies, advice = C.synth_case(SHAPES[name])
    fixed = [list(c) for c in fixed]
    j = sh.n_gate - 1
    row = sh.usable_rows - 2
    fixed[sh.fx_sel[j]][row] = 1
    want = [(W.GATE_BLINDED, j, row, 0, 0)]
    assert W.check(sh, fixed, copies, advice) == want
    case = Case(engine, SHAPES[name], fixed, copies, advice)
    assert case.check() == ([1, 0, 1, 0, 0], want)
    adv = [list(c) for c in advice]
    for r in range(sh.usable_rows, sh.n):  # whatever the window's blinded rows hold (its two usable rows belong to real gates too)
        adv[j][r] = (r * 977 + 5) % R
    assert W.check(sh, fixed, copies, adv) == want
    case.load(adv)
    assert case.check() == ([1, 0, 1, 0, 0], want)
    case.close()


# ---- 4. compressed selectors -----------------------------------------------------------------------------------------------------
def test_idle_gate_columns_produce_no_gate_failure(engine):
    t = SHAPES["idle"]
    sh, fixed, copies, advice = C.synth_case(t)
    A, idle = t[0], t[5]
    adv = [list(c) for c in advice]
    for j in range(A - idle, A):  # never-enabled gate columns: a + b c != d everywhere
        for r in range(sh.usable_rows):
            adv[j][r] = (3 * r + j + 1) % R
    assert W.check(sh, fixed, copies, adv) == []
    case = Case(engine, t, fixed, copies, adv)
    assert_clean(case)
    # gate 0 shares its selector column with the first never-enabled one (form q (2 - q)): a broken gate there is seen
    row = next(r for r in range(sh.usable_rows - 3) if fixed[sh.fx_sel[0]][r])
    adv[0][row + 3] = (adv[0][row + 3] + 1) % R
    want = W.check(sh, fixed, copies, adv)
    assert (W.GATE, 0, row, 0, 0) in want and all(f[1] < A - idle for f in want if f[0] == W.GATE)
    case.load(adv)
    counts, got = case.check()
    assert got == want and counts == W.counts(want)
    case.close()


# ---- 5. lookup equivalence -------------------------------------------------------------------------------------------------------
def test_lookup_failures_iff_prove_refuses(engine):
    tried = 0
    for name in ("k19like", "wide", "k17like"):
        t = SHAPES[name]
        sh, fixed, copies, advice = C.synth_case(t)
        case = Case(engine, t, fixed, copies, advice)
        T = 1 << sh.lookup_bits
        if sh.single:
            looked = [(0, r) for r in range(sh.usable_rows) if fixed[sh.fx_qlookup][r]]
            unlooked = [(0, r) for r in range(sh.usable_rows) if not fixed[sh.fx_qlookup][r]]
        else:
            looked = [(sh.n_gate + l, r) for l in range(sh.n_lookup_cols) for r in (0, 5, sh.usable_rows - 1)]
            unlooked = []
        witnesses = [(advice, False)]
        for i, (j, r) in enumerate(looked[:3]):
            adv = [list(c) for c in advice]
            adv[j][r] = (T, R - 1, T + 12345)[i % 3]
            witnesses.append((adv, True))
        for j, r in unlooked[:1]:  # a large value where q_lookup = 0 is no lookup input (a broken gate at most)
            adv = [list(c) for c in advice]
            adv[j][r] = R - 1 if adv[j][r] != R - 1 else R - 2
            witnesses.append((adv, False))
        for adv, off_table in witnesses:
            case.load(adv)
            counts, _ = case.check()
            assert (counts[E.ZK_FAIL_LOOKUP] != 0) == off_table == (W.counts(W.check(sh, fixed, copies, adv))[W.LOOKUP] != 0)
            if off_table or counts[0] == 0 or sh.single:
                try:
                    engine.prove(case.pk, case.polys, bytes(32), E.ZK_TRANSCRIPT_EVM)
                    refused = False
                except zk.ZkError as e:
                    assert e.code == -6
                    refused = True
                assert refused == off_table
                tried += 1
        case.close()
    assert tried >= 10


# ---- 6. file-read keys -----------------------------------------------------------------------------------------------------------
def sigma_offset(sh, c, r):
    """Byte offset of sigma value (c, r) in a RawBytes ProvingKey::write image."""
    n, N = sh.n, 4 * sh.n
    n_sel = sh.n_gate + (1 if sh.single else 0)
    vk = 8 + (sh.n_fix + len(sh.perm_cols)) * 64 + n_sel * (n // 8)
    ext3 = 3 * (4 + N * 32)
    fixed = 2 * (4 + sh.n_fix * (4 + n * 32)) + (4 + sh.n_fix * (4 + N * 32))
    return vk + ext3 + fixed + 4 + c * (4 + n * 32) + 4 + r * 32


@pytest.mark.parametrize("name", ["k17like", "k19like"])
def test_file_read_keys(engine, name):
    t = SHAPES[name]
    sh, fixed, copies, advice = C.synth_case(t)
    bad, _ = C.plant(sh, fixed, copies, advice, 41)
    case = Case(engine, t, fixed, copies, bad)
    want = case.check(cap=4096)
    assert want[1] == W.check(sh, fixed, copies, bad)
    img = engine.pk_write(case.pk, E.ZK_SERDE_RAW_BYTES)
    pk2 = engine.pk_read(case.p, img, E.ZK_SERDE_RAW_BYTES)
    assert case.check(cap=4096, pk=pk2) == want
    engine.pk_free(pk2)
    # one sigma value overwritten by something that is no label delta^c w^r (zero), read without validation
    c, r = len(sh.perm_cols) - 1, 9
    off = sigma_offset(sh, c, r)
    sigma = prover.build_sigma(sh, copies)
    assert bytes(img[off:off + 32]) == cops.fr_mont([sigma[c][r]]).tobytes()  # (the offset is the sigma value's)
    img = img.copy()
    img[off:off + 32] = 0
    pk3 = engine.pk_read(case.p, img, E.ZK_SERDE_RAW_BYTES_UNCHECKED)
    for _ in range(2):  # the verdict on the key is kept
        with pytest.raises(zk.ZkError) as e:
            case.check(pk=pk3)
        assert e.value.code == -1
    engine.pk_free(pk3)
    assert case.check(cap=4096) == want
    case.close()


# ---- 7. / 8. full size -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["K17", "K19"])
def full(request, engine):
    p = getattr(zk.circuit, request.param)
    t = (p.num_advice, p.num_lookup_advice, p.num_fixed, p.degree, p.lookup_bits)
    asg = zk.circuit.synthesize(p, 0x5EED0019)
    engine.srs_setup(p.degree)
    case = Case.__new__(Case)
    case.eng, case.t, case.p, case.n = engine, t, p, 1 << p.degree
    case.pk = engine.keygen(p, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
    case.polys = [engine.poly(case.n) for _ in asg.advice]
    case.limbs = [asg.to_limbs(c) for c in asg.advice]
    case.load(case.limbs)
    case.asg, case.sh = asg, W.shape_of(t)
    yield case
    case.close()


def put_cell(case, adv, j, r, v):
    """Advice as lists with one cell changed; the column goes to the device."""
    adv = [adv[i] if i != j else list(adv[i]) for i in range(len(adv))]
    adv[j][r] = v
    a = case.limbs[j].copy()
    a[r] = C.limbs([v])[0]
    case.eng.upload_canonical(case.polys[j], a)
    return adv


def test_full_size_clean_pair_and_gate(full, engine):
    case, sh, asg = full, full.sh, full.asg
    F = sh.num_fixed
    assert_clean(case)
    # (a) one member of a copy PAIR
    cyc = C.cycles(asg.copies)
    pair = next(c for c in cyc if len(c) == 2 and all(col >= F for col, _ in c))
    (ca, ra), (cb, rb) = pair
    adv = put_cell(case, asg.advice, ca - F, ra, (asg.advice[ca - F][ra] + 1) % R)
    want = sorted((W.gate_failures_around(sh, asg.fixed, adv, ca - F, ra) if ca - F < sh.n_gate else []) +
                  W.lookup_failures_at(sh, asg.fixed, adv, ca - F, ra) +  # (a cell that held 2^lookup_bits - 1 leaves the table by + 1)
                  [(W.COPY, ca, ra, cb, rb), (W.COPY, cb, rb, ca, ra)])
    counts, got = case.check()
    print(case.p.degree, "pair", pair, counts, got)
    assert got == want and counts == W.counts(want) and counts[E.ZK_FAIL_COPY] == 2
    # (b) one gate output that no copy constraint names
    in_cycle = {cell for c in cyc for cell in c}
    row = next(r for r in range(4 * 1000, sh.usable_rows - 3, 4) if asg.fixed[sh.fx_sel[0]][r] and (F, r + 3) not in in_cycle)
    case.load(case.limbs)
    adv = put_cell(case, asg.advice, 0, row + 3, (asg.advice[0][row + 3] + 1) % R)
    want = W.gate_failures_around(sh, asg.fixed, adv, 0, row + 3)
    assert (W.GATE, 0, row, 0, 0) in want
    counts, got = case.check()
    print(case.p.degree, "gate", row, counts, got)
    assert got == want and counts == W.counts(want)
    if case.p.degree == 19:
        # the point of the feature: the prover proves the broken witness without a word, no verifier accepts the proof, and the
        # check names the row
        proof = engine.prove(case.pk, case.polys, b"\x09" * 32, E.ZK_TRANSCRIPT_BLAKE2B)
        assert not engine.verify(case.pk, proof, E.ZK_TRANSCRIPT_BLAKE2B)
        assert case.check()[1] == want
    case.load(case.limbs)
    assert_clean(case)
    proof = engine.prove(case.pk, case.polys, b"\x09" * 32, E.ZK_TRANSCRIPT_BLAKE2B)
    assert engine.verify(case.pk, proof, E.ZK_TRANSCRIPT_BLAKE2B)


def test_many_failures_are_listed_deterministically(full, engine):
    """10 000 broken gates, cap 64: two calls give the same list — the first 64 in (kind, index, row) order."""
    case, sh = full, full.sh
    a = case.limbs[0].copy()
    rows = [r for r in range(0, sh.usable_rows - 3, 4) if case.asg.fixed[sh.fx_sel[0]][r]][:10000]
    for r in rows:
        a[r + 3, 0] ^= np.uint64(1)
    engine.upload_canonical(case.polys[0], a)
    c1, f1 = case.check(cap=64)
    c2, f2 = case.check(cap=64)
    assert (c1, f1) == (c2, f2) and c1[E.ZK_FAIL_GATE] >= 10000 and len(f1) == 64
    assert f1 == [(E.ZK_FAIL_GATE, 0, r, 0, 0) for r in rows[:64]]
    assert f1 == sorted(f1)
    case.load(case.limbs)
    assert_clean(case)


# ---- 8. no side effects ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k10single", "k10batched"])
def test_check_leaves_proofs_alone_and_is_ordered_under_the_audit(name):
    eng = zk.Engine(0)
    eng.set_option(E.ZK_OPT_STREAM_AUDIT, 1)
    t = SHAPES[name]
    sh, fixed, copies, advice = C.synth_case(t)
    case = Case(eng, t, fixed, copies, advice)
    seed = b"\x33" * 32
    before = eng.prove(case.pk, case.polys, seed, E.ZK_TRANSCRIPT_EVM)
    assert_clean(case)
    assert eng.prove(case.pk, case.polys, seed, E.ZK_TRANSCRIPT_EVM) == before
    bad, _ = C.plant(sh, fixed, copies, advice, 5)
    case.load(bad)
    counts, got = case.check(cap=4096)
    assert got == W.check(sh, fixed, copies, bad)
    case.load(advice)
    assert eng.prove(case.pk, case.polys, seed, E.ZK_TRANSCRIPT_EVM) == before
    for _ in range(3):  # interleaved on one context
        assert_clean(case)
        assert eng.prove(case.pk, case.polys, seed, E.ZK_TRANSCRIPT_BLAKE2B) == eng.prove(case.pk, case.polys, seed, E.ZK_TRANSCRIPT_BLAKE2B)
    checks, violations, msg = eng.audit_report()
    assert checks > 0 and violations == 0, msg
    case.close()
    eng.close()


# ---- 9. errors -------------------------------------------------------------------------------------------------------------------
def test_error_codes(engine):
    t = SHAPES["k17like"]
    sh, fixed, copies, advice = C.synth_case(t)
    case = Case(engine, t, fixed, copies, advice)
    L = engine.L
    hs = (ctypes.c_uint64 * len(case.polys))(*[p.h for p in case.polys])
    counts = (ctypes.c_uint64 * 5)(*[77] * 5)
    out = (E.WitnessFailureC * 4)()

    def call(pk, handles, n_adv, outp, cap):
        rc = L.zk_witness_check(engine.ctx, pk, handles, n_adv, outp, cap, counts)
        assert list(counts) == [77] * 5 or rc == 0  # outputs untouched on error
        return rc

    assert call(case.pk, hs, len(case.polys), out, 4) == 0 and list(counts) == [0] * 5
    counts[:] = [77] * 5
    assert call(case.pk, hs, len(case.polys) - 1, out, 4) == -1   # wrong n_advice
    assert call(case.pk, hs, len(case.polys), None, 4) == -1      # cap > 0 without a buffer
    assert call(case.pk + 1000, hs, len(case.polys), out, 4) == -1  # no such key
    short = engine.poly(case.n // 2)
    hs2 = (ctypes.c_uint64 * len(case.polys))(*([short.h] + [p.h for p in case.polys[1:]]))
    assert call(case.pk, hs2, len(case.polys), out, 4) == -1       # a vector of another length
    hs2[0] = 0xDEAD0000
    assert call(case.pk, hs2, len(case.polys), out, 4) == -1       # no such vector
    short.free()
    vk = engine.vk_read(case.p, engine.vk_write(case.pk))
    assert call(vk, hs, len(case.polys), out, 4) == -5             # verifying-only key: ZK_ESTATE
    fc, pc, tr = engine.vk_export(case.pk)
    vk2 = engine.vk_from_parts(case.p, fc, pc, tr)
    assert call(vk2, hs, len(case.polys), out, 4) == -5
    engine.pk_free(vk)
    engine.pk_free(vk2)
    engine.srs_setup(t[3], b"\x01" * 32)                           # the key's SRS replaced
    assert call(case.pk, hs, len(case.polys), out, 4) == -5
    case.close()


# ---- 10. the Python layer --------------------------------------------------------------------------------------------------------
def test_python_layer(tmp_path):
    api = zk.ecdsa_p256
    api.shutdown()
    pkp = str(tmp_path / "proving_key.pk")
    try:
        api.download_keys(17, pkp)
        p = zk.circuit.K17
        asg = zk.circuit.synthesize(p, 0x5EED0019 + 1)
        cols = [asg.to_limbs(c) for c in asg.advice]
        assert api.mock_verify_advice(cols, pkp, 17) == []
        plain = api.create_proof_from_advice(cols, pkp, 17, E.ZK_TRANSCRIPT_EVM, rng_seed=bytes(32))
        assert api.create_proof_from_advice(cols, pkp, 17, E.ZK_TRANSCRIPT_EVM, rng_seed=bytes(32), check=True) == plain
        sh = W.shape_of((p.num_advice, p.num_lookup_advice, p.num_fixed, p.degree, p.lookup_bits))
        in_cycle = {cell for c in C.cycles(asg.copies) for cell in c}
        row = next(r for r in range(400, sh.usable_rows - 3, 4) if asg.fixed[sh.fx_sel[2]][r] and (sh.num_fixed + 2, r + 3) not in in_cycle)
        bad = [c.copy() for c in cols]
        bad[2][row + 3, 0] ^= np.uint64(1)
        want = [(E.ZK_FAIL_GATE, 2, row, 0, 0)]
        assert api.mock_verify_advice(bad, pkp, 17) == want
        with pytest.raises(api.WitnessError) as e:
            api.create_proof_from_advice(bad, pkp, 17, E.ZK_TRANSCRIPT_EVM, rng_seed=bytes(32), check=True)
        assert e.value.failures == want and e.value.counts == [1, 1, 0, 0, 0]
        assert isinstance(e.value, ValueError)
        assert api.create_proof_from_advice(cols, pkp, 17, E.ZK_TRANSCRIPT_EVM, rng_seed=bytes(32), check=True) == plain
    finally:
        api.shutdown()
