"""zk_prove_multi (csrc/prover_lockstep.h): ONE proof over N circuits of one key — halo2's create_proof with several circuits.

With one circuit the call is zk_prove, byte for byte, at every prover shape and all four transcript x scheme pairs.  With more it is
compared byte for byte with tests/halo2_ref.py, the plain-Python statement of the rule (tied to the pinned oracle at N = 1 by
tests/test_multi_ref.py): a wrong chain weight of the accumulating quotient passes, a wrong RNG order or a wrong query order each
change the bytes.  The accumulating quotient kernel is driven through the forms a key selects (4 and 16 lanes per row, whole domain,
and one lane per row on three cosets; the 32-term folds of its lazy sums are reached by tests/test_gpu_quotient_device.py only), the merged MSM passes through widths that fill, overflow and split unevenly; refusals leave the
outputs untouched; zk_prove and zk_prove_batch on the same key return the bytes they returned before."""
import ctypes

import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
from zkoracle.hashes import ChaCha20Rng
from prover_shapes import SHAPES
import halo2_ref
from multi_cases import PAIRINGS, SEED, engine_key, oracle_key, params_of, witnesses

pytestmark = pytest.mark.gpu

KIND = {"evm": E.ZK_TRANSCRIPT_EVM, "blake2b": E.ZK_TRANSCRIPT_BLAKE2B}
SCHEME = {"gwc": E.ZK_SCHEME_GWC, "shplonk": E.ZK_SCHEME_SHPLONK}
ALL_PAIRS = [(k, s) for k in ("evm", "blake2b") for s in ("gwc", "shplonk")]


def reference(opk, asgs, kind, scheme):
    return halo2_ref.create_proof(opk, [a.advice for a in asgs], None, ChaCha20Rng(SEED), kind, scheme)


@pytest.mark.parametrize("name", list(SHAPES))
def test_one_circuit_is_zk_prove(name):
    eng = zk.Engine(0)
    asgs = witnesses(name, 1)
    pk, sets = engine_key(eng, name, asgs)
    for kind, scheme in ALL_PAIRS:
        t, s = KIND[kind], SCHEME[scheme]
        want = eng.prove(pk, sets[0], SEED, t, s)
        assert eng.prove_multi(pk, sets, SEED, t, s) == want, (kind, scheme)
        assert eng.proof_size_multi(pk, 1, t, s) == eng.proof_size(pk, t, s) == len(want)
        bad = bytearray(want)
        bad[len(bad) // 2] ^= 1
        for proof in (want, bytes(bad), want[:-1]):
            assert eng.verify_multi(pk, 1, proof, t, s) == eng.verify(pk, proof, t, s) == (proof == want)
    eng.close()


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("name", ["k19like", "k18like", "k17like", "wide", "idle"])
def test_bytes_of_the_reference(name, N):
    eng = zk.Engine(0)
    asgs = witnesses(name, N)
    opk = oracle_key(name, asgs[0])
    pk, sets = engine_key(eng, name, asgs)
    pairs = PAIRINGS + ([("blake2b", "gwc"), ("evm", "shplonk")] if name == "k17like" else [])
    for kind, scheme in pairs:
        got = eng.prove_multi(pk, sets, SEED, KIND[kind], SCHEME[scheme])
        assert got == reference(opk, asgs, kind, scheme), (kind, scheme)
        assert len(got) == eng.proof_size_multi(pk, N, KIND[kind], SCHEME[scheme])
    eng.close()


@pytest.mark.parametrize("name,kind,scheme", [("manycols", "evm", "gwc"), ("manycols_k8", "blake2b", "shplonk")])
def test_accumulating_quotient_many_columns(name, kind, scheme):
    """Both shapes run quotient_sliced_kernel with 16 lanes per row (quotient_log_slices(9, 36) = quotient_log_slices(10, 44) = 4),
    plain for circuit 0 and accumulating for circuit 1: the lanes add their shares through LDS before the pass adds to the running
    quotient.  Per lane at most 3 gate terms, 4 l_0 terms, 2 l_last terms and 4 active-row terms: the row's 36 / 49 / 49 (manycols)
    terms never meet in one sum, so the 32-term fold of the lazy sums is not reached (tests/test_gpu_quotient_device.py does that)."""
    eng = zk.Engine(0)
    asgs = witnesses(name, 2)
    opk = oracle_key(name, asgs[0])
    pk, sets = engine_key(eng, name, asgs)
    # (one pairing per shape: the plain-Python reference takes seconds per proof at these widths)
    assert eng.prove_multi(pk, sets, SEED, KIND[kind], SCHEME[scheme]) == reference(opk, asgs, kind, scheme)
    eng.close()


def test_accumulating_quotient_whole_domain_and_three_cosets():
    """k17like (4 gate columns, k = 7).  Whole domain: 512 rows, quotient_sliced_kernel with 4 lanes per row, per lane 1 gate term,
    3 l_0 terms, 2 l_last terms and 3 active-row terms.  Three cosets: 384 rows are no multiple of 256, so the launcher falls back
    to quotient_kernel, one lane per row with 4 gate terms, 5 l_0 terms, 2 l_last terms and 5 active-row terms.  Each route runs
    its plain form for circuit 0 and its accumulating form for circuit 1; no sum comes near a fold."""
    eng = zk.Engine(0)
    asgs = witnesses("k17like", 2)
    opk = oracle_key("k17like", asgs[0])
    pk, sets = engine_key(eng, "k17like", asgs)
    kind, scheme = PAIRINGS[0]
    want = reference(opk, asgs, kind, scheme)
    for domain in (1, 2):  # 1: the whole extended domain; 2: three of its four cosets, coset-major rows
        eng.set_option(E.ZK_OPT_QUOTIENT_DOMAIN, domain)
        assert eng.prove_multi(pk, sets, SEED, KIND[kind], SCHEME[scheme]) == want, domain
    eng.close()


@pytest.mark.parametrize("name,N", [("k10batched", 3), ("k10batched", 5), ("k10single", 9)])
def test_batched_msm_passes(name, N):
    """k = 10: the commitments go through the window tables in merged passes — a pass that is filled, one that overflows, and an odd
    count above the default pass width.  The proofs are accepted by zk_verify_multi and by the reference verifier (O(1) in n)."""
    eng = zk.Engine(0)
    asgs = witnesses(name, N)
    opk = oracle_key(name, asgs[0])
    pk, sets = engine_key(eng, name, asgs)
    for kind, scheme in PAIRINGS:
        t, s = KIND[kind], SCHEME[scheme]
        proof = eng.prove_multi(pk, sets, SEED, t, s)
        assert eng.verify_multi(pk, N, proof, t, s)
        assert halo2_ref.verify(opk.vk, proof, [[]] * N, kind, scheme)
        assert not eng.verify_multi(pk, N - 1, proof, t, s)
        # every further circuit adds its own points and scalars, nothing else
        sh = opk.shape
        per = (sh.n_adv + 3 * sh.n_lookups + sh.n_chunks) * (64 if kind == "evm" else 32) + 32 * (len(sh.advice_queries) + 3 * sh.n_chunks - 1 + 5 * sh.n_lookups)
        sizes = [eng.proof_size_multi(pk, m, t, s) for m in range(1, E.ZK_PROVE_MULTI_MAX + 1)]
        assert {b - a for a, b in zip(sizes, sizes[1:])} == {per}
        assert len(proof) == sizes[N - 1]
    eng.close()


_DEFAULT_WIDTH = {}


def _default_width_proofs(name, N):
    """(witnesses, {pairing: proof}) of a fresh engine at the default pass width, made once per shape: each proof is accepted by
    zk_verify_multi and by the reference verifier (O(1) in n)."""
    if name not in _DEFAULT_WIDTH:
        eng = zk.Engine(0)
        asgs = witnesses(name, N)
        opk = oracle_key(name, asgs[0])
        pk, sets = engine_key(eng, name, asgs)
        proofs = {}
        for kind, scheme in PAIRINGS:
            proof = eng.prove_multi(pk, sets, SEED, KIND[kind], SCHEME[scheme])
            assert eng.verify_multi(pk, N, proof, KIND[kind], SCHEME[scheme]), (kind, scheme)
            assert halo2_ref.verify(opk.vk, proof, [[]] * N, kind, scheme), (kind, scheme)
            proofs[kind, scheme] = proof
        eng.close()
        _DEFAULT_WIDTH[name] = (asgs, proofs)
    return _DEFAULT_WIDTH[name]


@pytest.mark.parametrize("name", ["k10batched", "k10single"])
@pytest.mark.parametrize("cols", [1, 3, 6, 16])
def test_pass_width_does_not_change_the_proof(cols, name):
    """ZK_OPT_BATCH_PASS_COLUMNS under zk_prove_multi, which shares its passes with zk_prove_batch (tests/test_gpu_prove_batch.py
    test_pass_width_does_not_change_proofs: the same widths).  Six circuits at k = 10, the smallest size at which passes are merged at
    all.  Width 1: every commitment its own pass, and the pipelined route of the one-column key is off (more lanes than a pass
    takes); 3: a circuit's columns split across passes; 6: the pipelined route with as many lanes as a pass takes — the twelve a' /
    s' columns need four passes on two lanes, so the queue collects the advice pass and squeezes theta before it writes any a' —;
    16: wider than the default.  The bytes are those of a fresh engine at the default width, which both verifiers accept."""
    N = 6
    asgs, want = _default_width_proofs(name, N)
    eng = zk.Engine(0)
    eng.set_option(E.ZK_OPT_BATCH_PASS_COLUMNS, cols)
    pk, sets = engine_key(eng, name, asgs)
    for kind, scheme in PAIRINGS:
        assert eng.prove_multi(pk, sets, SEED, KIND[kind], SCHEME[scheme]) == want[kind, scheme], (cols, kind, scheme)
    eng.close()


def _raw_prove_multi(eng, pk, sets, cap, transcript=E.ZK_TRANSCRIPT_BLAKE2B, null_out=False, length=0x5A5A):
    na = len(sets[0])
    hs = (ctypes.c_uint64 * (len(sets) * na))(*[p.h for a in sets for p in a])
    buf = ctypes.create_string_buffer(b"\xa5" * cap, cap) if cap else None
    ln = ctypes.c_size_t(length)
    rc = eng.L.zk_prove_multi(eng.ctx, pk, len(sets), hs, na, SEED, transcript, E.ZK_SCHEME_DEFAULT, None if null_out else buf, cap, ctypes.byref(ln))
    return rc, ln.value, (buf.raw if buf else b"")


def test_refusals():
    eng = zk.Engine(0)
    asgs = witnesses("k19like", 3)
    pk, sets = engine_key(eng, "k19like", asgs)
    size = eng.proof_size_multi(pk, 3)
    for bad_n in (0, E.ZK_PROVE_MULTI_MAX + 1):
        ln = ctypes.c_size_t()
        assert eng.L.zk_proof_size_multi(eng.ctx, pk, bad_n, E.ZK_TRANSCRIPT_BLAKE2B, E.ZK_SCHEME_DEFAULT, ctypes.byref(ln)) == -1
    assert _raw_prove_multi(eng, pk, [sets[0]] * 17, 64)[0] == -1
    hs = (ctypes.c_uint64 * 1)(sets[0][0].h)
    ln = ctypes.c_size_t(7)
    assert eng.L.zk_prove_multi(eng.ctx, pk, 0, hs, 1, SEED, 0, 0, None, 0, ctypes.byref(ln)) == -1 and ln.value == 7
    # a verifying-only key proves nothing
    vk = eng.vk_read(params_of("k19like"), eng.vk_write(pk))
    assert _raw_prove_multi(eng, vk, sets[:2], size)[0] == -5
    # circuit 1 of 3 looks a value up that is off the table: the call fails as a whole, buffer and length as they were
    lay = asgs[1].layout
    ql = asgs[1].fixed[lay.fx_qlookup]
    row = next(r for r in range(lay.usable_rows) if ql[r])
    col = list(asgs[1].advice[0])
    col[row] = 1 << 20
    h = eng.poly(1 << 7)
    eng.upload_canonical(h, zk.circuit.Assignment.to_limbs(col))
    rc, ln_, raw = _raw_prove_multi(eng, pk, [sets[0], [h], sets[2]], size)
    assert (rc, ln_, raw) == (-6, 0x5A5A, b"\xa5" * size)
    assert eng.witness_check(pk, [h])[0][E.ZK_FAIL_LOOKUP] > 0 and eng.witness_check(pk, sets[0])[0][0] == 0  # (which circuit it was)
    # the context proves on: length alone without a buffer, a short buffer as zk_prove treats one
    want = eng.prove_multi(pk, sets, SEED)
    assert _raw_prove_multi(eng, pk, sets, 0, null_out=True)[:2] == (0, len(want))
    rc, ln_, raw = _raw_prove_multi(eng, pk, sets, size - 1)
    hs1 = (ctypes.c_uint64 * 1)(sets[0][0].h)
    one = eng.proof_size(pk)
    buf1 = ctypes.create_string_buffer(b"\xa5" * (one - 1), one - 1)
    ln1 = ctypes.c_size_t(0x5A5A)
    rc1 = eng.L.zk_prove(eng.ctx, pk, hs1, 1, SEED, 0, 0, buf1, one - 1, ctypes.byref(ln1))
    assert (rc, ln_ == size, raw == b"\xa5" * (size - 1)) == (rc1, ln1.value == one, buf1.raw == b"\xa5" * (one - 1))
    rc, ln_, raw = _raw_prove_multi(eng, pk, sets, size)
    assert (rc, ln_, raw) == (0, size, want)
    eng.close()


def test_too_many_grand_products_for_one_scan():
    """manycols has 37 grand products per circuit: seven circuits are 259, beyond the one-workgroup chain scan."""
    eng = zk.Engine(0)
    asgs = witnesses("manycols", 1)
    pk, sets = engine_key(eng, "manycols", asgs)
    assert _raw_prove_multi(eng, pk, sets * 7, 64)[0] == -1
    eng.close()


def test_nothing_else_moves():
    eng = zk.Engine(0)
    asgs = witnesses("k17like", 3)
    pk, sets = engine_key(eng, "k17like", asgs)
    seeds = [bytes([70 + i]) * 32 for i in range(3)]
    t = E.ZK_TRANSCRIPT_EVM
    lone = eng.prove(pk, sets[0], seeds[0], t)
    batch = eng.prove_batch(pk, sets, seeds, t)
    multi = eng.prove_multi(pk, sets, SEED, t)
    assert eng.prove(pk, sets[0], seeds[0], t) == lone
    assert eng.prove_batch(pk, sets, seeds, t) == batch
    assert eng.prove_multi(pk, sets, SEED, t) == multi and eng.verify_multi(pk, 3, multi, t)
    assert batch[0] == lone
    eng.close()


def test_under_the_stream_audit():
    eng = zk.Engine(0)
    eng.set_option(E.ZK_OPT_STREAM_AUDIT, 1)
    asgs = witnesses("k10batched", 3)
    pk, sets = engine_key(eng, "k10batched", asgs)
    try:
        proof = eng.prove_multi(pk, sets, SEED, E.ZK_TRANSCRIPT_EVM)
    except zk.ZkError as e:
        raise AssertionError("%s under the audit: %s" % (e, eng.audit_report())) from e
    checks, violations, msg = eng.audit_report()
    assert violations == 0, msg
    assert checks > 0
    assert eng.verify_multi(pk, 3, proof, E.ZK_TRANSCRIPT_EVM)
    eng.close()
