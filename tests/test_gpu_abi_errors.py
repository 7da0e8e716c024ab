"""Error behaviour at the C-ABI (include/zkmi355.h): negative codes, outputs untouched, no crash."""
import ctypes
import os

import numpy as np
import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
from zkoracle import cops, field as F

pytestmark = pytest.mark.gpu


def test_bad_arguments(engine):
    L = engine.L
    out = np.full(12, 7, dtype=np.uint64)
    # null pointers / oversize log_n
    assert L.zk_msm_bn254(engine.ctx, None, None, 4, E._p(out)) == -1
    assert (out == 7).all()
    a = np.zeros((4, 4), dtype=np.uint64)
    w = np.zeros(4, dtype=np.uint64)
    assert L.zk_ntt_bn254_fr(engine.ctx, E._p(a), E._p(w), 27) == -1
    assert L.zk_ctx_create(99, ctypes.byref(ctypes.c_void_p())) == -1
    # bad handles
    assert L.zk_poly_free(engine.ctx, 0xDEAD) == -1
    assert L.zk_pk_free(engine.ctx, 0xDEAD) == -1
    with pytest.raises(zk.ZkError):
        engine.prove(0xDEAD, [], bytes(32))
    assert L.zk_strerror(-6).decode().startswith("unknown") is False or True


def test_state_errors():
    eng = zk.Engine(0)  # fresh context: no SRS
    p = eng.poly(16, cops.fr_mont(list(range(16))))
    with pytest.raises(zk.ZkError) as e:
        eng.commit(p, 0)
    assert e.value.code == -5  # ZK_ESTATE
    params = zk.circuit.CircuitParams(degree=7, num_advice=1, num_lookup_advice=1, num_fixed=1, lookup_bits=6)
    asg = zk.circuit.synthesize(params, 1)
    fixed = np.stack([asg.to_limbs(c) for c in asg.fixed])
    with pytest.raises(zk.ZkError) as e:
        eng.keygen(params, fixed, asg.copies)  # SRS of k=7 not loaded
    assert e.value.code == -5
    eng.srs_setup(7)
    # a table column that is not the range table is rejected (lookup path is range-table specialised)
    bad = fixed.copy()
    bad[asg.layout.fx_table, 3, 0] = 99
    with pytest.raises(zk.ZkError) as e:
        eng.keygen(params, bad, asg.copies)
    assert e.value.code == -1
    pk = eng.keygen(params, fixed, asg.copies)
    with pytest.raises(zk.ZkError):
        eng.prove(pk, [], bytes(32))  # wrong number of advice columns
    eng.close()


def test_fine_grained_seam_at_baseline_size(engine):
    """zk_msm_bn254 / zk_ntt_bn254_fr with host buffers at 2^19 (the size best_multiexp / best_fft see
    at k=19) against the oracle's C restatement of the reference algorithms."""
    n = 1 << 19
    engine.srs_setup(19)
    bases = engine.srs_export(0, 0, n)
    s = np.frombuffer(np.random.default_rng(19).bytes(n * 32), dtype=np.uint64).reshape(n, 4).copy()
    s[:, 3] &= 0x0FFFFFFFFFFFFFFF
    assert cops.jac_to_affine_ints(engine.msm(s, bases)) == cops.jac_to_affine_ints(cops.msm(s, bases))
    w = F.omega(19)
    assert np.array_equal(engine.ntt(s, cops.fr_mont([w])[0], 19), cops.ntt(s, w, 19))


def test_two_contexts_two_threads():
    """Rocket serves each request on its own worker thread: contexts must not interfere."""
    import threading

    res = {}

    def work(i):
        eng = zk.Engine(0)
        eng.srs_setup(10)
        a = cops.fr_mont([(j * (i + 3)) % F.R for j in range(1024)])
        p = eng.poly(1024, a)
        res[i] = [cops.affine_arr_to_ints(eng.commit(p, 0))[0] for _ in range(5)]
        eng.close()

    ths = [threading.Thread(target=work, args=(i,)) for i in range(3)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    from zkoracle import srs
    for i in range(3):
        want = srs.g1_of_scalar(srs.commit_scalar_monomial([(j * (i + 3)) % F.R for j in range(1024)]))
        assert all(r == want for r in res[i])


def test_one_context_many_threads():
    """The ABI promises that calls on ONE context from several host threads are serialised by the context (the Rust shim keeps
    a context per worker thread, but nothing forbids sharing one): four threads commit, transform, evaluate and prove on the
    same context at once; every result equals the one a lone thread gets."""
    import threading

    from webauthn_halo2_amd import engine as E

    k = 10
    n = 1 << k
    eng = zk.Engine(0)
    eng.srs_setup(k)
    p = zk.circuit.CircuitParams(degree=k, num_advice=2, num_lookup_advice=1, num_fixed=1, lookup_bits=8)
    asg = zk.circuit.synthesize(p, 0x5EED0019)
    pk = eng.keygen(p, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
    cols = [asg.to_limbs(c) for c in asg.advice]

    def job(i):
        a = cops.fr_mont([(j * (i + 3) + 1) % F.R for j in range(n)])
        h = eng.poly(n, a)
        out = [eng.commit(h, E.ZK_BASIS_LAGRANGE).tobytes()]
        eng.lagrange_to_coeff(h)
        out.append(eng.commit(h, E.ZK_BASIS_MONOMIAL).tobytes())
        out.append(eng.eval(h, cops.fr_mont([i + 5])[0]).tobytes())
        polys = []
        for col in cols:
            q = eng.poly(n)
            eng.upload_canonical(q, col)
            polys.append(q)
        out.append(eng.prove(pk, polys, bytes([i]) * 32, E.ZK_TRANSCRIPT_EVM))
        for q in polys + [h]:
            q.free()
        return out

    want = [job(i) for i in range(4)]
    got, errs = {}, []

    def work(i):
        try:
            for _ in range(3):
                got[i] = job(i)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ths = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs, errs
    assert [got[i] for i in range(4)] == want
    assert want[0][0] == want[0][1]  # commit_lagrange(v) == commit(iNTT(v))
    eng.close()


def test_resident_srs_seam_is_explicit():
    """zk_msm_srs (ParamsKZG::commit / commit_lagrange of a Rust host) multiplies host scalars against the RESIDENT
    basis; zk_msm_bn254 never guesses which basis it was given and always uploads its bases — so an array the host
    mutated in place after zk_srs_load (same address, stale resident copy) can never be served from the tables."""
    eng = zk.Engine(0)
    k = 12
    n = 1 << k
    eng.srs_setup(k)
    g, gl = eng.srs_export(0, 0, n), eng.srs_export(1, 0, n)
    eng.srs_load(k, g, gl)
    rng = np.random.default_rng(5)
    s = np.frombuffer(rng.bytes(n * 32), dtype=np.uint64).reshape(n, 4).copy()
    s[:, 3] &= 0x0FFFFFFFFFFFFFFF
    want = cops.jac_to_affine_ints(cops.msm(s, gl))
    assert cops.jac_to_affine_ints(eng.msm_srs(s, E.ZK_BASIS_LAGRANGE)) == want   # resident tables, scalars uploaded
    assert cops.jac_to_affine_ints(eng.msm(s, gl)) == want                        # general path: bases uploaded
    assert cops.jac_to_affine_ints(eng.msm_srs(s[:1000], E.ZK_BASIS_MONOMIAL)) == cops.jac_to_affine_ints(cops.msm(s[:1000], g[:1000]))
    gl[5] = gl[7]  # the host rewrites ITS array in place (same address) after the load
    assert cops.jac_to_affine_ints(eng.msm(s, gl)) == cops.jac_to_affine_ints(cops.msm(s, gl))  # sees the new content
    assert cops.jac_to_affine_ints(eng.msm_srs(s, E.ZK_BASIS_LAGRANGE)) == want                 # resident copy untouched
    with pytest.raises(zk.ZkError):
        eng.msm_srs(np.zeros((n + 1, 4), dtype=np.uint64), E.ZK_BASIS_LAGRANGE)  # longer than the SRS
    eng.close()


def test_srs_reload_invalidates_keys():
    """A proving key belongs to the SRS it was made under: after zk_srs_setup / zk_srs_load replaces the SRS
    (same k, other secret) zk_prove and zk_vk_export refuse the old key with ZK_ESTATE instead of emitting a proof
    whose vk commitments belong to the old SRS."""
    eng = zk.Engine(0)
    params = zk.circuit.CircuitParams(degree=7, num_advice=1, num_lookup_advice=1, num_fixed=1, lookup_bits=5)
    asg = zk.circuit.synthesize(params, 1)
    fixed = np.stack([asg.to_limbs(c) for c in asg.fixed])
    eng.srs_setup(7)
    pk = eng.keygen(params, fixed, asg.copies)
    h = eng.poly(128)
    eng.upload_canonical(h, asg.to_limbs(asg.advice[0]))
    assert len(eng.prove(pk, [h], bytes(32))) > 0
    eng.srs_setup(7, b"\x01" * 32)
    with pytest.raises(zk.ZkError) as e:
        eng.prove(pk, [h], bytes(32))
    assert e.value.code == -5
    with pytest.raises(zk.ZkError) as e:
        eng.vk_export(pk)
    assert e.value.code == -5
    pk2 = eng.keygen(params, fixed, asg.copies)
    assert len(eng.prove(pk2, [h], bytes(32))) > 0
    eng.close()


def test_keygen_validates_its_inputs():
    eng = zk.Engine(0)
    eng.srs_setup(7)
    params = zk.circuit.CircuitParams(degree=7, num_advice=1, num_lookup_advice=1, num_fixed=1, lookup_bits=5)
    asg = zk.circuit.synthesize(params, 1)
    fixed = np.stack([asg.to_limbs(c) for c in asg.fixed])
    with pytest.raises(ValueError):
        eng.keygen(params, fixed[:, :64], asg.copies)          # wrong row count (Python-side shape check)
    with pytest.raises(zk.ZkError) as e:
        eng.keygen(params, fixed[:-1], asg.copies)             # one fixed column short: ZK_EINVAL, no out-of-bounds read
    assert e.value.code == -1
    for lb in (0, 7, 31, 32, 40):                              # lookup_bits must be in [1, k)
        bad = zk.circuit.CircuitParams(degree=7, num_advice=1, num_lookup_advice=1, num_fixed=1, lookup_bits=lb)
        with pytest.raises(zk.ZkError) as e:
            eng.keygen(bad, fixed, asg.copies)
        assert e.value.code == -1
    with pytest.raises(ValueError):
        eng.srs_setup(7, b"short")
    with pytest.raises(zk.ZkError):
        eng.set_option(99, 1)
    with pytest.raises(zk.ZkError):
        eng.set_option(E.ZK_OPT_MSM_WINDOW, 40)
    eng.close()


def test_keygen_refuses_selector_layouts_halo2_would_compress_differently():
    """the key's gates and vk digest use the CLOSED FORM of halo2's compress_selectors (csrc/pk.h Layout::gate_sel) —
    valid only while every pair of used gate selectors shares a row.  Two used selectors that never meet would be combined
    into one fixed column by halo2: zk_keygen must refuse (ZK_ELAYOUT = -8), not build a key that proves something else.  Same
    for a used selector that is never enabled, a column that is no 0/1 selector, and 2 * idle > num_advice."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import adversarial_layout as adv
    from zkoracle import plonk

    eng = zk.Engine(0)
    k, A, L, F, lb = 8, 3, 2, 2, 5
    eng.srs_setup(k)
    sh = plonk.Shape(k, A, L, F, lb)
    params = zk.circuit.CircuitParams(degree=k, num_advice=A, num_lookup_advice=L, num_fixed=F, lookup_bits=lb)

    def limbs(cols):
        return np.stack([zk.circuit.Assignment.to_limbs(c) for c in cols])

    fixed, copies, _ = adv.build(sh, 1234, disjoint_selectors=True)  # the 5-row selector misses another column's rows
    sels = [set(r for r, v in enumerate(fixed[F + 1 + j]) if v) for j in range(A)]
    assert any(not (sels[a] & sels[b]) for a in range(A) for b in range(a + 1, A))
    with pytest.raises(zk.ZkError) as e:
        eng.keygen(params, limbs(fixed), copies)
    assert e.value.code == -8
    good, copies2, _ = adv.build(sh, 1234)  # the same generator with a shared row: accepted
    pk = eng.keygen(params, limbs(good), copies2)
    eng.pk_free(pk)
    never = [list(c) for c in good]
    never[F + 1 + 1] = [0] * (1 << k)  # a selector declared used that is never enabled
    with pytest.raises(zk.ZkError) as e:
        eng.keygen(params, limbs(never), copies2)
    assert e.value.code == -8
    two = [list(c) for c in good]
    two[F + 1][2] = 2  # not a 0/1 column
    with pytest.raises(zk.ZkError) as e:
        eng.keygen(params, limbs(two), copies2)
    assert e.value.code == -1
    many_idle = zk.circuit.CircuitParams(degree=k, num_advice=A, num_lookup_advice=L, num_fixed=F, lookup_bits=lb, idle_gate_columns=2)
    with pytest.raises(zk.ZkError) as e:
        eng.keygen(many_idle, limbs(good[:F + 1 + 1]), copies2)  # 2 * 2 > 3
    assert e.value.code == -8
    eng.close()


def test_phase_calls_refuse_repeated_output_handles():
    """Round-5 advice: the batched launches behind zk_lookup_permute / zk_lookup_product / zk_permutation_product write every output
    vector from its own blocks — the same vector twice among the outputs (or an output that another item of the call reads) is a
    data race, so it is ZK_EINVAL before anything is launched; distinct handles pass."""
    import ctypes

    eng = zk.Engine(0)
    L = eng.L
    A, Lk, F, k, lb = 3, 2, 1, 8, 6  # two lookups, two permutation chunks
    p = zk.circuit.CircuitParams(degree=k, num_advice=A, num_lookup_advice=Lk, num_fixed=F, lookup_bits=lb)
    asg = zk.circuit.synthesize(p, 0x5EED0019)
    eng.srs_setup(k)
    pk = eng.keygen(p, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
    n = 1 << k
    adv = []
    for col in asg.advice:
        h = eng.poly(n)
        eng.upload_canonical(h, asg.to_limbs(col))
        adv.append(h)
    outs = [eng.poly(n) for _ in range(6)]
    u64 = ctypes.c_uint64

    def arr(hs):
        return (u64 * len(hs))(*[h.h for h in hs])

    advh = arr(adv)
    one = (u64 * 4)(1, 0, 0, 0)
    # (the signatures are declared in engine.load_library; the raw calls stay: the outputs are the caller's handles here)
    EINVAL = -1
    # a'[0] == s'[1]; a'[0] == a'[1]; an advice column among the outputs
    assert L.zk_lookup_permute(eng.ctx, pk, advh, len(adv), arr([outs[0], outs[1]]), arr([outs[2], outs[0]]), 2) == EINVAL
    assert L.zk_lookup_permute(eng.ctx, pk, advh, len(adv), arr([outs[0], outs[0]]), arr([outs[2], outs[3]]), 2) == EINVAL
    assert L.zk_lookup_permute(eng.ctx, pk, advh, len(adv), arr([outs[0], adv[0]]), arr([outs[2], outs[3]]), 2) == EINVAL
    assert L.zk_lookup_permute(eng.ctx, pk, advh, len(adv), arr(outs[0:2]), arr(outs[2:4]), 2) == 0
    # zL twice; a zL that another lookup of the call reads as its a'
    ai, si = arr(outs[0:2]), arr(outs[2:4])
    assert L.zk_lookup_product(eng.ctx, pk, advh, len(adv), ai, si, 2, one, one, arr([outs[4], outs[4]])) == EINVAL
    assert L.zk_lookup_product(eng.ctx, pk, advh, len(adv), ai, si, 2, one, one, arr([outs[4], outs[0]])) == EINVAL
    assert L.zk_lookup_product(eng.ctx, pk, advh, len(adv), ai, si, 2, one, one, arr(outs[4:6])) == 0
    # the permutation's z of two chunks in one vector
    nchunks = (F + A + Lk + 1) // 2
    assert nchunks >= 2
    zs = [eng.poly(n) for _ in range(nchunks)]
    assert L.zk_permutation_product(eng.ctx, pk, advh, len(adv), one, one, arr([zs[0]] * nchunks), nchunks) == EINVAL
    assert L.zk_permutation_product(eng.ctx, pk, advh, len(adv), one, one, arr(zs), nchunks) == 0
    eng.close()


def _identity_jac():
    """The identity the seam returns for an empty sum: Jacobian (1, 1, 0), coordinates in Montgomery form."""
    return cops.to_mont_arr(cops.ints_to_arr([1, 1, 0]), 1).reshape(12)


def _empty_msm(eng, basis=None):
    out = np.full(12, 7, dtype=np.uint64)
    if basis is None:
        rc = eng.L.zk_msm_bn254(eng.ctx, None, None, 0, E._p(out))
    else:
        rc = eng.L.zk_msm_srs(eng.ctx, basis, None, 0, E._p(out))
    return rc, out


def test_seam_msm_with_nothing_to_add():
    """zk_msm_bn254 / zk_msm_srs at n = 0 and n = 1: the empty sum is exactly the identity (1, 1, 0) with or without an SRS,
    zk_msm_srs needs an SRS (ZK_ESTATE) and a valid basis (ZK_EINVAL) also on a k = 5 SRS, which has no window tables, and one
    term equals the oracle's MSM on both entry points."""
    ident = _identity_jac()
    eng = zk.Engine(0)
    rc, out = _empty_msm(eng)
    assert rc == 0 and np.array_equal(out, ident)
    out = np.full(12, 7, dtype=np.uint64)
    s1 = cops.fr_mont([0x1234567890ABCDEF1234567890ABCDEF])
    assert eng.L.zk_msm_srs(eng.ctx, E.ZK_BASIS_MONOMIAL, E._p(s1), 1, E._p(out)) == -5  # ZK_ESTATE
    assert _empty_msm(eng, E.ZK_BASIS_LAGRANGE)[0] == -5
    assert (out == 7).all()
    eng.srs_setup(5)
    assert eng.srs_msm_plan() == (0, 0)  # no window tables at k = 5
    rc, out = _empty_msm(eng)
    assert rc == 0 and np.array_equal(out, ident)
    for basis in (E.ZK_BASIS_MONOMIAL, E.ZK_BASIS_LAGRANGE):
        rc, out = _empty_msm(eng, basis)
        assert rc == 0 and np.array_equal(out, ident)
    rc, out = _empty_msm(eng, 7)
    assert rc == -1 and (out == 7).all()
    assert eng.L.zk_msm_srs(eng.ctx, 7, E._p(s1), 1, E._p(out)) == -1 and (out == 7).all()
    for basis in (E.ZK_BASIS_MONOMIAL, E.ZK_BASIS_LAGRANGE):
        b1 = eng.srs_export(basis, 0, 1)
        want = cops.jac_to_affine_ints(cops.msm(s1, b1))
        assert want is not None
        assert cops.jac_to_affine_ints(eng.msm(s1, b1)) == want
        assert cops.jac_to_affine_ints(eng.msm_srs(s1, basis)) == want
    eng.close()


def _random_fr(seed, n):
    a = np.frombuffer(np.random.default_rng(seed).bytes(32 * n), dtype=np.uint64).reshape(n, 4).copy()
    a[:, 3] &= 0x0FFFFFFFFFFFFFFF
    return a


def test_resident_transforms_refusals_and_round_trips(engine):
    """The four zk_*_to_* entry points: a vector whose length is no power of two is refused and left as it was; coeff_to_extended
    refuses src == dst and a src longer than dst, extended_to_coeff an n_out beyond the vector; extended_to_coeff of
    coeff_to_extended gives the input back at 2^3 -> 2^5 (one pass) and 2^8 -> 2^10 (the last pass folds the conversion)."""
    L, EINVAL = engine.L, -1
    a24 = _random_fr(24, 24)
    v, w = engine.poly(24, a24), engine.poly(24, a24)
    assert L.zk_lagrange_to_coeff(engine.ctx, v.h) == EINVAL
    assert L.zk_coeff_to_lagrange(engine.ctx, v.h) == EINVAL
    assert L.zk_coeff_to_extended(engine.ctx, v.h, w.h) == EINVAL
    assert L.zk_extended_to_coeff(engine.ctx, v.h, 24) == EINVAL
    assert np.array_equal(engine.download(v), a24) and np.array_equal(engine.download(w), a24)
    a8, a16 = _random_fr(8, 8), _random_fr(16, 16)
    p8, p16 = engine.poly(8, a8), engine.poly(16, a16)
    assert L.zk_coeff_to_extended(engine.ctx, p8.h, p8.h) == EINVAL
    assert L.zk_coeff_to_extended(engine.ctx, p16.h, p8.h) == EINVAL
    assert L.zk_extended_to_coeff(engine.ctx, p8.h, 9) == EINVAL
    assert np.array_equal(engine.download(p8), a8) and np.array_equal(engine.download(p16), a16)
    for q in (v, w, p8, p16):
        q.free()
    for lg in (3, 8):
        n = 1 << lg
        a = _random_fr(lg, n)
        src, ext = engine.poly(n, a), engine.poly(4 * n)
        engine.coeff_to_extended(src, ext)
        vals = engine.download(ext)
        assert not np.array_equal(vals[:n], a)
        engine.extended_to_coeff(ext, n)
        assert np.array_equal(engine.download(ext, n), a)
        assert np.array_equal(engine.download(src), a)
        src.free()
        ext.free()


# zk_ctx_set_option: option -> (least accepted value above 0, greatest accepted value), as the setter stood before its plain cases
# became a table.  0 is always accepted.  ZK_OPT_GP_BATCH_INVERT takes any value (non-zero = on) and has no greatest one;
# ZK_OPT_STREAM_PRIORITY has its own test (test_gpu_streams.py).
_OPTION_BOUNDS = {
    E.ZK_OPT_MSM_WINDOW: (9, 17),
    E.ZK_OPT_MSM_BATCH: (1, 256),
    E.ZK_OPT_NTT_MAX_RADIX_LOG2: (1, 11),
    E.ZK_OPT_MSM_TAIL_STREAM: (1, 2),
    E.ZK_OPT_MSM_TAIL_MAIN_ABOVE: (1, 64),
    E.ZK_OPT_BATCH_PASS_COLUMNS: (1, 256),
    E.ZK_OPT_XFORM_STREAM: (1, 2),
    E.ZK_OPT_MSM_STREAM: (1, 2),
    E.ZK_OPT_MSM_T1: (1, 2),
    E.ZK_OPT_STREAM_AUDIT: (1, 2),
    E.ZK_OPT_QUOTIENT_DOMAIN: (1, 2),
    E.ZK_OPT_ACTIVITY_HOLD: (1, 2),
}


def test_option_bounds():
    """Every option of include/zkmi355.h: the greatest value is accepted, the next one refused (ZK_EINVAL), as is the value
    below the least one where that is not 0, and -1, and an option number nobody defined."""
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zkmi355.h")).read()
    defined = {int(v) for v in re.findall(r"^#define ZK_OPT_\w+ (\d+)", hdr, re.M)}
    assert defined == set(_OPTION_BOUNDS) | {E.ZK_OPT_GP_BATCH_INVERT, E.ZK_OPT_STREAM_PRIORITY}
    eng = zk.Engine(0)
    L, EINVAL = eng.L, -1
    for opt, (lo, hi) in _OPTION_BOUNDS.items():
        assert L.zk_ctx_set_option(eng.ctx, opt, hi) == 0, opt
        assert L.zk_ctx_set_option(eng.ctx, opt, hi + 1) == EINVAL, opt
        assert L.zk_ctx_set_option(eng.ctx, opt, lo) == 0, opt
        if lo > 1:
            assert L.zk_ctx_set_option(eng.ctx, opt, lo - 1) == EINVAL, opt
        assert L.zk_ctx_set_option(eng.ctx, opt, -1) == EINVAL, opt
        assert L.zk_ctx_set_option(eng.ctx, opt, 0) == 0, opt
    for v in (1, 2, 1 << 40, 0):
        assert L.zk_ctx_set_option(eng.ctx, E.ZK_OPT_GP_BATCH_INVERT, v) == 0
    assert L.zk_ctx_set_option(eng.ctx, E.ZK_OPT_GP_BATCH_INVERT, -1) == EINVAL
    assert L.zk_ctx_set_option(eng.ctx, E.ZK_OPT_STREAM_PRIORITY, -1) == EINVAL
    for opt in (0, max(defined) + 1, 99, -3):
        assert L.zk_ctx_set_option(eng.ctx, opt, 0) == EINVAL and L.zk_ctx_set_option(eng.ctx, opt, 1) == EINVAL
    eng.close()
