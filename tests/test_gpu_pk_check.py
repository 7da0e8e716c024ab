"""zk_pk_check on the device — the audit of a resident proving key — against the plain reference over key images
(tests/pk_check_ref.py).  Expected results are exact: clean keys of every shape (made by zk_keygen and read back in the three
formats), planted single-element corruptions through the file route with their 1 / n / 4n signatures, what zk_pk_read itself
refuses, the consequence of a damaged coset (a proof no verifier accepts), keys of a foreign SRS, no side effect on proofs, key
image and witness check, the stream audit, the full-size k = 17 and k = 19 rows, error codes and the Python layer."""
import ctypes
import json

import numpy as np
import pytest

import pk_check_ref as ref
import webauthn_halo2_amd as zk
import witness_cases as C
from prover_shapes import DRAW_SEED, SHAPES, random_shapes
from webauthn_halo2_amd import engine as E
from zkoracle import cops, fastprover as fp
from zkoracle.field import R, omega

pytestmark = pytest.mark.gpu

FMTS = [E.ZK_SERDE_PROCESSED, E.ZK_SERDE_RAW_BYTES, E.ZK_SERDE_RAW_BYTES_UNCHECKED]
FILE_SHAPES = {"single": (1, 1, 1, 7, 6, 0), "multi": (4, 1, 1, 7, 5, 0), "idle": (5, 2, 2, 7, 5, 2)}  # tests/test_gpu_serde.py's
CLEAN = (E.ZK_PK_CHECK_ALL | E.ZK_PK_CHECK_REPR, [])


def test_constants_agree_with_the_reference():
    assert (E.ZK_PK_PART_FIXED_COMMIT, E.ZK_PK_PART_SIGMA_COMMIT, E.ZK_PK_PART_FIXED_POLY, E.ZK_PK_PART_SIGMA_POLY, E.ZK_PK_PART_FIXED_COSET,
            E.ZK_PK_PART_SIGMA_COSET, E.ZK_PK_PART_L_COSET, E.ZK_PK_PART_SIGMA_LABEL, E.ZK_PK_PART_SIGMA_MAP) == tuple(range(1, 10))
    assert (E.ZK_PK_CHECK_COMMITMENTS, E.ZK_PK_CHECK_POLYS, E.ZK_PK_CHECK_COSETS, E.ZK_PK_CHECK_SIGMA, E.ZK_PK_CHECK_ALL,
            E.ZK_PK_CHECK_REPR) == (ref.CHECK_COMMITMENTS, ref.CHECK_POLYS, ref.CHECK_COSETS, ref.CHECK_SIGMA, ref.CHECK_ALL, ref.CHECK_REPR)


def make_key(eng, t, seed=0x5EED0019, srs_seed=None):
    """(params, shape, fixed, copies, advice, key) of shape tuple t on eng, the SRS of its k set up first."""
    sh, fixed, copies, advice = C.synth_case(t, seed)
    p = C.params_of(t)
    eng.srs_setup(p.degree, *([srs_seed] if srs_seed else []))
    return p, sh, fixed, copies, advice, eng.keygen(p, np.stack([C.limbs(c) for c in fixed]), copies)


def upload(eng, sh, advice):
    polys = [eng.poly(sh.n) for _ in advice]
    for h, col in zip(polys, advice):
        eng.upload_canonical(h, C.limbs(col))
    return polys


# ---- 1. clean keys ---------------------------------------------------------------------------------------------------------------
def clean_everywhere(engine, t):
    p, sh, fixed, copies, advice, pk = make_key(engine, t)
    assert engine.pk_check(pk) == CLEAN
    assert engine.pk_check(pk, cap=0) == CLEAN  # (no buffer at all)
    for fmt in FMTS:
        pk2 = engine.pk_read(p, engine.pk_write(pk, fmt), fmt)
        assert engine.pk_check(pk2) == CLEAN, fmt
        engine.pk_free(pk2)
    assert engine.pk_check(pk) == CLEAN
    engine.pk_free(pk)


@pytest.mark.parametrize("name", list(SHAPES))
def test_clean_key_of_every_shape(engine, name):
    clean_everywhere(engine, SHAPES[name])


@pytest.mark.parametrize("t", random_shapes(20, DRAW_SEED), ids=lambda t: "A%dL%dF%dk%dlb%di%d" % t)
def test_clean_key_of_random_shapes(engine, t):
    clean_everywhere(engine, t)


# ---- 2. planted corruptions through the file route -----------------------------------------------------------------------------------
def element_bytes(value, fmt):
    return int(value).to_bytes(32, "little") if fmt == E.ZK_SERDE_PROCESSED else cops.fr_mont([value])[0].tobytes()


def planted(img, off, fmt, rng, value=None):
    """The image with the element at `off` replaced: by `value` (a canonical integer), else by another reduced value (RAW_BYTES) /
    by arbitrary bytes (RAW_BYTES_UNCHECKED)."""
    out = np.array(img, dtype=np.uint8, copy=True)
    if value is not None:
        new = element_bytes(value, fmt)
    elif fmt == E.ZK_SERDE_RAW_BYTES_UNCHECKED:
        new = bytes(rng.bytes(32))
    else:
        new = element_bytes(int.from_bytes(rng.bytes(32), "little") % R, fmt)
    assert new != out[off:off + 32].tobytes()
    out[off:off + 32] = np.frombuffer(new, dtype=np.uint8)
    return out


def audit_of_image(eng, p, img, fmt, cap=64):
    pk = eng.pk_read(p, img, fmt)
    try:
        return eng.pk_check(pk, cap)
    finally:
        eng.pk_free(pk)


def label(sh, c, r):
    return pow(ref.DELTA, c, R) * pow(omega(sh.k), r, R) % R


def fixed_point(sh, copies, c):
    """A usable row of permutation column c whose cell no copy constraint touches (sigma maps it to itself)."""
    used = {cell for pair in copies for cell in (tuple(pair[0]), tuple(pair[1]))}
    return next(r for r in range(sh.usable_rows - 1, -1, -1) if (c, r) not in used)


@pytest.mark.parametrize("fmt", [E.ZK_SERDE_RAW_BYTES, E.ZK_SERDE_RAW_BYTES_UNCHECKED])
@pytest.mark.parametrize("name", list(FILE_SHAPES))
def test_planted_corruptions_are_found_exactly(engine, name, fmt):
    t = FILE_SHAPES[name]
    p, sh, fixed, copies, advice, pk = make_key(engine, t)
    img = engine.pk_write(pk, fmt)
    engine.pk_free(pk)
    n, F, m = sh.n, sh.n_fix, len(sh.perm_cols)
    rng = np.random.default_rng(0xC0FFEE + fmt)
    cases = []
    # coefficients and coset elements of every kind of column — constants, the table, selectors; first, middle, last column and index
    for part, cols, idxs in ((ref.FIXED_POLY, (0, F // 2, F - 1), (0, n // 2, n - 1)), (ref.SIGMA_POLY, (0, m // 2, m - 1), (n - 1, 0, n // 2)),
                             (ref.FIXED_COSET, (0, F // 2, F - 1), (4 * n - 1, 0, 2 * n)), (ref.SIGMA_COSET, (0, m // 2, m - 1), (2 * n, 4 * n - 1, 0)),
                             (ref.L_COSET, (0, 1, 2), (0, 4 * n - 1, 2 * n + 1))):
        cases += [(part, col, i, None) for col, i in zip(cols, idxs)]
    cases += [(ref.FIXED_COSET, sh.fx_table, 7, None)]  # (the table's COEFFICIENTS are zk_pk_read's own spot check: refused there)
    # values: constants columns and sigma columns only (zk_pk_read refuses a changed table / selector value)
    cases += [(ref.FIXED_VAL, 0, 0, None), (ref.FIXED_VAL, sh.num_fixed - 1, n - 1, None)]
    c_last = m - 1
    r_fix = fixed_point(sh, copies, c_last)
    cases += [(ref.SIGMA_VAL, 0, n // 2, None), (ref.SIGMA_VAL, c_last, n - 1, None),       # no labels (LABEL + MAP)
              (ref.SIGMA_LABEL, c_last, r_fix, 5),                                         # no label, a small value
              (ref.SIGMA_MAP, c_last, r_fix, label(sh, 0, 1)),                             # another cell's label: MAP alone
              (ref.SIGMA_LABEL, m // 2, fixed_point(sh, copies, m // 2), label(sh, 0, n - 1))]  # a usable cell mapped into the blinded rows
    for part, col, i, value in cases:
        bad = planted(img, ref.offset_of(sh, fmt, part, col, i), fmt, rng, value)
        want = ref.check(sh, bad, fmt)
        got = audit_of_image(engine, p, bad, fmt)
        print(name, fmt, part, col, i, "->", got)
        assert want[1], "the planted element must be found"
        assert got == want, (part, col, i)
    # the stated signatures, spelled out once
    off = ref.offset_of(sh, fmt, ref.SIGMA_POLY, 1, 3)
    assert audit_of_image(engine, p, planted(img, off, fmt, rng), fmt)[1] == [(E.ZK_PK_PART_SIGMA_POLY, 1, 3, 1), (E.ZK_PK_PART_SIGMA_COSET, 1, 0, 4 * n)]
    off = ref.offset_of(sh, fmt, ref.FIXED_VAL, 0, 9)
    assert audit_of_image(engine, p, planted(img, off, fmt, rng), fmt)[1] == [(E.ZK_PK_PART_FIXED_COMMIT, 0, 0, 1), (E.ZK_PK_PART_FIXED_POLY, 0, 0, n)]
    off = ref.offset_of(sh, fmt, ref.SIGMA_MAP, c_last, r_fix)
    flags, found = audit_of_image(engine, p, planted(img, off, fmt, rng, label(sh, 0, 1)), fmt)
    assert found == [(E.ZK_PK_PART_SIGMA_COMMIT, c_last, 0, 1), (E.ZK_PK_PART_SIGMA_POLY, c_last, 0, n), (E.ZK_PK_PART_SIGMA_MAP, c_last, r_fix, 1)]
    assert flags == E.ZK_PK_CHECK_REPR | E.ZK_PK_CHECK_COSETS
    # a vk commitment replaced by another curve point (not the table column's: zk_pk_read recommits that one itself)
    g = 32 if fmt == E.ZK_SERDE_PROCESSED else 64
    src = ref.offset_of(sh, fmt, ref.SIGMA_COMMIT, 0)
    for part, col in ((ref.FIXED_COMMIT, 0), (ref.FIXED_COMMIT, F - 1), (ref.SIGMA_COMMIT, m - 1)):
        bad = np.array(img, copy=True)
        off = ref.offset_of(sh, fmt, part, col)
        bad[off:off + g] = img[src:src + g]
        want = ref.check(sh, bad, fmt)
        assert want == (E.ZK_PK_CHECK_ALL & ~E.ZK_PK_CHECK_COMMITMENTS | E.ZK_PK_CHECK_REPR, [(part, col, 0, 1)])
        assert audit_of_image(engine, p, bad, fmt) == want
    # two corruptions in different parts: both, in order; cap below the total truncates the list and leaves the total
    bad = planted(planted(img, ref.offset_of(sh, fmt, ref.SIGMA_COSET, m - 1, 11), fmt, rng), ref.offset_of(sh, fmt, ref.FIXED_POLY, 0, 2), fmt, rng)
    want = ref.check(sh, bad, fmt)
    assert [f[0] for f in want[1]] == [ref.FIXED_POLY, ref.FIXED_COSET, ref.SIGMA_COSET]
    pk2 = engine.pk_read(p, bad, fmt)
    assert engine.pk_check(pk2) == want
    assert engine.pk_check(pk2) == want  # the same key, the same report
    for cap in (0, 1, 2):
        out = (E.PkFindingC * max(cap, 1))()
        flags, total = ctypes.c_uint32(0), ctypes.c_size_t(0)
        assert engine.L.zk_pk_check(engine.ctx, pk2, ctypes.byref(flags), out if cap else None, cap, ctypes.byref(total)) == 0
        assert total.value == 3 and flags.value == want[0]
        assert [(f.part, f.column, f.index, f.count) for f in out[:cap]] == want[1][:cap]
    engine.pk_free(pk2)


@pytest.mark.parametrize("name", list(FILE_SHAPES))
def test_pk_read_still_refuses_table_and_selector_values(engine, name):
    """What zk_pk_read refused before the audit existed it still refuses: a changed value of the table or of a selector column,
    and a changed coefficient of the table column (its spot check recommits the table in both forms)."""
    p, sh, fixed, copies, advice, pk = make_key(engine, FILE_SHAPES[name])
    fmt = E.ZK_SERDE_RAW_BYTES
    img = engine.pk_write(pk, fmt)
    engine.pk_free(pk)
    rng = np.random.default_rng(3)
    sel = sh.fx_sel[0]
    for col, row in ((sh.fx_table, 3), (sh.fx_table, sh.n - 1), (sel, 0), (sel, sh.n // 2)):
        with pytest.raises(zk.ZkError) as e:
            engine.pk_read(p, planted(img, ref.offset_of(sh, fmt, ref.FIXED_VAL, col, row), fmt, rng), fmt)
        assert e.value.code == -1
    with pytest.raises(zk.ZkError) as e:
        engine.pk_read(p, planted(img, ref.offset_of(sh, fmt, ref.FIXED_POLY, sh.fx_table, 5), fmt, rng), fmt)
    assert e.value.code == -1


# ---- 3. the consequence ------------------------------------------------------------------------------------------------------------
def test_a_damaged_sigma_coset_proves_into_a_proof_nobody_accepts(engine):
    p, sh, fixed, copies, advice, pk = make_key(engine, SHAPES["k17like"])
    polys = upload(engine, sh, advice)
    fmt = E.ZK_SERDE_RAW_BYTES
    img = engine.pk_write(pk, fmt)
    c, i = len(sh.perm_cols) - 2, 3 * sh.n + 5
    bad = engine.pk_read(p, planted(img, ref.offset_of(sh, fmt, ref.SIGMA_COSET, c, i), fmt, np.random.default_rng(8)), fmt)
    seed = b"\x21" * 32
    for tr in (E.ZK_TRANSCRIPT_BLAKE2B, E.ZK_TRANSCRIPT_EVM):
        proof = engine.prove(bad, polys, seed, tr)  # ZK_OK
        assert not engine.verify(bad, proof, tr) and not engine.verify(pk, proof, tr)
        good = engine.prove(pk, polys, seed, tr)
        assert engine.verify(pk, good, tr)
    assert engine.pk_check(bad) == (E.ZK_PK_CHECK_ALL & ~E.ZK_PK_CHECK_COSETS | E.ZK_PK_CHECK_REPR, [(E.ZK_PK_PART_SIGMA_COSET, c, i, 1)])
    assert engine.pk_check(pk) == CLEAN
    for h in polys:
        h.free()
    engine.pk_free(bad)
    engine.pk_free(pk)


# ---- 4. a foreign SRS --------------------------------------------------------------------------------------------------------------
def test_keys_of_a_foreign_srs():
    t = FILE_SHAPES["idle"]
    fmt = E.ZK_SERDE_RAW_BYTES
    eng, other = zk.Engine(0), zk.Engine(0)
    p, sh, fixed, copies, advice, pk = make_key(eng, t)
    _, _, _, _, _, pk9 = make_key(other, t, srs_seed=bytes([9]) * 32)
    img, img9 = eng.pk_write(pk, fmt), other.pk_write(pk9, fmt)
    other.close()
    # the vk section of the other SRS's key, the table column's commitment kept (zk_pk_read recommits that one)
    hybrid = np.array(img, copy=True)
    lo, hi = 8, 8 + 64 * (sh.n_fix + len(sh.perm_cols))
    hybrid[lo:hi] = img9[lo:hi]
    t_off = ref.offset_of(sh, fmt, ref.FIXED_COMMIT, sh.fx_table)
    hybrid[t_off:t_off + 64] = img[t_off:t_off + 64]
    want = ref.check(sh, hybrid, fmt)
    zero_cols = [f for f in range(sh.n_fix) if not any(fixed[f])]
    listed = {(part, col) for part, col, _, _ in want[1]}
    assert listed == ({(ref.FIXED_COMMIT, f) for f in range(sh.n_fix) if f != sh.fx_table and f not in zero_cols} |
                      {(ref.SIGMA_COMMIT, c) for c in range(len(sh.perm_cols))})
    assert want[0] == E.ZK_PK_CHECK_ALL & ~E.ZK_PK_CHECK_COMMITMENTS | E.ZK_PK_CHECK_REPR
    assert audit_of_image(eng, p, hybrid, fmt, cap=256) == want
    # the key itself after its SRS was replaced: ZK_ESTATE
    eng.srs_setup(t[3], b"\x01" * 32)
    with pytest.raises(zk.ZkError) as e:
        eng.pk_check(pk)
    assert e.value.code == -5
    eng.close()


# ---- 5. no side effects, and the stream audit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k10single", "k10batched", "idle"])
def test_a_check_changes_nothing_and_is_ordered_under_the_audit(name):
    eng = zk.Engine(0)
    eng.set_option(E.ZK_OPT_STREAM_AUDIT, 1)
    p, sh, fixed, copies, advice, pk = make_key(eng, SHAPES[name])
    sets = [upload(eng, sh, advice) for _ in range(3)]
    polys = sets[0]
    seed = b"\x33" * 32
    seeds = [bytes([7 + j]) * 32 for j in range(3)]

    def snapshot():
        return (eng.prove(pk, polys, seed, E.ZK_TRANSCRIPT_EVM), eng.prove(pk, polys, seed, E.ZK_TRANSCRIPT_BLAKE2B),
                eng.prove_batch(pk, sets, seeds, E.ZK_TRANSCRIPT_BLAKE2B), eng.pk_write(pk).tobytes(), eng.witness_check(pk, polys))

    before = snapshot()
    assert eng.pk_check(pk) == CLEAN
    assert snapshot() == before
    for _ in range(3):  # prove - check - prove on one context
        assert eng.pk_check(pk) == CLEAN
        assert eng.prove(pk, polys, seed, E.ZK_TRANSCRIPT_EVM) == before[0]
    # a key with findings, audited on the same context between proofs of the good one
    fmt = E.ZK_SERDE_RAW_BYTES_UNCHECKED
    bad_img = planted(eng.pk_write(pk, fmt), ref.offset_of(sh, fmt, ref.SIGMA_POLY, 0, 1), fmt, np.random.default_rng(4))
    bad = eng.pk_read(p, bad_img, fmt)
    assert eng.pk_check(bad) == ref.check(sh, bad_img, fmt)
    eng.pk_free(bad)
    assert snapshot() == before
    checks, violations, msg = eng.audit_report()
    assert checks > 0 and violations == 0, msg
    for h in [h for st in sets for h in st]:
        h.free()
    eng.pk_free(pk)
    eng.close()


# ---- 6. full size ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["K17", "K19"])
def test_full_size_keys(engine, which):
    p = getattr(zk.circuit, which)
    asg = zk.circuit.synthesize(p, 0x5EED0019)
    engine.srs_setup(p.degree)
    pk = engine.keygen(p, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
    assert engine.pk_check(pk) == CLEAN
    if which == "K17":
        # one element, the last of the last sigma coset, through the file route
        sh = C.W.shape_of((p.num_advice, p.num_lookup_advice, p.num_fixed, p.degree, p.lookup_bits))
        fmt = E.ZK_SERDE_RAW_BYTES
        img = engine.pk_write(pk, fmt)
        m, n = len(sh.perm_cols), sh.n
        off = ref.offset_of(sh, fmt, ref.SIGMA_COSET, m - 1, 4 * n - 1)
        assert off + 32 == img.size
        img[off] ^= 1
        bad = engine.pk_read(p, img, fmt)
        assert engine.pk_check(bad) == (E.ZK_PK_CHECK_ALL & ~E.ZK_PK_CHECK_COSETS | E.ZK_PK_CHECK_REPR, [(E.ZK_PK_PART_SIGMA_COSET, m - 1, 4 * n - 1, 1)])
        engine.pk_free(bad)
        assert engine.pk_check(pk) == CLEAN
    engine.pk_free(pk)


# ---- 7. errors and the Python layer ------------------------------------------------------------------------------------------------
def test_error_codes_and_the_repr_bit(engine):
    p, sh, fixed, copies, advice, pk = make_key(engine, SHAPES["k17like"])
    L = engine.L
    out = (E.PkFindingC * 4)()
    flags, total = ctypes.c_uint32(77), ctypes.c_size_t(77)

    def call(h, fl, outp, cap, tot):
        rc = L.zk_pk_check(engine.ctx, h, fl, outp, cap, tot)
        assert rc == 0 or (flags.value, total.value) == (77, 77)  # outputs untouched on error
        return rc

    assert call(pk + 1000, ctypes.byref(flags), out, 4, ctypes.byref(total)) == -1   # no such key
    assert call(pk, None, out, 4, ctypes.byref(total)) == -1                           # NULL flags
    assert call(pk, ctypes.byref(flags), out, 4, None) == -1                           # NULL n_findings
    assert call(pk, ctypes.byref(flags), None, 4, ctypes.byref(total)) == -1           # cap > 0 without a buffer
    vk = engine.vk_read(p, engine.vk_write(pk))
    assert call(vk, ctypes.byref(flags), out, 4, ctypes.byref(total)) == -5            # verifying-only key: ZK_ESTATE
    engine.pk_free(vk)
    assert call(pk, ctypes.byref(flags), None, 0, ctypes.byref(total)) == 0
    assert (flags.value, total.value) == (E.ZK_PK_CHECK_ALL | E.ZK_PK_CHECK_REPR, 0)
    # a host override of transcript_repr with another value clears the informational bit and nothing else
    engine.pk_set_transcript_repr(pk, cops.fr_mont([12345])[0])
    assert engine.pk_check(pk) == (E.ZK_PK_CHECK_ALL, [])
    engine.srs_setup(p.degree, b"\x01" * 32)                                           # the key's SRS replaced
    flags.value, total.value = 77, 77
    assert call(pk, ctypes.byref(flags), out, 4, ctypes.byref(total)) == -5
    engine.pk_free(pk)


def test_python_layer(tmp_path, monkeypatch):
    api = zk.ecdsa_p256
    api.shutdown()
    cfg = tmp_path / "ecdsa_circuit.config"
    cfg.write_text(json.dumps({"degree": 10, "num_advice": 3, "num_lookup_advice": 2, "num_fixed": 1, "lookup_bits": 8}) + "\n")
    monkeypatch.setenv("ECDSA_CONFIG", str(cfg))
    pkp = str(tmp_path / "proving_key.pk")
    try:
        # the defaults do not call the check
        calls = []
        real = zk.Engine.pk_check
        monkeypatch.setattr(zk.Engine, "pk_check", lambda self, pk, cap=64: calls.append(pk) or real(self, pk, cap))
        api.download_keys(10, pkp)
        zk.proving_server.setup(degree=10, proving_key_path=pkp)
        assert calls == []
        assert api.check_keys(pkp, 10) == CLEAN and len(calls) == 1
        # check=True without a key file: the resident key alone
        api.download_keys(10, pkp, check=True)
        assert len(calls) == 2
        # a good key file passes, a damaged one raises with the report
        eng, p, pk = api._resident_key(pkp, 10, 0)
        img = eng.pk_write(pk, E.ZK_SERDE_RAW_BYTES)
        with open(pkp, "wb") as f:
            f.write(img.tobytes())
        api.download_keys(10, pkp, check=True)
        zk.proving_server.setup(degree=10, proving_key_path=pkp, check_keys=True)
        sh = C.W.shape_of((3, 2, 1, 10, 8))
        off = ref.offset_of(sh, E.ZK_SERDE_RAW_BYTES, ref.FIXED_COSET, sh.fx_table, 17)
        img[off] ^= 1
        with open(pkp, "wb") as f:
            f.write(img.tobytes())
        for fn in (lambda: api.download_keys(10, pkp, check=True), lambda: zk.proving_server.setup(degree=10, proving_key_path=pkp, check_keys=True)):
            with pytest.raises(api.ProvingKeyError) as e:
                fn()
            assert e.value.findings == [(E.ZK_PK_PART_FIXED_COSET, sh.fx_table, 17, 1)]
            assert e.value.flags == E.ZK_PK_CHECK_ALL & ~E.ZK_PK_CHECK_COSETS | E.ZK_PK_CHECK_REPR and isinstance(e.value, ValueError)
        api.download_keys(10, pkp)  # the default still never looks at the file
        assert api.check_keys(pkp, 10) == CLEAN
    finally:
        api.shutdown()
