"""The file codecs of csrc/serde.hip on an MI355X against the oracle's plain-integer codec (oracle/zkoracle/serde.py), on the matrix
of tests/serde_cases.py: good images whose vectors span several blocks and hold identities and both parities; every malformed
point class at the first element, both sides of a 64-thread block edge and the end of a launch; the streamed reader with a bad
point on either side of its staging-chunk seam; every malformed scalar class at both ends of a key image and inside it; the G2
half and the points of a verifying key.  A verdict is the oracle's on the altered element alone, never the engine's own."""
import ctypes

import numpy as np
import pytest

import serde_cases as sc
import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
from zkoracle import cops, curve as C, fastprover as fp, serde
from zkoracle.vkrepr import halo2_fixed_order

pytestmark = pytest.mark.gpu
FMTS = [E.ZK_SERDE_PROCESSED, E.ZK_SERDE_RAW_BYTES, E.ZK_SERDE_RAW_BYTES_UNCHECKED]
CHECKED = [E.ZK_SERDE_PROCESSED, E.ZK_SERDE_RAW_BYTES]
RAW = E.ZK_SERDE_RAW_BYTES
assert (E.ZK_SERDE_PROCESSED, E.ZK_SERDE_RAW_BYTES, E.ZK_SERDE_RAW_BYTES_UNCHECKED) == (sc.PROCESSED, sc.RAW_BYTES, sc.RAW_BYTES_UNCHECKED)


def g2_words(pt):
    """a G2 point (None: the identity) -> the 16 Montgomery words zk_srs_set_g2 takes"""
    return np.frombuffer(serde.g2_bytes(pt, serde.RAW_BYTES), dtype=np.uint64).copy()


def code_of(call, *args):
    try:
        call(*args)
        return 0
    except zk.ZkError as e:
        return e.code


def row(pt):
    return sc._points_arr([pt])[0]


def scalars(n, seed):
    a = np.frombuffer(np.random.default_rng(seed).bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    a[:, 3] &= 0x0FFFFFFFFFFFFFFF
    return a


def commitments(eng, n):
    p = eng.poly(n, scalars(n, 11))
    out = (eng.commit(p, 0).copy(), eng.commit(p, 1).copy())
    p.free()
    return out


# ------------------------------------------------------------------------------------------------ good images ---

@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("k", sc.KS)
def test_built_sections_write_and_read_as_the_oracle(k, fmt):
    """Identities, the generator and its negative, x = p - 1 and both parities through g1_compress_kernel / g1_decompress_kernel /
    g1_validate_kernel: one partial and two full 256-thread blocks, two and eight 64-thread blocks."""
    n = 1 << k
    g, gl = sc.sections(k)
    eng = zk.Engine(0)
    eng.srs_load(k, g, gl)
    eng.srs_set_g2(*[g2_words(p) for p in sc.g2_points()])
    img = sc.srs_image(k, fmt)
    assert eng.srs_write(fmt).tobytes() == img
    other = zk.Engine(0)
    other.srs_read(img, fmt)
    assert np.array_equal(other.srs_export(0, 0, n), g) and np.array_equal(other.srs_export(1, 0, n), gl)
    assert other.srs_write(RAW).tobytes() == sc.srs_image(k, RAW)
    # the commitments under the built sections are the oracle's MSMs: the points that were read are the points that are used
    a = scalars(n, 11)
    got = commitments(other, n)
    assert [cops.affine_arr_to_ints(c)[0] for c in got] == [cops.jac_to_affine_ints(cops.msm(a, b)) for b in (g, gl)]
    other.close()
    eng.close()


@pytest.fixture(scope="module")
def keys():
    """k -> (engine with the SRS of that size, CircuitParams, oracle shape, assignment, resident key), made once"""
    made = {}

    def get(k):
        if k not in made:
            kw, sh = sc.key_shape(k)
            p = zk.circuit.CircuitParams(**kw)
            asg = zk.circuit.synthesize(p, 0x5EED0019)
            eng = zk.Engine(0)
            eng.srs_setup(k)
            pk = eng.keygen(p, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
            made[k] = (eng, p, sh, asg, pk)
        return made[k]

    yield get
    for eng, p, sh, asg, pk in made.values():
        eng.pk_free(pk)
        eng.close()


def advice_polys(eng, sh, asg):
    polys = []
    for col in asg.advice:
        h = eng.poly(sh.n)
        eng.upload_canonical(h, asg.to_limbs(col))
        polys.append(h)
    return polys


def test_k9_key_files_equal_the_oracle_images_and_round_trip(keys):
    """n = 512 is two blocks of the scalar kernels, 4n = 2048 eight: every length-n and length-4n vector of the key beside the oracle"""
    eng, p, sh, asg, pk = keys(9)
    fpk = fp.keygen(sh, asg.fixed, asg.copies)
    polys = advice_polys(eng, sh, asg)
    seed = b"\x51" * 32
    want = eng.prove(pk, polys, seed, E.ZK_TRANSCRIPT_EVM)
    for fmt in FMTS:
        vk_img = eng.vk_write(pk, fmt).tobytes()
        assert vk_img == serde.vk_bytes(sh, fpk.vk.fixed_commitments, fpk.vk.permutation_commitments, serde.selectors_of(sh, asg.fixed), fmt)
        pk_img = eng.pk_write(pk, fmt)
        assert pk_img.tobytes() == serde.pk_bytes(fpk, asg.fixed, fmt)
        other = zk.Engine(0)
        other.srs_read(eng.srs_write(fmt), fmt)
        pk2 = other.pk_read(p, pk_img, fmt)
        polys2 = advice_polys(other, sh, asg)
        assert other.prove(pk2, polys2, seed, E.ZK_TRANSCRIPT_EVM) == want
        assert other.pk_write(pk2, RAW).tobytes() == serde.pk_bytes(fpk, asg.fixed, serde.RAW_BYTES)
        other.close()
    for h in polys:
        h.free()


# ------------------------------------------------------------------------------------------ malformed points ---

@pytest.mark.parametrize("fmt", CHECKED)
@pytest.mark.parametrize("k", sc.KS)
def test_malformed_points_get_the_oracle_verdict_at_every_position(k, fmt):
    n = 1 << k
    arrays = sc.sections(k)
    base = sc.srs_image(k, fmt)
    cases = sc.point_cases(k, fmt)
    assert len(cases) == len(sc.G1_CLASSES[fmt]) * 6
    eng = zk.Engine(0)
    eng.srs_read(base, fmt)
    before, commits = eng.srs_write(RAW).tobytes(), commitments(eng, n)
    assert before == sc.srs_image(k, RAW)
    refused = [c for c in cases if not c.admit]
    assert len(refused) == (len(sc.G1_CLASSES[fmt]) - 1) * 6
    for c in refused:
        assert code_of(eng.srs_read, c.image, fmt) == -1, (c.cls, c.section, c.index)
    # a refused file leaves the resident SRS, and what is computed under it, as they were
    assert eng.srs_write(RAW).tobytes() == before
    assert all(np.array_equal(a, b) for a, b in zip(commitments(eng, n), commits))
    for c in cases:
        if not c.admit:
            continue
        assert code_of(eng.srs_read, c.image, fmt) == 0, (c.cls, c.section, c.index)
        want = [a.copy() for a in arrays]
        want[c.section][c.index] = row(c.decoded)  # the oracle's point: -donor for the flipped sign, (0, 0) for the identity
        assert np.array_equal(eng.srs_export(0, 0, n), want[0]) and np.array_equal(eng.srs_export(1, 0, n), want[1]), (c.cls, c.section, c.index)
    eng.close()


def test_unchecked_format_admits_an_off_curve_point_as_given():
    """RawBytesUnchecked validates nothing: the bytes come back as given.  Nothing is computed with such an SRS."""
    k, n = 7, 128
    c = next(c for c in sc.point_cases(k, sc.RAW_BYTES) if c.cls == "y_plus_1" and (c.section, c.index) == (sc.G, 64))
    assert not c.admit
    eng = zk.Engine(0)
    assert code_of(eng.srs_read, c.image, RAW) == -1
    eng.srs_read(c.image, E.ZK_SERDE_RAW_BYTES_UNCHECKED)
    assert eng.srs_write(E.ZK_SERDE_RAW_BYTES_UNCHECKED).tobytes() == c.image
    assert eng.srs_export(0, 64, 1).tobytes() == c.element
    eng.close()


# --------------------------------------------------------------------------- the streamed reader across chunks ---

K_STREAM = 19


@pytest.fixture(scope="module")
def stream_images():
    eng = zk.Engine(0)
    eng.srs_setup(K_STREAM)
    images = {fmt: eng.srs_write(fmt).tobytes() for fmt in CHECKED}
    eng.srs_setup(17)
    images["k17"] = eng.srs_write(RAW).tobytes()
    eng.close()
    return images


@pytest.mark.parametrize("fmt", CHECKED)
def test_streamed_reader_intact_into_k17_and_k19(stream_images, fmt):
    img = stream_images[fmt]
    eng = zk.Engine(0)
    eng.srs_read_downsize(img, 17, fmt)
    assert eng.srs_write(RAW).tobytes() == stream_images["k17"]
    eng.srs_read_downsize(img, K_STREAM, fmt)  # keeps the whole of both staging chunks
    got = eng.srs_write(RAW).tobytes()
    assert got == stream_images[RAW]
    other = zk.Engine(0)
    other.srs_read(img, fmt)
    assert other.srs_write(RAW).tobytes() == got
    other.close()
    eng.close()


@pytest.mark.parametrize("fmt", CHECKED)
def test_streamed_reader_refuses_a_bad_point_on_either_side_of_the_chunk_seam(stream_images, fmt):
    img = stream_images[fmt]
    N = 1 << K_STREAM
    gs = sc.g1_size(fmt)
    eng = zk.Engine(0)
    eng.srs_read_downsize(img, 17, fmt)
    before = eng.srs_write(RAW).tobytes()
    assert before == stream_images["k17"]
    for section, index in sc.stream_positions(K_STREAM):
        off = sc.g1_offset(N, fmt, section, index)
        donor = serde.g1_parse(img[off:off + gs], fmt)
        assert donor is not None
        enc = sc.NONRESIDUE_X if fmt == sc.PROCESSED else sc.offcurve_raw(donor)
        admitted, _ = sc.oracle_verdict(serde.g1_parse, enc, fmt)
        assert not admitted
        bad = bytearray(img)
        bad[off:off + gs] = enc
        assert code_of(eng.srs_read_downsize, bytes(bad), 17, fmt) == -1, (section, index)
    assert eng.srs_write(RAW).tobytes() == before
    eng.close()


# ------------------------------------------------------------------------------------------ malformed scalars ---

@pytest.mark.parametrize("fmt", CHECKED)
@pytest.mark.parametrize("k", sc.KS)
def test_malformed_scalars_get_the_oracle_verdict_at_every_position(keys, k, fmt):
    """fr_validate_kernel / fr_to_mont_kernel / fr_from_mont_kernel at the first and the last element of the file, at the end of a 4n
    vector and inside a length-n one.  What this cannot show is a thread past the end of a vector looking at it (`i > n` for
    `i >= n`): every vector is its own exact allocation, so that thread reads out of bounds and nothing defined can be asserted."""
    eng, p, sh, asg, pk = keys(k)
    img = eng.pk_write(pk, fmt)
    cases = sc.scalar_cases(sh, img, fmt)
    assert len(cases) == (5 if fmt == sc.RAW_BYTES else 4) * 5
    assert sum(c.admit for c in cases) == 5
    for c in cases:
        bad = img.copy()
        bad[c.offset:c.offset + 32] = np.frombuffer(c.element, dtype=np.uint8)
        if not c.admit:
            assert code_of(eng.pk_read, p, bad, fmt) == -1, (c.cls, c.position)
            continue
        # r - 1 is a scalar: the key loads, and writes back the very image (fr_to_mont after fr_from_mont at the top of the range).
        # Such a key is only read and written, never proved with.
        h = eng.pk_read(p, bad, fmt)
        assert np.array_equal(eng.pk_write(h, fmt), bad), (c.cls, c.position)
        eng.pk_free(h)


# -------------------------------------------------------------------------------------- G2 and the vk's points ---

@pytest.mark.parametrize("fmt", CHECKED)
def test_g2_classes_get_the_oracle_verdict(fmt):
    k, n = 7, 128
    eng = zk.Engine(0)
    eng.srs_read(sc.srs_image(k, fmt), fmt)
    valid = sc.g2_points()
    g1_part = sc.srs_image(k, RAW)[:4 + 2 * n * 64]
    cases = sc.g2_cases(k, fmt)
    assert len(cases) == 2 * len(sc.G2_CLASSES[fmt]) and any(c.admit for c in cases) and not all(c.admit for c in cases)
    for c in cases:
        want_img = g1_part + b"".join(serde.g2_bytes(c.decoded if w == c.which else valid[w], serde.RAW_BYTES) for w in (0, 1))
        assert code_of(eng.srs_read, c.image, fmt) == (0 if c.admit else -1), (c.cls, c.which)
        if c.admit:  # the flipped sign shows the negated y, the all-zero encoding the identity
            assert eng.srs_write(RAW).tobytes() == want_img, (c.cls, c.which)
            eng.srs_read(sc.srs_image(k, fmt), fmt)
        if fmt == sc.RAW_BYTES:
            words = [np.frombuffer(c.element, dtype=np.uint64) if w == c.which else g2_words(valid[w]) for w in (0, 1)]
            assert code_of(eng.srs_set_g2, *words) == (0 if c.admit else -1), (c.cls, c.which)
            if c.admit:
                assert eng.srs_write(RAW).tobytes() == want_img, (c.cls, c.which)
                eng.srs_set_g2(*[g2_words(p) for p in valid])
        assert eng.srs_write(RAW).tobytes() == sc.srs_image(k, RAW)  # a refusal changed nothing
    eng.close()


def test_vk_points_non_residue_and_flipped_sign(keys):
    eng, p, sh, asg, pk = keys(7)
    fmt = E.ZK_SERDE_PROCESSED
    vk_img, pk_img = eng.vk_write(pk, fmt).tobytes(), eng.pk_write(pk, fmt)
    tr = eng.vk_export(pk)[2]
    polys = advice_polys(eng, sh, asg)
    proof = eng.prove(pk, polys, b"\x07" * 32, E.ZK_TRANSCRIPT_EVM)
    for h in polys:
        h.free()
    off = 8  # the first commitment of the file: the range table's column
    point = serde.g1_parse(vk_img[off:off + 32], fmt)
    assert point is not None
    good = eng.vk_read(p, vk_img, fmt, tr)
    assert eng.verify(good, proof, E.ZK_TRANSCRIPT_EVM)
    eng.pk_free(good)
    # no curve point has this x
    assert not sc.oracle_verdict(serde.g1_parse, sc.NONRESIDUE_X, fmt)[0]
    bad_vk = sc.splice(vk_img, off, sc.NONRESIDUE_X)
    bad_pk = pk_img.copy()
    bad_pk[off:off + 32] = np.frombuffer(sc.NONRESIDUE_X, dtype=np.uint8)
    assert code_of(eng.vk_read, p, bad_vk, fmt, tr) == -1
    assert code_of(eng.vk_load, pk, bad_vk, fmt) == -1
    assert code_of(eng.pk_read, p, bad_pk, fmt) == -1
    # the other sign bit: a curve point (the oracle decodes the negative), but not the key's own commitment
    flipped = sc.G1_CLASSES[sc.PROCESSED]["control_sign_flipped"][1](point)
    assert serde.g1_parse(flipped, fmt) == C.neg(point)
    neg_vk = sc.splice(vk_img, off, flipped)
    assert code_of(eng.vk_load, pk, neg_vk, fmt) == -1
    other = eng.vk_read(p, neg_vk, fmt, tr)
    assert cops.affine_arr_to_ints(eng.vk_export(other)[0])[halo2_fixed_order(sh)[0]] == C.neg(point)
    assert eng.verify(other, proof, E.ZK_TRANSCRIPT_EVM) is False
    eng.pk_free(other)
    assert eng.verify(pk, proof, E.ZK_TRANSCRIPT_EVM)  # the resident key is as it was


# ------------------------------------------------------------------------------------- size query and capacity ---

@pytest.mark.parametrize("fmt", FMTS)
def test_writers_size_query_and_short_capacity(keys, fmt):
    eng, p, sh, asg, pk = keys(7)
    L = eng.L
    writers = [("srs", lambda *a: L.zk_srs_write(eng.ctx, fmt, *a), eng.srs_write(fmt)),
               ("vk", lambda *a: L.zk_vk_write(eng.ctx, pk, fmt, *a), eng.vk_write(pk, fmt)),
               ("pk", lambda *a: L.zk_pk_write(eng.ctx, pk, fmt, *a), eng.pk_write(pk, fmt))]
    for name, fn, img in writers:
        ln = ctypes.c_size_t(0)
        assert fn(None, 0, ctypes.byref(ln)) == 0 and ln.value == len(img), name  # out = NULL: the size alone
        buf = np.full(len(img), 0xA5, dtype=np.uint8)
        ln = ctypes.c_size_t(0)
        assert fn(buf.ctypes.data, len(img) - 1, ctypes.byref(ln)) == -1, name  # one byte short
        assert ln.value == len(img) and (buf == 0xA5).all(), name
        assert fn(buf.ctypes.data, len(img), ctypes.byref(ln)) == 0 and np.array_equal(buf, img), name
