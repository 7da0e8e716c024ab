"""tests/pk_check_ref.py — the reference the device's zk_pk_check is held to (tests/test_gpu_pk_check.py) — tied to the oracle:
the oracle's own key images (serde.pk_bytes of fastprover.keygen) have no finding, and every planted single-element corruption
has exactly the signature include/zkmi355.h states (counts 1 / n / 4n).  No GPU."""
import pytest

import pk_check_ref as ref
import webauthn_halo2_amd as zk
from zkoracle import cops, fastprover as fp, plonk, serde
from zkoracle.field import R, omega

SHAPES = {"single": (1, 1, 1, 7, 6, 0), "multi": (4, 1, 1, 7, 5, 0), "idle": (5, 2, 2, 7, 5, 2)}  # tests/test_gpu_serde.py's
FMTS = [serde.PROCESSED, serde.RAW_BYTES, serde.RAW_BYTES_UNCHECKED]
_IMAGES = {}


def image(name, fmt=serde.RAW_BYTES):
    if (name, fmt) not in _IMAGES:
        A, L, Fx, k, lb, idle = SHAPES[name]
        p = zk.circuit.CircuitParams(degree=k, num_advice=A, num_lookup_advice=L, num_fixed=Fx, lookup_bits=lb, idle_gate_columns=idle)
        sh = plonk.Shape(k, A, L, Fx, lb, idle)
        asg = zk.circuit.synthesize(p, 0x5EED0019)
        _IMAGES[(name, fmt)] = (sh, serde.pk_bytes(fp.keygen(sh, asg.fixed, asg.copies), asg.fixed, fmt))
    return _IMAGES[(name, fmt)]


def put(img, off, value, fmt):
    """The image with the field element at byte `off` replaced by the canonical integer `value`."""
    b = bytearray(img)
    b[off:off + 32] = (cops.fr_mont([value])[0].tobytes() if fmt != serde.PROCESSED else int(value).to_bytes(32, "little"))
    return bytes(b)


def label(sh, c, r):
    return pow(ref.DELTA, c, R) * pow(omega(sh.k), r, R) % R


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_oracle_key_images_have_no_finding(name, fmt):
    sh, img = image(name, fmt)
    assert ref.check(sh, img, fmt) == (ref.CHECK_ALL | ref.CHECK_REPR, [])


@pytest.mark.parametrize("name", list(SHAPES))
def test_single_element_corruptions_have_their_exact_signature(name):
    fmt = serde.RAW_BYTES
    sh, img = image(name, fmt)
    n, m, F = sh.n, len(sh.perm_cols), sh.n_fix
    junk = 0x1234567890ABCDEF1234567890ABCDEF % R
    # a damaged VALUE of a constants column: 1 commitment finding + every coefficient
    for row in (0, n // 2, n - 1):
        flags, found = ref.check(sh, put(img, ref.offset_of(sh, fmt, ref.FIXED_VAL, 0, row), junk, fmt), fmt)
        assert found == [(ref.FIXED_COMMIT, 0, 0, 1), (ref.FIXED_POLY, 0, 0, n)]
        assert flags == (ref.CHECK_ALL | ref.CHECK_REPR) & ~(ref.CHECK_COMMITMENTS | ref.CHECK_POLYS)
    # a damaged COEFFICIENT: 1 in POLY, the whole extended coset; a damaged COSET ELEMENT: 1 in COSET — first, middle, last column
    for part_p, part_e, cols in ((ref.FIXED_POLY, ref.FIXED_COSET, (0, F // 2, F - 1)), (ref.SIGMA_POLY, ref.SIGMA_COSET, (0, m // 2, m - 1))):
        for col in cols:
            for i in (0, n // 2, n - 1):
                flags, found = ref.check(sh, put(img, ref.offset_of(sh, fmt, part_p, col, i), junk, fmt), fmt)
                assert found == [(part_p, col, i, 1), (part_e, col, 0, 4 * n)]
                assert flags == (ref.CHECK_ALL | ref.CHECK_REPR) & ~(ref.CHECK_POLYS | ref.CHECK_COSETS)
            for i in (0, 2 * n, 4 * n - 1):
                flags, found = ref.check(sh, put(img, ref.offset_of(sh, fmt, part_e, col, i), junk, fmt), fmt)
                assert found == [(part_e, col, i, 1)]
                assert flags == (ref.CHECK_ALL | ref.CHECK_REPR) & ~ref.CHECK_COSETS
    for which in range(3):
        flags, found = ref.check(sh, put(img, ref.offset_of(sh, fmt, ref.L_COSET, which, 4 * n - 1), junk, fmt), fmt)
        assert found == [(ref.L_COSET, which, 4 * n - 1, 1)] and flags == (ref.CHECK_ALL | ref.CHECK_REPR) & ~ref.CHECK_COSETS


@pytest.mark.parametrize("name", list(SHAPES))
def test_sigma_findings(name):
    fmt = serde.RAW_BYTES
    sh, img = image(name, fmt)
    n, m, usable = sh.n, len(sh.perm_cols), sh.usable_rows
    key = ref.parse(sh, img, fmt)
    table = ref.label_table(sh)
    raw = [v.tobytes() for v in key["sigma_val"]]
    # a cell that maps to itself, in the last permutation column
    c = m - 1
    r = next(r for r in range(usable - 1, -1, -1) if table[raw[c][32 * r:32 * r + 32]] == (c, r))
    # its value replaced by ANOTHER cell's label: still a label, but nobody names (c, r) any more
    flags, found = ref.check(sh, put(img, ref.offset_of(sh, fmt, ref.SIGMA_LABEL, c, r), label(sh, 0, 1), fmt), fmt)
    assert found == [(ref.SIGMA_COMMIT, c, 0, 1), (ref.SIGMA_POLY, c, 0, n), (ref.SIGMA_MAP, c, r, 1)]
    assert flags & ref.CHECK_SIGMA == 0
    # replaced by a value that is no label: LABEL 1 + MAP 1
    flags, found = ref.check(sh, put(img, ref.offset_of(sh, fmt, ref.SIGMA_LABEL, c, r), 5, fmt), fmt)
    assert found == [(ref.SIGMA_COMMIT, c, 0, 1), (ref.SIGMA_POLY, c, 0, n), (ref.SIGMA_LABEL, c, r, 1), (ref.SIGMA_MAP, c, r, 1)]
    # a usable cell mapped into the rows the prover blinds, and a blinded row that is not its own label: LABEL findings too
    flags, found = ref.check(sh, put(img, ref.offset_of(sh, fmt, ref.SIGMA_LABEL, c, r), label(sh, 0, n - 1), fmt), fmt)
    assert (ref.SIGMA_LABEL, c, r, 1) in found and (ref.SIGMA_MAP, c, r, 1) in found
    flags, found = ref.check(sh, put(img, ref.offset_of(sh, fmt, ref.SIGMA_LABEL, 0, n - 1), label(sh, 0, 0), fmt), fmt)
    assert (ref.SIGMA_LABEL, 0, n - 1, 1) in found and (ref.SIGMA_MAP, 0, n - 1, 1) in found


def test_a_non_reduced_alias_is_a_mismatch_and_enters_the_recomputation_as_its_element():
    fmt = serde.RAW_BYTES_UNCHECKED
    sh, img = image("multi", fmt)
    n = sh.n
    off = ref.offset_of(sh, fmt, ref.FIXED_POLY, 0, 3)
    v = int.from_bytes(img[off:off + 32], "little")
    assert v + R < 1 << 256
    b = bytearray(img)
    b[off:off + 32] = (v + R).to_bytes(32, "little")
    # the same field element: the coset recomputed from it is the key's; the image differs from the recomputed coefficient
    assert ref.check(sh, bytes(b), fmt)[1] == [(ref.FIXED_POLY, 0, 3, 1)]


def test_offsets_cover_the_image():
    for name in SHAPES:
        for fmt in FMTS:
            sh, img = image(name, fmt)
            m = len(sh.perm_cols)
            assert ref.offset_of(sh, fmt, ref.SIGMA_COSET, m - 1, 4 * sh.n - 1) + 32 == len(img)
            assert ref.offset_of(sh, fmt, ref.L_COSET, 0, 0) == ref.vk_len(sh, fmt) + 4
            # the table column is the first fixed column of the file
            assert ref.offset_of(sh, fmt, ref.FIXED_COMMIT, sh.fx_table) == 8
