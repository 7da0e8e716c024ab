"""The file-codec matrix of tests/serde_cases.py, pinned without a GPU: every class carries the verdict the oracle's plain-integer
codec gives its altered element, every class sits at every position, and the oracle's G2 parser inverts its writer."""
import pytest

import serde_cases as sc
import webauthn_halo2_amd as zk
from zkoracle import curve as C, fastprover as fp, serde
from zkoracle.field import MONT_R, P, R, inv
from zkoracle.srs import TAU


def test_residue_facts():
    qr = lambda a: pow(a % P, (P - 1) // 2, P) == 1
    assert not qr(3) and not qr(4 ** 3 + 3) and not qr(10 ** 3 + 3) and qr(2)
    assert sc.Y_OF_XPM1 ** 2 % P == 2 and C.is_on_curve((P - 1, sc.Y_OF_XPM1))
    assert P % 4 == 3 and P < R + P < 2 * P < 1 << 255  # x + p and v + r fit their 32 bytes; x + p fits below the sign bit


@pytest.mark.parametrize("k", sc.KS)
def test_sections_hold_what_the_issue_lists(k):
    n = 1 << k
    g, gl = sc.section_points(k)
    for pts in (g, gl):
        assert [i for i, pt in enumerate(pts) if pt is None] == [0, 63, 64, n - 1]
        assert pts[sc.GEN_AT] == (1, 2) and pts[sc.NEG_GEN_AT] == (1, P - 2) and pts[sc.XPM1_AT][0] == P - 1
        assert {pt[1] & 1 for pt in pts if pt is not None} == {0, 1}
        assert pts[sc.DONOR_AT] is not None and len(pts) == n
    assert g != gl and g[sc.XPM1_AT] == C.neg(gl[sc.XPM1_AT])
    for fmt in (sc.PROCESSED, sc.RAW_BYTES, sc.RAW_BYTES_UNCHECKED):
        img = sc.srs_image(k, fmt)
        gs = sc.g1_size(fmt)
        assert len(img) == 4 + 2 * n * gs + 2 * sc.g2_size(fmt)
        assert [serde.g1_parse(img[4 + gs * i:4 + gs * (i + 1)], fmt) for i in range(2 * n)] == list(g) + list(gl)
        assert tuple(serde.g2_parse(img[sc.g2_offset(n, fmt, w):sc.g2_offset(n, fmt, w) + sc.g2_size(fmt)], fmt) for w in (0, 1)) == sc.g2_points()


@pytest.mark.parametrize("fmt", sc.CHECKED)
@pytest.mark.parametrize("k", sc.KS)
def test_point_classes_carry_the_oracle_verdict_at_every_position(k, fmt):
    n = 1 << k
    cases = sc.point_cases(k, fmt)
    classes = sc.G1_CLASSES[fmt]
    want_pos = [(0, 0), (0, 63), (0, 64), (0, n - 1), (1, 0), (1, n - 1)]
    assert [(c.cls, c.section, c.index) for c in cases] == [(name, s, i) for name in classes for s, i in want_pos]  # nothing left out
    base = sc.srs_image(k, fmt)
    donor = sc.section_points(k)
    for c in cases:
        assert c.admit == classes[c.cls][0], (c.cls, c.section, c.index)
        off = sc.g1_offset(n, fmt, c.section, c.index)
        assert c.image[off:off + len(c.element)] == c.element and c.image[:off] == base[:off] and c.image[off + len(c.element):] == base[off + len(c.element):]
        if c.cls == "control_sign_flipped":
            assert c.decoded == C.neg(donor[c.section][sc.DONOR_AT]) and c.decoded is not None
        if c.cls == "control_identity":
            assert c.decoded is None
    names = set(classes)
    if fmt == sc.PROCESSED:
        assert names == {"x_eq_p", "x_eq_p_signed", "x_eq_p_plus_1", "x_all_ones", "x_4_nonresidue", "x_10_nonresidue", "x_0_signed", "control_sign_flipped"}
        el = {c.cls: int.from_bytes(c.element, "little") for c in cases}
        assert el["x_eq_p"] == P and el["x_eq_p_signed"] == P | sc.TOP and el["x_eq_p_plus_1"] == P + 1 and el["x_all_ones"] == sc.TOP - 1
        assert el["x_4_nonresidue"] == 4 and el["x_10_nonresidue"] & (sc.TOP - 1) == 10 and el["x_0_signed"] == sc.TOP
    else:
        assert names == {"x_plus_p", "y_plus_p", "y_plus_1", "x_zeroed", "y_zeroed", "control_identity"}
        rinv = inv(MONT_R, P)
        for c in cases:
            d = donor[c.section][sc.DONOR_AT]
            xm, ym = int.from_bytes(c.element[:32], "little"), int.from_bytes(c.element[32:], "little")
            if c.cls in ("x_plus_p", "y_plus_p"):  # the same point mod p, one coordinate out of range: the unchecked parser decodes the donor
                assert max(xm, ym) >= P and (xm * rinv % P, ym * rinv % P) == d
                assert serde.g1_parse(c.element, sc.RAW_BYTES_UNCHECKED) == d
            if c.cls == "y_plus_1":
                assert xm < P and ym < P and not C.is_on_curve((xm * rinv % P, ym * rinv % P))


@pytest.mark.parametrize("fmt", sc.CHECKED)
def test_g2_classes_carry_the_oracle_verdict(fmt):
    cases = sc.g2_cases(7, fmt)
    classes = sc.G2_CLASSES[fmt]
    assert [(c.cls, c.which) for c in cases] == [(name, w) for name in classes for w in (0, 1)]
    for c in cases:
        assert c.admit == classes[c.cls][0], (c.cls, c.which)
        d = sc.g2_points()[c.which]
        if c.cls == "control_sign_flipped":
            assert c.decoded == (d[0], ((-d[1][0]) % P, (-d[1][1]) % P))
        if c.cls == "control_all_zero":
            assert c.decoded is None
    if fmt == sc.PROCESSED:
        assert {"x_c0_eq_p", "x_c1_eq_p", "x_not_on_twist", "control_all_zero", "control_sign_flipped"} <= set(classes)
        x = sc.G2_X_OFF
        rhs = C.f2add(C.f2mul(C.f2mul(x, x), x), serde.G2_B)
        assert pow((rhs[0] ** 2 + rhs[1] ** 2) % P, (P - 1) // 2, P) == P - 1  # its norm is a non-residue: no square root in Fq2
    else:
        assert {"x_c0_plus_p", "x_c1_plus_p", "y_c0_plus_p", "y_c1_plus_p", "y_c0_plus_1"} <= set(classes)


@pytest.mark.parametrize("k", sc.KS)
def test_scalar_classes_and_positions_on_the_oracle_key_image(k):
    kw, sh = sc.key_shape(k)
    asg = zk.circuit.synthesize(zk.circuit.CircuitParams(**kw), 0x5EED0019)
    fpk = fp.keygen(sh, asg.fixed, asg.copies)
    n = sh.n
    for fmt in sc.CHECKED:
        img = serde.pk_bytes(fpk, asg.fixed, fmt)
        cases = sc.scalar_cases(sh, img, fmt)
        pos = sc.scalar_positions(sh, fmt)
        assert list(pos) == ["l0_first", "l_active_row_last", "fixed_polys_inner", "last_sigma_coset_first", "last_sigma_coset_last"]
        want_cls = [name for name, (admit, fmts, make) in sc.SCALAR_CLASSES.items() if fmt in fmts]
        assert want_cls == ["eq_r", "r_plus_1", "all_ones"] + (["valid_plus_r"] if fmt == sc.RAW_BYTES else []) + ["control_r_minus_1"]
        assert [(c.cls, c.position) for c in cases] == [(a, b) for a in want_cls for b in pos]
        for c in cases:
            assert c.admit == sc.SCALAR_CLASSES[c.cls][0] and c.offset == pos[c.position]
            if c.cls == "valid_plus_r":
                assert int.from_bytes(c.element, "little") - R == int.from_bytes(img[c.offset:c.offset + 32], "little") < R
            if c.cls == "control_r_minus_1":
                assert c.value == (R - 1 if fmt == sc.PROCESSED else (R - 1) * inv(MONT_R, R) % R)
        # the positions are the elements the issue names, found again from the oracle's own vectors
        at = lambda off: bytes(img[off:off + 32])
        assert pos["last_sigma_coset_last"] == len(img) - 32 and pos["last_sigma_coset_first"] == len(img) - 32 * 4 * n
        assert at(pos["l0_first"]) == serde.fr_vec_bytes(fpk.l0_e[:1], fmt)
        assert at(pos["last_sigma_coset_first"]) == serde.fr_vec_bytes(fpk.sig_e[-1][:1], fmt)
        assert at(pos["last_sigma_coset_last"]) == serde.fr_vec_bytes(fpk.sig_e[-1][-1:], fmt)
        from zkoracle.vkrepr import halo2_fixed_order
        col = halo2_fixed_order(sh)[-1]
        assert col != sh.fx_table and at(pos["fixed_polys_inner"]) == serde.fr_vec_bytes(fpk.fix_c[col][n // 2 + 1:n // 2 + 2], fmt)
        assert img[pos["l_active_row_last"] + 32:pos["l_active_row_last"] + 36] == serde.be32(sh.n_fix)  # the next word opens fixed_values


def test_stream_positions():
    assert sc.stream_positions(19) == [(0, (1 << 18) - 1), (0, 1 << 18), (0, (1 << 18) + 5), (1, (1 << 19) - 1)]
    with pytest.raises(ValueError):
        serde.g1_parse(sc.NONRESIDUE_X, sc.PROCESSED)
    with pytest.raises(ValueError):
        serde.g1_parse(sc.offcurve_raw(C.mul(C.G1_GEN, TAU)), sc.RAW_BYTES)
