"""Inputs and expected verdicts of the file-codec matrix (tests/test_serde_cases.py pins them on the CPU, tests/test_serde_host.py
holds the host codec of csrc/serde_host.h against them, tests/test_gpu_serde_edges.py the device kernels of csrc/serde.hip).

Everything is exact.  A case is one altered element inside an otherwise valid image; its verdict and its decoded value are the
oracle's plain-integer codec (zkoracle.serde.g1_parse / g2_parse / fr_parse) applied to that element alone, never the engine's.
Every class carries the verdict its name promises (`admit`), and the pin test checks the oracle agrees with each name.

Residue facts the classes rest on (test_serde_cases.py re-derives them): 3, 67 = 4^3 + 3 and 1003 = 10^3 + 3 are non-residues
mod p, so no curve point has x = 0, 4 or 10; 2 is a residue, so x = p - 1 has one (y^2 = -1 + 3)."""
import random
from collections import namedtuple

import numpy as np

from zkoracle import cops, curve as C, serde
from zkoracle.field import MONT_R, P, R

PROCESSED, RAW_BYTES, RAW_BYTES_UNCHECKED = serde.PROCESSED, serde.RAW_BYTES, serde.RAW_BYTES_UNCHECKED
CHECKED = (PROCESSED, RAW_BYTES)
KS = (7, 9)  # n = 128: half a 256-thread block, two 64-thread blocks; n = 512: two and eight
G, G_LAGRANGE = 0, 1
TOP = 1 << 255


def le(v):
    return int(v).to_bytes(32, "little")


def g1_size(fmt):
    return 32 if fmt == PROCESSED else 64


def g2_size(fmt):
    return 64 if fmt == PROCESSED else 128


# ------------------------------------------------------------------------------------------------- G1 sections ---

def identity_indices(n):
    return (0, 63, 64, n - 1)


def g_positions(n):
    """Where every malformed-point class goes in g: the first element, both sides of a 64-thread block edge, the end of the launch."""
    return (0, 63, 64, n - 1)


def gl_positions(n):
    return (0, n - 1)


def point_positions(n):
    return [(G, i) for i in g_positions(n)] + [(G_LAGRANGE, i) for i in gl_positions(n)]


GEN_AT, NEG_GEN_AT, XPM1_AT, DONOR_AT = 1, 2, 3, 5  # the generator, its negative, the point with x = p - 1, the classes' donor
Y_OF_XPM1 = serde.fq_sqrt(2)  # (p - 1)^3 + 3 = 2


def _points_arr(pts):
    """[(x, y) | None] -> (n, 8) Montgomery affine array"""
    flat = []
    for pt in pts:
        flat += [0, 0] if pt is None else [pt[0], pt[1]]
    return cops.to_mont_arr(cops.ints_to_arr(flat), 1).reshape(-1, 8)


_sections = {}


def sections(k):
    """(g, g_lagrange): two different (n, 8) Montgomery affine arrays of known multiples of the generator, with the identity at
    0, 63, 64 and n - 1, the generator, its negative and the point with x = p - 1.  Not an SRS of any tau: the codecs do not care."""
    if k not in _sections:
        n = 1 << k
        out = []
        for sec in (G, G_LAGRANGE):
            rnd = random.Random(0x5E7DE + 16 * k + sec)
            s = [rnd.randrange(2, R) for _ in range(n)]
            s[GEN_AT], s[NEG_GEN_AT] = 1, R - 1
            a = cops.fixed_base_g1(cops.fr_mont(s))
            a[XPM1_AT] = _points_arr([(P - 1, Y_OF_XPM1 if sec == G else P - Y_OF_XPM1)])[0]
            for i in identity_indices(n):
                a[i] = 0
            pts = cops.affine_arr_to_ints(a)
            assert pts[GEN_AT] == C.G1_GEN and pts[NEG_GEN_AT] == C.neg(C.G1_GEN) and pts[XPM1_AT][0] == P - 1
            assert all(pts[i] is None for i in identity_indices(n)) and sum(pt is None for pt in pts) == 4
            assert all(C.is_on_curve(pt) for pt in pts if pt is not None)
            assert {pt[1] & 1 for pt in pts if pt is not None} == {0, 1}  # both parities of y: both branches of the sign rule
            out.append(a)
        assert not np.array_equal(out[0], out[1])
        _sections[k] = tuple(out)
    return _sections[k]


def section_points(k):
    return tuple(cops.affine_arr_to_ints(a) for a in sections(k))


def srs_image(k, fmt):
    g, gl = sections(k)
    return serde.srs_bytes(k, fmt, g, gl)


def g1_offset(n, fmt, section, index):
    return 4 + (section * n + index) * g1_size(fmt)


def g2_offset(n, fmt, which):
    """which: 0 = g2, 1 = s_g2"""
    return 4 + 2 * n * g1_size(fmt) + which * g2_size(fmt)


def splice(img, off, enc):
    assert 0 <= off and off + len(enc) <= len(img)
    return img[:off] + enc + img[off + len(enc):]


# --------------------------------------------------------------------------------------- malformed G1 points ---
# class: name -> (admit, donor point -> the element's bytes).  The donor is a valid non-identity point of the section; a class that
# needs none ignores it.

def _proc(x, sign):
    return le(x | (TOP if sign else 0))


def _raw(xm, ym):
    return le(xm) + le(ym)


def _mont(v):
    return v * MONT_R % P


G1_CLASSES = {
    PROCESSED: {
        "x_eq_p": (False, lambda d: _proc(P, 0)),
        "x_eq_p_signed": (False, lambda d: _proc(P, 1)),
        "x_eq_p_plus_1": (False, lambda d: _proc(P + 1, 0)),
        "x_all_ones": (False, lambda d: _proc(TOP - 1, 0)),
        "x_4_nonresidue": (False, lambda d: _proc(4, 0)),
        "x_10_nonresidue": (False, lambda d: _proc(10, 1)),
        "x_0_signed": (False, lambda d: _proc(0, 1)),  # 3 is a non-residue: no point, and not the identity
        "control_sign_flipped": (True, lambda d: _proc(d[0], 1 - (d[1] & 1))),  # -> -donor
    },
    RAW_BYTES: {
        "x_plus_p": (False, lambda d: _raw(_mont(d[0]) + P, _mont(d[1]))),  # on the curve mod p: only the range check refuses it
        "y_plus_p": (False, lambda d: _raw(_mont(d[0]), _mont(d[1]) + P)),
        "y_plus_1": (False, lambda d: _raw(_mont(d[0]), (_mont(d[1]) + 1) % P)),
        "x_zeroed": (False, lambda d: _raw(0, _mont(d[1]))),
        "y_zeroed": (False, lambda d: _raw(_mont(d[0]), 0)),
        "control_identity": (True, lambda d: _raw(0, 0)),
    },
}

PointCase = namedtuple("PointCase", "k fmt cls section index admit image element decoded")


def oracle_verdict(parse, enc, fmt):
    """(admitted, decoded value) of one element by the oracle's codec"""
    try:
        return True, parse(enc, fmt)
    except ValueError:
        return False, None


def point_cases(k, fmt):
    """Every class of `fmt` at every position: the image with that one element replaced, the oracle's verdict on the element and
    what it decodes to (None: the identity, or refused)."""
    n = 1 << k
    base = srs_image(k, fmt)
    pts = section_points(k)
    out = []
    for cls, (admit, make) in G1_CLASSES[fmt].items():
        for section, index in point_positions(n):
            enc = make(pts[section][DONOR_AT])
            assert len(enc) == g1_size(fmt)
            ok, dec = oracle_verdict(serde.g1_parse, enc, fmt)
            out.append(PointCase(k, fmt, cls, section, index, ok, splice(base, g1_offset(n, fmt, section, index), enc), enc, dec))
    return out


def offcurve_raw(donor):
    """The off-curve class of the unchecked format and of the streamed reader: (x, y + 1)"""
    return G1_CLASSES[RAW_BYTES]["y_plus_1"][1](donor)


NONRESIDUE_X = _proc(4, 0)


def stream_positions(K):
    """Where the streamed reader (staging chunk 2^18 points) gets a bad point at K = 19: the last point of the first chunk, the first of
    the second, one further in (beyond a kept k = 17), the last point of g_lagrange."""
    chunk = 1 << 18
    assert (1 << K) > chunk + 5
    return [(G, chunk - 1), (G, chunk), (G, chunk + 5), (G_LAGRANGE, (1 << K) - 1)]


# ------------------------------------------------------------------------------------------------------- G2 ---

_g2_points = []


def g2_points():
    """(g2, s_g2) of every image here: the generator and [tau]G2, as serde.srs_bytes writes them"""
    if not _g2_points:
        from zkoracle.srs import TAU

        _g2_points.extend((C.G2_GEN, C.g2_mul(C.G2_GEN, TAU)))
    return tuple(_g2_points)


def _g2_x_not_on_twist():
    """The first x = (c, 1) for which x^3 + b' is no square in Fq2 (its norm is a non-residue)"""
    for c in range(1, 64):
        x = (c, 1)
        if serde.fq2_sqrt(C.f2add(C.f2mul(C.f2mul(x, x), x), serde.G2_B)) is None:
            return x
    raise AssertionError("no non-square among the first counters")


G2_X_OFF = _g2_x_not_on_twist()


# a point of the twist whose y is purely imaginary: x^3 + b' = -4 lies in Fq and is a non-residue there, so its root is 2u — the
# one case in which a square root in Fq2 has no real part (the sign bit then says nothing: both roots have y.c0 = 0)
G2_X_IMAGINARY_Y = (0x0A0D4094608728F1B8F623B4CDF0CCB597EB4EB88CDC572E1DCC383891B6E830,
                    0x1162DBBBA03B247009EEB574E73A5C682869A85A205124F4E630B6CAB40A5EFC)
assert serde.g2_on_curve((G2_X_IMAGINARY_Y, (0, 2)))


def _g2_proc(x0, x1, sign):
    return le(x0) + le(x1 | (TOP if sign else 0))


def _g2_raw(d, add=(0, 0, 0, 0), mod=False):
    c = [_mont(v) + a for v, a in zip((d[0][0], d[0][1], d[1][0], d[1][1]), add)]
    return b"".join(le(v % P if mod else v) for v in c)


G2_CLASSES = {
    PROCESSED: {
        "x_c0_eq_p": (False, lambda d: _g2_proc(P, d[0][1], d[1][0] & 1)),
        "x_c0_plus_p": (False, lambda d: _g2_proc(d[0][0] + P, d[0][1], d[1][0] & 1)),
        "x_c1_eq_p": (False, lambda d: _g2_proc(d[0][0], P, d[1][0] & 1)),
        "x_c1_plus_p_signed": (False, lambda d: _g2_proc(d[0][0], d[0][1] + P, 1)),
        "x_not_on_twist": (False, lambda d: _g2_proc(G2_X_OFF[0], G2_X_OFF[1], 0)),
        "x_not_on_twist_signed": (False, lambda d: _g2_proc(G2_X_OFF[0], G2_X_OFF[1], 1)),
        "control_y_imaginary": (True, lambda d: _g2_proc(G2_X_IMAGINARY_Y[0], G2_X_IMAGINARY_Y[1], 0)),
        "control_y_imaginary_signed": (True, lambda d: _g2_proc(G2_X_IMAGINARY_Y[0], G2_X_IMAGINARY_Y[1], 1)),
        "control_all_zero": (True, lambda d: bytes(64)),  # the identity, as for G1
        "control_sign_flipped": (True, lambda d: _g2_proc(d[0][0], d[0][1], 1 - (d[1][0] & 1))),  # -> y negated
    },
    RAW_BYTES: {
        "x_c0_plus_p": (False, lambda d: _g2_raw(d, (P, 0, 0, 0))),
        "x_c1_plus_p": (False, lambda d: _g2_raw(d, (0, P, 0, 0))),
        "y_c0_plus_p": (False, lambda d: _g2_raw(d, (0, 0, P, 0))),
        "y_c1_plus_p": (False, lambda d: _g2_raw(d, (0, 0, 0, P))),
        "y_c0_plus_1": (False, lambda d: _g2_raw(d, (0, 0, 1, 0), mod=True)),
        "control_all_zero": (True, lambda d: bytes(128)),
    },
}

G2Case = namedtuple("G2Case", "k fmt cls which admit image element decoded")


def g2_cases(k, fmt):
    """Every G2 class of `fmt` on g2 (which = 0) and on s_g2 (1) of the k image"""
    n = 1 << k
    base = srs_image(k, fmt)
    out = []
    for cls, (admit, make) in G2_CLASSES[fmt].items():
        for which, donor in enumerate(g2_points()):
            enc = make(donor)
            assert len(enc) == g2_size(fmt)
            ok, dec = oracle_verdict(serde.g2_parse, enc, fmt)
            out.append(G2Case(k, fmt, cls, which, ok, splice(base, g2_offset(n, fmt, which), enc), enc, dec))
    return out


# -------------------------------------------------------------------------------------- scalars of a key image ---
# class: name -> (admit, the valid 32 bytes at the position -> the element's bytes).  Processed holds the canonical value, RawBytes
# the Montgomery limb image; the rule is the same on both: the stored integer is below r.

SCALAR_CLASSES = {
    "eq_r": (False, (PROCESSED, RAW_BYTES), lambda v: le(R)),
    "r_plus_1": (False, (PROCESSED, RAW_BYTES), lambda v: le(R + 1)),
    "all_ones": (False, (PROCESSED, RAW_BYTES), lambda v: le((1 << 256) - 1)),
    "valid_plus_r": (False, (RAW_BYTES,), lambda v: le(int.from_bytes(v, "little") + R)),
    "control_r_minus_1": (True, (PROCESSED, RAW_BYTES), lambda v: le(R - 1)),
}


def vk_len(sh, fmt):
    return 8 + (sh.n_fix + len(sh.perm_cols)) * g1_size(fmt) + (sh.n_gate + (1 if sh.single else 0)) * (sh.n // 8)


def pk_len(sh, fmt):
    n, N, m = sh.n, 4 * sh.n, len(sh.perm_cols)
    return vk_len(sh, fmt) + 3 * (4 + 32 * N) + 6 * 4 + (sh.n_fix + m) * (2 * (4 + 32 * n) + 4 + 32 * N)


def scalar_positions(sh, fmt):
    """name -> byte offset in the ProvingKey image of the shape: the first scalar of the file, the end of a 4n vector, one element of
    a length-n slice (a fixed_polys column that is not the range table, which the reader recommits), both ends of the last vector."""
    n, N = sh.n, 4 * sh.n
    poly_n, poly_N = 4 + 32 * n, 4 + 32 * N
    l0 = vk_len(sh, fmt)
    fixed_values = l0 + 3 * poly_N
    fixed_polys = fixed_values + 4 + sh.n_fix * poly_n
    assert sh.n_fix >= 2  # file position 0 is the table column (vkrepr.halo2_fixed_order); the last one is a selector / constants column
    end = pk_len(sh, fmt)
    return {
        "l0_first": l0 + 4,
        "l_active_row_last": l0 + 3 * poly_N - 32,
        "fixed_polys_inner": fixed_polys + 4 + (sh.n_fix - 1) * poly_n + 4 + 32 * (n // 2 + 1),
        "last_sigma_coset_first": end - 32 * N,
        "last_sigma_coset_last": end - 32,
    }


def check_pk_walk(sh, img, fmt):
    """The positions above rest on this walk: every length word of the image is where the layout says (u32 BE)."""
    n, N, m = sh.n, 4 * sh.n, len(sh.perm_cols)
    assert len(img) == pk_len(sh, fmt)
    pos = vk_len(sh, fmt)
    be = lambda o: int.from_bytes(bytes(img[o:o + 4]), "big")
    for _ in range(3):
        assert be(pos) == N
        pos += 4 + 32 * N
    for count, ln in ((sh.n_fix, n), (sh.n_fix, n), (sh.n_fix, N), (m, n), (m, n), (m, N)):
        assert be(pos) == count
        pos += 4
        for _ in range(count):
            assert be(pos) == ln
            pos += 4 + 32 * ln
    assert pos == len(img)


KEY_SHAPES = {7: (4, 1, 1, 7, 5, 0), 9: (2, 1, 1, 9, 8, 0)}  # (advice, lookup advice, fixed, k, lookup bits, idle gate columns)


def key_shape(k):
    """(CircuitParams arguments, oracle Shape) of the key the scalar classes go through: n = 128 is half a 256-thread block of the
    scalar kernels, n = 512 two blocks (4n = 2048: eight)."""
    from zkoracle import plonk

    A, L, Fx, k_, lb, idle = KEY_SHAPES[k]
    return dict(degree=k_, num_advice=A, num_lookup_advice=L, num_fixed=Fx, lookup_bits=lb, idle_gate_columns=idle), plonk.Shape(k_, A, L, Fx, lb, idle)


ScalarCase = namedtuple("ScalarCase", "fmt cls position offset admit element value")


def scalar_cases(sh, img, fmt):
    """Every scalar class of `fmt` at every position of the valid key image `img` (bytes or a uint8 array): the case names the offset
    and the 32 bytes to put there (the image is large; the test splices)."""
    check_pk_walk(sh, img, fmt)
    out = []
    for cls, (admit, fmts, make) in SCALAR_CLASSES.items():
        if fmt not in fmts:
            continue
        for name, off in scalar_positions(sh, fmt).items():
            valid = bytes(img[off:off + 32])
            serde.fr_parse(valid, fmt)  # the position holds a scalar of the valid image
            enc = make(valid)
            assert len(enc) == 32
            ok, val = oracle_verdict(serde.fr_parse, enc, fmt)
            out.append(ScalarCase(fmt, cls, name, off, ok, enc, val))
    return out
