"""The Fr NTT (csrc/ntt.hip) at every size, plan, entry point and radix option, whole vectors, bit-exact.

  a. zk_ntt_bn254_fr with the standard root and its inverse at every log_n in 0..24 and 26 on canonical random input (words up to
     r - 1, tests/ntt_cases.py), the structured r - 1 patterns where the lazy bounds of the first pass are largest, impulses against
     the closed form (a reference that shares no butterfly with anything);
  b. non-standard primitive roots: own twiddle table, no folded last pass, one to three passes;
  c. the resident entry points: zk_lagrange_to_coeff / zk_coeff_to_lagrange at every k in 0..22, zk_coeff_to_extended over the source
     lengths around the three-quarters-zero edge (N/4 is the last length the zero-quarter first pass takes), zk_extended_to_coeff
     over n_out values that are no multiple of 3 or of a tile, on all three LDS tiles; round trips;
  d. ZK_OPT_NTT_MAX_RADIX_LOG2 = 1..11 over (a) and (c): the option changes the plan (1 to 22 passes here, all three tiles, both
     ping-pong parities of an in-place transform, radix 2 .. 2^11 in every pass position) and not one byte.

The oracle side (zkoracle.cops.ntt: a C restatement of best_fft) is computed once per size and shared; tests/test_ntt_cases.py pins
the references on the CPU.  Nothing here needs an SRS."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ntt_cases as NC  # noqa: E402
from webauthn_halo2_amd import engine as E  # noqa: E402
from zkoracle import cops  # noqa: E402
from zkoracle.field import R, omega  # noqa: E402

pytestmark = pytest.mark.gpu

OPT = E.ZK_OPT_NTT_MAX_RADIX_LOG2
CACHE_LOG_N = 22  # oracle vectors up to this size are kept for the option sweep (128 MiB each at 2^22)
_seam, _structured, _coset = {}, {}, {}


def root(log_n, inverse):
    return NC.omega_inv(log_n) if inverse else omega(log_n)


def seam_input(log_n):
    return NC.canonical_random(np.random.default_rng(7000 + log_n), 1 << log_n)


def seam_case(log_n, inverse):
    """(input, oracle transform) of the random case of size 2^log_n: one input per size, both directions."""
    if log_n > CACHE_LOG_N:
        a = seam_input(log_n)
        return a, cops.ntt(a, root(log_n, inverse), log_n)
    if ("in", log_n) not in _seam:
        _seam["in", log_n] = seam_input(log_n)
    a = _seam["in", log_n]
    if (log_n, inverse) not in _seam:
        _seam[log_n, inverse] = cops.ntt(a, root(log_n, inverse), log_n)
    return a, _seam[log_n, inverse]


def structured_case(log_n, name, inverse):
    a = NC.structured(1 << log_n, name)
    if log_n not in (11, 22):  # the two sizes that are run again under option 11
        return a, cops.ntt(a, root(log_n, inverse), log_n)
    key = (log_n, name, inverse)
    if key not in _structured:
        _structured[key] = cops.ntt(a, root(log_n, inverse), log_n)
    return a, _structured[key]


def coset_case(ext_k):
    """The coset pair of size N = 2^ext_k: a source of N/4 coefficients with its extended form, a full extended vector with its
    coefficients."""
    if ext_k not in _coset:
        N = 1 << ext_k
        rng = np.random.default_rng(9000 + ext_k)
        f = NC.canonical_random(rng, max(N // 4, 1))
        e = NC.canonical_random(rng, N)
        c = (f, NC.coeff_to_extended(f, ext_k), e, NC.extended_to_coeff(e, ext_k))
        if ext_k > CACHE_LOG_N:
            return c
        _coset[ext_k] = c
    return _coset[ext_k]


def run_seam(engine, a, log_n, inverse):
    return engine.ntt(a, NC.mont1(root(log_n, inverse)), log_n)


def mismatch(got, want):
    """Where two vectors differ: count, first and last index, the residues mod 3 and mod 512 of the first few (the period of the
    coset factors, the smallest tile)."""
    bad = np.flatnonzero((got != want).any(axis=1))
    if not bad.size:
        return "equal"
    head = bad[:64]
    return "%d of %d differ, first %d, last %d, first indices %s, mod 3 %s, mod 512 %s" % (
        bad.size, got.shape[0], bad[0], bad[-1], bad[:8].tolist(), sorted(set((head % 3).tolist())), sorted(set((head % 512).tolist()))[:16])


def check(got, want, what):
    assert np.array_equal(got, want), (what, mismatch(got, want))


# ------------------------------------------------------------------ a. the seam at every size ----

@pytest.mark.parametrize("log_n", list(range(25)))
def test_seam_every_size(engine, log_n):
    for inverse in (False, True):
        a, want = seam_case(log_n, inverse)
        check(run_seam(engine, a, log_n, inverse), want, (log_n, inverse))


def test_seam_largest_size(engine):
    """2^26, the largest transform the call accepts: once per direction, random input (2 GiB per host array)."""
    log_n = 26
    a = seam_input(log_n)
    for inverse in (False, True):
        want = cops.ntt(a, root(log_n, inverse), log_n)
        got = run_seam(engine, a, log_n, inverse)
        ok = np.array_equal(got, want)
        what = "equal" if ok else mismatch(got, want)
        del got, want
        assert ok, (log_n, inverse, what)
    del a


@pytest.mark.parametrize("log_n", [10, 16, 18, 20, 22, 24])
def test_seam_largest_stored_words(engine, log_n):
    """Stored r - 1 everywhere, alternating with 0 and on every third index, through first passes of radix 2^5, 2^8, 2^9, 2^10 and the
    four-pass plans: the operands at which the lazy bounds of round0 / bfly_mul (multiples of p, ntt.hip) are largest."""
    for name in NC.STRUCTURED:
        for inverse in (False, True):
            a, want = structured_case(log_n, name, inverse)
            check(run_seam(engine, a, log_n, inverse), want, (log_n, name, inverse))


@pytest.mark.parametrize("log_n", [9, 16, 18, 20, 21, 23])
def test_seam_impulses_against_closed_form(engine, log_n):
    """c e_j -> c w^(i j): at the first two elements of the first two rows of the first pass's R x N/R view, the middle and the end."""
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    for inverse in (False, True):
        w = root(log_n, inverse)
        for q, j in enumerate(NC.impulse_positions(log_n)):
            c = R - 1 if q % 2 == 0 else int(cops.fr_ints(NC.canonical_random(rng, 1))[0]) or 1
            got = run_seam(engine, NC.impulse(n, j, c), log_n, inverse)
            check(got, NC.impulse_response(n, j, c, w), (log_n, inverse, j))


# ------------------------------------------------------------------ b. non-standard primitive roots ----

@pytest.mark.parametrize("log_n", [1, 3, 5, 6, 7, 8, 9, 12, 16, 17, 19, 21])
def test_seam_nonstandard_roots(engine, log_n):
    """w = omega^e, e odd: the call makes its own twiddle table (a 64-power walk, on a table shorter than one walk below 2^6), gets
    no folded last pass and no post-scale."""
    n = 1 << log_n
    a = seam_case(log_n, False)[0]
    for e in sorted({5, n - 3}):
        w = pow(omega(log_n), e, R)
        check(engine.ntt(a, NC.mont1(w), log_n), cops.ntt(a, w, log_n), (log_n, e))


# ------------------------------------------------------------------ c. resident entry points ----

@pytest.mark.parametrize("k", list(range(23)))
def test_lagrange_coeff_every_size(engine, k):
    n = 1 << k
    v = NC.canonical_random(np.random.default_rng(8000 + k), n)
    p = engine.poly(n, v)
    try:
        engine.lagrange_to_coeff(p)
        coeff = engine.download(p)
        check(coeff, NC.lagrange_to_coeff(v, k), ("lagrange_to_coeff", k))
        engine.coeff_to_lagrange(p)
        check(engine.download(p), v, ("coeff_to_lagrange o lagrange_to_coeff", k))
        engine.coeff_to_lagrange(p)
        check(engine.download(p), NC.coeff_to_lagrange(v, k), ("coeff_to_lagrange", k))
        engine.lagrange_to_coeff(p)
        check(engine.download(p), v, ("lagrange_to_coeff o coeff_to_lagrange", k))
    finally:
        p.free()


EXT_KS = [2, 3, 5, 8, 9, 10, 11, 12, 14, 16, 17, 18, 19, 20, 21, 23]


def source_lengths(N):
    """N/4 is the last length of the zero-quarter first pass; its neighbours, the ends, and one that is no power of two."""
    return sorted({ln for ln in (N // 4, N // 4 + 1, N // 4 - 1, 1, 3, N // 2, N, 3 * N // 16 + 5) if 1 <= ln <= N})


def padded(f, N):
    out = np.zeros((N, 4), dtype=np.uint64)
    out[:f.shape[0]] = f
    return out


@pytest.mark.parametrize("ext_k", EXT_KS)
def test_coeff_to_extended_source_lengths(engine, ext_k):
    """The whole destination against the reference for every source length; the source is left as it was; the destination's earlier
    contents (junk, then the previous length's result, then coefficients) do not matter; extended_to_coeff brings f back,
    zero-padded."""
    N = 1 << ext_k
    rng = np.random.default_rng(8100 + ext_k)
    dst = engine.poly(N, NC.all_max(N))
    try:
        for ln in source_lengths(N):
            if ln == max(N // 4, 1):
                f, want = coset_case(ext_k)[:2]
            else:
                f = NC.canonical_random(rng, ln)
                want = NC.coeff_to_extended(f, ext_k)
            src = engine.poly(ln, f)
            try:
                engine.coeff_to_extended(src, dst)
                check(engine.download(dst), want, ("coeff_to_extended", ext_k, ln))
                check(engine.download(src), f, ("source after coeff_to_extended", ext_k, ln))
                if ln in (N // 4, 3 * N // 16 + 5, N):
                    engine.extended_to_coeff(dst, N)
                    check(engine.download(dst), padded(f, N), ("extended_to_coeff o coeff_to_extended", ext_k, ln))
                    engine.coeff_to_extended(src, dst)  # over coefficients this time
                    check(engine.download(dst), want, ("coeff_to_extended again", ext_k, ln))
            finally:
                src.free()
    finally:
        dst.free()


@pytest.mark.parametrize("ext_k", [11, 19, 21])
def test_coeff_to_extended_largest_words_by_residue(engine, ext_k):
    """A random source of N/4 coefficients with stored r - 1 on i % 3 == m: the largest operand under each of the period-3
    pre-factors 1, zeta, zeta^2 of the zero-quarter first pass (2^11: one pass; 2^19: tile 2^11; 2^21: tile 2^9)."""
    N = 1 << ext_k
    dst = engine.poly(N)
    try:
        for m in range(3):
            f = coset_case(ext_k)[0].copy()
            f[m::3] = NC.R_MINUS_1
            src = engine.poly(N // 4, f)
            try:
                engine.coeff_to_extended(src, dst)
                check(engine.download(dst), NC.coeff_to_extended(f, ext_k), (ext_k, m))
            finally:
                src.free()
    finally:
        dst.free()


@pytest.mark.parametrize("ext_k", EXT_KS)
def test_extended_to_coeff_truncations(engine, ext_k):
    """The first n_out coefficients (what the header promises) for n_out around the multiples of 3 and the ends."""
    N = 1 << ext_k
    e, want = coset_case(ext_k)[2:]
    ext = engine.poly(N)
    try:
        for n_out in sorted({0, 1, 2, 3, 4, N // 4, 3 * N // 4, 3 * N // 4 + 1, N - 1, N}):
            engine.upload(ext, e)
            engine.extended_to_coeff(ext, n_out)
            if n_out:
                check(engine.download(ext, n_out), want[:n_out], ("extended_to_coeff", ext_k, n_out))
    finally:
        ext.free()


# ------------------------------------------------------------------ d. the radix option ----

OPT_SEAM_SIZES = [1, 4, 6, 7, 8, 9, 11, 12, 16, 17, 19, 21, 22]
OPT_COSET_SIZES = [6, 9, 11, 12, 17, 19, 21]


@pytest.mark.parametrize("value", list(range(1, 12)))
def test_radix_option_changes_no_byte_of_the_seam(engine, value):
    engine.set_option(OPT, value)
    try:
        for log_n in OPT_SEAM_SIZES:
            for inverse in (False, True):
                a, want = seam_case(log_n, inverse)
                check(run_seam(engine, a, log_n, inverse), want, (value, log_n, inverse))
    finally:
        engine.set_option(OPT, 0)


@pytest.mark.parametrize("value", list(range(1, 12)))
def test_radix_option_changes_no_byte_of_the_coset_pair(engine, value):
    """zk_coeff_to_extended from N/4 coefficients and zk_extended_to_coeff to 3N/4, in place: pre-factors, the zero-quarter pass at
    radices 2^4 .. 2^11, the post-factors in a general last pass, staging copies at odd pass counts."""
    engine.set_option(OPT, value)
    try:
        for ext_k in OPT_COSET_SIZES:
            N = 1 << ext_k
            f, want_ext, e, want_coeff = coset_case(ext_k)
            src, dst = engine.poly(N // 4, f), engine.poly(N, e)
            try:
                n_out = 3 * N // 4
                engine.extended_to_coeff(dst, n_out)
                check(engine.download(dst, n_out), want_coeff[:n_out], (value, "extended_to_coeff", ext_k))
                engine.coeff_to_extended(src, dst)
                check(engine.download(dst), want_ext, (value, "coeff_to_extended", ext_k))
            finally:
                src.free()
                dst.free()
    finally:
        engine.set_option(OPT, 0)


@pytest.mark.parametrize("log_n", [11, 22])
def test_radix_option_eleven_largest_stored_words(engine, log_n):
    """An 11-stage first pass (4 x 32 + 1 after round0, + 3 per later stage: 156 p of the 160 p the reductions assume), the
    largest bound the code can reach, on the largest stored words."""
    engine.set_option(OPT, 11)
    try:
        for name in NC.STRUCTURED:
            for inverse in (False, True):
                a, want = structured_case(log_n, name, inverse)
                check(run_seam(engine, a, log_n, inverse), want, (log_n, name, inverse))
    finally:
        engine.set_option(OPT, 0)


def test_radix_option_rejects_values_out_of_range(engine):
    from webauthn_halo2_amd import ZkError

    for bad in (-1, 12, 1 << 20):
        with pytest.raises(ZkError):
            engine.set_option(OPT, bad)
    a, want = seam_case(9, False)  # and the refusals left the default in place
    check(run_seam(engine, a, 9, False), want, "after refused values")
