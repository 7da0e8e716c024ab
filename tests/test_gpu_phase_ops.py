"""The phase-level provers of the C ABI (zk_lookup_permute, zk_lookup_product, zk_permutation_product, zk_poly_lincomb,
zk_random_poly, zk_pk_export_poly, zk_poly_upload_range, zk_poly_copy_range) against the plain-integer oracle of tests/phase_ref.py
on the inputs a host of that ABI may hand them and zk_prove never does: lookup columns of every multiplicity pattern, beta and
gamma chosen so that a denominator or a numerator of a grand product IS zero, coefficient lists that put zk_poly_lincomb's
lazy sums at their bounds, block counters across the 32-bit carry.  Every comparison is exact over all rows the header promises
(a', s': rows 0 .. n - 8; every z: rows 0 .. n - 7); the rows behind them carry random values in every input.

Branches and the tests that reach them:
  phase_grand_products, Q == 0 -> fallback     test_placed_zero_*, test_k17_against_array_reference (default option); also
                                               test_grand_products_honest_* where beta = 0 or p - 1 meets a' = 0 or 1
  lk_fill_kernel, hist[0] == 0                 test_lookup_permute[multi-* / short-*], test_lookup_permute_manycols, k = 17
                                               ("all_top", "all_one", "nozero", "two_values"); hist[0] > 0: the "one" shapes
  lincomb_kernel at 40 / 121 inputs of p - 1   test_lincomb_worst_operands; unit / non-unit grouping: every test_lincomb_*
  chacha_fr_kernel, carry into counter word 13 test_random_poly_block_counter[2^32-3], [2^32], [2^63]
Flipping each of these conditions in a scratch build of the library turns the tests named on its line red (and those that
take their a', s' from the same call), the rest of the module stays green."""
import functools
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phase_ref as PR  # noqa: E402
import webauthn_halo2_amd as zk  # noqa: E402
import witness_cases as C  # noqa: E402
from webauthn_halo2_amd import engine as E  # noqa: E402
from zkoracle import cops, prover  # noqa: E402
from zkoracle.field import DELTA, R, inv, omega  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EWITNESS = -1, -5, -6
SHAPES = {"one": (1, 1, 1), "multi": (3, 2, 1), "short": (3, 2, 2)}  # (A, L, F); "short": 7 permutation columns, last chunk of one
SIZES = [(6, 4), (8, 3), (8, 7), (11, 10), (12, 4), (12, 11), (13, 12)]  # (k, lookup_bits): n below / one / two / four scan blocks
MANYCOLS = (36, 12, 2, 7, 5)  # 50 permutation columns: 25 chunks, 12 lookups in one launch
GRID = [(s, k, lb) for s in SHAPES for k, lb in SIZES]


def shape_tuple(name, k, lb):
    return MANYCOLS if name == "manycols" else SHAPES[name] + (k, lb)


def mont(ints):
    return cops.fr_mont([v % R for v in ints])


def m1(v):
    return mont([v])[0]


@functools.lru_cache(maxsize=None)
def host_case(t):
    """(shape, fixed, copies, advice, sigma) of a synthesized circuit; the advice rows the host blinds hold random values."""
    sh, fixed, copies, advice = C.synth_case(t)
    pr = random.Random(hash(t) & 0xFFFF)
    advice = [list(c[:sh.usable_rows]) + [pr.randrange(R) for _ in range(sh.n - sh.usable_rows)] for c in advice]
    return sh, fixed, copies, advice, prover.build_sigma(sh, copies)


class Dev:
    """A key of shape t and resident advice columns on `eng`; `adv` mirrors the device's columns as integers."""

    def __init__(self, eng, t, case=None):
        self.eng, self.t = eng, t
        self.sh, self.fixed, copies, advice, self.sigma = case or host_case(t)
        self.n, self.usable, self.T = self.sh.n, self.sh.usable_rows, 1 << self.sh.lookup_bits
        eng.srs_setup(self.sh.k)
        self.pk = eng.keygen(C.params_of(t), np.stack([C.limbs(c) for c in self.fixed]), copies)
        self.adv = [list(c) for c in advice]
        self.polys = [eng.poly(self.n) for _ in advice]
        for j in range(len(advice)):
            self.put(j, self.adv[j])
        self.tmp = []

    def put(self, j, col):
        self.adv[j] = list(col)
        self.eng.upload_canonical(self.polys[j], C.limbs(col))

    def lookup_column(self, l):
        return 0 if self.sh.single else self.sh.n_gate + l

    def set_lookup_inputs(self, cols):
        """cols[l]: `usable` values for lookup l's column (a_0 for the one-column shape); the blinded rows keep theirs."""
        for l, col in enumerate(cols):
            j = self.lookup_column(l)
            self.put(j, list(col) + self.adv[j][self.usable:])

    def keep(self, polys):
        self.tmp += polys
        return polys

    def release(self):
        for p in self.tmp:
            p.free()
        self.tmp = []

    def close(self):
        self.release()
        for p in self.polys:
            p.free()
        self.eng.pk_free(self.pk)

    # -- reference and device side by side
    def permute(self, blind_seed=1):
        """zk_lookup_permute against PR.permuted_pair -> (a' polys, s' polys, a' ints, s' ints) with the host's 7 blinding rows
        written (random) behind the usable rows, on the device and in the integers."""
        sh, usable = self.sh, self.usable
        want = [PR.permuted_pair(PR.lookup_input(sh, self.fixed, self.adv, l), self.fixed[sh.fx_table], usable)
                for l in range(sh.n_lookups)]
        a, s = self.eng.lookup_permute(self.pk, self.polys)
        self.keep(a + s)
        pr = random.Random(blind_seed)
        ai, si = [], []
        for l in range(sh.n_lookups):
            for got, exp, what, out in ((a[l], want[l][0], "a'", ai), (s[l], want[l][1], "s'", si)):
                assert np.array_equal(self.eng.download(got)[:usable], mont(exp)), (self.t, what, l)
                blind = [pr.randrange(R) for _ in range(self.n - usable)]
                self.eng.upload_range(got, usable, mont(blind))
                out.append(list(exp) + blind)
        return a, s, ai, si

    def check_perm_products(self, beta, gamma, tag=""):
        want = PR.permutation_products(self.sh, self.fixed, self.sigma, self.adv, beta, gamma)
        z = self.eng.permutation_product(self.pk, self.polys, m1(beta), m1(gamma))
        try:
            for ci, (got, exp) in enumerate(zip(z, want)):
                assert np.array_equal(self.eng.download(got)[:self.usable + 1], mont(exp)), (self.t, tag, "chunk", ci)
        finally:
            for p in z:
                p.free()
        return want

    def check_lookup_products(self, a, s, ai, si, beta, gamma, tag=""):
        want = PR.lookup_products(self.sh, self.fixed, self.adv, ai, si, beta, gamma)
        z = self.eng.lookup_product(self.pk, self.polys, a, s, m1(beta), m1(gamma))
        try:
            for l, (got, exp) in enumerate(zip(z, want)):
                assert np.array_equal(self.eng.download(got)[:self.usable + 1], mont(exp)), (self.t, tag, "lookup", l)
        finally:
            for p in z:
                p.free()
        return want


class batch_invert:
    """ZK_OPT_GP_BATCH_INVERT = 1 for the block, the built-in choice afterwards."""

    def __init__(self, eng, on):
        self.eng, self.on = eng, on

    def __enter__(self):
        self.eng.set_option(E.ZK_OPT_GP_BATCH_INVERT, 1 if self.on else 0)

    def __exit__(self, *exc):
        self.eng.set_option(E.ZK_OPT_GP_BATCH_INVERT, 0)


# ---- A. zk_lookup_permute on arbitrary input columns ---------------------------------------------------------------------------
DISTS = ["zero", "all_top", "all_one", "nozero", "once_then_top", "once_then_zero", "two_values", "uniform", "descending"]


def dist_column(name, usable, T, pr):
    if name == "zero":
        return [0] * usable
    if name == "all_top":
        return [T - 1] * usable
    if name == "all_one":
        return [1] * usable
    if name == "nozero":
        return [pr.randrange(1, T) for _ in range(usable)]
    if name in ("once_then_top", "once_then_zero"):
        col = list(range(T)) + [T - 1 if name == "once_then_top" else 0] * (usable - T)
        pr.shuffle(col)
        return col
    if name == "two_values":
        return [pr.choice((1, T - 1)) for _ in range(usable)]
    if name == "uniform":
        return [pr.randrange(T) for _ in range(usable)]
    assert name == "descending"
    return [T - 1 - (r * T) // usable for r in range(usable)]


def lookup_failures(dev):
    """rows of each lookup whose input is off the table, by the integers"""
    sh = dev.sh
    return sum(sum(1 for v in PR.lookup_input(sh, dev.fixed, dev.adv, l)[:dev.usable] if v >= dev.T) for l in range(sh.n_lookups))


def permute_and_verdict(dev):
    """zk_lookup_permute's verdict must be zk_witness_check's: counts[ZK_FAIL_LOOKUP] != 0 iff ZK_EWITNESS."""
    bad = lookup_failures(dev)
    counts, _ = dev.eng.witness_check(dev.pk, dev.polys, cap=0)
    assert counts[E.ZK_FAIL_LOOKUP] == bad, dev.t
    if bad:
        with pytest.raises(zk.ZkError) as e:
            dev.eng.lookup_permute(dev.pk, dev.polys)
        assert e.value.code == EWITNESS
        return None
    return dev.permute()


def run_permute_cases(dev, seed):
    pr = random.Random(seed)
    nl, usable, T = dev.sh.n_lookups, dev.usable, dev.T
    cases = [(d, [d] * nl) for d in DISTS] + [("mixed", [DISTS[(3 + 2 * l) % len(DISTS)] for l in range(nl)])]
    for tag, names in cases:
        dev.set_lookup_inputs([dist_column(nm, usable, T, pr) for nm in names])
        hist0 = [PR.lookup_input(dev.sh, dev.fixed, dev.adv, l)[:usable].count(0) for l in range(nl)]
        print(dev.t, tag, "hist[0] per lookup", hist0)
        if dev.sh.single:
            assert all(hist0), "the one-column shape's unselected rows give 0: the hist[0] > 0 side"
        elif tag in ("all_top", "all_one", "nozero", "two_values"):
            assert not any(hist0), "hist[0] == 0 must be reached here"
        assert permute_and_verdict(dev) is not None, tag
        dev.release()
    # off the table: ZK_EWITNESS on the usable rows, not on the rows the host blinds
    base = dist_column("uniform", usable, T, pr)
    j = dev.lookup_column(nl - 1)
    if dev.sh.single:  # rows q_lookup selects (the others give 0 whatever a_0 holds)
        rows = [r for r in range(usable) if dev.fixed[dev.sh.fx_qlookup][r]]
        first, last = rows[0], rows[-1]
    else:
        first, last = 0, usable - 1
    for row, v in ((first, T), (last, T), (first, (1 << 32) + 1), (last, (5 << 64) + T - 1), (first, R - 1)):
        col = list(base)
        col[row] = v
        dev.set_lookup_inputs([base] * (nl - 1) + [col])
        assert lookup_failures(dev) == 1
        assert permute_and_verdict(dev) is None, (row, v)
    for row in (usable, dev.n - 1):
        for v in (T, (1 << 32) + 1, R - 1):
            dev.set_lookup_inputs([base] * nl)
            col = list(dev.adv[j])
            col[row] = v
            dev.put(j, col)
            assert permute_and_verdict(dev) is not None, (row, v)
            dev.release()


@pytest.mark.parametrize("name,k,lb", GRID, ids=["%s-k%d-lb%d" % g for g in GRID])
def test_lookup_permute(engine, name, k, lb):
    dev = Dev(engine, shape_tuple(name, k, lb))
    try:
        run_permute_cases(dev, 1000 * k + lb)
    finally:
        dev.close()


def test_lookup_permute_manycols(engine):
    dev = Dev(engine, MANYCOLS)
    try:
        assert dev.sh.n_lookups == 12 and dev.sh.n_chunks == 25
        run_permute_cases(dev, 77)
    finally:
        dev.close()


# ---- B. grand products with honest challenges, both device paths ----------------------------------------------------------------
def run_honest_products(dev, seed, dists):
    pr = random.Random(seed)
    nl, usable, T = dev.sh.n_lookups, dev.usable, dev.T
    for d in dists:
        dev.set_lookup_inputs([dist_column(DISTS[(DISTS.index(d) + l) % len(DISTS)] if l else d, usable, T, pr) for l in range(nl)])
        a, s, ai, si = dev.permute()
        for beta, gamma in ((pr.randrange(R), pr.randrange(R)), (R - 1, R - 1), (0, 1)):
            for forced in (False, True):
                with batch_invert(dev.eng, forced):
                    tag = (d, beta, gamma, "batch_invert" if forced else "default")
                    dev.check_perm_products(beta, gamma, tag)
                    dev.check_lookup_products(a, s, ai, si, beta, gamma, tag)
        dev.release()


@pytest.mark.parametrize("name,k,lb", GRID, ids=["%s-k%d-lb%d" % g for g in GRID])
def test_grand_products_honest_challenges(engine, name, k, lb):
    dev = Dev(engine, shape_tuple(name, k, lb))
    try:
        # every distribution of part A below three scan blocks; above, the plain-integer reference sets the pace
        run_honest_products(dev, 31 * k + lb, DISTS if k <= 11 else ["nozero", "once_then_zero", "all_top", "uniform"])
    finally:
        dev.close()


def test_grand_products_honest_challenges_manycols(engine):
    dev = Dev(engine, MANYCOLS)
    try:
        run_honest_products(dev, 5, ["nozero", "once_then_top", "uniform"])
    finally:
        dev.close()


# ---- C. grand products with a zero factor placed on purpose (option at its default: Q == 0 detection) -------------------------
def perm_value(dev, c, r):
    col = dev.sh.perm_cols[c]
    return (dev.fixed[col[1]] if col[0] == "fixed" else dev.adv[col[1]])[r]


def coset_label(dev, c, r):
    return pow(DELTA, c, R) * pow(omega(dev.sh.k), r, R) % R


def zero_rows(dev):
    return [0, dev.usable // 2 + 3, dev.usable - 1, dev.usable, dev.n - 1]


def chunk_picks(dev):
    nc = dev.sh.n_chunks
    return sorted({0, nc // 2, nc - 1})


def run_placed_zero_permutation(dev, seed, rows, chunks):
    pr = random.Random(seed)
    sh, usable = dev.sh, dev.usable
    for ci in chunks:
        cols = range(ci * sh.chunk_len, min(len(sh.perm_cols), (ci + 1) * sh.chunk_len))
        for r in rows:
            c = pr.choice(list(cols))
            beta = pr.randrange(R)
            gamma = -(perm_value(dev, c, r) + beta * dev.sigma[c][r]) % R
            want = dev.check_perm_products(beta, gamma, ("zero denominator", "chunk", ci, "column", c, "row", r))
            if r < usable:  # the reference's own statement of what a collapsed product does to the chain
                assert not any(want[ci][r + 1:]) and all(not any(z) for z in want[ci + 1:])
                assert r == 0 or any(want[ci][:r + 1])
            else:
                assert all(all(z) for z in want), "a zero behind the usable rows leaves every promised row as it was"


def zero_denominators(dev, beta, gamma):
    """rows (all n of them: the device multiplies the blinded rows into its total too) on which some permutation denominator is zero"""
    return [(c, r) for c in range(len(dev.sh.perm_cols)) for r in range(dev.n)
            if (perm_value(dev, c, r) + beta * dev.sigma[c][r] + gamma) % R == 0]


def run_zero_numerators(dev, seed):
    """a zero numerator with NO zero denominator (the fast path is kept, z is 0 from row r + 1 on), and one beside a zero denominator
    in both orders.  Under a satisfied copy constraint the cell that sigma maps onto (c, r) holds the same value, so its denominator
    vanishes with (c, r)'s numerator: the first case takes a cell of a copy cycle and gives it another value."""
    pr = random.Random(seed)
    sh, usable = dev.sh, dev.usable
    m = len(sh.perm_cols)
    for ci in chunk_picks(dev):
        cells = [(c, r) for c in range(ci * sh.chunk_len, min(m, (ci + 1) * sh.chunk_len)) if sh.perm_cols[c][0] == "advice"
                 for r in range(1, usable - 1) if dev.sigma[c][r] != coset_label(dev, c, r)]
        if not cells:
            continue
        c, r = pr.choice(cells)
        j = sh.perm_cols[c][1]
        kept = list(dev.adv[j])
        col = list(kept)
        col[r] = pr.randrange(1 << 200, R)
        dev.put(j, col)
        beta = pr.randrange(R)
        gamma = -(perm_value(dev, c, r) + coset_label(dev, c, r) * beta) % R
        assert not zero_denominators(dev, beta, gamma)
        want = dev.check_perm_products(beta, gamma, ("zero numerator", "column", c, "row", r))
        assert all(want[ci][:r + 1]) and not any(want[ci][r + 1:]) and all(not any(z) for z in want[ci + 1:])
        dev.put(j, kept)
    for order in ("numerator first", "denominator first"):
        c1, c2 = pr.randrange(m), pr.randrange(m)
        r1, r2 = sorted(pr.sample(range(1, usable - 1), 2))
        if order == "denominator first":
            r1, r2 = r2, r1
        # numerator of (c1, r1) and denominator of (c2, r2) zero:  gamma + label beta = -v1,  gamma + sigma beta = -v2
        lab, sg = coset_label(dev, c1, r1), dev.sigma[c2][r2]
        assert lab != sg
        beta = (perm_value(dev, c2, r2) - perm_value(dev, c1, r1)) * inv((lab - sg) % R, R) % R
        gamma = -(perm_value(dev, c1, r1) + lab * beta) % R
        assert (perm_value(dev, c2, r2) + sg * beta + gamma) % R == 0
        dev.check_perm_products(beta, gamma, (order, (c1, r1), (c2, r2)))


def run_placed_zero_lookup(dev, seed, rows):
    pr = random.Random(seed)
    sh, usable, T, nl = dev.sh, dev.usable, dev.T, dev.sh.n_lookups
    # lookup 0 holds {1, T - 1}; the others never hold T - 1 (nor 0): beta = -(T - 1) zeroes lookup 0 alone
    cols = [[pr.choice((1, T - 1)) for _ in range(usable)]] + [[pr.randrange(1, T - 1) for _ in range(usable)] for _ in range(nl - 1)]
    dev.set_lookup_inputs(cols)
    a, s, ai, si = dev.permute(blind_seed=seed)
    honest = None
    for l in sorted({0, nl - 1}):
        for r in rows:
            beta, gamma = pr.randrange(R), -si[l][r] % R
            want = dev.check_lookup_products(a, s, ai, si, beta, gamma, ("gamma = -s'[r]", "lookup", l, "row", r))
            if r >= usable:  # a blinding value of lookup l alone: no promised row changes, the call still falls back
                assert all(all(z) for z in want)
        r = pr.randrange(usable)
        want = dev.check_lookup_products(a, s, ai, si, -ai[l][r] % R, pr.randrange(R), ("beta = -a'[r]", "lookup", l, "row", r))
    if nl > 1 and not sh.single:
        beta, gamma = -(T - 1) % R, pr.randrange(R)
        want = dev.check_lookup_products(a, s, ai, si, beta, gamma, "beta = -(T - 1): lookup 0 alone")
        honest = PR.lookup_products(sh, dev.fixed, dev.adv, ai, si, beta, gamma)
        assert not all(want[0]) and all(all(z) for z in want[1:]) and want == honest
    dev.release()


PLACED = [("one", 8, 7), ("multi", 8, 7), ("short", 8, 3), ("multi", 12, 11), ("short", 13, 12), ("one", 13, 12)]


@pytest.mark.parametrize("name,k,lb", PLACED, ids=["%s-k%d-lb%d" % g for g in PLACED])
def test_placed_zero_permutation(engine, name, k, lb):
    dev = Dev(engine, shape_tuple(name, k, lb))
    try:
        if k <= 8:
            run_placed_zero_permutation(dev, 7 * k, zero_rows(dev), chunk_picks(dev))
        else:  # the fallback's scan crosses its blocks: a thinned draw of rows x chunks (every row kind, every chunk kind once)
            rows, chunks = zero_rows(dev), chunk_picks(dev)
            for i, r in enumerate(rows):
                run_placed_zero_permutation(dev, 7 * k + i, [r], [chunks[i % len(chunks)]])
        run_zero_numerators(dev, 13 * k)
    finally:
        dev.close()


@pytest.mark.parametrize("name,k,lb", PLACED, ids=["%s-k%d-lb%d" % g for g in PLACED])
def test_placed_zero_lookup(engine, name, k, lb):
    dev = Dev(engine, shape_tuple(name, k, lb))
    try:
        run_placed_zero_lookup(dev, 3 * k + lb, zero_rows(dev) if k <= 8 else [zero_rows(dev)[i] for i in (1, 2, 3)])
    finally:
        dev.close()


def test_placed_zero_manycols(engine):
    dev = Dev(engine, MANYCOLS)
    try:
        run_placed_zero_permutation(dev, 99, zero_rows(dev), chunk_picks(dev))
        run_zero_numerators(dev, 98)
        run_placed_zero_lookup(dev, 97, zero_rows(dev))
    finally:
        dev.close()


# ---- k = 17, lookup_bits = 16: 64 blocks of the three-way scan and of the grand-product scans ----------------------------------
def test_k17_against_array_reference(engine):
    t = (4, 1, 1, 17, 16)
    sh, fixed, copies, advice = C.synth_case(t)
    n, usable, T = sh.n, sh.usable_rows, 1 << 16
    rs = np.random.default_rng(17)

    def rand_rows(count):
        a = np.frombuffer(rs.bytes(count * 32), dtype=np.uint64).reshape(count, 4).copy()
        a[:, 3] &= 0x0FFFFFFFFFFFFFFF  # below r
        return a

    def small_mont(v):
        c = np.zeros((len(v), 4), dtype=np.uint64)
        c[:, 0] = v
        return cops.to_mont_arr(c)

    fx = [mont(c) for c in fixed]
    sg = [mont(c) for c in prover.build_sigma(sh, copies)]  # the oracle's sigma, never the device's
    av = [mont(c) for c in advice]
    for a in av:
        a[usable:] = rand_rows(n - usable)
    eng = engine
    eng.srs_setup(17)
    pk = eng.keygen(C.params_of(t), np.stack([C.limbs(c) for c in fixed]), copies)
    polys = [eng.poly(n, a) for a in av]
    made = []
    try:
        lcol = sh.n_gate
        for dist in ("nozero", "once_then_top"):
            if dist == "nozero":
                v = rs.integers(1, T, usable, dtype=np.uint64)
            else:
                v = np.concatenate([np.arange(T, dtype=np.uint64), np.full(usable - T, T - 1, dtype=np.uint64)])
                rs.shuffle(v)
            av[lcol][:usable] = small_mont(v)
            eng.upload(polys[lcol], av[lcol])
            wa, ws = PR.permuted_pair_fast(av[lcol], fx[sh.fx_table], usable)
            a, s = eng.lookup_permute(pk, polys)
            made += a + s
            assert np.array_equal(eng.download(a[0])[:usable], wa), dist
            assert np.array_equal(eng.download(s[0])[:usable], ws), dist
        ap = np.concatenate([wa, rand_rows(n - usable)])
        sp = np.concatenate([ws, rand_rows(n - usable)])
        eng.upload_range(a[0], usable, ap[usable:])
        eng.upload_range(s[0], usable, sp[usable:])

        def check(beta, gamma, tag):
            wz = PR.permutation_products_fast(sh, fx, sg, av, beta, gamma)
            wl = PR.lookup_products_fast(sh, fx, av, [ap], [sp], beta, gamma)
            z = eng.permutation_product(pk, polys, m1(beta), m1(gamma))
            zl = eng.lookup_product(pk, polys, a, s, m1(beta), m1(gamma))
            try:
                for ci in range(sh.n_chunks):
                    assert np.array_equal(eng.download(z[ci])[:usable + 1], wz[ci]), (tag, "chunk", ci)
                assert np.array_equal(eng.download(zl[0])[:usable + 1], wl[0]), (tag, "lookup")
            finally:
                for p in z + zl:
                    p.free()
            return wz, wl

        beta, gamma = 0x1234567 * 0x89ABCDEF % R, pow(5, 77, R)
        for forced in (False, True):
            with batch_invert(eng, forced):
                wz, wl = check(beta, gamma, ("honest", forced))
                assert all(z.any(axis=1).all() for z in wz + wl)
        # a zero denominator in the middle chunk, far into the column: the fallback's 64-block scan, then an all-zero chunk
        c, r = 3, 100003
        col = sh.perm_cols[c]
        v = cops.fr_ints((fx if col[0] == "fixed" else av)[col[1]][r:r + 1])[0]
        gamma0 = -(v + beta * cops.fr_ints(sg[c][r:r + 1])[0]) % R
        wz, wl = check(beta, gamma0, "zero denominator, chunk 1")
        ci = c // sh.chunk_len
        assert ci == 1 and wz[ci][r].any() and not wz[ci][r + 1:].any() and not wz[ci + 1].any()
        # zL: gamma = -s'[usable], a blinding row — no promised row changes
        wz, wl = check(beta, -cops.fr_ints(sp[usable:usable + 1])[0] % R, "zero in the blinding of s'")
        assert wl[0].any(axis=1).all()
        wz, wl = check(beta, -cops.fr_ints(sp[70001:70002])[0] % R, "gamma = -s'[70001]")
        assert not wl[0][70002:].any()
    finally:
        for p in polys + made:
            p.free()
        eng.pk_free(pk)


# ---- D. zk_poly_lincomb -------------------------------------------------------------------------------------------------------
PATTERNS = ["all_nonunit", "all_unit", "unit_every_fourth", "single_nonunit", "UNNNNU"]


def unit_mask(pattern, count):
    if pattern == "all_nonunit":
        return [False] * count
    if pattern == "all_unit":
        return [True] * count
    if pattern == "unit_every_fourth":
        return [j % 4 == 3 for j in range(count)]
    if pattern == "single_nonunit":
        return [j != count // 2 for j in range(count)]
    return [(j % 6) in (0, 5) for j in range(count)]


class Pool:
    """`count` resident vectors of length n with known integer contents"""

    def __init__(self, eng, n, count, seed, value=None):
        pr = random.Random(seed)
        self.eng, self.n = eng, n
        self.ints = [[pr.randrange(R) if value is None else value for _ in range(n)] for _ in range(count if value is None else 1)]
        self.polys = [eng.poly(n, mont(v)) for v in self.ints]
        if value is not None:  # one vector, handed in `count` times
            self.ints, self.polys = self.ints * count, self.polys * count
        self.out = eng.poly(n, mont([pr.randrange(R) for _ in range(n)]))  # the old content must not leak in

    def check(self, count, coeffs, sub_low, tag):
        want = PR.lincomb(self.ints[:count], coeffs, sub_low or ())
        self.eng.poly_lincomb(self.out, self.polys[:count], mont(coeffs), mont(sub_low) if sub_low else None)
        assert np.array_equal(self.eng.download(self.out), mont(want)), tag

    def close(self):
        for p in set(self.polys) | {self.out}:
            p.free()


LENGTHS = [1, 7, 8, 9, 255, 256, 257, 4096, 70000]
COUNTS = [1, 3, 4, 5, 39, 40, 41, 80, 81, 121]


@pytest.mark.parametrize("n", LENGTHS)
def test_lincomb_lengths_and_low_coefficients(engine, n):
    """every n_low at every length; of n_low low coefficients only the min(n_low, n) that exist are subtracted (zkmi355.h)"""
    pr = random.Random(n)
    pool = Pool(engine, n, 6, n)
    try:
        for n_low in (0, 1, 2, 8):
            for pattern in ("UNNNNU", "all_nonunit"):
                cs = [1 if u else pr.randrange(2, R) for u in unit_mask(pattern, 6)]
                low = [pr.choice((pr.randrange(R), R - 1)) for _ in range(n_low)]
                pool.check(6, cs, low, (n, n_low, pattern))
        pool.check(1, [1], [R - 1] * 8, (n, "one unit input, sub_low = p - 1"))
    finally:
        pool.close()


@pytest.mark.parametrize("count", COUNTS)
def test_lincomb_counts_and_patterns(engine, count):
    """1 .. 4 launches with `accumulate`, every grouping of unit and non-unit coefficients, random operands"""
    pr = random.Random(count)
    pool = Pool(engine, 257, count, count)
    zeros = Pool(engine, 257, count, count, value=0)
    try:
        for pattern in PATTERNS:
            cs = [1 if u else pr.randrange(2, R) for u in unit_mask(pattern, count)]
            for n_low in (0, 8) if count in (40, 41, 121) else (pr.choice((0, 1, 2, 8)),):
                pool.check(count, cs, [pr.randrange(R) for _ in range(n_low)], (count, pattern, n_low))
            zeros.check(count, cs, [R - 1, 0, 1], (count, pattern, "all-zero inputs"))
    finally:
        pool.close()
        zeros.close()


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", [257, 4096])
def test_lincomb_worst_operands(engine, n, count):
    """every input element p - 1, every non-unit coefficient p - 1, sub_low p - 1: the lazy sums of lincomb_kernel at the bounds its
    comment derives (40 inputs per launch, the old value under `accumulate`, the subtractions) — count 40 and 121 are the point"""
    top = Pool(engine, n, count, 0, value=R - 1)
    try:
        for pattern in PATTERNS:
            cs = [1 if u else R - 1 for u in unit_mask(pattern, count)]
            for low in ([], [R - 1] * 8, [R - 1]):
                top.check(count, cs, low, (n, count, pattern, len(low)))
        if count >= 2:  # p - 1 times p - 1 beside 1 times p - 1 at the launch boundary
            cs = [R - 1] * count
            cs[min(count - 1, 39)] = 1
            top.check(count, cs, [R - 1] * 8, (n, count, "unit at the end of the first launch"))
    finally:
        top.close()


def test_lincomb_refuses_out_among_the_inputs(engine):
    pool = Pool(engine, 16, 3, 1)
    try:
        before = engine.download(pool.out)
        with pytest.raises(zk.ZkError) as e:
            engine.poly_lincomb(pool.out, [pool.polys[0], pool.out], mont([2, 3]))
        assert e.value.code == EINVAL
        with pytest.raises(zk.ZkError) as e:
            engine.poly_lincomb(pool.out, pool.polys[:2], mont([2, 3]), mont([1] * 9))  # n_low <= 8
        assert e.value.code == EINVAL
        assert np.array_equal(engine.download(pool.out), before)
    finally:
        pool.close()


# ---- E. the small ones ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 1, (1 << 32) - 3, 1 << 32, 1 << 63], ids=["0", "1", "2^32-3", "2^32", "2^63"])
def test_random_poly_block_counter(engine, first):
    """300 draws (a block of 256 lanes and a part of one) from `first`: the run from 2^32 - 3 carries into counter word 13"""
    key = bytes(range(100, 132))
    want = PR.chacha_fr(key, first, 300)
    assert all(v < R for v in want) and len(set(want)) == 300
    p = engine.poly(300, mont([5] * 300))
    try:
        engine.random_poly(key, first, p)
        got = engine.download(p)
        assert np.array_equal(got, mont(want))
        assert cops.fr_ints(got) == want  # canonical: the Montgomery image decodes to the value itself, below r
    finally:
        p.free()


def test_upload_range_and_copy_range_at_their_ends(engine):
    n = 64
    pr = random.Random(2)
    base = [pr.randrange(R) for _ in range(n)]
    src_i = [pr.randrange(R) for _ in range(n)]
    p, src = engine.poly(n, mont(base)), engine.poly(n, mont(src_i))
    try:
        cur = list(base)
        for first, count in ((0, 1), (0, 7), (29, 1), (29, 7), (n - 1, 1), (n - 7, 7), (0, n), (0, 0), (31, 0), (n, 0)):
            vals = [pr.randrange(R) for _ in range(count)]
            engine.upload_range(p, first, mont(vals) if count else np.zeros((0, 4), dtype=np.uint64))
            cur[first:first + count] = vals
            assert np.array_equal(engine.download(p), mont(cur)), ("upload_range", first, count)
        for first, count in ((n - 6, 7), (n, 1), (n + 1, 0), (1, n)):
            with pytest.raises(zk.ZkError) as e:
                engine.upload_range(p, first, mont([1] * count) if count else np.zeros((0, 4), dtype=np.uint64))
            assert e.value.code == EINVAL
            assert np.array_equal(engine.download(p), mont(cur)), ("refused upload_range", first, count)
        for dfirst, sfirst, count in ((0, 5, 1), (0, 0, 7), (30, 11, 7), (n - 7, 0, 7), (0, n - 7, 7), (n - 1, n - 1, 1), (0, 0, n),
                                      (9, 9, 0), (n, n, 0)):
            engine.copy_range(p, dfirst, src, sfirst, count)
            cur[dfirst:dfirst + count] = src_i[sfirst:sfirst + count]
            assert np.array_equal(engine.download(p), mont(cur)), ("copy_range", dfirst, sfirst, count)
        for dfirst, sfirst, count in ((n - 6, 0, 7), (0, n - 6, 7), (n + 1, 0, 0), (0, n + 1, 0), (0, 0, n + 1)):
            with pytest.raises(zk.ZkError) as e:
                engine.copy_range(p, dfirst, src, sfirst, count)
            assert e.value.code == EINVAL
            assert np.array_equal(engine.download(p), mont(cur)), ("refused copy_range", dfirst, sfirst, count)
        # within one vector: disjoint ranges copy, overlapping ranges are ZK_EINVAL and change nothing (zkmi355.h)
        engine.copy_range(p, 0, p, 10, 10)
        cur[0:10] = cur[10:20]
        engine.copy_range(p, 40, p, 33, 7)
        cur[40:47] = cur[33:40]
        assert np.array_equal(engine.download(p), mont(cur))
        for dfirst, sfirst, count in ((0, 5, 10), (5, 0, 10), (7, 7, 1), (0, 0, n)):
            with pytest.raises(zk.ZkError) as e:
                engine.copy_range(p, dfirst, p, sfirst, count)
            assert e.value.code == EINVAL
        assert np.array_equal(engine.download(p), mont(cur))
        assert np.array_equal(engine.download(src), mont(src_i))
    finally:
        p.free()
        src.free()


@pytest.mark.parametrize("t", [(3, 2, 2, 8, 6), (1, 1, 1, 8, 7)], ids=["multi-column", "one-column"])
def test_pk_export_poly_in_query_order(engine, t):
    """every fixed column (constants, lookup table, selector columns: the proof's order of fixed evaluations) and every sigma, back
    in Lagrange form, are the oracle's fixed values and build_sigma values.  The multi-column circuit is tests/adversarial_layout.py's:
    its constants and selector columns all differ (the synthesized circuit's constants column equals the head of its table)."""
    case = None
    if t[0] > 1:
        sh, fixed, copies, advice = C.adv_case(t, 4321)
        case = (sh, fixed, copies, advice, prover.build_sigma(sh, copies))
    dev = Dev(engine, t, case)
    eng = engine
    dst = eng.poly(dev.n)
    try:
        sh = dev.sh
        assert sh.fixed_queries == [(f, 0) for f in range(sh.n_fix)]
        for which, cols in ((E.ZK_PK_FIXED_POLY, dev.fixed), (E.ZK_PK_SIGMA_POLY, dev.sigma)):
            assert len({tuple(c) for c in cols}) == len(cols), "distinct columns: an index mix-up shows"
            for i, col in enumerate(cols):
                eng.pk_export_poly(dev.pk, which, i, dst)
                eng.coeff_to_lagrange(dst)
                assert np.array_equal(eng.download(dst), mont(col)), (which, i)
            before = eng.download(dst)
            for bad_which, index in ((which, len(cols)), (which, 1 << 40), (7, 0)):
                with pytest.raises(zk.ZkError) as e:
                    eng.pk_export_poly(dev.pk, bad_which, index, dst)
                assert e.value.code == EINVAL
            assert np.array_equal(eng.download(dst), before)
        short = eng.poly(dev.n // 2)
        with pytest.raises(zk.ZkError) as e:
            eng.pk_export_poly(dev.pk, E.ZK_PK_FIXED_POLY, 0, short)
        assert e.value.code == EINVAL
        short.free()
        vk = eng.vk_read(C.params_of(t), eng.vk_write(dev.pk))
        with pytest.raises(zk.ZkError) as e:
            eng.pk_export_poly(vk, E.ZK_PK_FIXED_POLY, 0, dst)
        assert e.value.code == ESTATE
        with pytest.raises(zk.ZkError) as e:
            eng.permutation_product(vk, dev.polys, m1(1), m1(1))
        assert e.value.code == ESTATE
        eng.pk_free(vk)
    finally:
        dst.free()
        dev.close()
