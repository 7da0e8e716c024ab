"""GPU parity for the STANDARD MSM plan (msm_standard.hip.h, msm.hip msm_run_standard) at every window, pass width and column length:
the plan of every SRS below 2^16 and from 2^22, of every zk_msm_bn254 call, and of any size under ZK_OPT_MSM_WINDOW = 9 .. 14.
Every expected value is exact — the tau-oracle of the seed-generated SRS, the C Pippenger for loaded bases — and compared after
affine normalisation.  The grid is data (tests/msm_cases.py; tests/test_msm_cases.py checks which branch each case reaches);
where a test claims a path it asserts what the ABI shows of it: zk_srs_msm_plan, and the pass / column / wide-tail counters of
zk_timer_stats."""
import os
import random
import sys
from contextlib import contextmanager

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_cases as MC  # noqa: E402
from zkoracle import cops, field as F, srs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture()
def planned(engine):
    """select(window bits, pass width) before the SRS is set up; afterwards the defaults and a small SRS for whoever comes next"""
    from webauthn_halo2_amd import engine as E

    def select(bits=0, width=0):
        engine.set_option(E.ZK_OPT_MSM_WINDOW, bits)
        engine.set_option(E.ZK_OPT_MSM_BATCH, width)
        return engine

    yield select
    engine.set_option(E.ZK_OPT_MSM_WINDOW, 0)
    engine.set_option(E.ZK_OPT_MSM_BATCH, 0)
    engine.srs_setup(10)


@contextmanager
def counted(eng, passes, columns, wide=0):
    """the MSM passes and columns the block runs, and how many of the passes took the wide path (ZK_T_MSM_TAIL counts those only)"""
    from webauthn_halo2_amd import engine as E

    which = (E.ZK_T_MSM, E.ZK_T_MSM_COLUMNS, E.ZK_T_MSM_TAIL)
    before = [eng.timer_stats(w)[1] for w in which]
    yield
    after = [eng.timer_stats(w)[1] for w in which]
    assert [a - b for a, b in zip(after, before)] == [passes, columns, wide]


def affine(row):
    return cops.affine_arr_to_ints(np.asarray(row).reshape(1, 8))[0]


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- A: every window ---

@pytest.mark.parametrize("k", MC.A_KS)
@pytest.mark.parametrize("bits", MC.A_BITS)
def test_every_standard_window_matches_tau_oracle(planned, bits, k):
    """ZK_OPT_MSM_WINDOW = 9 .. 14 over a short SRS: bucket sets of 256 .. 8192, bit-sum splits 1, 2, 4 and the capped 4.  The
    single commits run random, zero, sparse, ones, zero, random first — dense bucket parts left under empty and nearly empty
    bucket sets, which the bit sums must not read (msm_used_parts) — then one batched pass, both bases."""
    eng = planned(bits)
    n = 1 << k
    eng.srs_setup(k)
    assert eng.srs_msm_plan() == (bits, 254 // bits + 1)
    cols = dict(MC.columns(bits, k))
    cols["last"] = MC.last_points(n, 7000 + 100 * bits + k)
    want = {name: MC.tau_commit(d) for name, d in cols.items()}
    polys = {name: eng.poly(n, d) for name, d in cols.items()}
    assert want["zero"] is None and sorted(MC.A_SINGLE_ORDER) == sorted(list(cols) + ["zero", "random"])
    with counted(eng, len(MC.A_SINGLE_ORDER), len(MC.A_SINGLE_ORDER)):
        for step, name in enumerate(MC.A_SINGLE_ORDER):
            assert affine(eng.commit(polys[name], 0)) == want[name], (bits, k, step, name)
    names = list(cols)
    plist = [polys[x] for x in names]
    with counted(eng, 1, len(names)):
        got = eng.commit_batch(plist, 0)
    for j, name in enumerate(names):
        assert affine(got[j]) == want[name], (bits, k, "batch", name)
    with counted(eng, 1, len(names)):
        gl = eng.commit_batch(plist, 1)
    for j, p in enumerate(plist):
        assert (gl[j] == eng.commit(p, 1)).all(), (bits, k, "lagrange", names[j])
    # commit_lagrange(v) == commit(iNTT(v)), every column
    for j, p in enumerate(plist):
        eng.lagrange_to_coeff(p)
        assert (eng.commit(p, 0) == gl[j]).all(), (bits, k, "intt", names[j])
        p.free()


# ------------------------------------------------------------------ B: long columns ---

@pytest.mark.parametrize("k,bits", MC.B_CASES)
def test_long_columns_on_the_standard_plan(planned, k, bits):
    """n >= 2^18 under a 9 .. 14-bit window: the two-level counting sort (4 coarse bins at 9 bits, 128 at 14; 15.2 M table indexes
    at (19, 9), the nearest any plan comes to the 24-bit field) and, where windows x 2^k exceeds 2^24 (13 bits at 2^20), the
    one-pass scatter with one launch per column.  Last points, 18-bit values and the zero column, singly and in one pass."""
    width = MC.b_width(k)
    eng = planned(bits, width)
    n = 1 << k
    eng.srs_setup(k)
    assert eng.srs_msm_plan() == (bits, 254 // bits + 1)
    p = MC.plan("fixed", n, bits, width)
    assert p["fused"] and p["pass_max"] >= MC.B_COLUMNS and p["sort2"] == (k < 20 or bits > 13) and p["percol"] == (not p["sort2"])
    data = [MC.last_points(n, 100 * k + bits), MC.small18(n, 100 * k + bits + 1), np.zeros((n, 4), dtype=np.uint64)]
    want = [MC.tau_commit(d) for d in data[:2]] + [None]
    polys = [eng.poly(n, d) for d in data]
    with counted(eng, 3, 3):
        for j, q in enumerate(polys):
            assert affine(eng.commit(q, 0)) == want[j], (k, bits, j)
    with counted(eng, 1, 3):
        got = eng.commit_batch(polys, 0)
    for j in range(3):
        assert affine(got[j]) == want[j], (k, bits, "batch", j)
    # the same pass after a zero-first one: the order of the columns in the pass is not the order of their regions' use
    with counted(eng, 1, 3):
        got = eng.commit_batch(polys[::-1], 0)
    for j in range(3):
        assert affine(got[2 - j]) == want[j], (k, bits, "reversed batch", j)
    for q in polys:
        q.free()
    lengths = MC.B_SRS_LENGTHS.get((k, bits), ())
    if lengths:
        # zk_msm_srs at and around ZK_SORT2_MIN_N with n != stride: the prefixes' tau-oracles in one forward pass
        from webauthn_halo2_amd import engine as E

        a = data[0]
        ints = cops.fr_ints(a[:max(lengths)])
        acc, tp, prefix, marks = 0, 1, {}, set(lengths)
        for i, v in enumerate(ints):
            if i in marks:
                prefix[i] = acc
            acc = (acc + v * tp) % F.R
            tp = tp * srs.TAU % F.R
        prefix[len(ints)] = acc
        for m in lengths:
            assert MC.plan("fixed", n, bits, width, length=m)["sort2"] == (m >= 1 << 18)
            with counted(eng, 1, 1):
                got = cops.jac_to_affine_ints(eng.msm_srs(a[:m], E.ZK_BASIS_MONOMIAL))
            assert got == srs.g1_of_scalar(prefix[m]), (k, bits, m)


# -------------------------------------------------------------------- C: pass widths ---

def small_columns(n, count, seed):
    rng = np.random.default_rng(seed)
    cols = [MC.rand_col(rng, n) for _ in range(count)]
    if count > 2:
        cols[1][:] = 0                # the zero column
        cols[2][:, 1:] = 0            # a hot one: 16-bit values
        cols[2][:, 0] &= 0xFFFF
    return cols


def check_batches(eng, polys, singles, want8, count, width, wide=False):
    passes = ceil_div(count, width)
    with counted(eng, passes, count, passes if wide else 0):
        got = eng.commit_batch(polys[:count], 0)
    assert got.shape == (count, 8) and np.array_equal(got, singles[:count]), (count, width, np.nonzero((got != singles[:count]).any(axis=1))[0][:8])
    for j in range(min(8, count)):
        assert affine(got[j]) == want8[j], (count, width, j)


def test_pass_counts_at_the_default_width_of_256(planned):
    """k = 10, default window, default width (2^20 / 2^10 -> 256, the most a pass takes): 1, 255, 256, 257 and 300 columns — a
    full pass has a 2 KiB kernel argument, blockIdx.y up to 255 and 256 results on the host's stack; 257 starts a second."""
    eng = planned()
    n = 1 << MC.C_K
    eng.srs_setup(MC.C_K)
    assert eng.srs_msm_plan() == (9, 29) and MC.plan("fixed", n)["pass_max"] == 256
    cols = small_columns(n, max(MC.C_COUNTS), 0xC0)
    want8 = [MC.tau_commit(d) for d in cols[:8]]
    polys = [eng.poly(n, d) for d in cols]
    with counted(eng, len(polys), len(polys)):
        singles = np.stack([eng.commit(q, 0) for q in polys])
    assert not singles[1].any() and len({bytes(r) for r in singles}) == len(polys)
    for count in MC.C_COUNTS:
        check_batches(eng, polys, singles, want8, count, 256)
    for q in polys:
        q.free()


@pytest.mark.parametrize("width", MC.C_WIDTHS)
def test_seventy_columns_in_passes_of_1_3_7(planned, width):
    """ZK_OPT_MSM_BATCH = 1, 3, 7 at k = 10: ceil(70 / w) passes, the last one short (70 = 23 x 3 + 1 = 10 x 7), the same
    commitments as one column at a time."""
    eng = planned(0, width)
    n = 1 << MC.C_K
    eng.srs_setup(MC.C_K)
    cols = small_columns(n, MC.C_WIDTH_COLUMNS, 0xC1)
    want8 = [MC.tau_commit(d) for d in cols[:8]]
    polys = [eng.poly(n, d) for d in cols]
    singles = np.stack([eng.commit(q, 0) for q in polys])
    check_batches(eng, polys, singles, want8, MC.C_WIDTH_COLUMNS, width)
    for q in polys:
        q.free()


@pytest.mark.parametrize("k,bits,count,widths", MC.C_WIDE)
def test_pass_widths_on_the_wide_path(planned, k, bits, count, widths):
    """the same bookkeeping where msm_run_wide takes the pass: 11 columns in passes of 1 and 5 (k = 10 with 15 bits, k = 16 by
    default); at k = 10 also 257 columns at the default width — a full wide pass and a one-column one."""
    eng = planned(bits)
    n = 1 << k
    eng.srs_setup(k)
    assert eng.srs_msm_plan()[0] == (bits or 16) and MC.plan("fixed", n, bits)["wide"]
    total = MC.C_WIDE_FULL[2] if (k, bits) == MC.C_WIDE_FULL[:2] else count
    cols = small_columns(n, total, 0xC2 + k)
    want8 = [MC.tau_commit(d) for d in cols[:8]]
    polys = [eng.poly(n, d) for d in cols]
    with counted(eng, total, total, total):
        singles = np.stack([eng.commit(q, 0) for q in polys])
    from webauthn_halo2_amd import engine as E
    for w in widths:
        eng.set_option(E.ZK_OPT_MSM_BATCH, w)
        check_batches(eng, polys, singles, want8, count, w, wide=True)
    eng.set_option(E.ZK_OPT_MSM_BATCH, 0)
    if total > count:
        check_batches(eng, polys, singles, want8, total, 256, wide=True)
    for q in polys:
        q.free()


def test_workspace_regrown_when_the_width_rises_and_kept_when_it_falls(planned):
    """A context of its own, so that its lane holds no workspace yet (the session's is 256 columns wide after any default-width
    commit at k = 10 and would never regrow): width 3 is set BEFORE its first MSM — a 3-column workspace; then 16 — the lane's
    workspace is too narrow, get_msm_ws destroys it and makes a 16-column one, and a full 16-column pass runs in it at once;
    then 2 — the wider one is kept.  Twenty columns each time, single commits under every width as well; the expected
    bytes are the OTHER context's single commits, and eight of them the tau-oracle's."""
    import webauthn_halo2_amd as zk
    from webauthn_halo2_amd import engine as E

    ref = planned()
    n = 1 << MC.C_K
    ref.srs_setup(MC.C_K)
    cols = small_columns(n, MC.C_REGROW_COLUMNS, 0xC3)
    want8 = [MC.tau_commit(d) for d in cols[:8]]
    ref_polys = [ref.poly(n, d) for d in cols]
    singles = np.stack([ref.commit(q, 0) for q in ref_polys])
    for q in ref_polys:
        q.free()
    regrow = [c for c in MC.grid() if c[0] == "C-regrow"]
    assert [c[4] for c in regrow] == list(MC.C_REGROW) and MC.lane_events(regrow) == ["created", "regrown", "kept"]
    eng = zk.Engine(0)
    try:
        eng.set_option(E.ZK_OPT_MSM_BATCH, MC.C_REGROW[0])  # before the context's first MSM
        eng.srs_setup(MC.C_K)
        assert eng.srs_msm_plan() == ref.srs_msm_plan() == (9, 29)
        polys = [eng.poly(n, d) for d in cols]
        for w in MC.C_REGROW:
            eng.set_option(E.ZK_OPT_MSM_BATCH, w)
            check_batches(eng, polys, singles, want8, MC.C_REGROW_COLUMNS, w)
            with counted(eng, len(polys), len(polys)):
                again = np.stack([eng.commit(q, 0) for q in polys])
            assert np.array_equal(again, singles), w
        for q in polys:
            q.free()
    finally:
        eng.close()


# ------------------------------------------------------------------ D: short columns ---

@pytest.mark.parametrize("k,lengths", [(MC.D_K, MC.D_LENGTHS), (MC.D_WIDE[0], (MC.D_WIDE[1],))])
def test_polynomials_shorter_than_the_srs(planned, k, lengths):
    """zk_commit / zk_commit_batch / zk_msm_srs of m < 2^k scalars (ParamsKZG::commit of a short polynomial): the window tables
    are strided by the SRS, the digit planes by the workspace, everything else by m.  Monomial basis against the tau-oracle,
    Lagrange basis against the C Pippenger over the exported points.  k = 12 on the standard plan, k = 16 on the wide path."""
    from webauthn_halo2_amd import engine as E

    eng = planned()
    n = 1 << k
    eng.srs_setup(k)
    wide = MC.plan("fixed", n)["wide"]
    assert wide == (k >= 16)
    gl = eng.srs_export(E.ZK_BASIS_LAGRANGE, 0, n)
    for m in lengths:
        cols = [MC.last_points(m, 0xD0 + m + j) for j in range(MC.D_BATCH)]
        polys = [eng.poly(m, d) for d in cols]
        for basis in (E.ZK_BASIS_MONOMIAL, E.ZK_BASIS_LAGRANGE):
            if basis == E.ZK_BASIS_MONOMIAL:
                want = [MC.tau_commit(d) for d in cols]
            else:
                want = [cops.jac_to_affine_ints(cops.msm(d, gl[:m])) for d in cols]
            with counted(eng, 1, 1, 1 if wide else 0):
                assert affine(eng.commit(polys[0], basis)) == want[0], (k, m, basis)
            with counted(eng, 1, MC.D_BATCH, 1 if wide else 0):
                got = eng.commit_batch(polys, basis)
            for j in range(MC.D_BATCH):
                assert affine(got[j]) == want[j], (k, m, basis, j)
            if not wide:  # (zk_msm_srs on the wide path: test_wide_partial_length_msm_srs)
                assert cops.jac_to_affine_ints(eng.msm_srs(cols[1], basis)) == want[1], (k, m, basis, "msm_srs")
        for q in polys:
            q.free()


# ------------------------------------------------------------------ E: degenerate SRS ---

@pytest.mark.parametrize("with_identity", [False, True])
@pytest.mark.parametrize("bits", MC.E_BITS)
def test_degenerate_srs_at_other_bucket_counts(planned, bits, with_identity):
    """The construction of test_fixed_base_commit_over_degenerate_srs (equal points under equal scalars, a run of 20 equal
    points, a P / -P pair, optionally two identities) at 1024 and 8192 buckets: the unchecked accumulation's redo and the
    checked loop, single and batched, both bases, against the C Pippenger."""
    eng = planned(bits)
    k = MC.E_K
    n = 1 << k
    rng = random.Random(1234 + bits)
    g = cops.fixed_base_g1(cops.fr_powers(srs.TAU, n))
    g[20] = g[21]
    g[22] = g[21]
    g[23] = g[21]
    for i in range(40, 60):
        g[i] = g[40]
    neg = cops.affine_arr_to_ints(g[30:31])[0]
    g[31] = cops.to_mont_arr(cops.ints_to_arr([neg[0], (-neg[1]) % F.P]), 1).reshape(8)
    if with_identity:
        g[10] = 0
        g[700] = 0
    gl = g[::-1].copy()
    eng.srs_load(k, g, gl)
    assert eng.srs_msm_plan() == (bits, 254 // bits + 1)
    s = [rng.randrange(F.R) for _ in range(n)]
    s[20] = s[21] = s[22] = s[23] = 5
    for i in range(40, 60):
        s[i] = 9
    s[30] = s[31] = 7
    sm = cops.fr_mont(s)
    ones = cops.fr_mont([1] * n)
    p, q = eng.poly(n, sm), eng.poly(n, ones)
    for basis, arr_ in ((0, g), (1, gl)):
        want = [cops.jac_to_affine_ints(cops.msm(x, arr_)) for x in (sm, ones)]
        with counted(eng, 2, 2):
            assert affine(eng.commit(p, basis)) == want[0], (bits, with_identity, basis)
            assert affine(eng.commit(q, basis)) == want[1], (bits, with_identity, basis, "ones")
        with counted(eng, 1, 3):
            both = eng.commit_batch([p, q, p], basis)
        assert [affine(r) for r in both] == [want[0], want[1], want[0]], (bits, with_identity, basis, "batch")
    p.free()
    q.free()


# ---------------------------------------------------------------- F: arbitrary bases ---

# the lengths of the grid, grouped by the SRS they are exported from
F_GROUPS = [(16, (1 << 16,)), (17, (1 << 17, (1 << 16) + 1)), (20, ((1 << 20) - 1, 1 << 20)), (21, (1 << 21,))]
assert sorted(n for _, ls in F_GROUPS for n in ls) == sorted(MC.F_LENGTHS)


@pytest.mark.parametrize("k,lengths", F_GROUPS)
def test_arbitrary_bases_at_every_generic_window(planned, k, lengths):
    """zk_msm_bn254 over bases exported from the SRS: 12-bit windows at 2^16, 2^17 and 2^16 + 1 (a 2^17 workspace, n != stride),
    14 at 2^20 - 1 and 2^20, 15 at 2^21 — 16384 buckets, two sweeps of msm_sort_kernel over 8192 LDS counters.  Last points with
    the edge scalars 0, 1, R - 1, 2, 2^128 - 1, 2^253 in front; at 2^21 also halves(15): every digit -2^14, the int16 edge."""
    eng = planned()
    eng.srs_setup(k)
    bases = eng.srs_export(0, 0, 1 << k)
    for n in lengths:
        p = MC.plan("generic", n)
        assert p["c"] == (12 if n <= 1 << 17 else 14 if n <= 1 << 20 else 15) and p["sweeps"] == (2 if n == 1 << 21 else 1)
        a = MC.edge_head(MC.last_points(n, 0xF0 + n % 1000))
        with counted(eng, 1, 1):
            got = cops.jac_to_affine_ints(eng.msm(a, bases[:n]))
        assert got == MC.tau_commit(a), n
        if n == MC.F_HALVES_AT:
            h = MC.halves_scalar(15)
            with counted(eng, 1, 1):
                got = cops.jac_to_affine_ints(eng.msm(cops.fr_mont([h] * n), bases[:n]))
            assert got == MC.constant_tau_commit(h, n), (n, "halves")


# ------------------------------------------------------------- the swept sort, k = 22 ---

def test_k22_fixed_base_swept_sort_runs_one_column_per_pass(planned):
    """From 2^22 the table indexes leave the wide path's 26 bits: 15-bit windows on the swept sort (two sweeps over 8192 LDS
    counters, every window into ONE bucket set), which msm_run runs one column at a time.  ZK_OPT_MSM_BATCH = 3 used to make
    zk_commit_batch hand it a three-column pass (ZK_EHIP); the widest pass of that plan is 1 (msm_plan.h msm_max_pass): three
    passes.  Columns whose tau-oracle is cheap at this size: a constant one (halves(15): every digit -2^14, one bucket), zero,
    and 2^16 random scalars in front with the last points at the end."""
    k = 22
    n = 1 << k
    eng = planned(0, 3)
    eng.srs_setup(k)
    assert eng.srs_msm_plan() == (15, 17)
    p = MC.plan("fixed", n, 0, 3)
    assert not p["wide"] and not p["fused"] and p["sweeps"] == 2 and p["pass_max"] == 1
    h = MC.halves_scalar(15)
    head = MC.last_points(1 << 16, 0x22)
    ends = np.zeros((n, 4), dtype=np.uint64)
    ends[:1 << 16] = head
    ends[n - MC.LAST_POINTS:] = head[-1]
    last = cops.fr_ints(head[-1:])[0]
    want_ends = (srs.commit_scalar_monomial(cops.fr_ints(head)) + last * sum(pow(srs.TAU, i, F.R) for i in range(n - MC.LAST_POINTS, n))) % F.R
    data = [np.tile(cops.fr_mont([h]), (n, 1)), np.zeros((n, 4), dtype=np.uint64), ends]
    want = [MC.constant_tau_commit(h, n), None, srs.g1_of_scalar(want_ends)]
    polys = [eng.poly(n, d) for d in data]
    with counted(eng, 3, 3):
        got = eng.commit_batch(polys, 0)
    for j in range(3):
        assert affine(got[j]) == want[j], j
    with counted(eng, 1, 1):
        assert affine(eng.commit(polys[2], 0)) == want[2]
    for q in polys:
        q.free()
