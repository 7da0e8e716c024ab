"""The case set and the model of tests/test_gpu_msm_wide_device.py, without a GPU: the designed columns meet the conditions they
are designed for (asserted from the model alone), the six entry layouts are the documented ones, the model's own pipeline
(simulate: entries in a seeded arbitrary order inside their buckets) passes every stage check under two orders and ends at the
oracle's MSM — and every stage check FAILS on a simulated dump with one thing altered, one alteration per rule."""
import copy
import functools

import numpy as np
import pytest

from zkoracle import cops

import msm_wide_cases as C
import msm_wide_model as W

GEO_IDS = ["c%d-2^%d" % (c, S.bit_length() - 1) for c, S in C.GEOMETRIES]
geos = pytest.mark.parametrize("c,S", C.GEOMETRIES, ids=GEO_IDS)


def sim_passes(c, S):
    """the passes the simulation runs: every designed column and the random ones up to 64 scalars (a simulated point costs an
    oracle scalar multiplication; the long random and witness-like columns add entries, not rules)"""
    designed = {"one bucket", "halves", "ladder", "seam", "edges", "zero", "empty"}
    return {pi for pi, p in enumerate(C.passes(c, S)) if p.n <= 64 or set(p.kinds) <= designed}


@functools.lru_cache(maxsize=None)
def simulated(c, S, seed):
    return C.simulate(c, S, seed, only=sim_passes(c, S))


def columns(c, S, kind):
    """(pass index, column index, pass, Column) of every column of a kind"""
    g = W.Geo(c, S)
    return [(pi, q, p, W.Column(g, C.bases()[p.basis], p.cols[q])) for pi, p in enumerate(C.passes(c, S)) for q, k in enumerate(p.kinds) if k == kind]


@geos
def test_layouts_are_the_six_documented_ones(c, S):
    g = W.Geo(c, S)
    assert (g.ib, g.fb, g.bins, g.esc) == C.LAYOUTS[(c, S)]
    assert g.keys * g.bins == g.nb and g.esc == g.keys // 2 - 1 and g.nwin * S <= 1 << g.ib
    assert len(set(C.LAYOUTS.values())) == 6 and sorted(C.LAYOUTS) == sorted(C.GEOMETRIES)


@geos
def test_class_counts(c, S):
    ps = C.passes(c, S)
    kinds = [k for p in ps for k in p.kinds]
    for k in ("random", "zero", "empty", "one bucket", "halves", "ladder", "seam", "edges", "mix", "bool", "top", "sparse", "equal points",
              "opposite points", "identity sum"):
        assert k in kinds, k
    lengths = {p.n for p in ps for k in p.kinds if k == "random"}
    assert set(C.RANDOM_LENGTHS) | {1100} <= lengths and ((4096 in lengths) == (S == 4096))
    for k in ("mix", "bool", "top", "sparse"):
        assert [p.n for _, _, p, _ in columns(c, S, k)] == [1100]
    widths = "".join("e" if p.n == 0 else str(len(p.cols)) for p in ps)
    assert "313" in widths and "12113" in widths and "2e2" in widths
    assert any(a.n >= 1100 and b.n == 17 for a, b in zip(ps, ps[1:]))
    assert all(len(p.cols) <= C.MAX_BATCH and p.n <= len(C.bases()[p.basis]) and p.n <= S for p in ps)
    # every kind of the degenerate basis runs unchecked and checked; the basis with identity points runs checked only
    assert {p.may for p in ps if p.basis == 1 and "equal points" in p.kinds} == {False, True}
    assert 0 not in C.bases()[1] and 0 in C.bases()[2] and all(p.may for p in ps if p.basis == 2)
    assert {p.ident for p in ps if p.basis == 1} == {0, 1, 2} and 2 in {p.ident for p in ps if p.basis == 2}
    assert any(0 in C.bases()[2][:p.n] for p in ps if p.basis == 2)
    assert {p.t1 for p in ps if "seam" in p.kinds} == {0, 1}


@geos
def test_one_bucket_and_halves_columns(c, S):
    g = W.Geo(c, S)
    cols = columns(c, S, "one bucket")
    assert all(m.buckets == [0] for _, _, _, m in cols)
    counts = sorted(m.count for _, _, _, m in cols)
    n1 = C.one_bucket_n(c)
    assert abs(n1 * g.nwin - W.SUB) <= g.nwin // 2 and (c != 16 or n1 * g.nwin == W.SUB)
    assert counts[:2] == [n1 * g.nwin, (n1 + 1) * g.nwin] and counts[0] <= W.SUB + g.nwin // 2 < counts[1]
    big = [m for _, _, p, m in cols if p.n == 640]
    assert len(big) == 2 and all(m.slots_of(0) > 512 and len(W.heads_of(0, -(-m.slots_of(0) // 8))) >= 2 for m in big)
    for _, _, _, m in columns(c, S, "halves"):
        assert g.nb - 1 in m.buckets and all(e & W.SIGN for e in m.ents[g.nb - 1])


@geos
def test_gap_ladder(c, S):
    g = W.Geo(c, S)
    cols = columns(c, S, "ladder")
    assert len(cols) >= 3
    pi, q, p, m = [x for x in cols if x[2].basis == 0 and len(x[2].cols) == 1][0]
    assert 20 <= sum(1 for s in p.cols[q] if s) <= 60 and all(1 <= sum(1 for d in W.digits(s, c) if d) <= 4 for s in p.cols[q] if s)
    gaps, firsts, prev = set(), set(), None
    for b in m.buckets:
        if prev is not None and prev >> g.fb == b >> g.fb:
            gaps.add(b - prev - 1)
        else:
            firsts.add(b >> g.fb)
        prev = b
    assert {g.esc - 1, g.esc, g.esc + 1, 0} <= gaps and {0, g.bins // 2, g.bins - 1} <= firsts
    assert set(m.dist(g).values()) >= {0, g.esc - 1, g.esc}
    local = {}
    for b in m.buckets:
        local.setdefault(b >> g.fb, []).append(b & (g.keys - 1))
    assert [g.keys - 1] in local.values()
    if g.keys == 128:
        assert any(l == [62, 63, 64, 65] for l in local.values())
    _, err, stats, _, first_flag = W.walk(g, C.bases()[0], simulated(c, S, 1).passes[pi].cols[q])
    assert not err and first_flag >= 1
    assert any(nd + ne >= 5 and nd >= 1 and ne >= 1 for nd, ne in stats)


@geos
def test_seam_and_edges(c, S):
    g = W.Geo(c, S)
    for _, _, _, m in columns(c, S, "seam"):
        assert m.buckets == list(C.SEAM_BUCKETS) and tuple(m.slots_of(b) for b in m.buckets) == C.SEAM_SLOTS == (W.LMAX - 1, W.LMAX, W.LMAX + 1, W.LMAX + 2)
    for _, q, p, m in columns(c, S, "edges"):
        want = {0, 255, 256, 257, g.nb - 256, g.nb - 1} | {256 * h + 255 for h in range(g.rows)}
        assert set(m.buckets) == want and all(m.totals[b] == 1 for b in want - {0})
        idx = [e & ((1 << g.ib) - 1) for b in m.buckets for e in m.ents[b]]
        assert len({i % S for i in idx}) == len(idx) - 1  # a base of its own each; the carry of bucket nb - 1 shares one
        assert len({C.bases()[0][i % S] for i in idx}) == len(idx) - 1


@geos
def test_degenerate_columns(c, S):
    g, a = W.Geo(c, S), C.bases()[1]
    assert a[0] == a[1] and (a[2] + a[3]) % W.R == 0
    for kind, i in (("equal points", 0), ("opposite points", 2)):
        for pi, q, p, m in columns(c, S, kind):
            b = [b for b in m.buckets if sorted(e & ((1 << g.ib) - 1) for e in m.ents[b]) == [2 * S + i, 2 * S + i + 1]]
            assert len(b) == 1 and m.bstart[b[0]] % W.WL != W.WL - 1  # the pair is alone in its bucket and in one lane
            assert (m.bk[b[0]] == 0) == (kind == "opposite points")
            for seed in (1, 2):
                _, err, _, exc, _ = W.walk(g, a, simulated(c, S, seed).passes[pi].cols[q])
                assert not err and exc, "no lane meets the pair"
                assert bool(simulated(c, S, seed).passes[pi].redone) == (not p.may)
    for _, q, p, m in columns(c, S, "identity sum"):
        assert m.msm == 0 and m.count > 0 and any(m.bk[b] for b in m.buckets)


@geos
@pytest.mark.parametrize("seed", [1, 2])
def test_simulation_passes_every_stage_check_and_ends_at_the_oracle(c, S, seed):
    g, d, ps = W.Geo(c, S), simulated(c, S, seed), C.passes(c, S)
    assert sorted(d.passes) == sorted(sim_passes(c, S))
    pts, msm_k, msm_want, msm_got = W.Points(), [], [], []
    par = 0
    for pi in sorted(d.passes):
        p = ps[pi]
        a = C.bases()[p.basis]
        par ^= 1 if p.n else 0
        verdict = W.check_pass(g, a, p, d.passes[pi], pts, "pass %d: " % pi, par)
        assert not any(verdict.values()), (pi, p.kinds, {k: v[:3] for k, v in verdict.items() if v})
        if p.n:
            bp = np.ascontiguousarray(C.basis_points(p.basis)[:p.n])
            msm_want += [cops.jac_to_affine_ints(cops.msm(cops.fr_mont(col), bp)) for col in p.cols]
            msm_k += [W.Column(g, a, col).msm for col in p.cols]
            msm_got += [W.affine_of("jac", d.passes[pi].cols[q].result) for q in range(len(p.cols))]
    assert pts.failures() == []
    assert msm_want == W.points_of(msm_k) == msm_got
    if seed == 2:  # the two orders differ inside the buckets and nowhere else
        other = simulated(c, S, 1)
        pi = [pi for pi in sorted(d.passes) if "one bucket" in ps[pi].kinds][0]
        e1, e2 = other.passes[pi].cols[0].entries, d.passes[pi].cols[0].entries
        assert not np.array_equal(e1, e2) and np.array_equal(other.passes[pi].cols[0].bstart, d.passes[pi].cols[0].bstart)


# ---- every rule bites: one alteration each, on the designed pass (ladder, seam, edges) of the first geometry ----
def _first_of(g, d, nth):
    """position of the first entry of the nth non-empty bucket"""
    return int(np.nonzero(d.entries & W.FLAG)[0][nth])


def _alter_distance(g, pd):
    pd.cols[0].entries[_first_of(g, pd.cols[0], 3)] ^= 1 << g.ib


def _alter_missing_flag(g, pd):
    pd.cols[0].entries[_first_of(g, pd.cols[0], 4)] &= ~np.uint32(W.FLAG)


def _alter_second_flag(g, pd):
    pd.cols[0].entries[_first_of(g, pd.cols[0], 4) + 1] |= W.FLAG


def _alter_lane_b(g, pd):
    pd.cols[1].lane_b[2] += 1


def _alter_wrong_bucket(g, pd):
    e, m = pd.cols[0].entries, np.uint32((1 << g.ib) - 1)
    i, j = _first_of(g, pd.cols[0], 2), _first_of(g, pd.cols[0], 5)
    e[i], e[j] = (e[i] & ~m) | (e[j] & m), (e[j] & ~m) | (e[i] & m)


def _alter_slot(g, pd):
    s = sorted(pd.cols[2].slots)
    pd.cols[2].slots[s[1]] = pd.cols[2].slots[s[2]]


def _alter_missing_head(g, pd):
    del pd.cols[1].parts[sorted(pd.cols[1].parts)[1]]


def _alter_row_sum(g, pd):
    pd.cols[2].rc[g.rows - 1] = pd.cols[2].rc[0]


def _alter_column_sum(g, pd):
    pd.cols[2].rc[g.rows + 255] = pd.cols[2].rc[g.rows]


def _alter_bit_sum(g, pd):
    pd.cols[2].sums[12] = pd.cols[2].sums[3]


def _alter_counter(g, pd):
    pd.other = [(1, 7, 2)]


ALTERATIONS = (
    ("a distance field", _alter_distance, "head"), ("a missing flag", _alter_missing_flag, "head"), ("a second flag", _alter_second_flag, "head"),
    ("lane_b", _alter_lane_b, "head"), ("an entry in the wrong bucket", _alter_wrong_bucket, "head"), ("a slot", _alter_slot, "accumulation"),
    ("a missing head", _alter_missing_head, "t1"), ("a row sum", _alter_row_sum, "t2"), ("a column sum", _alter_column_sum, "t2"),
    ("one of the twenty sums", _alter_bit_sum, "t3"), ("a counter of the other set", _alter_counter, "counters"))


@pytest.mark.parametrize("name,alter,stage", ALTERATIONS, ids=[a[0].replace(" ", "-") for a in ALTERATIONS])
def test_every_stage_check_fails_on_one_alteration(name, alter, stage):
    c, S = C.GEOMETRIES[0]
    g, ps = W.Geo(c, S), C.passes(c, S)
    pi = [pi for pi, p in enumerate(ps) if p.kinds == ("ladder", "seam", "edges")][0]
    pd = copy.deepcopy(simulated(c, S, 1).passes[pi])
    assert not any(W.check_pass(g, C.bases()[0], ps[pi], pd).values())
    alter(g, pd)
    verdict = W.check_pass(g, C.bases()[0], ps[pi], pd)
    assert verdict[stage], "%s goes unnoticed" % name
    assert [s for s, e in verdict.items() if e] == [stage], verdict
