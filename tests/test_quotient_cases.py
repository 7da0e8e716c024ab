"""The case set of the quotient kernels' device harness (tests/quotient_cases.py), checked without a GPU: its reference against
the oracle's evaluate_h on honest keys, its term-count model against quotient.hip's rule and against what the rest of the suite
reaches, and the set's coverage — counted by the model alone."""
import os
import re

import numpy as np
import pytest

import quotient_cases as Q
from prover_shapes import DRAW_SEED, SHAPES, random_shapes

import webauthn_halo2_amd as zk
from zkoracle import fastprover as fp, field as F, plonk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sets():
    return Q.build_sets()


@pytest.fixture(scope="module")
def cover(sets):
    return Q.coverage(sets)


# ---- the reference ------------------------------------------------------------------------------------------------------------

def _as_vec(name, index, a):
    return Q.Vec(name, index, "rand", data=np.ascontiguousarray(a).view("<u4").reshape(-1, 8).copy())


@pytest.mark.parametrize("shape", [(1, 1, 1, 6, 4, 0), (4, 1, 1, 6, 4, 0), (5, 2, 2, 6, 4, 2)], ids=["single", "gates", "idle"])
def test_reference_equals_the_oracle_on_honest_keys(shape):
    """One key of each kind fastprover.evaluate_h takes (one gate column; several; combined selectors), made by the oracle's keygen
    from a synthesized circuit; the witness-side cosets are random elements (the row expression is evaluated as it stands)."""
    A, L, Fx, k, lb, idle = shape
    p = zk.circuit.CircuitParams(degree=k, num_advice=A, num_lookup_advice=L, num_fixed=Fx, lookup_bits=lb, idle_gate_columns=idle)
    asg = zk.circuit.synthesize(p, 0x5EED0019)
    sh = plonk.Shape(k, A, L, Fx, lb, idle)
    opk = fp.keygen(sh, asg.fixed, asg.copies)
    lay = Q.Layout(A, L, Fx, idle)
    assert (lay.gate_sel, lay.perm_cols, lay.n_chunks, lay.chunk_len, lay.n_lookups, lay.n_fix, lay.n_adv, lay.last_rot) == \
           (sh.gate_sel, sh.perm_cols, sh.n_chunks, sh.chunk_len, sh.n_lookups, sh.n_fix, sh.n_adv, sh.last_rot)
    assert (lay.fx_table, lay.fx_qlookup or 0) == (sh.fx_table, sh.fx_qlookup or 0)
    N = 4 * sh.n
    rng = np.random.default_rng(11)
    rand = lambda: Q._rand_rows(rng, N).view(np.uint64).reshape(N, 4)
    adv_e = [rand() for _ in range(sh.n_adv)]
    z_e = [rand() for _ in range(sh.n_chunks)]
    lk_e = [(rand(), rand(), rand()) for _ in range(sh.n_lookups)]  # (a', s', z)
    ch = [int.from_bytes(rng.bytes(31), "little") for _ in range(3)]
    ds = Q.DataSet("honest", lay, k + 2, "mixed", *ch)
    active = [(1 - a - b) % F.R for a, b in zip(fp.cops.fr_ints(opk.llast_e), fp.cops.fr_ints(opk.lblind_e))]
    by_name = {"adv": adv_e, "fix": opk.fix_e, "sigma": opk.sig_e, "z": z_e, "lk_z": [t[2] for t in lk_e], "lk_a": [t[0] for t in lk_e],
               "lk_s": [t[1] for t in lk_e], "l0": [opk.l0_e], "l_last": [opk.llast_e], "l_active": [fp.cops.fr_mont(active)],
               "xs": [opk.xs], "prev": [rand()]}
    for name, idx in Q.vector_order(lay):
        ds.vecs.append(_as_vec(name, idx, by_name[name][idx]))
    for divide in (1, 0):
        want = fp.evaluate_h(opk, adv_e, z_e, lk_e, *ch, divide=bool(divide))
        got = Q.expected(ds, Q.Launch(0, 0, divide, 0))
        assert np.array_equal(got, want.view("<u4").reshape(N, 8)), divide
    # the derived forms, from the same rows
    prev = fp.cops.fr_ints(by_name["prev"][0])
    plain = fp.cops.fr_ints(Q.expected(ds, Q.Launch(0, 0, 1, 0)).view(np.uint64).reshape(N, 4))
    acc = fp.cops.fr_ints(Q.expected(ds, Q.Launch(1, 0, 1, 0)).view(np.uint64).reshape(N, 4))
    assert acc == [(a + b) % F.R for a, b in zip(prev, plain)]
    c3 = Q.expected(ds, Q.Launch(0, 1, 1, 0))
    n = sh.n
    assert c3.shape == (3 * n, 8)
    for j, r in [(0, 0), (1, 0), (2, 5), (2, n - 1)]:
        assert np.array_equal(c3[j * n + r], Q.expected(ds, Q.Launch(0, 0, 1, 0))[4 * r + j])


def test_periodic_and_explicit_vectors_read_the_same():
    rng = np.random.default_rng(3)
    ds = Q.DataSet("x", Q.Layout(1, 1, 1), 8, "mixed", 1, 2, 3)
    alt = Q.make_vec(rng, "adv", 0, "alt", 256)
    st = ds.stored(alt)
    assert st[0] == 0 and st[1] == F.R - 1 and st[254] == 0 and st[255] == F.R - 1
    one = Q.make_vec(rng, "adv", 0, "one", 256)
    assert set((ds.stored(one) * Q.MONT_INV % F.R).tolist()) == {1}
    sel = Q.make_vec(rng, "fix", 0, "sel01", 256)
    assert set((ds.stored(sel) * Q.MONT_INV % F.R).tolist()) == {0, 1}
    r = Q.make_vec(rng, "adv", 0, "rand", 256)
    assert all(0 <= v < F.R for v in ds.stored(r).tolist()) and len(set(ds.stored(r).tolist())) == 256
    big = [int.from_bytes(row.tobytes(), "little") for row in Q._rand_rows(rng, 4096)]
    assert max(big) < F.R and sum(v > 3 * F.R // 4 for v in big) > 500 and sum(v < F.R // 4 for v in big) > 500  # the whole range


# ---- the model ----------------------------------------------------------------------------------------------------------------

def test_log_slices_rule_at_the_documented_points():
    src = open(os.path.join(ROOT, "webauthn-halo2_amd", "csrc", "quotient.hip")).read()
    # the rule this model restates: about 2^16 lanes in all, at most 16 per row, not more lanes than gates
    assert re.search(r"#define ZK_QUOT_LANES_LOG 16\b", src)
    assert "while (ls < 4 && log_ext + ls < ZK_QUOT_LANES_LOG && (2u << ls) <= n_gate) ls++;" in src
    assert "if (++cnt == 32)" in src and "cnt = 1;" in src
    assert src.count("log_slices == 0 || N < 256 || (N & 255)") == 2
    ls = Q.quotient_log_slices
    # the bench rows (k, gate columns): 14 / 34, 13 / 68, 12 / 139, 11 / 291; the k = 17 and k = 19 proofs; manycols (k = 7, 36 gates)
    assert [ls(16, 34), ls(15, 68), ls(14, 139), ls(13, 291)] == [0, 1, 2, 3]
    assert ls(19, 8) == 0 and ls(21, 1) == 0 and ls(9, 36) == 4 and ls(10, 44) == 4
    assert [ls(8, g) for g in (1, 2, 3, 4, 7, 8, 15, 16, 352)] == [0, 1, 1, 2, 2, 3, 3, 4, 4]
    assert [ls(le, 352) for le in (11, 12, 13, 14, 15, 16, 17)] == [4, 4, 3, 2, 1, 0, 0]
    # the fallback: 192 and 384 rows of three cosets run one lane per row whatever log_slices says; 768 rows do not
    assert [Q.effective_log_slices(le, 3, 1) for le in (8, 9, 10)] == [0, 0, 3]
    assert [Q.effective_log_slices(le, 3, 0) for le in (7, 8, 9, 10)] == [0, 3, 3, 3]
    assert Q.fold_positions(31) == [] and Q.fold_positions(32) == [32] and Q.fold_positions(62) == [32]
    assert Q.fold_positions(63) == [32, 63] and Q.fold_positions(96) == [32, 63, 94]
    # a legal key at its widest (k >= 14: one lane per row): nine folds of the gate sum
    assert Q.folds(302) == 9 and Q.folds(352) == 11


def test_lane_terms_add_up_to_the_whole_row():
    """every term of the row is taken by exactly one lane, whatever the number of lanes"""
    for lay in [Q.Layout(1, 1, 1), Q.Layout(5, 2, 2, idle=2), Q.Layout(36, 12, 2), Q.Layout(264, 49, 1), Q.Layout(2, 1, 1, inst=1)]:
        whole = Q.lane_terms(lay, 1, 0)
        assert whole == {"gates": lay.n_gate, "l0": lay.n_chunks + 2 * lay.n_lookups, "l_last": 1 + lay.n_lookups,
                         "active": lay.n_chunks + 2 * lay.n_lookups}
        assert sum(whole.values()) == lay.n_terms
        for ls in range(1, 5):
            per = [Q.lane_terms(lay, 1 << ls, sl) for sl in range(1 << ls)]
            assert {g: sum(p[g] for p in per) for g in Q.GROUPS} == whole


def test_what_the_rest_of_the_suite_reaches():
    """The shapes of tests/prover_shapes.py and tests/test_gpu_cosets3.py, through the product's own choice of lanes: on the 4n route
    no lane holds more than 4 terms of any sum — 6 in the two draws with two gate columns and three lookups, where two lanes share
    1 + 1 + 2 * 2 terms of l_0 — so the folds of q_acc are reached by none of them."""
    import test_gpu_cosets3 as c3
    shapes = {n: s for n, s in SHAPES.items()}
    shapes.update({"draw%d" % i: s for i, s in enumerate(random_shapes(20, DRAW_SEED))})
    shapes.update({"cosets3_%d" % i: s for i, s in enumerate(c3.SHAPES)})
    worst = {}
    for name, s in shapes.items():
        A, L, Fx, k = s[:4]
        lay = Q.Layout(A, L, Fx, s[5] if len(s) > 5 else 0)
        worst[name] = Q.launch_terms(lay, k + 2, Q.quotient_log_slices(k + 2, A), 0)
        assert max(worst[name].values()) <= (6 if (A, L) == (2, 3) else 4), (name, worst[name])
    assert Q.quotient_log_slices(9, 36) == 4 and worst["manycols"] == {"gates": 3, "l0": 4, "l_last": 2, "active": 4}
    assert Q.quotient_log_slices(10, 44) == 4 and worst["manycols_k8"] == {"gates": 3, "l0": 4, "l_last": 2, "active": 4}
    assert worst["k17like"] == {"gates": 1, "l0": 3, "l_last": 2, "active": 3} and worst["k19like"] == {"gates": 1, "l0": 3, "l_last": 2, "active": 3}
    # on three cosets the small shapes fall back to one lane per row; the largest sum there stays far below a fold as well
    for s in c3.SHAPES:
        lay = Q.Layout(s[0], s[1], s[2], s[5])
        t = Q.launch_terms(lay, s[3] + 2, Q.quotient_log_slices(s[3] + 2, s[0]), 1)
        assert max(t.values()) < 32, (s, t)


def test_fold_shapes_are_what_the_model_says():
    for t in (31, 32, 33):
        lay = Q.choose_fold_layout(t, True)
        assert {g: Q.lane_terms(lay, 1, 0)[g] for g in Q.FOLDING} == {g: t for g in Q.FOLDING}
    for t, nf in ((63, 2), (96, 3)):
        lay = Q.choose_fold_layout(t, False)
        lt = Q.lane_terms(lay, 1, 0)
        assert lt["gates"] == t and all(lt[g] >= t and Q.folds(lt[g]) == nf for g in Q.FOLDING)
    for ls, gates in ((1, 66), (2, 132), (3, 264)):
        lay = Q.choose_slice_fold_layout(ls)
        assert lay.n_gate == gates
    # 16 lanes: no legal layout folds any sum
    widest = max(max(Q.lane_terms(lay, 16, sl).values()) for lay in (Q.Layout(302, 49, 1), Q.Layout(295, 56, 1), Q.Layout(256, 56, 3))
                 for sl in range(16))
    assert widest < 32
    assert -(-Q.MAX_ADV // 16) == 22 and 1 + -(-(Q.MAX_CHUNKS - 1) // 16) + 2 * -(-Q.MAX_LOOKUPS // 16) < 32


# ---- the set ------------------------------------------------------------------------------------------------------------------

def test_case_set_reaches_every_class(sets, cover):
    c = lambda *k: cover.get(k, 0)
    names = [n for n, _, _, _ in Q.shapes()]
    assert names == ["single", "two_gates", "idle", "perm7", "inst_joins", "inst_own", "fold31", "fold32", "fold33", "fold63", "fold96",
                     "widest", "slicefold1", "slicefold2", "slicefold3"]
    for ds in sets:
        assert ds.log_ext in Q.LOG_EXTS
        assert all(v.data is None or v.data.shape == (ds.N, 8) for v in ds.vecs)
        assert [(v.name, v.index) for v in ds.vecs] == Q.vector_order(ds.lay)
        # every form, in every combination, for every data set
        want = {(a, c3, d, ls) for a in (0, 1) for c3 in (0, 1) for d in (0, 1) for ls in range(5) if (1 << ls) <= ds.lay.n_gate}
        assert {(l.acc, l.c3, l.divide, l.log_slices) for l in ds.launches} == want and len(ds.launches) == len(want)
    for n in names:
        assert c("round", n, "allmax") >= 1 and c("round", n, "mixed") >= 1, n   # one round all p - 1, the rest mixed
    for n in names[:6]:
        assert all(c("size", n, le) >= 2 for le in Q.LOG_EXTS), n
    # forms: plain / ACC x 4n / C3 x divide on / off x log_slices 0 .. 4
    for a in (0, 1):
        for c3 in (0, 1):
            for d in (0, 1):
                for ls in range(5):
                    assert c("form", a, c3, d, ls) >= 8, (a, c3, d, ls)
    # all eight instantiations, each on all-(p - 1) operands and on mixed ones
    for kern in ("rows", "sliced"):
        for c3 in (0, 1):
            for a in (0, 1):
                assert c("kernel_round", kern, c3, a, "allmax") >= 10 and c("kernel_round", kern, c3, a, "mixed") >= 10, (kern, c3, a)
    for ls in (1, 2, 3, 4):
        assert c("sliced_lanes", ls, 0) >= 10 and c("sliced_lanes", ls, 1) >= 10, ls
    assert c("c3_fallback", 8) >= 50 and c("c3_fallback", 9) >= 50  # 192 and 384 rows with log_slices > 0
    # shapes
    assert c("single_path", "allmax") == 3 and c("single_path", "mixed") == 9
    for form in (0, 1, 2):
        assert c("selector_form", form, "allmax") >= 3 and c("selector_form", form, "mixed") >= 6, form
    assert c("last_chunk_holds_one") >= 9
    assert c("instance", "joins_chunk") >= 9 and c("instance", "own_chunk") >= 9
    # folds with one lane per row: each of the three sums at exactly 31, 32 and 33 terms, at two folds (>= 63) and three (>= 96)
    for g in Q.FOLDING:
        for a in (0, 1):
            for c3 in (0, 1):
                for t in (31, 32, 33):
                    assert c("lane_terms", g, t, c3, a) >= 6, (g, t, c3, a)
                assert sum(v for k, v in cover.items() if k[0] == "lane_terms" and k[1] == g and 63 <= k[2] < 94 and k[3:] == (c3, a)) >= 6
                assert sum(v for k, v in cover.items() if k[0] == "lane_terms" and k[1] == g and k[2] >= 96 and k[3:] == (c3, a)) >= 6
        for nf in (0, 1, 2, 3, 8):
            assert c("lane_folds", g, nf, "allmax") >= 1 and c("lane_folds", g, nf, "mixed") >= 1, (g, nf)
        # folds inside a slice, at 2, 4 and 8 lanes, on both routes and in both store forms
        for ls in (1, 2, 3):
            for c3 in (0, 1):
                for a in (0, 1):
                    assert c("slice_folds", ls, g, c3, a) >= 2, (ls, g, c3, a)
        assert not any(k[0] == "slice_folds" and k[1] == 4 for k in cover)  # 16 lanes cannot fold
    assert c("lane_folds", "l_last", 1, "allmax") >= 1 and c("lane_folds", "l_last", 1, "mixed") >= 1
    assert c("lane_folds", "gates", 9, "allmax") >= 1 and c("lane_folds", "gates", 9, "mixed") >= 1  # the widest legal key
    # operands: every kind on witness-side and on key-side vectors, on every kind of vector; selectors in {0, 1}; preloads
    for side in ("witness", "key"):
        for kind in Q.KINDS:
            assert c("operand", side, kind) >= 50, (side, kind)
    for name in Q.WITNESS_SIDE + Q.KEY_SIDE:
        for kind in Q.KINDS:
            assert c("operand_of", name, kind) >= 1, (name, kind)
    assert c("operand", "key", "sel01") >= 100
    for kind in Q.PRELOADS:
        assert c("acc_preload", kind) >= 100, kind
    for ds in sets:
        if ds.round_kind == "allmax":
            assert all(v.kind == "max" for v in ds.vecs[:-1]) and (ds.beta, ds.gamma, ds.y) == (F.R - 1,) * 3
            assert [c * Q.MONT % F.R for c in ds.t_inv()] == [F.R - 1] * 4  # the stored t_inv as well
        else:
            assert all(v.kind == "rand" for v in ds.vecs[:-1]) or ds.round_kind == "mixed"
            x0 = F.ZETA
            assert ds.t_inv()[0] * (pow(x0, ds.N >> 2, F.R) - 1) % F.R == 1
            assert all(0 < ch < 1 << 248 for ch in (ds.beta, ds.gamma, ds.y))
