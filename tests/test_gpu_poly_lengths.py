"""zk_eval, zk_eval_batch and zk_kate_division at every length and point class of tests/poly_cases.py, bit for bit on the Montgomery
words against the references there (plain Python up to 2^13 coefficients, the C oracle above; tests/test_poly_cases.py ties the two
and the restated shapes of csrc/poly_plan.h together without a GPU).  No tolerance, no case skipped.

  eval        up to 8193: every length x every point x {random, max, sparse}; the four lengths from 2^20 up: {random, sparse} x
              {0, 1, a root of the stride, one random point}; the zero vector once per length; sparse also against sum x^i by pow
  eval_batch  every length: the reference AND zk_eval pair by pair, several vectors and every point class in one call; at 4097 the
              table of 16 distinct points filled, overflowed and hit (counts 1 .. 130), 64 pairs on one point, 64 points all
              different; the out buffer holds a pattern before and none of it after, and nothing behind its end is written
  division    every length of lengths_kd(), out of place and in place, every coefficient, q[n - 1] = 0, p untouched by the out of
              place form, and p(x) = q(x) (x - z) + p(z) through the device's own zk_eval
  order       long, short and batch calls in one context against fresh contexts (the scratch is shared and never cleared)
  opening     one KZG opening of 1000 coefficients at k = 10 against the oracle's tau
  audit       one length per class under ZK_OPT_STREAM_AUDIT = 1
  refusals    lengths that differ, n > 2^26: the code, and nothing written

Found by this test: nothing - every value of the matrix equals its reference.  That it can find something: each of four one-line
value-only changes to a scratch build, run once, failed it - z raised to M - 1 in launch_eval_batch (the batch up to 8193 at 4097, the first
length with two workgroups; the table function at its first pair; every length from 2^20 up), zpw[7] for zpw[8] in
poly_sum_batch_kernel (the four lengths from 2^20 up: more than 256 partial results), the copy for an equal point without zpw (the
batch up to 8193 at 4097; the table function at count 18, pair 17 - the first hit; every length from 2^20 up), zpow[0] for
zpow[last - t] in kd_apply_kernel (every division from 2049 coefficients on) - and the audit function with each of them.

Wall time of the module on an MI355X: 7 s for its 28 cases (the slowest, the divisions at 2^22 + 1, 1.0 s); the random rows of
the long vectors are made once per module."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poly_cases as PC  # noqa: E402
import webauthn_halo2_amd as zk  # noqa: E402
from webauthn_halo2_amd import engine as E  # noqa: E402
from zkoracle import cops, curve as C, srs  # noqa: E402
from zkoracle.field import R  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = -1
PATTERN = 0xA5A5A5A5A5A5A5A5
U64P = ctypes.POINTER(ctypes.c_uint64)
KINDS3 = ("random", "max", "sparse")


@pytest.fixture(scope="module")
def base():
    """2^22 + 1 rows of random stored words, made once: the random vector of length n is its first n rows"""
    a = PC.random_rows(np.random.default_rng(0x901F), (1 << 22) + 1)
    a.setflags(write=False)
    yield a
    del a


def to_int(row):
    return cops.fr_ints(np.ascontiguousarray(row).reshape(1, 4))[0]


def eval_batch_raw(eng, polys, xs_mont):
    """zk_eval_batch into a buffer that holds PATTERN, with one row more than the call may write -> (code, rows, the row behind)"""
    count = len(polys)
    out = np.full((count + 1, 4), PATTERN, dtype=np.uint64)
    xs = np.ascontiguousarray(xs_mont, dtype=np.uint64).reshape(count, 4)
    rc = eng.L.zk_eval_batch(eng.ctx, (ctypes.c_uint64 * count)(*[p.h for p in polys]), xs.ctypes.data_as(U64P), count,
                             out.ctypes.data_as(U64P))
    return rc, out[:count], out[count]


def check_batch(eng, polys, vecs, pairs, what):
    """One zk_eval_batch over `pairs` = [(vector index, point)]: every row is the reference and zk_eval of its pair, the pattern is
    gone from every row and the row behind the end still holds it.  The references are computed once per distinct pair."""
    xs = PC.mont_points([x for _, x in pairs])
    rc, got, behind = eval_batch_raw(eng, [polys[i] for i, _ in pairs], xs)
    assert rc == 0, (what, rc)
    assert (behind == PATTERN).all(), (what, "written behind the end")
    assert not (got == PATTERN).all(axis=1).any(), (what, "a row keeps the pattern")
    want, single = {}, {}
    for j, (i, x) in enumerate(pairs):
        if (i, x) not in want:
            want[(i, x)] = PC.mont1(PC.eval_ref(vecs[i], x))
            single[(i, x)] = eng.eval(polys[i], xs[j])
        assert np.array_equal(got[j], want[(i, x)]), (what, "pair", j, "vector", i, "against the reference")
        assert np.array_equal(got[j], single[(i, x)]), (what, "pair", j, "vector", i, "against zk_eval")
    return got


# ---------------------------------------------------------------------------------------------------------------- eval ---
def test_eval_every_point_up_to_8193(engine, base):
    for n in PC.EVAL_SMALL:
        for kind in KINDS3:
            a = PC.coefficients(n, kind, base=base)
            p = engine.poly(n, a)
            for name, x in PC.points(n):
                want = PC.eval_ref(a, x)
                got = to_int(engine.eval(p, PC.mont1(x)))
                print("eval", n, kind, name, "ok" if got == want else "WRONG")
                assert got == want, (n, kind, name)
                if kind == "sparse":
                    assert got == PC.sparse_value(n, x), (n, name, "closed form")
            p.free()
        z = engine.poly(n, PC.coefficients(n, "zero"))
        assert not engine.eval(z, PC.mont1(PC.points(n)[-1][1])).any(), (n, "zero vector")
        z.free()


@pytest.mark.parametrize("n", PC.EVAL_LARGE)
def test_eval_and_eval_batch_from_2_20_up(engine, base, n):
    """{random, sparse} x {0, 1, a root of the stride, one random point} through zk_eval, and six pairs over the two vectors and the
    four points in one zk_eval_batch (at 2^22 + 1: M = 17, workgroups 964 .. 1023 hold no coefficient)."""
    vecs = [PC.coefficients(n, "random", base=base), PC.coefficients(n, "sparse")]
    polys = [engine.poly(n, a) for a in vecs]
    pts = PC.points_few_eval(n)
    for i, a in enumerate(vecs):
        for name, x in pts:
            want = PC.eval_ref(a, x)
            got = to_int(engine.eval(polys[i], PC.mont1(x)))
            print("eval", n, ("random", "sparse")[i], name, "ok" if got == want else "WRONG")
            assert got == want, (n, i, name)
            if i == 1:
                assert got == PC.sparse_value(n, x), (n, name, "closed form")
    p = dict(pts)
    pairs = [(0, p["zero"]), (1, p["one"]), (0, p["w_stride"]), (1, p["w_stride"]), (0, p["random0"]), (1, p["random0"])]
    check_batch(engine, polys, vecs, pairs, ("eval_batch", n))
    engine.upload(polys[1], PC.coefficients(n, "zero"))
    assert not engine.eval(polys[1], PC.mont1(p["random0"])).any(), (n, "zero vector")
    for q in polys:
        q.free()


# ---------------------------------------------------------------------------------------------------------- eval_batch ---
def test_eval_batch_every_point_up_to_8193(engine, base):
    """One call per length: three vectors (random, max, sparse) x the eleven points, neighbours on different vectors."""
    for n in PC.EVAL_SMALL:
        vecs = [PC.coefficients(n, kind, base=base) for kind in KINDS3]
        polys = [engine.poly(n, a) for a in vecs]
        pairs = PC.mixed_pairs(3, [x for _, x in PC.points(n)])
        assert len(pairs) == 33
        check_batch(engine, polys, vecs, pairs, ("eval_batch", n))
        for q in polys:
            q.free()


def test_eval_batch_point_table_filled_overflowed_and_hit(engine, base):
    """n = 4097 (two workgroups, M = 9): 20 distinct points, each used twice, the second uses behind the sixteenth distinct point
    (tests/test_poly_cases.py restates which pairs fill, overflow and hit the table of a launch); then 64 pairs on ONE point (63
    copies) and 64 points that all differ (48 computed behind the full table)."""
    n = 4097
    vecs = [PC.coefficients(n, kind, base=base) for kind in KINDS3]
    polys = [engine.poly(n, a) for a in vecs]
    pts = PC.table_points(0)
    for count in PC.TABLE_COUNTS:
        check_batch(engine, polys, vecs, PC.table_pairs(count, 3, pts), ("table", count))
    rng = random.Random(0x0E)
    x1 = rng.randrange(2, R - 1)
    check_batch(engine, polys, vecs, [(i % 3, x1) for i in range(64)], "one point")
    check_batch(engine, polys, vecs, [(i % 3, rng.randrange(2, R - 1)) for i in range(64)], "64 points")
    for q in polys:
        q.free()


# ------------------------------------------------------------------------------------------------------------ division ---
def check_division(eng, n, a, zs, what):
    """q = (p - p(z)) / (X - z) for every z of zs: out of place and in place against the reference, every coefficient; p untouched
    by the out of place form; the identity at one random x through zk_eval."""
    rng = random.Random(n)
    p, q, w = eng.poly(n, a), eng.poly(n), eng.poly(n)
    for name, z in zs:
        zm = PC.mont1(z)
        want = PC.kd_ref(a, z)
        eng.upload_range(q, n - 1, np.full((1, 4), 7, dtype=np.uint64))  # (q[n - 1] = 0 is written, not left over)
        eng.kate_division(p, zm, q)
        got = eng.download(q)
        ok = np.array_equal(got, want)
        print("division", n, what, name, "ok" if ok else "WRONG: first row %d" % int(np.argmax((got != want).any(axis=1))))
        assert ok, (n, what, name, "out of place")
        assert not got[n - 1].any()
        eng.copy(w, p)
        eng.kate_division(w, zm)
        assert np.array_equal(eng.download(w), want), (n, what, name, "in place")
        x = rng.randrange(R)
        xm = PC.mont1(x)
        px, qx, pz = (to_int(v) for v in (eng.eval(p, xm), eng.eval(q, xm), eng.eval(p, zm)))
        assert px == (qx * (x - z) + pz) % R, (n, what, name, "identity")
    assert np.array_equal(eng.download(p), a), (n, what, "p was written")
    for h in (p, q, w):
        h.free()


@pytest.mark.parametrize("n", PC.KD_ALL_Z)
def test_kate_division_every_point_up_to_2_19(engine, base, n):
    check_division(engine, n, PC.coefficients(n, "random", base=base), PC.points(n), "random")
    for kind in ("max", "sparse"):
        check_division(engine, n, PC.coefficients(n, kind), PC.points_few_kd(n), kind)


@pytest.mark.parametrize("n", PC.KD_FEW_Z)
def test_kate_division_long(engine, base, n):
    """2^21 - 7 and 2^21 (1024 blocks of 8-coefficient chunks), 2^21 + 1 and + 8 (the first 16-coefficient chunks), 2^22 + 1 (32)."""
    check_division(engine, n, PC.coefficients(n, "random", base=base), PC.points_few_kd(n), "random")
    check_division(engine, n, PC.coefficients(n, "sparse"), PC.points_few_kd(n)[3:], "sparse")


# --------------------------------------------------------------------------------------------------- order independence ---
def test_results_do_not_depend_on_what_ran_before(base):
    """One context: a division at 2^21 + 1, at 9, at 2049, an eval_batch at 4097, a division at 2^21 - the scratch (suf | agg | tpow |
    zpow, the batch's items and partial results) is laid out per call over the same memory and never cleared.  Each result equals
    what a fresh context gives."""
    rng = random.Random(0x0D)
    pts = PC.table_points(1)
    pairs = PC.table_pairs(65, 2, pts)
    steps = [("kd", (1 << 21) + 1, rng.randrange(R)), ("kd", 9, rng.randrange(R)), ("kd", 2049, rng.randrange(R)), ("batch", 4097, 0),
             ("kd", 1 << 21, rng.randrange(R))]

    def run(eng, step):
        kind, n, z = step
        a = PC.coefficients(n, "random", base=base)
        if kind == "kd":
            p = eng.poly(n, a)
            eng.kate_division(p, PC.mont1(z))
            out = eng.download(p)
            p.free()
            return out
        polys = [eng.poly(n, a), eng.poly(n, PC.coefficients(n, "sparse"))]
        rc, out, _ = eval_batch_raw(eng, [polys[i] for i, _ in pairs], PC.mont_points([x for _, x in pairs]))
        assert rc == 0
        for h in polys:
            h.free()
        return out.copy()

    eng = zk.Engine(0)
    together = [run(eng, s) for s in steps]
    eng.close()
    for s, got in zip(steps, together):
        fresh = zk.Engine(0)
        alone = run(fresh, s)
        fresh.close()
        assert np.array_equal(got, alone), s[:2]
    # (and the short division against its reference, so that "equal" is not "equally wrong")
    assert np.array_equal(together[1], PC.kd_ref(PC.coefficients(9, "random", base=base), steps[1][2]))


# ------------------------------------------------------------------------------------------------------- a KZG opening ---
def test_kzg_opening_at_an_odd_length(base):
    """commit(p) - [p(z)] G = [tau - z] commit(q) for p of 1000 coefficients over the SRS of k = 10 from the seed, with the oracle's
    tau (the one of tests/msm_cases.tau_commit)."""
    eng = zk.Engine(0)
    eng.srs_setup(10)
    n = 1000
    a = PC.coefficients(n, "random", base=base)
    z = random.Random(0x0C).randrange(R)
    p, q = eng.poly(n, a), eng.poly(n)
    eng.kate_division(p, PC.mont1(z), q)
    cp = cops.affine_arr_to_ints(eng.commit(p, 0))[0]
    cq = cops.affine_arr_to_ints(eng.commit(q, 0))[0]
    pz = to_int(eng.eval(p, PC.mont1(z)))
    assert pz == PC.eval_ref(a, z)
    assert cp == srs.g1_of_scalar(srs.commit_scalar_monomial(cops.fr_ints(a)))
    lhs = C.add(cp, C.neg(C.mul(C.G1_GEN, pz)))
    assert lhs == C.mul(cq, (srs.TAU - z) % R)
    eng.close()


# ----------------------------------------------------------------------------------------------------------- the audit ---
def test_one_length_per_class_under_the_stream_audit(base):
    eng = zk.Engine(0)
    eng.set_option(E.ZK_OPT_STREAM_AUDIT, 1)
    rng = random.Random(0x0A)
    for n in PC.AUDIT_EVAL:
        a = PC.coefficients(n, "random", base=base)
        p = eng.poly(n, a)
        x = rng.randrange(R)
        want = PC.mont1(PC.eval_ref(a, x))
        assert np.array_equal(eng.eval(p, PC.mont1(x)), want), n
        got = eng.eval_batch([p, p, p], PC.mont_points([x, 1, x]))
        assert np.array_equal(got[0], want) and np.array_equal(got[2], want), n
        p.free()
    for n in PC.AUDIT_KD:
        a = PC.coefficients(n, "random", base=base)
        p = eng.poly(n, a)
        z = rng.randrange(R)
        eng.kate_division(p, PC.mont1(z))
        assert np.array_equal(eng.download(p), PC.kd_ref(a, z)), n
        p.free()
    checks, violations, first = eng.audit_report()
    print("audit: %d checks, %d violations" % (checks, violations))
    assert violations == 0, first
    eng.close()


# ------------------------------------------------------------------------------------------------------------ refusals ---
def test_refusals_write_nothing(base):
    eng = zk.Engine(0)
    n = 4097
    a = PC.coefficients(n, "random", base=base)
    p, other = eng.poly(n, a), eng.poly(n + 1, base[:n + 1])
    xs = PC.mont_points([3, 5])
    # zk_eval_batch: lengths that differ
    rc, rows, behind = eval_batch_raw(eng, [p, other], xs)
    assert rc == EINVAL and (rows == PATTERN).all() and (behind == PATTERN).all()
    rc, rows, _ = eval_batch_raw(eng, [p, p], xs)
    assert rc == 0 and not (rows == PATTERN).all(axis=1).any()
    # zk_kate_division: p and q of different lengths, either way round
    zm = PC.mont1(7)
    for src, dst in ((p, other), (other, p)):
        with pytest.raises(zk.ZkError) as e:
            eng.kate_division(src, zm, dst)
        assert e.value.code == EINVAL
    assert np.array_equal(eng.download(p), a) and np.array_equal(eng.download(other), base[:n + 1])
    # zk_kate_division: 2^26 + 1 coefficients (2^26 is the longest it takes); the head and the tail of the vector stay as they were
    big = (1 << 26) + 1
    v = eng.poly(big)
    eng.upload_range(v, 0, base[:1024])
    eng.upload_range(v, big - 1024, base[1024:2048])
    with pytest.raises(zk.ZkError) as e:
        eng.kate_division(v, zm)
    assert e.value.code == EINVAL
    assert np.array_equal(eng.download(v, 1024), base[:1024])
    tail = eng.poly(1024)
    eng.copy_range(tail, 0, v, big - 1024, 1024)
    assert np.array_equal(eng.download(tail), base[1024:2048])
    eng.close()
