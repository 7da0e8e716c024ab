"""The phase-level forms with public inputs and N circuits (zk_permutation_product_public, zk_quotient_multi, zk_eval_batch) through
Engine, against tests/phase_public_ref.py - the CPU restatement that tests/test_phase_public_ref.py ties to the whole proofs of
tests/halo2_ref.py - with beta, gamma and y of the test's own choosing.

  fallback    on a key without the column: permutation_product_public(instance None) is zk_permutation_product byte for byte,
              quotient_multi with one circuit is zk_quotient byte for byte, divide 0 and 1
  eval_batch  every result is zk_eval of its pair; a repeated handle; 1, 63, 64 and 65 pairs (one launch takes 64)
  lists       k19like (the column joins a chunk), k17like (it opens one), wide (two lookups, two constants columns): three circuits
              of ONE key with 0, 1 and 9 public inputs - every circuit's z over rows 0 .. n - 7, and the h pieces of the ONE quotient
              over the three, exactly; the undivided quotient on the whole coset at k19like
  refusals    every one the header lists, with its code, and a sentinel in the outputs before and after"""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phase_public_ref as PPR  # noqa: E402
import webauthn_halo2_amd as zk  # noqa: E402
from multi_public_cases import engine_lanes, lanes  # noqa: E402
from public_cases import engine_key, mont, params_of, reference_key, witness  # noqa: E402
from zkoracle import cops  # noqa: E402
from zkoracle.field import R  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5
BF = 6


def m1(v):
    return mont([v % R])[0]


def rand_mont(pr, rows):
    return mont([pr.randrange(R) for _ in range(rows)])


def to_ext(eng, col, n):
    """The extended-coset form of a resident Lagrange column: a copy through zk_lagrange_to_coeff and zk_coeff_to_extended."""
    p = eng.poly(n)
    eng.copy(p, col)
    eng.lagrange_to_coeff(p)
    e = eng.poly(4 * n)
    eng.coeff_to_extended(p, e)
    p.free()
    return e


def instance_poly(eng, n, vals):
    """The resident instance vector of a host's list: rows 0 .. m - 1 the Montgomery values, zero behind them."""
    col = np.zeros((n, 4), dtype=np.uint64)
    if vals:
        col[:len(vals)] = mont(vals)
    return eng.poly(n, col)


def raises(code, fn, *args, **kw):
    with pytest.raises(zk.ZkError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, code)


# ------------------------------------------------------------------------------------------------------------ fallback ---
@pytest.mark.parametrize("name", ["k19like", "k17like"])
def test_without_the_column_the_public_forms_are_the_plain_ones(name):
    eng = zk.Engine(0)
    asg = witness(name, 0, n_inst=0)
    pk, (adv,) = engine_key(eng, name, [asg], n_inst=0)
    sh = eng.pk_shape(pk)
    n = 1 << sh["k"]
    pr = random.Random(0x5EED0B01)
    beta, gamma, y = (m1(pr.randrange(R)) for _ in range(3))
    z0 = eng.permutation_product(pk, adv, beta, gamma)
    z1 = eng.permutation_product_public(pk, adv, None, beta, gamma)
    assert len(z0) == len(z1) == sh["n_chunks"]
    for a, b in zip(z0, z1):
        assert np.array_equal(eng.download(a)[:n - BF], eng.download(b)[:n - BF])
    # any vectors over the extended coset: the two entry points are compared with each other
    ext = lambda: eng.poly(4 * n, rand_mont(pr, 4 * n))
    adv_e, z_e = [ext() for _ in adv], [ext() for _ in z0]
    lk_e = [(ext(), ext(), ext()) for _ in range(sh["n_lookups"])]
    h0, h1 = eng.poly(4 * n), eng.poly(4 * n)
    for divide in (False, True):
        eng.quotient(pk, adv_e, z_e, lk_e, beta, gamma, y, h0, divide=divide)
        eng.quotient_multi(pk, [adv_e], None, [z_e], [lk_e], beta, gamma, y, h1, divide=divide)
        assert np.array_equal(eng.download(h0), eng.download(h1)), divide
    eng.close()


# ---------------------------------------------------------------------------------------------------------- eval_batch ---
def test_eval_batch_is_eval_pair_by_pair():
    eng = zk.Engine(0)
    n = 128
    pr = random.Random(0x5EED0B02)
    polys = [eng.poly(n, rand_mont(pr, n)) for _ in range(5)]
    few = [m1(pr.randrange(R)) for _ in range(3)]  # (a proof opens at a handful of points: the launch shares their powers)
    for count in (1, 63, 64, 65):
        ps = [polys[(3 * i) % 5] for i in range(count)]  # every handle repeats
        xs = np.stack([few[i % 3] if i % 2 else m1(pr.randrange(R)) for i in range(count)])
        got = eng.eval_batch(ps, xs)
        assert got.shape == (count, 4)
        for i in range(count):
            assert np.array_equal(got[i], eng.eval(ps[i], xs[i])), (count, i)
    # refusals: no pair, lengths that differ, a dead handle, a null pointer - and nothing is written
    other = eng.poly(2 * n, rand_mont(pr, 2 * n))
    out = np.full((2, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    before = out.copy()
    u64p = ctypes.POINTER(ctypes.c_uint64)
    call = lambda hs, cnt, o=out: eng.L.zk_eval_batch(eng.ctx, (ctypes.c_uint64 * 2)(*hs), xs.ctypes.data_as(u64p), cnt, o.ctypes.data_as(u64p))
    assert call([polys[0].h, polys[1].h], 0) == EINVAL
    assert call([polys[0].h, other.h], 2) == EINVAL
    assert call([polys[0].h, 0xDEAD0000], 2) == EINVAL
    assert eng.L.zk_eval_batch(eng.ctx, (ctypes.c_uint64 * 2)(polys[0].h, polys[1].h), xs.ctypes.data_as(u64p), 2, None) == EINVAL
    assert np.array_equal(out, before)
    assert call([polys[0].h, polys[1].h], 2) == 0 and not np.array_equal(out, before)
    eng.close()


# ---------------------------------------------------------------------------------------- lists of 0, 1 and 9 values ---
class Lanes:
    """Three circuits of ONE key with the column - 0, 1 and 9 public inputs - resident on `eng` and as integers: advice with random
    blinding rows, a', s' and zL of the device's own lookup provers (blinded), for beta and gamma of the test's choosing."""

    def __init__(self, eng, name, seed, lengths=(0, 1, 9)):
        self.eng, self.name = eng, name
        made = lanes(name, lengths)
        self.rpk = reference_key(name, made[0][0])
        self.sh = self.rpk.shape
        self.pk, self.adv, _ = engine_lanes(eng, name, made)
        self.lists = [vals for _, vals in made]
        assert [len(v) for v in self.lists] == list(lengths)
        sh, n, usable = self.sh, self.sh.n, self.sh.usable_rows
        self.n = n
        pr = self.pr = random.Random(seed)
        self.beta, self.gamma, self.y = (pr.randrange(R) for _ in range(3))
        self.inst = [instance_poly(eng, n, vals) for vals in self.lists]
        self.cols = []  # per circuit: the integer mirror of what the device holds
        self.ap, self.sp, self.zl = [], [], []
        for c, (asg, _) in enumerate(made):
            for p in self.adv[c]:
                eng.upload_range(p, usable, rand_mont(pr, n - usable))
            a, s = eng.lookup_permute(self.pk, self.adv[c])
            for p in a + s:
                eng.upload_range(p, usable, rand_mont(pr, n - usable))
            zl = eng.lookup_product(self.pk, self.adv[c], a, s, m1(self.beta), m1(self.gamma))
            for p in zl:
                eng.upload_range(p, n - BF, rand_mont(pr, BF))
            self.ap.append(a), self.sp.append(s), self.zl.append(zl)
            ints = lambda ps: [cops.fr_ints(eng.download(p)) for p in ps]
            self.cols.append(dict(adv=ints(self.adv[c]), ap=ints(a), sp=ints(s), zl=ints(zl), instances=self.lists[c]))

    def products(self):
        """zk_permutation_product_public of every circuit against the restatement, rows 0 .. n - 7; the z columns, blinded, are
        kept on both sides for the quotient."""
        eng, sh, n = self.eng, self.sh, self.n
        self.z = []
        for c, d in enumerate(self.cols):
            want = PPR.permutation_products_public(sh, self.rpk.fixed, self.rpk.sigma, d["adv"], d["instances"], self.beta, self.gamma)
            z = eng.permutation_product_public(self.pk, self.adv[c], self.inst[c], m1(self.beta), m1(self.gamma))
            assert len(z) == len(want) == sh.n_chunks
            d["z"] = []
            for ci, (got, exp) in enumerate(zip(z, want)):
                assert np.array_equal(eng.download(got)[:n - BF], mont(exp)), (self.name, "circuit", c, "chunk", ci)
                blind = [self.pr.randrange(R) for _ in range(BF)]
                eng.upload_range(got, n - BF, mont(blind))
                d["z"].append(list(exp) + blind)
            self.z.append(z)

    def cosets(self):
        eng, n = self.eng, self.n
        e = lambda ps: [to_ext(eng, p, n) for p in ps]
        self.adv_e = [e(ps) for ps in self.adv]
        self.z_e = [e(ps) for ps in self.z]
        self.lk_e = [[tuple(e([a, s, z])) for a, s, z in zip(self.ap[c], self.sp[c], self.zl[c])] for c in range(len(self.adv))]
        self.inst_e = e(self.inst)


@pytest.mark.parametrize("name", ["k19like", "k17like", "wide"])
def test_lists_of_0_1_and_9_values_against_the_restatement(name):
    eng = zk.Engine(0)
    L = Lanes(eng, name, 0x5EED0B10 + len(name))
    sh, n = L.sh, L.n
    assert (len(sh.perm_cols) % sh.chunk_len == 1) == (name == "k17like")  # the column opens a chunk of its own there alone
    L.products()
    # a circuit's product reads ITS column: circuit 2's advice with circuit 1's list is another z (the 9 exposed cells differ)
    other = eng.permutation_product_public(L.pk, L.adv[2], L.inst[1], m1(L.beta), m1(L.gamma))
    assert any(not np.array_equal(eng.download(a)[:n - BF], eng.download(b)[:n - BF]) for a, b in zip(other, L.z[2]))
    L.cosets()
    beta, gamma, y = m1(L.beta), m1(L.gamma), m1(L.y)
    h = eng.poly(4 * n)
    eng.quotient_multi(L.pk, L.adv_e, L.inst_e, L.z_e, L.lk_e, beta, gamma, y, h)
    want = PPR.quotient_multi(sh, L.rpk.fixed, L.rpk.sigma, L.cols, L.beta, L.gamma, L.y)
    pieces, above = PPR.h_pieces(sh, want)
    assert not any(above), "the columns satisfy the circuit: h has n_h pieces"
    assert np.array_equal(eng.download(h), mont(want))
    eng.extended_to_coeff(h, sh.n_h * n)
    got = eng.download(h)
    for i, piece in enumerate(pieces):
        assert np.array_equal(got[i * n:(i + 1) * n], mont(piece)), (name, "h piece", i)
    if name == "k19like":
        eng.quotient_multi(L.pk, L.adv_e, L.inst_e, L.z_e, L.lk_e, beta, gamma, y, h, divide=False)
        raw = PPR.quotient_multi(sh, L.rpk.fixed, L.rpk.sigma, L.cols, L.beta, L.gamma, L.y, divide=False)
        assert np.array_equal(eng.download(h), mont(raw))
        # one circuit with its 9 values: the N = 1 form on a key with the column
        eng.quotient_multi(L.pk, L.adv_e[2:], L.inst_e[2:], L.z_e[2:], L.lk_e[2:], beta, gamma, y, h)
        one = PPR.quotient_multi(sh, L.rpk.fixed, L.rpk.sigma, L.cols[2:], L.beta, L.gamma, L.y)
        assert np.array_equal(eng.download(h), mont(one))
    eng.close()


# ------------------------------------------------------------------------------------------------------------ refusals ---
def test_refusals_leave_the_outputs_untouched():
    eng = zk.Engine(0)
    name = "k17like"
    L = Lanes(eng, name, 0x5EED0B20, lengths=(9, 1))
    L.products()
    L.cosets()
    pk, sh, n = L.pk, L.sh, L.n
    beta, gamma, y = m1(L.beta), m1(L.gamma), m1(L.y)
    pr = random.Random(7)
    sentinel = rand_mont(pr, n)
    zs = [eng.poly(n, sentinel) for _ in range(sh.n_chunks)]
    adv, inst = L.adv[0], L.inst[0]
    pp = lambda key, a, i, z: eng.permutation_product_public(key, a, i, beta, gamma, z_out=z)
    # -- zk_permutation_product_public
    raises(EINVAL, pp, pk, adv, None, zs)                 # a key with the column and no instance vector
    raises(EINVAL, pp, pk, adv[:-1], inst, zs)            # wrong counts
    raises(EINVAL, pp, pk, adv, inst, zs[:-1])
    raises(EINVAL, pp, pk, adv, inst, zs + [eng.poly(n, sentinel)])
    raises(EINVAL, pp, pk, adv, inst, [zs[0]] * sh.n_chunks)     # an output twice
    raises(EINVAL, pp, pk, adv, inst, [adv[0]] + zs[1:])         # an advice column as an output
    raises(EINVAL, pp, pk, adv, inst, zs[:-1] + [inst])          # the instance vector as an output
    raises(EINVAL, pp, pk, adv, L.inst_e[0], zs)                 # an instance vector of another length
    raises(EINVAL, eng.permutation_product, pk, adv, beta, gamma)  # the form without the column keeps refusing the key
    vk = eng.vk_read(params_of(name), eng.vk_write(pk))
    raises(ESTATE, pp, vk, adv, inst, zs)
    for z in zs:
        assert np.array_equal(eng.download(z), sentinel)
    assert np.array_equal(eng.download(adv[0]), mont(L.cols[0]["adv"][0])) and np.array_equal(eng.download(inst)[:9], mont(L.lists[0]))
    # -- zk_quotient_multi
    N4 = 4 * n
    sent4 = rand_mont(pr, N4)
    h = eng.poly(N4, sent4)
    qm = lambda key, a, i, z, lk, out: eng.quotient_multi(key, a, i, z, lk, beta, gamma, y, out)
    A, I, Z, K = L.adv_e, L.inst_e, L.z_e, L.lk_e
    raises(EINVAL, qm, pk, A, None, Z, K, h)                      # a key with the column and no instance cosets
    raises(EINVAL, qm, pk, [a[:-1] for a in A], I, Z, K, h)       # wrong counts
    raises(EINVAL, qm, pk, A, I, [z[:-1] for z in Z], K, h)
    raises(EINVAL, qm, pk, A, I, Z, [k + k for k in K], h)
    raises(EINVAL, qm, pk, [], I, Z, K, h)                        # no circuit
    raises(EINVAL, qm, pk, A * 9, I * 9, Z * 9, K * 9, h)         # 18 circuits: above ZK_PROVE_MULTI_MAX
    raises(EINVAL, qm, pk, A, [I[0], L.inst[1]], Z, K, h)         # an instance handle that is no extended vector
    for out in (A[1][0], I[1], Z[0][0], K[1][0][2]):              # the output among the inputs, of the second circuit too
        before = eng.download(out)
        raises(EINVAL, qm, pk, A, I, Z, K, out)
        assert np.array_equal(eng.download(out), before)
    raises(EINVAL, eng.quotient, pk, A[0], Z[0], K[0], beta, gamma, y, h)  # zk_quotient keeps refusing the key
    raises(ESTATE, qm, vk, A, I, Z, K, h)
    assert np.array_equal(eng.download(h), sent4)
    eng.pk_free(vk)
    # -- a key WITHOUT the column takes no instance handle
    asg0 = witness("k19like", 0, n_inst=0)
    # (another SRS of the same k: the key above is stale from here on)
    pk0, (adv0,) = engine_key(eng, "k19like", [asg0], n_inst=0)
    raises(ESTATE, pp, pk, adv, inst, zs)
    raises(ESTATE, qm, pk, A, I, Z, K, h)
    for z in zs:
        assert np.array_equal(eng.download(z), sentinel)
    assert np.array_equal(eng.download(h), sent4)
    sh0 = eng.pk_shape(pk0)
    z0 = [eng.poly(n, sentinel) for _ in range(sh0["n_chunks"])]
    raises(EINVAL, pp, pk0, adv0, inst, z0)
    ext = lambda: eng.poly(N4, rand_mont(pr, N4))
    a0, zz0, k0 = [[ext() for _ in adv0]], [[ext() for _ in z0]], [[(ext(), ext(), ext()) for _ in range(sh0["n_lookups"])]]
    raises(EINVAL, qm, pk0, a0, [I[0]], zz0, k0, h)
    for z in z0:
        assert np.array_equal(eng.download(z), sentinel)
    assert np.array_equal(eng.download(h), sent4)
    eng.close()
