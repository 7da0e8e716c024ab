"""zk_instance_eval (csrc/verify.hip): inst(x) = sum_{i<m} v_i l_i(x) of many (list, point) pairs in one launch on the device,
limb for limb what tests/halo2_ref.py's instance_eval computes - the value the host verifier (csrc/verifier.h) uses.

Sizes: k = 6, 10, 12; m = 0, 1, 2, 2^k and one below, at and one above every internal boundary of the kernel that fits the domain -
the inversion group (IE_GROUP), a lane's contiguous range (IE_LANE), what one workgroup covers in a pass (IE_SPAN = 64 lanes x
IE_LANE) and the slice a workgroup owns (IE_SLICE, the second grid dimension).  Points: random ones; x = w^i with i < m (the flag is
set, the value zero - the case in which the host verifier rejects) and with i >= m (x^n = 1: zero, flag clear)."""
import random
import types

import numpy as np
import pytest

import webauthn_halo2_amd as zk
import halo2_ref
from public_cases import mont
from zkoracle.field import R, omega

pytestmark = pytest.mark.gpu

# the kernel's constants (csrc/verify.hip)
IE_GROUP, IE_LANE, IE_WG = 8, 16, 64
IE_SPAN = IE_WG * IE_LANE
IE_SLICE = 2 * IE_SPAN


def sizes(k):
    n = 1 << k
    out = {0, 1, 2, n}
    for b in (IE_GROUP, IE_LANE, IE_SPAN, IE_SLICE):
        out |= {m for m in (b - 1, b, b + 1) if m <= n}
    return sorted(out)


def canon(limbs):
    return sum(int(limbs[i]) << (64 * i) for i in range(4)) * pow(1 << 256, -1, R) % R


def shape(k):
    return types.SimpleNamespace(k=k, n=1 << k)


def reference(k, vals, x):
    """(value, on_domain)"""
    try:
        return halo2_ref.instance_eval(shape(k), list(vals), x), False
    except ValueError:
        return 0, True


def check(eng, k, pairs):
    """pairs: [(list of ints - shared objects stay shared, x)]"""
    arrays = {}
    lists = [arrays.setdefault(id(v), mont(v) if v else None) for v, _ in pairs]
    out, flags = eng.instance_eval(k, lists, mont([x for _, x in pairs]))
    for j, (vals, x) in enumerate(pairs):
        want, on = reference(k, vals, x)
        assert (canon(out[j]), flags[j]) == (want, on), (k, j, len(vals))


@pytest.fixture(scope="module")
def eng():
    e = zk.Engine(0)  # (no SRS, no key)
    yield e
    e.close()


@pytest.mark.parametrize("k", [6, 10, 12])
def test_every_boundary_at_random_points(eng, k):
    pr = random.Random(0x5EED0B00 + k)
    full = [pr.randrange(R) for _ in range(1 << k)]
    pairs = [(full[:m], pr.randrange(R)) for m in sizes(k)]
    check(eng, k, pairs)
    assert any(len(v) > IE_SLICE for v, _ in pairs) == (k == 12)


@pytest.mark.parametrize("k", [6, 10, 12])
def test_points_on_the_domain(eng, k):
    pr = random.Random(0x5EED0B10 + k)
    n, w = 1 << k, omega(k)
    pairs, on = [], []
    for m in sizes(k):
        vals = [pr.randrange(1, R) for _ in range(m)]
        for i in sorted({0, m // 2, m - 1, m, n - 1} & set(range(n))):
            pairs.append((vals, pow(w, i, R)))
            on.append(i < m)
    assert [reference(k, v, x) for v, x in pairs] == [(0, f) for f in on]  # (zero either way; the flag tells which)
    check(eng, k, pairs)


def test_one_pair_and_thirty_seven(eng):
    k = 10
    pr = random.Random(0x5EED0B20)
    vals = [pr.randrange(R) for _ in range(9)]
    check(eng, k, [(vals, pr.randrange(R))])
    shared = [pr.randrange(R) for _ in range(300)]
    pairs = []
    for j in range(37):
        m = [0, 1, 9, 17, 300, 1023, 1024][j % 7]
        pairs.append((shared if m == 300 else [pr.randrange(R) for _ in range(m)], pr.randrange(R)))
    check(eng, k, pairs)
    out, flags = eng.instance_eval(k, [], np.zeros((0, 4), dtype=np.uint64))
    assert len(out) == 0 and flags == []


def test_bad_arguments(eng):
    k = 6
    x = mont([5])
    for lists, xs, kk in (([mont([1] * 65)], x, k),                        # more values than the domain has rows
                          ([np.full((1, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)], x, k),  # a value not below the modulus
                          ([mont([1])], np.full((1, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), k),  # a point not below the modulus
                          ([mont([1])], x, 27)):
        with pytest.raises(zk.ZkError) as e:
            eng.instance_eval(kk, lists, xs)
        assert e.value.code == -1
    check(eng, k, [([3, 4], 5)])  # (the context works on)
