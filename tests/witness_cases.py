"""Witnesses for the zk_witness_check tests (tests/test_witness_ref.py, tests/test_gpu_witness_check.py): the two generators'
circuits as plain lists, and a seeded planter of corrupted cells of every sort the check must tell apart."""
import random

import numpy as np

import webauthn_halo2_amd as zk
import witness_ref as W
from zkoracle.field import R


def limbs(col):
    """ints -> (n, 4) uint64 canonical little-endian limbs"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in col), dtype=np.uint64).reshape(-1, 4).copy()


def params_of(t):
    A, L, F, k, lb, idle = (tuple(t) + (0,))[:6]
    return zk.circuit.CircuitParams(degree=k, num_advice=A, num_lookup_advice=L, num_fixed=F, lookup_bits=lb, idle_gate_columns=idle)


def synth_case(t, seed=0x5EED0019):
    """(shape, fixed, copies, advice) of webauthn-halo2_amd/circuit.py's generator."""
    asg = zk.circuit.synthesize(params_of(t), seed)
    return W.shape_of(t), asg.fixed, asg.copies, asg.advice


def adv_case(t, seed):
    """The same of tests/adversarial_layout.py (shapes without idle gate columns)."""
    import adversarial_layout as adv

    sh = W.shape_of(t)
    fixed, copies, advice = adv.build(sh, seed)
    adv.check(sh, fixed, copies, advice)
    return sh, fixed, copies, advice


def cycles(copies):
    """The copy cycles (lists of (perm column, row), two cells or more) the copy constraints merge."""
    parent = {}

    def find(x):
        parent.setdefault(x, x)
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in copies:
        ra, rb = find(tuple(a)), find(tuple(b))
        if ra != rb:
            parent[ra] = rb
    groups = {}
    for x in list(parent):
        groups.setdefault(find(x), []).append(x)
    return [sorted(g) for g in groups.values() if len(g) > 1]


def plant(shape, fixed, copies, advice, seed):
    """A copy of `advice` with a seeded random mix of corrupted cells: gate inputs and outputs, members of copy cycles of two
    and of five or more cells, advice cells of cycles a constants cell sources, lookup inputs outside the table, the values
    r - 1 and 0.  -> (advice, corrupted (column, row) cells)"""
    rng = random.Random(seed)
    adv = [list(c) for c in advice]
    F, usable, T = shape.num_fixed, shape.usable_rows, 1 << shape.lookup_bits
    done = []

    def put(j, r, v):
        if (j, r) in done or adv[j][r] % R == v % R:
            return
        adv[j][r] = v % R
        done.append((j, r))

    def other(v):
        return rng.choice(((v + 1) % R, (v + rng.randrange(1, R)) % R, (v + R - 1) % R))

    gates = [(j, r) for j in range(shape.n_gate) for r in range(usable - 3) if W.effective_selector(shape, fixed, j, r)]
    for _ in range(2):
        j, r = rng.choice(gates)
        put(j, r + rng.randrange(3), other(adv[j][r]))   # an input
        j, r = rng.choice(gates)
        put(j, r + 3, other(adv[j][r + 3]))              # an output
    cyc = cycles(copies)
    sorts = ([c for c in cyc if len(c) == 2], [c for c in cyc if len(c) >= 5], [c for c in cyc if any(col < F for col, _ in c)])
    for group in sorts:
        for _ in range(2):
            if not group:
                continue
            cells = [(col - F, r) for col, r in rng.choice(group) if col >= F]
            if cells:
                j, r = rng.choice(cells)
                put(j, r, other(adv[j][r]))
    if shape.single:
        looked = [(0, r) for r in range(usable) if fixed[shape.fx_qlookup][r]]
    else:
        looked = [(shape.n_gate + l, r) for l in range(shape.n_lookup_cols) for r in range(usable)]
    for _ in range(2):
        j, r = rng.choice(looked)
        put(j, r, rng.choice((T, T + rng.randrange(1 << 20), 1 << 40, rng.randrange(T, R))))
    j, r = rng.choice(gates)
    put(j, r + rng.randrange(4), R - 1)
    j, r = rng.choice(gates)
    put(j, r + rng.randrange(4), 0)
    assert done
    return adv, done
