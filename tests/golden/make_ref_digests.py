#!/usr/bin/env python3
"""Generates tests/golden/ref_proof_sha256.json: case id -> SHA-256 of the proof that tests/halo2_ref.py makes for every (shape,
advice sets, instance lists, pairing, seed) of tests/test_halo2_ref.py, tests/test_multi_ref.py and
tests/test_phase_public_ref.py - or, where the witness does not satisfy the circuit, the prover's refusal.
tests/test_halo2_ref.py recomputes every case and compares.

The committed file was recorded from the three modules that halo2_ref replaced, one circuit with the column, N circuits without
and N circuits with, over a worktree of commit e545395 ("One lock-step driver for zk_prove_batch and zk_prove_multi"):
    python tests/golden/make_ref_digests.py --legacy <that worktree>/tests
There every case goes to each old module that can state it; where two can (N = 1 with the column, N >= 2 without) their proofs
must be equal or nothing is written.  Without the option the same file must come out of halo2_ref.

Run in the build container:  python tests/golden/make_ref_digests.py"""
import argparse
import functools
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
LEGACY = "--legacy" in sys.argv
if LEGACY:  # (before the imports below: the old case modules import the old references)
    sys.path.insert(0, sys.argv[sys.argv.index("--legacy") + 1])

from zkoracle.field import R  # noqa: E402
from zkoracle.hashes import ChaCha20Rng  # noqa: E402
import multi_cases  # noqa: E402  (witness generators and keys only; no engine is touched)
from multi_public_cases import lanes  # noqa: E402
from public_cases import PAIRINGS, SEED, reference_key, witness  # noqa: E402

NAMES = ("k19like", "k17like")
LENGTHS = [(9, 9), (0, 9), (1, 9, 2)]


@functools.lru_cache(None)
def public(name, n_public, n_inst=1):
    asg = witness(name, n_public, n_inst)
    return reference_key(name, asg, n_inst), asg


@functools.lru_cache(None)
def laned(name, lengths):
    made = lanes(name, lengths)
    return reference_key(name, made[0][0]), [a.advice for a, _ in made], [vals for _, vals in made]


@functools.lru_cache(None)
def multi(name):
    pk, asgs = multi_cases.setup(name, 3)
    return pk, [a.advice for a in asgs]


def broken_gate(advice, asg):
    """`advice` with one gate row of column 0 (a[r] + a[r+1] a[r+2] - a[r+3] with its selector on) violated."""
    sel = asg.fixed[asg.layout.fx_sel[0]]
    row = next(r for r in range(asg.layout.usable_rows - 3) if sel[r])
    bad = [list(c) for c in advice]
    bad[0][row + 3] = (bad[0][row + 3] + 1) % R
    return bad


def cases():
    """{id: (inputs, kind, scheme, seed)}; inputs() -> (pk, advice sets, instance lists)."""
    out = {}

    def add(cid, inputs, pairs, seed=SEED):
        for kind, scheme in pairs:
            out["%s/%s-%s" % (cid, kind, scheme)] = (inputs, kind, scheme, seed)

    for name in NAMES:
        def one(n_public, n_inst=1, more=(), name=name):
            pk, asg = public(name, n_public, n_inst)
            return pk, [asg.advice], [list(asg.instance) + list(more)]

        def one_off(name=name):
            pk, advs, (vals,) = one(9)
            return pk, advs, [[(vals[0] + 1) % R] + vals[1:]]

        add("one/%s/no-column" % name, lambda one=one: one(0, 0), PAIRINGS)
        add("one/%s/9" % name, lambda one=one: one(9), PAIRINGS)
        add("one/%s/9+zero" % name, lambda one=one: one(9, more=[0]), PAIRINGS)
        add("one/%s/9-first-value-off" % name, one_off, PAIRINGS[:1])
        add("lanes/%s/9" % name, lambda name=name: laned(name, (9,)), PAIRINGS)
        for i, lengths in enumerate(LENGTHS):
            add("lanes/%s/%s" % (name, "-".join(map(str, lengths))), lambda name=name, lengths=lengths: laned(name, lengths),
                PAIRINGS if i == 0 else [PAIRINGS[i % 2]])

    def twice():
        pk, asg = public("k19like", 0, 0)
        return pk, [asg.advice, asg.advice], [[], []]

    def lanes_swapped():
        pk, advs, lists = laned("k19like", (9, 9))
        return pk, advs[::-1], lists[::-1]

    add("one/k19like/no-column-twice", twice, [PAIRINGS[1], ("evm", "gwc")])
    add("lanes/k19like/9-9-both-swapped", lanes_swapped, PAIRINGS[:1])
    add("lanes/k19like/9-0-1", lambda: laned("k19like", (9, 0, 1)), PAIRINGS[1:])
    add("lanes/k17like/1-9", lambda: laned("k17like", (1, 9)), PAIRINGS[1:])

    def oracle(name, order):
        pk, advs = multi(name)
        return pk, [advs[i] for i in order], [[] for _ in order]

    def oracle_broken():
        pk, advs = multi("k18like")
        return pk, [advs[0], broken_gate(advs[1], multi_cases.witnesses("k18like", 2)[1])], [[], []]

    for name in ("k18like", "k19like"):
        add("oracle-key/%s/N1" % name, lambda name=name: oracle(name, (0,)), PAIRINGS, multi_cases.SEED)
    for N in (2, 3):
        add("oracle-key/k18like/N%d" % N, lambda N=N: oracle("k18like", range(N)), PAIRINGS, multi_cases.SEED)
    add("oracle-key/k18like/N2-reordered", lambda: oracle("k18like", (1, 0)), PAIRINGS[:1], multi_cases.SEED)
    add("oracle-key/k18like/N2-broken-gate", oracle_broken, PAIRINGS[:1], multi_cases.SEED)
    return out


def provers():
    """[(can state the case, prover)] over (pk, advice sets, instance lists, rng, kind, scheme)."""
    if not LEGACY:
        import halo2_ref
        return [(lambda pk, lists: True, halo2_ref.create_proof)]
    import multi_public_ref
    import multi_ref
    import public_ref
    column = lambda pk: getattr(pk.shape, "n_inst", None)  # (None: an oracle key, which only multi_ref takes)
    return [(lambda pk, lists: column(pk) is not None, multi_public_ref.create_proof_multi),
            (lambda pk, lists: column(pk) is not None and len(lists) == 1, lambda pk, a, l, *rest: public_ref.create_proof(pk, a[0], l[0], *rest)),
            (lambda pk, lists: not column(pk), lambda pk, a, l, *rest: multi_ref.create_proof_multi(pk, a, *rest))]


def digest(case, prove):
    inputs, kind, scheme, seed = case
    try:
        return hashlib.sha256(prove(*inputs(), ChaCha20Rng(seed), kind, scheme)).hexdigest()
    except AssertionError as e:
        assert "quotient degree" in str(e)
        return "refused: " + str(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legacy", metavar="DIR", help="the tests/ directory of a tree that still has the three old reference modules")
    ap.parse_args()
    out = {}
    for cid, case in cases().items():
        pk, _, lists = case[0]()
        got = [digest(case, prove) for can, prove in provers() if can(pk, lists)]
        assert got and all(g == got[0] for g in got), "%s: the references disagree: %s" % (cid, got)
        out[cid] = got[0]
        print("%-50s %d x %s" % (cid, len(got), got[0][:16]), flush=True)
    with open(os.path.join(HERE, "ref_proof_sha256.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
