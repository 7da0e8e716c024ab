"""Time of the lock-step batch WITH public inputs beside its alternatives, in one run.

    python tools/prove_public_forms_time.py [--rows k17,k19] [--batch 4] [--reps 5] [--device 0]

Rows: k = 17 EVM + GWC (four gate columns) and k = 19 Blake2b + SHPLONK (one advice column).  Per row one engine holds two keys of
the same fixed columns - without the instance column, and with it and nine exposed gate outputs - and B witnesses each.  Three calls
ALTERNATE rep by rep after one warm-up of each:
    zk_prove_batch_public(B)      the batch with one list of nine values per proof
    B x zk_prove_public           the same proofs one after the other, same build, same key
    zk_prove_batch(B)             the batch on the key without the column
The figure is the median wall time of a call over --reps (at least five) repetitions, host-timed around the call with the context
synchronised; the proofs of the first two are compared byte for byte before anything is timed.  No speed is claimed or gated;
prints one JSON line per row and a markdown table (docs/experiments.md)."""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import webauthn_halo2_amd as zk  # noqa: E402
from webauthn_halo2_amd import engine as E  # noqa: E402

ROWS = {
    "k19": (zk.circuit.K19, E.ZK_TRANSCRIPT_BLAKE2B, "k = 19 Blake2b + SHPLONK"),
    "k17": (zk.circuit.K17, E.ZK_TRANSCRIPT_EVM, "k = 17 EVM + GWC"),
}
N_PUBLIC = 9


def resident(eng, params, n_public, batch):
    """(key, advice sets, Montgomery lists) of `batch` witnesses of one structure"""
    asgs = [zk.circuit.synthesize(params, 0x5EED0019 + j, n_public=n_public) for j in range(batch)]
    pk = eng.keygen(params, np.stack([asgs[0].to_limbs(c) for c in asgs[0].fixed]), asgs[0].copies)
    sets = []
    for asg in asgs:
        polys = []
        for col in asg.advice:
            h = eng.poly(1 << params.degree)
            eng.upload_canonical(h, asg.to_limbs(col))
            polys.append(h)
        sets.append(polys)
    return pk, sets, [asg.to_mont_limbs(asg.instance) if asg.instance else None for asg in asgs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="k17,k19")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("the median of at least five repetitions")
    B = a.batch
    table = []
    for row in a.rows.split(","):
        params, tr, label = ROWS[row]
        eng = zk.Engine(a.device)
        eng.srs_setup(params.degree)
        pk0, sets0, _ = resident(eng, params, 0, B)
        pk1, sets1, lists = resident(eng, dataclasses.replace(params, num_instance_columns=1), N_PUBLIC, B)
        seeds = [bytes([j + 1]) * 32 for j in range(B)]
        calls = {
            "zk_prove_batch_public": lambda: eng.prove_batch_public(pk1, sets1, lists, seeds, tr),
            "B x zk_prove_public": lambda: [eng.prove_public(pk1, sets1[j], lists[j], seeds[j], tr) for j in range(B)],
            "zk_prove_batch": lambda: eng.prove_batch(pk0, sets0, seeds, tr),
        }
        warm = {name: fn() for name, fn in calls.items()}  # (warm-up: workspaces, window tables, coset copies)
        assert warm["zk_prove_batch_public"] == warm["B x zk_prove_public"]
        assert all(eng.verify_batch_public(pk1, warm["zk_prove_batch_public"], lists, tr))
        times = {name: [] for name in calls}
        for _ in range(a.reps):
            for name, fn in calls.items():
                eng.sync()
                t0 = time.perf_counter()
                fn()
                eng.sync()
                times[name].append((time.perf_counter() - t0) * 1e3)
        med = {name: statistics.median(v) for name, v in times.items()}
        print(json.dumps({"row": row, "batch": B, "reps": a.reps, "median_ms": med, "all_ms": times}), flush=True)
        table.append((label, med))
        eng.close()
    print("\n| shape, B = %d | zk_prove_batch_public (ms) | B x zk_prove_public (ms) | zk_prove_batch, no column (ms) |" % B)
    print("|---|---|---|---|")
    for label, med in table:
        print("| %s | %.2f | %.2f | %.2f |" % (label, med["zk_prove_batch_public"], med["B x zk_prove_public"], med["zk_prove_batch"]))


if __name__ == "__main__":
    main()
