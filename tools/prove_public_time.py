"""Time of a lone zk_prove_public with nine public inputs beside a lone zk_prove, in one run.

    python tools/prove_public_time.py [--rows k17,k19] [--reps 7] [--device 0]

Rows: k = 17 EVM + GWC (four gate columns) and k = 19 Blake2b + SHPLONK (one advice column).  Per row one engine holds two keys
of the same fixed columns - without the instance column, and with it and nine exposed gate outputs - and one witness each; the
two calls ALTERNATE rep by rep after one warm-up of each, and the figure is the median wall time of a call (host-timed around the
call, the context synchronised).  By counts the public form pays one more column of transforms (iNTT, extended coset) and one more
column in the last permutation chunk's products; at k = 17 the column starts a fourth chunk: one more z column - its grand product,
commitment and transforms - and three more evaluations.  No speed is claimed or gated; prints one JSON line per row and a markdown
table."""
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


def resident(eng, params, n_public):
    asg = zk.circuit.synthesize(params, 0x5EED0019, n_public=n_public)
    pk = eng.keygen(params, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
    polys = []
    for col in asg.advice:
        h = eng.poly(1 << params.degree)
        eng.upload_canonical(h, asg.to_limbs(col))
        polys.append(h)
    return pk, polys, asg.to_mont_limbs(asg.instance)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="k17,k19")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    table = []
    for row in a.rows.split(","):
        params, tr, label = ROWS[row]
        eng = zk.Engine(a.device)
        eng.srs_setup(params.degree)
        pk0, polys0, _ = resident(eng, params, 0)
        pk1, polys1, inst = resident(eng, dataclasses.replace(params, num_instance_columns=1), N_PUBLIC)
        seed = bytes(32)
        calls = {"zk_prove": lambda: eng.prove(pk0, polys0, seed, tr), "zk_prove_public": lambda: eng.prove_public(pk1, polys1, inst, seed, tr)}
        sizes = {name: len(fn()) for name, fn in calls.items()}  # (warm-up: workspaces, window tables, coset copies)
        assert eng.verify(pk0, calls["zk_prove"](), tr) and eng.verify_public(pk1, calls["zk_prove_public"](), inst, tr)
        times = {name: [] for name in calls}
        for _ in range(a.reps):
            for name, fn in calls.items():
                eng.sync()
                t0 = time.perf_counter()
                fn()
                eng.sync()
                times[name].append((time.perf_counter() - t0) * 1e3)
        med = {name: statistics.median(v) for name, v in times.items()}
        print(json.dumps({"row": row, "reps": a.reps, "median_ms": med, "all_ms": times, "proof_bytes": sizes}), flush=True)
        table.append((label, med, sizes))
        eng.close()
    print("\n| shape | zk_prove (ms) | zk_prove_public, 9 values (ms) | proof bytes |")
    print("|---|---|---|---|")
    for label, med, sizes in table:
        print("| %s | %.2f | %.2f | %d -> %d |" % (label, med["zk_prove"], med["zk_prove_public"], sizes["zk_prove"], sizes["zk_prove_public"]))


if __name__ == "__main__":
    main()
