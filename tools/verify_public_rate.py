"""zk_verify_batch_public with inst(x) on the host against inst(x) on the device (zk_verify_instance_eval_mode 1 against 2).

    python tools/verify_public_rate.py [--k 17] [--batches 1,64,1024] [--reps 5] [--device 0]

One key of the k = 17 server shape with the instance column and nine exposed gate outputs; ONE proof is made and verified `batch`
times per call (the verifier does the same work per proof whether or not the proofs differ), once with its nine values and once
with the same values padded with zeros to `usable` = n - 7 (the same column, a longer list: every value costs the verifier one
term of inst(x)).  Per (list length, batch) four series ALTERNATE rep by rep after a warm-up of each: option 1, option 2, and
option 1 a second and third time - the last two give the run-to-run spread of the SAME path, the yardstick for a difference
between the paths.  The figure is the median wall time of a call over --reps (at least five) repetitions.  A threshold for the
auto rule may be taken from this table only where the device path wins by more than that spread; prints one JSON line per cell
and a markdown table (docs/experiments.md)."""
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

N_PUBLIC = 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=17)
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("the median of at least five repetitions")
    base = {17: zk.circuit.K17, 19: zk.circuit.K19}[a.k]
    params = dataclasses.replace(base, num_instance_columns=1)
    tr = E.ZK_TRANSCRIPT_EVM
    eng = zk.Engine(a.device)
    eng.srs_setup(params.degree)
    asg = zk.circuit.synthesize(params, 0x5EED0019, n_public=N_PUBLIC)
    pk = eng.keygen(params, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
    polys = []
    for col in asg.advice:
        h = eng.poly(1 << params.degree)
        eng.upload_canonical(h, asg.to_limbs(col))
        polys.append(h)
    usable = (1 << params.degree) - 7
    table = []
    for m in (N_PUBLIC, usable):
        vals = asg.to_mont_limbs(list(asg.instance) + [0] * (m - N_PUBLIC))
        proof = eng.prove_public(pk, polys, vals, bytes(32), tr)
        for batch in [int(b) for b in a.batches.split(",")]:
            proofs, lists = [proof] * batch, [vals] * batch
            series = {"host": 1, "device": 2, "host again": 1, "host a third time": 1}
            for mode in (1, 2):  # warm-up: the verify workspace grows to the batch
                eng.set_verify_instance_eval(mode)
                assert all(eng.verify_batch_public(pk, proofs, lists, tr))
            times = {name: [] for name in series}
            for _ in range(a.reps):
                for name, mode in series.items():
                    eng.set_verify_instance_eval(mode)
                    eng.sync()
                    t0 = time.perf_counter()
                    eng.verify_batch_public(pk, proofs, lists, tr)
                    eng.sync()
                    times[name].append((time.perf_counter() - t0) * 1e3)
            med = {name: statistics.median(v) for name, v in times.items()}
            spread = abs(med["host again"] - med["host a third time"])
            print(json.dumps({"k": a.k, "values": m, "batch": batch, "reps": a.reps, "median_ms": med, "host_spread_ms": spread, "all_ms": times}),
                  flush=True)
            table.append((m, batch, med, spread))
    eng.set_verify_instance_eval(0)
    eng.close()
    print("\n| values per proof | batch | host (ms) | device (ms) | host, two more runs (ms) | spread (ms) |")
    print("|---|---|---|---|---|---|")
    for m, batch, med, spread in table:
        print("| %d | %d | %.2f | %.2f | %.2f / %.2f | %.2f |" % (m, batch, med["host"], med["device"], med["host again"], med["host a third time"], spread))


if __name__ == "__main__":
    main()
