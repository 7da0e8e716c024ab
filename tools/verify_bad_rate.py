#!/usr/bin/env python3
"""zk_verify_batch on batches that hold pairing-failing proofs: the host bisection (zk_verify_pairing_mode 1, the yardstick) against
the device pairing (mode 2) on the k = 17 EVM + GWC shape.  One process, one context.  Failing proofs are the same circuit's proofs
made under a second SRS: they decode, and fail at the pairing.  For every cell (batch size x number of failing proofs) the two
modes run alternately on the SAME batch; the cell reports each mode's median over --reps calls after --warmup calls of each, with
the zk_verify_pairing_stats delta of one call beside it (host checks, device pairs).  Every timed call ends in a device sync inside
the engine, so host wall-clock time around it is the latency.  Prints one JSON line per cell, then the table in markdown.

    python tools/verify_bad_rate.py [--batches 64,1024] [--reps 5] [--warmup 1]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import webauthn_halo2_amd as zk  # noqa: E402
from webauthn_halo2_amd import engine as E  # noqa: E402

MODES = (("host", E.ZK_VERIFY_PAIRING_HOST), ("device", E.ZK_VERIFY_PAIRING_DEVICE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--proofs", type=int, default=8, help="distinct good and distinct failing proofs (batches cycle through them)")
    a = ap.parse_args()
    reps = max(a.reps, 5)
    p, tr, sc = zk.circuit.K17, E.ZK_TRANSCRIPT_EVM, E.ZK_SCHEME_GWC
    eng = zk.Engine(0)
    asg = zk.circuit.synthesize(p, 0x5EED0019)
    fixed = np.stack([asg.to_limbs(c) for c in asg.fixed])
    adv = [eng.poly(1 << p.degree) for _ in asg.advice]
    for h, col in zip(adv, asg.advice):
        eng.upload_canonical(h, asg.to_limbs(col))
    eng.srs_setup(p.degree, b"\x5a" * 32)  # the second SRS: its proofs fail under the first
    pk = eng.keygen(p, fixed, asg.copies)
    bad = [eng.prove(pk, adv, bytes([0x80 + i]) * 32, tr, sc) for i in range(a.proofs)]
    eng.pk_free(pk)
    eng.srs_setup(p.degree, bytes(32))
    pk = eng.keygen(p, fixed, asg.copies)
    good = [eng.prove(pk, adv, bytes([i + 1]) * 32, tr, sc) for i in range(a.proofs)]
    fc, pc, trr = eng.vk_export(pk)
    for h in adv:
        h.free()
    eng.pk_free(pk)
    vk = eng.vk_from_parts(p, fc, pc, trr)
    rows = []
    for B in [int(x) for x in a.batches.split(",")]:
        for label, n_bad in (("0", 0), ("1", 1), ("8", min(8, B)), ("half", B // 2), ("all", B)):
            # the failing proofs spread evenly over the batch
            at = {(j * B) // n_bad for j in range(n_bad)} if n_bad else set()
            batch = [bad[j % len(bad)] if j in at else good[j % len(good)] for j in range(B)]
            want = [j not in at for j in range(B)]
            ts, stats = {m: [] for m, _ in MODES}, {}
            for it in range(a.warmup + reps):
                for m, mode in MODES:  # alternately, on the same batch
                    eng.verify_pairing_mode(mode)
                    s0 = eng.verify_pairing_stats()
                    t0 = time.perf_counter()
                    v = eng.verify_batch(vk, batch, tr, sc)
                    dt = time.perf_counter() - t0
                    s1 = eng.verify_pairing_stats()
                    assert v == want, (B, label, m)
                    stats[m] = (s1[0] - s0[0], s1[1] - s0[1])
                    if it >= a.warmup:
                        ts[m].append(dt)
            row = {"k": p.degree, "batch": B, "failing": label, "n_failing": n_bad, "reps": reps}
            for m, _ in MODES:
                row[m + "_ms_median"] = round(statistics.median(ts[m]) * 1e3, 3)
                row[m + "_ms_min"] = round(min(ts[m]) * 1e3, 3)
                row[m + "_host_checks"], row[m + "_device_pairs"] = stats[m]
            rows.append(row)
            print(json.dumps(row), flush=True)
    eng.verify_pairing_mode(E.ZK_VERIFY_PAIRING_AUTO)
    eng.pk_free(vk)
    eng.close()
    print("| batch | failing | host ms (median) | host checks | device ms (median) | host checks + device pairs |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print("| %d | %s | %.2f | %d | %.2f | %d + %d |" % (r["batch"], r["failing"], r["host_ms_median"], r["host_host_checks"], r["device_ms_median"],
                                                          r["device_host_checks"], r["device_device_pairs"]))


if __name__ == "__main__":
    main()
