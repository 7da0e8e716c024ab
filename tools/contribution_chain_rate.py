#!/usr/bin/env python3
"""A chain of ceremony receipts checked on the host and on the device.  The yardstick is the host route, one
zk_srs_contribution_check per receipt (what check_contributions does under "host"); the device route is one
zk_srs_contribution_check_batch call for the whole chain, one receipt per lane.  One process, one context without an SRS.  The
chains are honest: the receipts of as many zk_srs_update steps on a k = 4 SRS, made on a context of its own before anything is
timed.  For every count the two routes run alternately on the SAME chain; the cell reports each route's median and min over --reps calls after --warmup calls of each.  Every call ends in a device sync inside the
engine or never touches the device, so host wall-clock time around it is the latency.  Prints one JSON line per cell, then the
table in markdown and the count from which "auto" may move to the device: the smallest one at which the device median is below the
host median by more than the larger min-to-median spread of the two cells.

    python tools/contribution_chain_rate.py [--counts 1,8,64,512,4096] [--reps 5] [--warmup 1]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import webauthn_halo2_amd as zk  # noqa: E402
from webauthn_halo2_amd import engine as E  # noqa: E402

ALL = E.ZK_SRS_CONTRIB_SAME_SECRET | E.ZK_SRS_CONTRIB_LINKS | E.ZK_SRS_CONTRIB_NONTRIVIAL


def honest_chain(n):
    """n receipts of n zk_srs_update steps on a context of its own (a k = 4 SRS): each starts at the g[1] the one before left"""
    eng = zk.Engine(0)
    eng.srs_setup(4, b"\x42" * 32)
    out = []
    for i in range(n):
        out.append(eng.srs_update(i.to_bytes(4, "little") * 8))
        if i % 512 == 511:
            print("# chain: %d receipts" % (i + 1), flush=True)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,8,64,512,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    reps = max(a.reps, 5)
    counts = [int(x) for x in a.counts.split(",")]
    chain = honest_chain(max(counts))
    eng = zk.Engine(0)
    routes = (("host", lambda recs: [eng.srs_contribution_check(r) | (E.ZK_SRS_CONTRIB_CHAINED) for r in recs]),
              ("device", lambda recs: eng.srs_contribution_check_batch(recs)))
    rows = []
    for n in counts:
        recs = chain[:n]
        ts = {m: [] for m, _ in routes}
        for it in range(a.warmup + reps):
            for m, run in routes:  # alternately, on the same chain
                t0 = time.perf_counter()
                flags = run(recs)
                dt = time.perf_counter() - t0
                assert flags == [ALL | E.ZK_SRS_CONTRIB_CHAINED] * n, (n, m)
                print("# count %d %s call %d: %.3f ms" % (n, m, it, dt * 1e3), flush=True)
                if it >= a.warmup:
                    ts[m].append(dt)
        row = {"count": n, "reps": reps}
        for m, _ in routes:
            row[m + "_ms_median"] = round(statistics.median(ts[m]) * 1e3, 3)
            row[m + "_ms_min"] = round(min(ts[m]) * 1e3, 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    eng.close()
    print("| receipts | host ms (median) | host ms (min) | device ms (median) | device ms (min) | host / device |")
    print("|---|---|---|---|---|---|")
    move = None
    for r in rows:
        print("| %d | %.2f | %.2f | %.2f | %.2f | %.1f |" % (r["count"], r["host_ms_median"], r["host_ms_min"], r["device_ms_median"], r["device_ms_min"],
                                                         r["host_ms_median"] / r["device_ms_median"]))
        spread = max(r["host_ms_median"] - r["host_ms_min"], r["device_ms_median"] - r["device_ms_min"])
        if move is None and r["host_ms_median"] - r["device_ms_median"] > spread:
            move = r["count"]
    print("device median below host median by more than the larger min-to-median spread from: %s receipts" % (move if move is not None else "no measured count"))


if __name__ == "__main__":
    main()
