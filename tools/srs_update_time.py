"""Times one ceremony contribution on the device: at each k, zk_srs_update of a resident degree-k SRS beside zk_srs_downsize(k) of
the same SRS (the same G1 transform and window tables, without the scaling pass and the host's G2 / receipt work) and the bare
zk_g_to_lagrange, in one run.  One JSON line per measurement (median of --reps calls, host clock around calls that end in a
device synchronise; update and downsize calls alternate), and one line with the ratio update / downsize against the count
estimate 1 + 2 / k.

    python tools/srs_update_time.py [--reps 3] [--ks 17,19,21]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import webauthn_halo2_amd as zk  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ks", default="17,19,21")
    a = ap.parse_args()
    seed = bytes(range(7, 39))
    for k in [int(x) for x in a.ks.split(",") if x]:
        base = zk.Engine(0)
        base.srs_setup(k)

        def run(what):  # each call replaces its context's SRS: every call starts from a fresh context sharing the base one
            fresh = zk.Engine(0, share_with=base)
            t0 = time.perf_counter()
            if what == "update":
                fresh.srs_update(seed)
            else:
                fresh.srs_downsize(k)
            dt = (time.perf_counter() - t0) * 1e3
            fresh.close()
            return dt

        run("update"), run("downsize")  # warm-up: code objects
        ts = {"update": [], "downsize": []}
        for _ in range(a.reps):
            for what in ts:
                ts[what].append(run(what))
        g = base.srs_export(0, 0, 1 << k)
        base.g_to_lagrange(g, k)
        tl = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            base.g_to_lagrange(g, k)
            tl.append((time.perf_counter() - t0) * 1e3)
        for what, v in (("zk_srs_update", ts["update"]), ("zk_srs_downsize", ts["downsize"]), ("zk_g_to_lagrange", tl)):
            print(json.dumps({"what": what, "k": k, "ms_median": round(statistics.median(v), 2), "ms_min": round(min(v), 2)}), flush=True)
        ratio = statistics.median(ts["update"]) / statistics.median(ts["downsize"])
        print(json.dumps({"what": "update / downsize", "k": k, "ratio": round(ratio, 3), "by_counts": round(1 + 2 / k, 3)}), flush=True)
        base.close()


if __name__ == "__main__":
    main()
