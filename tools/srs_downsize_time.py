"""Times ParamsKZG::downsize on the device: zk_g_to_lagrange and zk_srs_downsize from a K = 21 SRS to k = 17, 19, 21, and
zk_srs_check at k = 17 and 19.  One JSON line per measurement (median of --reps calls, host clock around calls that end in a
device synchronise).

    python tools/srs_downsize_time.py [--reps 3] [--K 21] [--ks 17,19,21] [--check-ks 17,19]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import webauthn_halo2_amd as zk  # noqa: E402


def timed(fn, reps):
    fn()  # warm-up: code objects, twiddle tables
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--K", type=int, default=21)
    ap.add_argument("--ks", default="17,19,21")
    ap.add_argument("--check-ks", default="17,19")
    a = ap.parse_args()
    ks = [int(x) for x in a.ks.split(",") if x]
    base = zk.Engine(0)
    base.srs_setup(a.K)
    for k in ks:
        g = base.srs_export(0, 0, 1 << k)
        med, lo = timed(lambda: base.g_to_lagrange(g, k), a.reps)
        print(json.dumps({"what": "zk_g_to_lagrange", "k": k, "ms_median": round(med, 2), "ms_min": round(lo, 2)}), flush=True)
        def down():  # each downsize replaces its context's SRS: every call starts from a fresh context sharing the K one
            fresh = zk.Engine(0, share_with=base)
            t0 = time.perf_counter()
            fresh.srs_downsize(k)
            dt = (time.perf_counter() - t0) * 1e3
            fresh.close()
            return dt
        down()
        ts = [down() for _ in range(a.reps)]
        print(json.dumps({"what": "zk_srs_downsize", "K": a.K, "k": k, "ms_median": round(statistics.median(ts), 2),
                          "ms_min": round(min(ts), 2)}), flush=True)
    for k in [int(x) for x in a.check_ks.split(",") if x]:
        eng = zk.Engine(0)
        eng.srs_setup(k)
        flags = eng.srs_check()
        med, lo = timed(lambda: eng.srs_check(), a.reps)
        print(json.dumps({"what": "zk_srs_check", "k": k, "flags": flags, "ms_median": round(med, 2), "ms_min": round(lo, 2)}), flush=True)
        eng.close()
    base.close()


if __name__ == "__main__":
    main()
