"""Times zk_witness_check beside the proof it guards, per shape (the k = 17 server shape and k = 19 by default), one JSON line per
measurement: the one-off sigma decode of a key's first check; the per-call time on a clean witness, with 1 and with 10 000 planted
failures at cap = 64; and, in the same run, the lone zk_prove of that shape and the ratio check / proof.  Every clock is the host's
around calls that end in zk_sync; warm-up first, then enough calls to fill --min-seconds; median, min and max.

    python tools/witness_check_time.py [--ks 17,19] [--min-seconds 0.5]
    python tools/witness_check_time.py --prove-only                       # the lone-proof figures alone
    python tools/witness_check_time.py --ab-lib OTHER/libzkmi355.so [--ab-rounds 3]
        # "did zk_prove get slower": --prove-only in fresh child processes, this build and the other one (through ZKMI355_LIB)
        # alternating; the spread between the runs of one build is the margin
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, sync, min_seconds, warm=3, min_calls=20):
    for _ in range(warm):
        fn()
    sync()
    ts, t_end = [], time.perf_counter() + min_seconds
    while len(ts) < min_calls or time.perf_counter() < t_end:
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"calls": len(ts), "ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def run_shape(k, a):
    import numpy as np

    import webauthn_halo2_amd as zk
    from webauthn_halo2_amd import engine as E

    p = {17: zk.circuit.K17, 19: zk.circuit.K19}[k]
    asg = zk.circuit.synthesize(p, 0x5EED0019)
    eng = zk.Engine(0)
    eng.srs_setup(k)
    pk = eng.keygen(p, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
    cols = [asg.to_limbs(c) for c in asg.advice]
    polys = [eng.poly(1 << k, None) for _ in cols]
    for h, c in zip(polys, cols):
        eng.upload_canonical(h, c)
    eng.sync()
    out = {"k": k, "lib": os.environ.get("ZKMI355_LIB") or "this build"}
    if not a.prove_only:
        t0 = time.perf_counter()
        counts, _ = eng.witness_check(pk, polys)
        eng.sync()
        first = (time.perf_counter() - t0) * 1e3
        assert counts[0] == 0, counts
        clean = timed(lambda: eng.witness_check(pk, polys), eng.sync, a.min_seconds)
        print(json.dumps(dict(out, what="first check of the key (state + sigma decode + check)", ms=round(first, 3),
                              sigma_decode_ms=round(first - clean["ms_median"], 3))), flush=True)
        print(json.dumps(dict(out, what="witness_check, clean witness", **clean)), flush=True)
        sel = asg.fixed[asg.layout.fx_sel[0]]
        rows = [r for r in range(0, asg.layout.usable_rows - 3, 4) if sel[r]]
        for planted in (1, 10000):
            bad = cols[0].copy()
            for r in rows[:planted]:
                bad[r + 3, 0] ^= np.uint64(1)  # a gate output
            eng.upload_canonical(polys[0], bad)
            counts, lst = eng.witness_check(pk, polys, 64)
            assert counts[E.ZK_FAIL_GATE] == planted and len(lst) == min(64, counts[0]), counts
            res = timed(lambda: eng.witness_check(pk, polys, 64), eng.sync, a.min_seconds)
            print(json.dumps(dict(out, what="witness_check, %d planted failures, cap 64" % planted, failures=counts[0], **res)), flush=True)
        eng.upload_canonical(polys[0], cols[0])
    seed = b"\x11" * 32
    prove = timed(lambda: eng.prove(pk, polys, seed, E.ZK_TRANSCRIPT_BLAKE2B), eng.sync, a.min_seconds, warm=3)
    print(json.dumps(dict(out, what="lone zk_prove", **prove)), flush=True)
    if not a.prove_only:
        print(json.dumps(dict(out, what="ratio check / proof (clean witness, medians)", ratio=round(clean["ms_median"] / prove["ms_median"], 4))), flush=True)
    for h in polys:
        h.free()
    eng.pk_free(pk)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="17,19")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--prove-only", action="store_true")
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--ab-rounds", type=int, default=3)
    a = ap.parse_args()
    if a.ab_lib:
        for rnd in range(a.ab_rounds):
            for lib in (None, os.path.abspath(a.ab_lib)):
                env = dict(os.environ)
                env.pop("ZKMI355_LIB", None)
                if lib:
                    env["ZKMI355_LIB"] = lib
                # a fresh process per run; a run that fails or hangs ends the comparison (nothing more is started on the device)
                subprocess.run([sys.executable, os.path.abspath(__file__), "--prove-only", "--ks", a.ks, "--min-seconds", str(a.min_seconds)],
                               env=env, check=True, timeout=600)
        return
    for k in [int(x) for x in a.ks.split(",") if x]:
        run_shape(k, a)


if __name__ == "__main__":
    main()
