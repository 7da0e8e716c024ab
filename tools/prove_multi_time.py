"""Signatures per second of ONE proof over N circuits (zk_prove_multi) against N x zk_prove and zk_prove_batch(N), over the same
witnesses in one run.

    python tools/prove_multi_time.py [--rows k19,k17] [--contexts 1,4] [--ns 1,2,4,8] [--reps 3] [--device 0]

Rows: k = 19 Blake2b + SHPLONK (one advice column) and k = 17 EVM + GWC (four gate columns).  For every context count C, C pipelines
of one device (shared SRS) each hold 8 witnesses; every pipeline runs the same call from its own host thread, and a figure is
(signatures proved by all pipelines) / (wall time from the common start to the last pipeline's end), the median of --reps
repetitions after one warm-up.  Prints a markdown table (docs/experiments.md) and one JSON line per figure.  Memory: N workspaces per
pipeline (~1.4 GiB each at k = 19): N = 8 on four contexts at k = 19 needs ~45 GiB."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import webauthn_halo2_amd as zk  # noqa: E402
from webauthn_halo2_amd import batch  # noqa: E402
from webauthn_halo2_amd import engine as E  # noqa: E402

ROWS = {
    "k19": (zk.circuit.K19, E.ZK_TRANSCRIPT_BLAKE2B, "k = 19 Blake2b + SHPLONK"),
    "k17": (zk.circuit.K17, E.ZK_TRANSCRIPT_EVM, "k = 17 EVM + GWC"),
}
WITNESSES = 8


def timed(pipes, fn, reps):
    """median wall seconds of fn(pipeline) run on every pipeline at once"""
    out = []
    for r in range(reps + 1):
        gate = threading.Barrier(len(pipes) + 1)
        errs = []

        def work(pl):
            try:
                gate.wait()
                fn(pl)
                pl.eng.sync()
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=work, args=(pl,)) for pl in pipes]
        for t in ths:
            t.start()
        gate.wait()
        t0 = time.perf_counter()
        for t in ths:
            t.join()
        dt = time.perf_counter() - t0
        if errs:
            raise errs[0]
        if r:  # (the first repetition warms up: workspaces, window tables, coset copies)
            out.append(dt)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="k19,k17")
    ap.add_argument("--contexts", default="1,4")
    ap.add_argument("--ns", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    ns = [int(x) for x in a.ns.split(",")]
    if max(ns) > WITNESSES:
        ap.error("at most %d circuits" % WITNESSES)
    table = []
    for row in a.rows.split(","):
        params, tr, label = ROWS[row]
        fixed, copies = batch.structure(params)
        wit = batch.synthesize_jobs(params, list(range(WITNESSES)))
        for C in [int(x) for x in a.contexts.split(",")]:
            pipes = [batch.Pipeline(a.device, params, fixed, copies, deterministic_seeds=True)]
            for _ in range(C - 1):
                pipes.append(batch.Pipeline(a.device, params, fixed, copies, deterministic_seeds=True, share_srs_with=pipes[0]))
            for pl in pipes:
                for j in range(WITNESSES):
                    pl.load(j, wit[j])
            seed = bytes(32)
            for N in ns:
                sets = lambda pl: [pl.resident[j] for j in range(N)]
                fig = {
                    "multi": timed(pipes, lambda pl: pl.eng.prove_multi(pl.pk, sets(pl), seed, tr), a.reps),
                    "single": timed(pipes, lambda pl: [pl.eng.prove(pl.pk, s, seed, tr) for s in sets(pl)], a.reps),
                    "batch": timed(pipes, lambda pl: pl.eng.prove_batch(pl.pk, sets(pl), [seed] * N, tr), a.reps),
                }
                rates = {k: C * N / v for k, v in fig.items()}
                print(json.dumps({"row": row, "contexts": C, "N": N, "seconds": fig, "signatures_per_s": rates}), flush=True)
                table.append((label, C, N, rates))
            for pl in pipes[::-1]:
                pl.close()
    print("\n| shape | contexts | N | zk_prove_multi(N) | N x zk_prove | zk_prove_batch(N) |")
    print("|---|---|---|---|---|---|")
    for label, C, N, r in table:
        print("| %s | %d | %d | %.1f | %.1f | %.1f |" % (label, C, N, r["multi"], r["single"], r["batch"]))
    print("(signatures per second)")


if __name__ == "__main__":
    main()
