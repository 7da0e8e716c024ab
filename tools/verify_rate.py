#!/usr/bin/env python3
"""zk_verify latency and zk_verify_batch rate on one device, for the server's two shapes: k = 17 EVM + GWC (/verify_evm) and
k = 19 Blake2b + SHPLONK (/verify).  Proofs are made on the device first (distinct RNG seeds), the key is a verifying-only key
(zk_vk_from_parts of the prover's vk).  Every timed call ends in a device sync inside the engine (the verdicts come back to the
host), so host wall-clock time around it is the latency; warm-up calls come first.  Prints one JSON line per shape.

    python tools/verify_rate.py [--shapes k17,k19] [--batches 1,16,64,256] [--reps 5] [--warmup 2]

The host / device split is read from a kernel trace of the same run (rocprofv3 --kernel-trace --stats -- python tools/verify_rate.py
--shapes k17 --batches 64 --reps 1): verify_decode_kernel and verify_msm_kernel are the device part, the rest is host work
(transcripts, pairing)."""
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

SHAPES = {"k17": (zk.circuit.K17, E.ZK_TRANSCRIPT_EVM, E.ZK_SCHEME_GWC), "k19": (zk.circuit.K19, E.ZK_TRANSCRIPT_BLAKE2B, E.ZK_SCHEME_SHPLONK)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="k17,k19")
    ap.add_argument("--batches", default="1,16,64,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--proofs", type=int, default=8, help="distinct proofs made per shape (batches cycle through them)")
    a = ap.parse_args()
    eng = zk.Engine(0)
    for name in a.shapes.split(","):
        p, tr, sc = SHAPES[name]
        eng.srs_setup(p.degree, bytes(32))
        asg = zk.circuit.synthesize(p, 0x5EED0019)
        pk = eng.keygen(p, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
        adv = [eng.poly(1 << p.degree) for _ in asg.advice]
        for h, col in zip(adv, asg.advice):
            eng.upload_canonical(h, asg.to_limbs(col))
        proofs = [eng.prove(pk, adv, bytes([i + 1]) * 32, tr, sc) for i in range(a.proofs)]
        fc, pc, trr = eng.vk_export(pk)
        for h in adv:
            h.free()
        eng.pk_free(pk)  # the prover's key goes: what verifies is a verifying-only key
        vk = eng.vk_from_parts(p, fc, pc, trr)
        for _ in range(a.warmup):
            assert eng.verify(vk, proofs[0], tr, sc)
        lat = []
        for i in range(max(a.reps, 1) * 4):
            t0 = time.perf_counter()
            ok = eng.verify(vk, proofs[i % len(proofs)], tr, sc)
            lat.append(time.perf_counter() - t0)
            assert ok
        rows = {}
        for B in [int(x) for x in a.batches.split(",")]:
            batch = [proofs[i % len(proofs)] for i in range(B)]
            for _ in range(a.warmup):
                assert all(eng.verify_batch(vk, batch, tr, sc))
            ts = []
            for _ in range(max(a.reps, 1)):
                t0 = time.perf_counter()
                v = eng.verify_batch(vk, batch, tr, sc)
                ts.append(time.perf_counter() - t0)
                assert all(v)
            med = statistics.median(ts)
            rows[str(B)] = {"ms": round(med * 1e3, 3), "proofs_per_s": round(B / med, 1)}
        # one bad proof in a batch of 64: the bisection's cost
        batch = [proofs[i % len(proofs)] for i in range(64)]
        bad = bytearray(batch[31])
        bad[len(bad) // 2] ^= 1
        batch[31] = bytes(bad)
        eng.verify_batch(vk, batch, tr, sc)
        t0 = time.perf_counter()
        v = eng.verify_batch(vk, batch, tr, sc)
        one_bad = time.perf_counter() - t0
        assert v == [True] * 31 + [False] + [True] * 32
        eng.pk_free(vk)
        print(json.dumps({"shape": name, "k": p.degree, "transcript": "evm" if tr == E.ZK_TRANSCRIPT_EVM else "blake2b",
                          "scheme": "gwc" if sc == E.ZK_SCHEME_GWC else "shplonk", "proof_len": len(proofs[0]),
                          "single_ms_median": round(statistics.median(lat) * 1e3, 3), "single_ms_min": round(min(lat) * 1e3, 3),
                          "batch": rows, "b64_one_bad_ms": round(one_bad * 1e3, 3)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
