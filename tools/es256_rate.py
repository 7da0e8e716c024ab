"""The ES256 request check on the host against zk_es256_verify on the device, with the lone k = 17 EVM proof for scale.

    python tools/es256_rate.py [--batches 1,4,64,1024,16384] [--reps 7] [--host-calls 5] [--device 0] [--no-proof]

One run measures, in this order:
  - ecdsa_p256.es256_verify (the host check) per signature: --host-calls calls in a loop, each a different valid signature;
  - zk_es256_verify wall time (call to return, staging included) per batch size, valid signatures, after one warm-up call of that
    size (the first call of the context also builds the comb table of G; that call is timed on its own), as the median of --reps calls;
  - a lone k = 17 proof with the EVM transcript (the server's configuration), the median of --reps after a warm-up.
The signatures are made here with the module's own arithmetic, a few distinct ones repeated to fill a batch (the kernel's work per
lane does not depend on what the other lanes hold).  Prints one JSON line per figure and a markdown table (docs/experiments.md)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import webauthn_halo2_amd as zk  # noqa: E402
from webauthn_halo2_amd import engine as E  # noqa: E402


def signatures(api, count):
    out = []
    for i in range(count):
        d = int.from_bytes(bytes([0x11 + i]) * 32, "big") % api._N
        kk = int.from_bytes(bytes([0x71 + i]) * 32, "big") % api._N
        z = int.from_bytes(bytes([0x31 + i]) * 32, "big") % api._N
        q, r = api._p256_mul(d, api._G), api._p256_mul(kk, api._G)[0] % api._N
        s = pow(kk, -1, api._N) * (z + r * d) % api._N
        out.append(tuple(v.to_bytes(32, "little") for v in (q[0], q[1], r, s, z)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4,64,1024,16384")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-calls", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-proof", action="store_true")
    a = ap.parse_args()
    api = zk.ecdsa_p256
    sigs = signatures(api, 16)
    rows = []

    t0 = time.perf_counter()
    for i in range(a.host_calls):
        assert api.es256_verify(*sigs[i % len(sigs)])
    host_ms = (time.perf_counter() - t0) * 1e3 / a.host_calls
    print(json.dumps({"what": "host check", "calls": a.host_calls, "ms_per_signature": host_ms}), flush=True)
    rows.append(("host check (es256_verify), per signature", 1, host_ms, host_ms))

    eng = zk.Engine(a.device)
    one = b"".join(sigs[0])
    t0 = time.perf_counter()
    assert eng.es256_verify(one)[0] == [True]
    first_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"what": "first call of a context (builds the comb table)", "ms": first_ms}), flush=True)
    rows.append(("zk_es256_verify, first call of a context (builds the table)", 1, first_ms, first_ms))
    for batch in [int(b) for b in a.batches.split(",")]:
        blob = b"".join(b"".join(sigs[j % len(sigs)]) for j in range(batch))
        assert all(eng.es256_verify(blob)[0])  # warm-up: the staging buffers grow to the batch
        times = []
        for _ in range(a.reps):
            eng.sync()
            t0 = time.perf_counter()
            eng.es256_verify(blob)
            times.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(times)
        print(json.dumps({"what": "zk_es256_verify", "batch": batch, "reps": a.reps, "median_ms": med, "ms_per_signature": med / batch,
                          "all_ms": times}), flush=True)
        rows.append(("zk_es256_verify", batch, med, med / batch))
    eng.close()

    if not a.no_proof:
        params = zk.circuit.K17
        eng = zk.Engine(a.device)
        eng.srs_setup(params.degree)
        asg = zk.circuit.synthesize(params, 0x5EED0017)
        pk = eng.keygen(params, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
        polys = []
        for col in asg.advice:
            h = eng.poly(1 << params.degree)
            eng.upload_canonical(h, asg.to_limbs(col))
            polys.append(h)
        eng.prove(pk, polys, bytes(32), E.ZK_TRANSCRIPT_EVM)
        times = []
        for _ in range(a.reps):
            eng.sync()
            t0 = time.perf_counter()
            eng.prove(pk, polys, bytes(32), E.ZK_TRANSCRIPT_EVM)
            times.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(times)
        print(json.dumps({"what": "lone proof, k = 17, EVM transcript", "reps": a.reps, "median_ms": med, "all_ms": times}), flush=True)
        rows.append(("lone proof, k = 17, EVM transcript", 1, med, med))
        eng.close()

    print("\n| what | signatures per call | wall time of a call (ms) | per signature (ms) |")
    print("|---|---|---|---|")
    for what, batch, ms, per in rows:
        print("| %s | %d | %.3f | %.4f |" % (what, batch, ms, per))


if __name__ == "__main__":
    main()
