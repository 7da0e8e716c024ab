"""The WebAuthn assertion check by its three routes: the host route (ecdsa_p256.webauthn_verify), zk_webauthn_verify on the device,
and - the yardstick, in the same run - zk_es256_verify of the same count: the new call is that one plus two hashes, the byte rules
and a DER parse per lane, a second launch and a larger upload.

    python tools/webauthn_rate.py [--batches 1,64,1024,16384] [--reps 5] [--host-max 64] [--device 0]

Per batch size: the median wall time (call to return, staging included) of --reps calls after one warm-up call of that size, with
typical sizes (authenticatorData of 37 bytes, clientDataJSON of about 130); and one row with every assertion at the caps (1024 and
4096 bytes) at the largest batch size.  The host route is a Python loop of about 6 ms per assertion: it is timed up to --host-max
assertions per call and marked "extrapolated" (per-assertion time of the largest timed call x count) beyond.  The assertions are
made here with the module's own arithmetic, 16 distinct ones repeated to fill a batch (a lane's work does not depend on what the
other lanes hold).  Prints one JSON line per figure and a markdown table (docs/experiments.md)."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import webauthn_halo2_amd as zk  # noqa: E402

ORIGIN, RP_ID = "https://login.example.com", "login.example.com"


def der(r, s):
    def integer(v):
        b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
        return bytes([0x02, len(b) + (b[0] >> 7)]) + (b"\x00" if b[0] & 0x80 else b"") + b
    body = integer(r) + integer(s)
    return bytes([0x30, len(body)]) + body


def assertions(api, count, ad_len=37, cd_len=None):
    """`count` valid assertions (dicts as Engine.webauthn_verify takes them); cd_len: clientDataJSON lengthened to that by a trailing
    member."""
    out = []
    for i in range(count):
        d = int.from_bytes(bytes([0x11 + i]) * 32, "big") % api._N
        kk = int.from_bytes(bytes([0x71 + i]) * 32, "big") % api._N
        challenge = hashlib.sha256(b"challenge %d" % i).digest()
        ad = hashlib.sha256(RP_ID.encode()).digest() + bytes([0x05]) + (1000 + i).to_bytes(4, "big") + bytes(0x80 + j % 0x80 for j in range(ad_len - 37))
        cd = api.webauthn_expected_prefix(challenge, ORIGIN) + b"false"
        cd += b"}" if cd_len is None else b',"x":"' + b"y" * (cd_len - len(cd) - 8) + b'"}'
        z = int.from_bytes(hashlib.sha256(ad + hashlib.sha256(cd).digest()).digest(), "big")
        q, r = api._p256_mul(d, api._G), api._p256_mul(kk, api._G)[0] % api._N
        s = pow(kk, -1, api._N) * (z + r * d) % api._N
        out.append({"authenticator_data": ad, "client_data_json": cd, "signature": der(r, s), "pubkey_x": q[0].to_bytes(32, "big"),
                    "pubkey_y": q[1].to_bytes(32, "big"), "challenge": challenge, "origin": ORIGIN,
                    "rp_id_hash": hashlib.sha256(RP_ID.encode()).digest(), "flags_required": 0x05, "allow_cross_origin": False})
    return out


def host_call(api, qs):
    return [api.webauthn_verify(q["authenticator_data"], q["client_data_json"], q["signature"], q["pubkey_x"], q["pubkey_y"], q["challenge"],
                                q["origin"], q["rp_id_hash"], q["flags_required"], q["allow_cross_origin"]) for q in qs]


def median_ms(fn, reps, before=None):
    times = []
    for _ in range(reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,1024,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-max", type=int, default=64)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    api = zk.ecdsa_p256
    batches = [int(b) for b in a.batches.split(",")]
    typical, capped = assertions(api, 16), assertions(api, 16, ad_len=1024, cd_len=4096)
    print(json.dumps({"what": "sizes", "typical": [len(typical[0]["authenticator_data"]), len(typical[0]["client_data_json"])],
                      "caps": [len(capped[0]["authenticator_data"]), len(capped[0]["client_data_json"])]}), flush=True)
    eng = zk.Engine(a.device)
    first = time.perf_counter()
    ok, _, records, _ = eng.webauthn_verify(typical)
    first_ms = (time.perf_counter() - first) * 1e3
    assert all(ok)
    print(json.dumps({"what": "first call of a context (builds the comb table)", "assertions": 16, "ms": first_ms}), flush=True)
    rows = []
    host_per = None
    for kind, pool in (("typical", typical), ("caps", capped)):
        for batch in (batches if kind == "typical" else batches[-1:]):
            qs = [pool[j % len(pool)] for j in range(batch)]
            if batch <= a.host_max:
                host_ms, _ = median_ms(lambda: host_call(api, qs), a.reps)
                host_per, host_note = host_ms / batch, "timed"
            else:
                if host_per is None:
                    host_per = median_ms(lambda: host_call(api, qs[:a.host_max]), a.reps)[0] / min(batch, a.host_max)
                host_ms, host_note = host_per * batch, "extrapolated"
            packed = eng.webauthn_pack(qs)  # (marshalled once: the timed call is the library's, like es256_verify's of one blob)
            assert all(eng.webauthn_verify(packed)[0])  # warm-up: the staging buffers grow to the batch
            dev_ms, dev_all = median_ms(lambda: eng.webauthn_verify(packed), a.reps, eng.sync)
            blob = b"".join(records[j % len(records)] for j in range(batch))
            assert all(eng.es256_verify(blob)[0])
            es_ms, es_all = median_ms(lambda: eng.es256_verify(blob), a.reps, eng.sync)
            print(json.dumps({"what": kind, "batch": batch, "reps": a.reps, "host_ms": host_ms, "host": host_note, "zk_webauthn_verify_ms": dev_ms,
                              "zk_es256_verify_ms": es_ms, "webauthn_all_ms": dev_all, "es256_all_ms": es_all}), flush=True)
            rows.append((kind, batch, host_ms, host_note, dev_ms, es_ms))
        host_per = None
    eng.close()
    print("\n| sizes | assertions per call | host route (ms) | zk_webauthn_verify (ms) | zk_es256_verify, same count (ms) | difference (ms) |")
    print("|---|---|---|---|---|---|")
    for kind, batch, host_ms, note, dev_ms, es_ms in rows:
        print("| %s | %d | %.1f%s | %.3f | %.3f | %.3f |" % (kind, batch, host_ms, "" if note == "timed" else " (extrapolated)", dev_ms, es_ms, dev_ms - es_ms))


if __name__ == "__main__":
    main()
