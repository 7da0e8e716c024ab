"""The WebAuthn registration check by its routes: the host route (ecdsa_p256.webauthn_register), zk_webauthn_register on the device,
and - the yardstick, in the same run - zk_webauthn_verify of the same count: the new call is that one plus the CBOR walk, the
credential rules and the key's curve test per lane, with a larger upload (the object holds authData and the statement).

    python tools/webauthn_register_rate.py [--batches 1,64,1024,16384] [--reps 5] [--host-max 64] [--device 0]

Per batch size: the median wall time of the library call (call to return, staging included, every output asked for; Engine's
unpacking of the results into Python lists is not timed, for either call) of --reps calls after one warm-up call of that size, at a
typical size (packed self attestation, a credential id of 32 bytes: an object of about 280 bytes, clientDataJSON of about 130) and
with every registration at the caps (an object of 8192 bytes, its extension map filled up, and clientDataJSON of 4096).  Every
registration is self-attested and checked under ZK_WEBAUTHN_ATT_NONE_OR_SELF, so every lane hashes and verifies a signature, like
an assertion's; a row under ZK_WEBAUTHN_ATT_IGNORE (no hash, no curve verification) follows at the largest batch.  The host route is
a Python loop of several ms per registration: it is timed up to --host-max per call and marked "extrapolated" beyond.  The
registrations are made here with the module's own arithmetic, 16 distinct ones repeated to fill a batch (a lane's work does not
depend on what the other lanes hold).  Prints one JSON line per figure and a markdown table (docs/experiments.md)."""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import webauthn_halo2_amd as zk  # noqa: E402
from webauthn_rate import ORIGIN, RP_ID, assertions, der, median_ms  # noqa: E402


def bstr(b):
    n = len(b)
    return (bytes([0x40 | n]) if n < 24 else bytes([0x58, n]) if n < 256 else bytes([0x59]) + n.to_bytes(2, "big")) + b


def registrations(api, count, object_len=None, cd_len=None, policy=1):
    """`count` self-attested registrations (dicts as Engine.webauthn_register takes them); object_len: the object filled up to that
    by an extension map {0: <bytes>}; cd_len: clientDataJSON lengthened to that by a trailing member."""
    out = []
    for i in range(count):
        d = int.from_bytes(bytes([0x11 + i]) * 32, "big") % api._N
        kk = int.from_bytes(bytes([0x71 + i]) * 32, "big") % api._N
        challenge = hashlib.sha256(b"challenge %d" % i).digest()
        cd = api.webauthn_expected_prefix(challenge, ORIGIN, b"webauthn.create") + b"false"
        cd += b"}" if cd_len is None else b',"x":"' + b"y" * (cd_len - len(cd) - 8) + b'"}'
        q, r = api._p256_mul(d, api._G), api._p256_mul(kk, api._G)[0] % api._N
        key = bytes.fromhex("a5010203262001215820") + q[0].to_bytes(32, "big") + bytes.fromhex("225820") + q[1].to_bytes(32, "big")
        fill = None if object_len is None else object_len - 400
        for t in range(200):  # (the signature's length moves with s: the filler is searched, its bytes moving with the try)
            ext = b"" if fill is None else b"\xa1\x00" + bstr(bytes(0x80 + (j + t) % 0x80 for j in range(fill)))
            ad = (hashlib.sha256(RP_ID.encode()).digest() + bytes([0x45 | (0x80 if ext else 0)]) + (1000 + i).to_bytes(4, "big")
                  + hashlib.sha256(b"aaguid").digest()[:16] + (32).to_bytes(2, "big") + hashlib.sha256(b"id %d" % i).digest() + key + ext)
            z = int.from_bytes(hashlib.sha256(ad + hashlib.sha256(cd).digest()).digest(), "big")
            s = pow(kk, -1, api._N) * (z + r * d) % api._N
            obj = b"\xa3\x63fmt\x66packed\x67attStmt\xa2\x63alg\x26\x63sig" + bstr(der(r, s)) + b"\x68authData" + bstr(ad)
            if fill is None or len(obj) == object_len:
                break
            fill += object_len - len(obj) if abs(object_len - len(obj)) > 2 else (1 if len(obj) < object_len else -1)
        else:
            raise AssertionError("no object of %d bytes" % object_len)
        out.append({"attestation_object": obj, "client_data_json": cd, "challenge": challenge, "origin": ORIGIN,
                    "rp_id_hash": hashlib.sha256(RP_ID.encode()).digest(), "flags_required": 0x05, "allow_cross_origin": False,
                    "attestation_policy": policy})
    return out


def host_call(api, qs):
    return [api.webauthn_register(q["attestation_object"], q["client_data_json"], q["challenge"], q["origin"], q["rp_id_hash"], q["flags_required"],
                                  q["allow_cross_origin"], q["attestation_policy"]) for q in qs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,1024,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-max", type=int, default=64)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    api = zk.ecdsa_p256
    batches = [int(b) for b in a.batches.split(",")]
    typical, capped = registrations(api, 16), registrations(api, 16, object_len=8192, cd_len=4096)
    asserted = {"typical": assertions(api, 16), "caps": assertions(api, 16, ad_len=1024, cd_len=4096)}
    assert all(v[0] for v in host_call(api, typical[:2] + capped[:2]))
    print(json.dumps({"what": "sizes", "typical": [len(typical[0]["attestation_object"]), len(typical[0]["client_data_json"])],
                      "caps": [len(capped[0]["attestation_object"]), len(capped[0]["client_data_json"])]}), flush=True)
    eng = zk.Engine(a.device)
    first = time.perf_counter()
    got = eng.webauthn_register(typical)
    first_ms = (time.perf_counter() - first) * 1e3
    assert all(g[0] and g[2]["attestation"] == 1 for g in got)
    print(json.dumps({"what": "first call of a context (builds the comb table)", "registrations": 16, "ms": first_ms}), flush=True)
    rows = []
    for kind, pool in (("typical", typical), ("caps", capped)):
        host_per = None
        for batch in batches:
            qs = [pool[j % len(pool)] for j in range(batch)]
            if batch <= a.host_max:
                host_ms, _ = median_ms(lambda: host_call(api, qs), a.reps)
                host_per, host_note = host_ms / batch, "timed"
            else:
                if host_per is None:
                    host_per = median_ms(lambda: host_call(api, qs[:a.host_max]), a.reps)[0] / min(batch, a.host_max)
                host_ms, host_note = host_per * batch, "extrapolated"
            packed = eng.webauthn_register_pack(qs)  # (marshalled once: the timed call is the library's)
            assert all(g[0] for g in eng.webauthn_register(packed))  # warm-up: the staging buffers grow to the batch
            # both calls as the library's own, with every output asked for (Engine's unpacking into Python lists is not timed)
            verdicts, reasons, creds = (ctypes.c_uint8 * batch)(), (ctypes.c_uint8 * batch)(), (zk.engine.WebauthnCredentialC * batch)()
            reg_ms, reg_all = median_ms(lambda: eng._chk(eng.L.zk_webauthn_register(eng.ctx, batch, packed, verdicts, reasons, creds),
                                                         "zk_webauthn_register"), a.reps, eng.sync)
            assert all(verdicts)
            apacked = eng.webauthn_pack([asserted[kind][j % 16] for j in range(batch)])
            assert all(eng.webauthn_verify(apacked)[0])
            records, counts = (ctypes.c_uint8 * (160 * batch))(), (ctypes.c_uint32 * batch)()
            ver_ms, ver_all = median_ms(lambda: eng._chk(eng.L.zk_webauthn_verify(eng.ctx, batch, apacked, verdicts, reasons, records, counts),
                                                         "zk_webauthn_verify"), a.reps, eng.sync)
            assert all(verdicts)
            print(json.dumps({"what": kind, "batch": batch, "reps": a.reps, "host_ms": host_ms, "host": host_note, "zk_webauthn_register_ms": reg_ms,
                              "zk_webauthn_verify_ms": ver_ms, "register_all_ms": reg_all, "verify_all_ms": ver_all}), flush=True)
            rows.append((kind, batch, host_ms, host_note, reg_ms, ver_ms))
    # the same objects with the statement not judged: the walk and the rules alone, no hash and no curve verification
    batch = batches[-1]
    ignored = []
    for kind, pool in (("typical", typical), ("caps", capped)):
        packed = eng.webauthn_register_pack([dict(pool[j % len(pool)], attestation_policy=0) for j in range(batch)])
        assert all(g[0] and g[2]["attestation"] == 2 for g in eng.webauthn_register(packed))
        verdicts, reasons, creds = (ctypes.c_uint8 * batch)(), (ctypes.c_uint8 * batch)(), (zk.engine.WebauthnCredentialC * batch)()
        ms, every = median_ms(lambda: eng._chk(eng.L.zk_webauthn_register(eng.ctx, batch, packed, verdicts, reasons, creds), "zk_webauthn_register"),
                              a.reps, eng.sync)
        print(json.dumps({"what": kind + ", statement not judged", "batch": batch, "zk_webauthn_register_ms": ms, "all_ms": every}), flush=True)
        ignored.append((kind, batch, ms))
    eng.close()
    print("\n| sizes | registrations per call | host route (ms) | zk_webauthn_register (ms) | zk_webauthn_verify, same count (ms) | difference (ms) |")
    print("|---|---|---|---|---|---|")
    for kind, batch, host_ms, note, reg_ms, ver_ms in rows:
        print("| %s | %d | %.1f%s | %.3f | %.3f | %.3f |" % (kind, batch, host_ms, "" if note == "timed" else " (extrapolated)", reg_ms, ver_ms, reg_ms - ver_ms))
    for kind, batch, ms in ignored:
        print("| %s, statement not judged | %d | | %.3f | | |" % (kind, batch, ms))


if __name__ == "__main__":
    main()
