"""Times zk_pk_check beside the two calls that make the key it audits, per shape (the k = 17 server shape and k = 19 by default), one
JSON line per shape: the first check of a key (state made), a clean check, a check with one planted finding (one element of a
sigma coset changed through the file route), and — in the same run — zk_keygen and zk_pk_read of the same key.  Every clock is
the host's around calls that end synchronised; warm-up first; median, min and max.

    python tools/pk_check_time.py [--ks 17,19] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(statistics.median(ts), 2), "ms_min": round(min(ts), 2), "ms_max": round(max(ts), 2)}


def sigma_coset_offset(lay_n, n_fix, n_perm, n_sel, column, index):
    """Byte offset of element `index` of sigma coset `column` in a RawBytes ProvingKey::write image."""
    n, N = lay_n, 4 * lay_n
    vk = 8 + (n_fix + n_perm) * 64 + n_sel * (n // 8)
    fixed = 2 * (4 + n_fix * (4 + n * 32)) + (4 + n_fix * (4 + N * 32))
    sigma = 2 * (4 + n_perm * (4 + n * 32))
    return vk + 3 * (4 + N * 32) + fixed + sigma + 4 + column * (4 + N * 32) + 4 + index * 32


def run_shape(k, a):
    import numpy as np

    import webauthn_halo2_amd as zk
    from webauthn_halo2_amd import engine as E

    p = {17: zk.circuit.K17, 19: zk.circuit.K19}[k]
    asg = zk.circuit.synthesize(p, 0x5EED0019)
    fixed = np.stack([asg.to_limbs(c) for c in asg.fixed])
    eng = zk.Engine(0)
    eng.srs_setup(k)
    eng.sync()
    keys = []

    def keygen():
        keys.append(eng.keygen(p, fixed, asg.copies))
        while len(keys) > 1:
            eng.pk_free(keys.pop(0))

    t_keygen = timed(keygen, a.reps)
    pk = keys[0]
    t0 = time.perf_counter()
    first = eng.pk_check(pk)
    t_first = (time.perf_counter() - t0) * 1e3
    assert first == (E.ZK_PK_CHECK_ALL | E.ZK_PK_CHECK_REPR, []), first
    t_clean = timed(lambda: eng.pk_check(pk), a.reps)
    img = eng.pk_write(pk, E.ZK_SERDE_RAW_BYTES)
    read = []

    def pk_read():
        read.append(eng.pk_read(p, img, E.ZK_SERDE_RAW_BYTES))
        while len(read) > 1:
            eng.pk_free(read.pop(0))

    t_read = timed(pk_read, a.reps)
    eng.pk_free(read.pop())
    shape = eng.pk_shape(pk)
    n, n_perm = 1 << k, shape["n_perm"]
    n_sel = p.num_advice + (1 if p.num_advice == 1 else 0)
    col, idx = n_perm - 1, 4 * n - 1
    off = sigma_coset_offset(n, shape["n_fixed"], n_perm, n_sel, col, idx)
    assert off + 32 == img.size
    img[off] ^= 1
    bad = eng.pk_read(p, img, E.ZK_SERDE_RAW_BYTES)
    want = (E.ZK_PK_CHECK_ALL & ~E.ZK_PK_CHECK_COSETS | E.ZK_PK_CHECK_REPR, [(E.ZK_PK_PART_SIGMA_COSET, col, idx, 1)])
    assert eng.pk_check(bad) == want, eng.pk_check(bad)
    t_planted = timed(lambda: eng.pk_check(bad), a.reps)
    print(json.dumps({"k": k, "columns": {"fixed": shape["n_fixed"], "permutation": n_perm}, "key_image_MiB": round(img.size / 2**20, 1),
                      "pk_check_first_ms": round(t_first, 2), "pk_check_clean": t_clean, "pk_check_one_planted_finding": t_planted,
                      "zk_keygen": t_keygen, "zk_pk_read": t_read,
                      "ratio_check_to_keygen": round(t_clean["ms_median"] / t_keygen["ms_median"], 3),
                      "ratio_check_to_pk_read": round(t_clean["ms_median"] / t_read["ms_median"], 3)}), flush=True)
    eng.pk_free(bad)
    eng.pk_free(pk)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="17,19")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for k in [int(x) for x in a.ks.split(",") if x]:
        run_shape(k, a)


if __name__ == "__main__":
    main()
