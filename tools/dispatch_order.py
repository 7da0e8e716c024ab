"""Every kernel launch of one call in the order the host enqueued it — the check that a refactor of host code moved no
enqueue (profiles/README.md "dispatch_order").  Two halves:

  dispatch_order.py run lone|lone_public|lockstep4|multi4 [k19|k17]
      the traced program: sets up the shape (SRS, key, the advice columns uploaded once) and makes ONE zk_prove, ONE zk_prove_public
      (a key with the instance column, 3 x num_limbs exposed values), ONE zk_prove_batch of four, or ONE zk_prove_multi over four
      circuits; prints the SHA-256 of the proof(s).  k19 (the default): circuit.K19 with
      Blake2b + SHPLONK — one advice column, one lookup: the pipelined route; k17: circuit.K17 with EVM + GWC — four advice
      columns, three chained chunks: the plain route.  ZKMI355_LIB selects another build of the library; OPTS=5=2,8=2,9=2 sets
      context options before the SRS is made (zk_ctx_set_option(id, value), as tools/single_ab.py reads it): with these three the
      loaded regime — tails, transforms and MSM passes on the main stream, passes unsplit — is traced from one process.
      Run it under `rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/dispatch_order.py run lone`
      (no counters, no other tracing).
  dispatch_order.py order <kernel_trace.csv>
      the post-processing: the trace sorted by dispatch id, one line per launch: kernel, hardware queue (numbered by first
      appearance: the ids themselves differ from process to process) and grid.  Two builds launch the same work in the same
      order iff their outputs are equal line by line."""
import csv
import dataclasses
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(mode, shape="k19"):
    sys.path.insert(0, ROOT)
    import numpy as np
    import webauthn_halo2_amd as zk
    from webauthn_halo2_amd import engine as E

    if shape not in ("k19", "k17"):
        raise SystemExit(__doc__)
    p, tr = (zk.circuit.K19, E.ZK_TRANSCRIPT_BLAKE2B) if shape == "k19" else (zk.circuit.K17, E.ZK_TRANSCRIPT_EVM)
    n_public = 0
    if mode == "lone_public":
        p = dataclasses.replace(p, num_instance_columns=1)
        n_public = 3 * p.num_limbs
    eng = zk.Engine(0)
    for o in os.environ.get("OPTS", "").split(","):  # OPTS=8=2,5=1: zk_ctx_set_option(id, value)
        if o:
            eng.set_option(*[int(x) for x in o.split("=")])
    eng.srs_setup(p.degree)
    asg = zk.circuit.synthesize(p, 0x5EED0019, n_public=n_public)
    pk = eng.keygen(p, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
    hs = []
    for col in asg.advice:
        h = eng.poly(1 << p.degree)
        eng.upload_canonical(h, asg.to_limbs(col))
        hs.append(h)
    if mode == "lone":
        proofs = [eng.prove(pk, hs, bytes([1]) * 32, tr)]
    elif mode == "lone_public":
        proofs = [eng.prove_public(pk, hs, asg.to_mont_limbs(asg.instance), bytes([1]) * 32, tr)]
    elif mode == "lockstep4":
        proofs = eng.prove_batch(pk, [hs] * 4, [bytes([j + 1]) * 32 for j in range(4)], tr)
    elif mode == "multi4":
        proofs = [eng.prove_multi(pk, [hs] * 4, bytes([1]) * 32, tr)]
    else:
        raise SystemExit(__doc__)
    print(mode, shape, "opts", os.environ.get("OPTS", "-"), "library", E.lib_path(), "proofs", " ".join(hashlib.sha256(pf).hexdigest()[:16] for pf in proofs), flush=True)
    eng.close()


def kernel_name(full):
    s = full.replace("(anonymous namespace)::", "").replace("zk::", "").replace("void ", "")
    return s.split("(")[0].strip()


def order(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    queues = {}
    for r in rows:
        q = queues.setdefault(r["Queue_Id"], len(queues))
        grid = int(r["Grid_Size"]) if "Grid_Size" in r else int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
        print("%s q%d grid %d" % (kernel_name(r["Kernel_Name"]), q, grid))


if __name__ == "__main__":
    if len(sys.argv) in (3, 4) and sys.argv[1] == "run":
        run(*sys.argv[2:])
    elif len(sys.argv) == 3 and sys.argv[1] == "order":
        order(sys.argv[2])
    else:
        raise SystemExit(__doc__)
