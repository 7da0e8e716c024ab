#!/usr/bin/env python3
"""Generates tests/golden/public_proofs.json: the k10batched shape of tests/prover_shapes.py with the instance column, nine public
inputs, proven by tests/halo2_ref.py (the plain-Python statement of the public-input rule) under both reference pairings.
tests/test_gpu_prove_public.py makes the same key and witness on the device - at k = 10 the commitments go through the
column-batched MSM passes and the batched transforms - and compares zk_prove_public's bytes; tests/test_gpu_verify_public.py
verifies them.  The fixture keeps the Python prover out of the tests' run time.

Run in the build container:  python tests/golden/make_public_proofs.py
Only expected outputs are stored (instances, transcript_repr, proof hex); the inputs are regenerated from the seeds by the test."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from zkoracle.hashes import ChaCha20Rng  # noqa: E402
import halo2_ref  # noqa: E402
from public_cases import PAIRINGS, SEED, reference_key, witness  # noqa: E402  (witness generator only; no engine is touched)

NAME, N_PUBLIC = "k10batched", 9


def main():
    asg = witness(NAME, N_PUBLIC)
    pk = reference_key(NAME, asg)
    out = {"shape": NAME, "n_public": N_PUBLIC, "instances": [hex(v) for v in asg.instance], "transcript_repr": hex(pk.vk.transcript_repr),
           "proofs": {}}
    for kind, scheme in PAIRINGS:
        proof = halo2_ref.create_proof(pk, [asg.advice], [asg.instance], ChaCha20Rng(SEED), kind, scheme)
        assert halo2_ref.verify(pk.vk, proof, [asg.instance], kind, scheme) and len(proof) == halo2_ref.proof_size(pk.shape, 1, kind, scheme)
        out["proofs"][kind + "/" + scheme] = proof.hex()
        print("%s / %s  %d bytes" % (kind, scheme, len(proof)), flush=True)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "public_proofs.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
