#!/usr/bin/env python3
"""Generates tests/golden/multi_public_proofs.json: ONE proof over two circuits of the k10batched shape of tests/prover_shapes.py
with the instance column - lists of 9 and 1 values - made by tests/halo2_ref.py (the plain-Python statement of the multi
rule with public inputs) under both reference pairings.  tests/test_gpu_prove_multi_public.py makes the same key and witnesses on
the device - at k = 10 the commitments go through the column-batched MSM passes and the batched transforms - and compares
zk_prove_multi_public's bytes; tests/test_gpu_verify_public_forms.py verifies them.  The fixture keeps the Python prover out of
the tests' run time.

Run in the build container:  python tests/golden/make_multi_public_proofs.py
Only expected outputs are stored (instance lists, transcript_repr, proof hex); the inputs are regenerated from the seeds by the test."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from zkoracle.hashes import ChaCha20Rng  # noqa: E402
import halo2_ref  # noqa: E402
from multi_public_cases import lanes  # noqa: E402  (witness generator only; no engine is touched)
from public_cases import PAIRINGS, SEED, reference_key  # noqa: E402

NAME, LENGTHS = "k10batched", (9, 1)


def main():
    made = lanes(NAME, LENGTHS)
    pk = reference_key(NAME, made[0][0])
    lists = [vals for _, vals in made]
    out = {"shape": NAME, "lengths": list(LENGTHS), "instances": [[hex(v) for v in l] for l in lists],
           "transcript_repr": hex(pk.vk.transcript_repr), "proofs": {}}
    for kind, scheme in PAIRINGS:
        proof = halo2_ref.create_proof(pk, [a.advice for a, _ in made], lists, ChaCha20Rng(SEED), kind, scheme)
        assert halo2_ref.verify(pk.vk, proof, lists, kind, scheme)
        assert len(proof) == halo2_ref.proof_size(pk.shape, len(lists), kind, scheme)
        out["proofs"][kind + "/" + scheme] = proof.hex()
        print("%s / %s  %d bytes" % (kind, scheme, len(proof)), flush=True)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "multi_public_proofs.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
