"""Generates tests/golden/yul_verdicts.json: what the reference's generated verifier program
(proving-server/P256Verifier.yul of the reference tree) decides on the two EVM proofs the suite holds,
executed by oracle/tools/yul_exec.py.  Run where the reference tree is; the output is committed data:

  python tests/golden/make_yul_verdicts.py <reference tree>/proving-server/P256Verifier.yul

  golden  the reference's golden proof (golden_proof_k17_evm.hex) under the program as it is, and with
          byte 777 flipped
  engine  the device-made proof (engine_proof_k17_evm.json) under the program with that proof's 12 vk
          commitments and transcript_repr in place of the ECDSA circuit's, under the program as it is,
          and with byte 1500 flipped; plus the Fiat-Shamir challenges the program squeezed

tests/test_oracle_verifier.py holds the oracle verifier to these verdicts on the same bytes.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "oracle", "tools")]

import yul_exec  # noqa: E402

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
NAMES = ["theta", "beta", "gamma", "y", "x", "v", "u"]


def flip(proof, pos, mask):
    bad = bytearray(proof)
    bad[pos] ^= mask
    return bytes(bad)


def main(yul):
    golden = bytes.fromhex(open(os.path.join(HERE, "golden_proof_k17_evm.hex")).read().strip())
    ok, vm = yul_exec.run_verifier(yul, golden)
    out = {"golden": {"proof_sha256": hashlib.sha256(golden).hexdigest(), "accepted": ok,
                      "precompile_calls": {str(k): v for k, v in vm.precompile_calls.items()},
                      "flip": [777, 0x10], "flipped_accepted": yul_exec.run_verifier(yul, flip(golden, 777, 0x10))[0]}}
    d = json.load(open(os.path.join(HERE, "engine_proof_k17_evm.json")))
    proof = bytes.fromhex(d["proof"])
    pts = [(int(p[0], 16), int(p[1], 16)) for p in d["fixed_commitments"] + d["permutation_commitments"]]
    key = (int(d["transcript_repr"], 16), pts)
    ok, vm = yul_exec.run_verifier(yul, proof, vk=key)
    out["engine"] = {"proof_sha256": hashlib.sha256(proof).hexdigest(), "accepted_with_its_key": ok,
                     "precompile_calls": {str(k): v for k, v in vm.precompile_calls.items()},
                     "challenges": {n: hex(h % R) for n, (_, _, h) in zip(NAMES, vm.keccak_log)},
                     "accepted_with_the_programs_key": yul_exec.run_verifier(yul, proof)[0],
                     "flip": [1500, 0x01], "flipped_accepted_with_its_key": yul_exec.run_verifier(yul, flip(proof, 1500, 1), vk=key)[0]}
    json.dump(out, open(os.path.join(HERE, "yul_verdicts.json"), "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1])
