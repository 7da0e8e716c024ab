"""examples/prove_host_phases_multi.cpp - a host that owns the transcript, the ChaCha20 stream and the blinding and builds ONE proof
over N circuits, with their public inputs, from the phase-level C ABI alone (beside prove_host_phases' calls:
zk_permutation_product_public, zk_quotient_multi, zk_eval_batch) - run as a process of its own.  Its bytes are the whole-proof
calls' for the same key, advice, lists and seed:

  public        N = 1 with 9 public inputs                          zk_prove_public
  multi         N = 3 on a key without the instance column          zk_prove_multi
  multi-public  N = 2 and 3 with lists of 9, 0 (and 1) values       zk_prove_multi_public

on k19like (the column joins a permutation chunk), k17like (it opens one) and wide (two lookups, two constants columns) with the
reference's two pairings (EVM + GWC, Blake2b + SHPLONK), on k17like with the two crossed ones as well; and every proof is accepted
by zk_verify_public / zk_verify_multi / zk_verify_multi_public."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import webauthn_halo2_amd as zk  # noqa: E402
from webauthn_halo2_amd import engine as E  # noqa: E402
import multi_cases  # noqa: E402
from multi_public_cases import engine_lanes, lanes  # noqa: E402
from public_cases import COMBOS, PAIRINGS, SEED, params_of  # noqa: E402

HOST = os.path.join(ROOT, "examples", "prove_host_phases_multi")
pytestmark = pytest.mark.gpu

KIND = {"evm": E.ZK_TRANSCRIPT_EVM, "blake2b": E.ZK_TRANSCRIPT_BLAKE2B}
SCHEME = {"gwc": E.ZK_SCHEME_GWC, "shplonk": E.ZK_SCHEME_SHPLONK}
FORMS = {"public": (9,), "multi": None, "multi-public-2": (9, 0), "multi-public-3": (9, 0, 1)}
CASES = [(form, name, kind, scheme) for form in FORMS for name in ("k19like", "k17like", "wide")
         for kind, scheme in (COMBOS if name == "k17like" else PAIRINGS)]
HOST_TIMEOUT = 120  # seconds: a k = 8 proof with its process start, SRS and key read takes a few


@pytest.mark.parametrize("form,name,kind,scheme", CASES, ids=["-".join(c) for c in CASES])
def test_phase_level_host_proves_what_the_whole_proof_calls_prove(tmp_path, form, name, kind, scheme):
    assert os.path.exists(HOST), "examples/prove_host_phases_multi is built by build.sh / __graft_entry__.build()"
    eng = zk.Engine(0)
    t, s = KIND[kind], SCHEME[scheme]
    if form == "multi":  # three circuits, no instance column
        asgs = multi_cases.witnesses(name, 3)
        p = multi_cases.params_of(name)
        pk, sets = multi_cases.engine_key(eng, name, asgs)
        lists = [[], [], []]
        want = eng.prove_multi(pk, sets, SEED, t, s)
        verify = lambda proof: eng.verify_multi(pk, 3, proof, t, s)
    else:
        made = lanes(name, FORMS[form])
        asgs, lists = [a for a, _ in made], [v for _, v in made]
        p = params_of(name)
        pk, sets, mlists = engine_lanes(eng, name, made)
        if form == "public":
            want = eng.prove_public(pk, sets[0], mlists[0], SEED, t, s)
            verify = lambda proof: eng.verify_public(pk, proof, mlists[0], t, s)
        else:
            want = eng.prove_multi_public(pk, sets, mlists, SEED, t, s)
            verify = lambda proof: eng.verify_multi_public(pk, proof, mlists, t, s)
    N = len(asgs)
    (tmp_path / "srs.bin").write_bytes(eng.srs_write(E.ZK_SERDE_RAW_BYTES))
    (tmp_path / "pk.bin").write_bytes(eng.pk_write(pk, E.ZK_SERDE_RAW_BYTES))
    cols = np.stack([asg.to_limbs(c) for asg in asgs for c in asg.advice])
    (tmp_path / "advice.bin").write_bytes(np.ascontiguousarray(cols, dtype="<u8").tobytes())
    (tmp_path / "instances.bin").write_bytes(b"".join(
        struct.pack("<Q", len(v)) + (zk.circuit.Assignment.to_limbs(v).astype("<u8").tobytes() if v else b"") for v in lists))
    out = tmp_path / "proof.bin"
    r = subprocess.run([HOST, str(tmp_path / "srs.bin"), str(tmp_path / "pk.bin"), str(tmp_path / "advice.bin"),
                        str(tmp_path / "instances.bin"), str(out), str(p.degree), str(p.num_advice), str(p.num_lookup_advice),
                        str(p.num_fixed), str(p.lookup_bits), str(p.idle_gate_columns), str(p.num_instance_columns), str(N), kind,
                        SEED.hex(), scheme], capture_output=True, text=True, timeout=HOST_TIMEOUT)
    assert r.returncode == 0, r.stderr
    calls = re.search(r"(\d+) ABI calls for the proof", r.stderr)
    assert calls, r.stderr
    print("%s %s %s/%s N=%d: %s ABI calls" % (form, name, kind, scheme, N, calls.group(1)))
    got = out.read_bytes()
    assert got == want
    assert verify(got)
    eng.close()
