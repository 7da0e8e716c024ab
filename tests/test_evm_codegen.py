"""csrc/evm_codegen.h on the host (tests/evm_codegen_check.cpp, built here with hipcc; no GPU, no library): the Yul program generated
for a kind of proof, run in the oracle's interpreter (tests/yul_vm.py), accepts that kind's proofs and rejects everything else, with
the verdicts of tests/halo2_ref.py verify on the same bytes.

  the reference's key    the program for tests/golden/vk_k17.json accepts the reference's golden proof, rejects the recorded flip,
                         squeezes the recorded challenges and calls no more precompiles than the reference's own program
  the engine fixture     accepted under its own key's program, rejected under the reference key's
  every kind             N = 1 without the column, N = 1 with 9 and with 0 public inputs, N = 2 with [9, 1], N = 3 without the column,
                         at the k = 6 two-column and the k = 7 single-column shape, GWC and SHPLONK, through tests/yul_vm.py mutations
  dialect, determinism, --cost against what the interpreter counted, and the generator under the address and undefined-behaviour
  sanitizers (the stand-alone program only)."""
import functools
import json
import os
import shutil
import subprocess

import pytest

from zkoracle import srs
from zkoracle.hashes import ChaCha20Rng
import halo2_ref
import multi_cases
import multi_public_cases
import public_cases
import yul_vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "webauthn-halo2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "evm_codegen_check.cpp")
SEED = b"\x4c" * 32

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

SHAPES = ("k18like", "k19like")  # k = 6 (2, 1, 1, 6, 4) and the single-column k = 7 (1, 1, 1, 7, 6)
KINDS = {  # name: (circuits, instance counts or None = a key without the column)
    "one circuit": (1, None),
    "nine public inputs": (1, [9]),
    "the column, no value": (1, [0]),
    "two circuits, 9 and 1 inputs": (2, [9, 1]),
    "three circuits": (3, None),
}


def build(out, extra):
    # evm_codegen.h reaches the engine's headers, which name HIP types: hipcc -x hip, as tests/test_verify_multi_host.py
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-x", "hip"] + extra + ["-I", CSRC, "-I", os.path.join(ROOT, "tests"),
                                                                                                  SRC, "-o", out], stderr=subprocess.DEVNULL)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("evmgen") / "evm_codegen_check"), ["-O2"])


def description(shape, n_inst, repr_, fixed, perm, N, counts, scheme):
    lines = ["shape %d %d %d %d %d %d %d" % (tuple(shape) + (n_inst,)), "scheme " + scheme, "repr " + hex(repr_), "tau " + hex(srs.TAU),
             "circuits %d" % N, "instances " + " ".join(str(m) for m in counts)]
    lines += ["fixed %s %s" % (hex(p[0]), hex(p[1])) for p in fixed]
    lines += ["perm %s %s" % (hex(p[0]), hex(p[1])) for p in perm]
    return "\n".join(lines) + "\n"


def describe_vk(vk, N, counts, scheme):
    sh = vk.shape
    return description((sh.k, sh.num_advice, sh.num_lookup_advice, sh.num_fixed, sh.lookup_bits, sh.idle_gate_columns), getattr(sh, "n_inst", 0),
                       vk.transcript_repr, vk.fixed_commitments, vk.permutation_commitments, N, counts, scheme)


def describe_json(d, scheme="gwc"):
    pts = lambda key: [(int(p[0], 16), int(p[1], 16)) for p in d[key]]
    return description((d["k"], d.get("num_advice", 4), d.get("num_lookup_advice", 1), d.get("num_fixed", 1), d.get("lookup_bits", 16), 0), 0,
                       int(d["transcript_repr"], 16), pts("fixed_commitments"), pts("permutation_commitments"), 1, [0], scheme)


def generate(exe, desc, cost=False):
    out = subprocess.run([exe] + (["--cost"] if cost else []), input=desc, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    if cost:
        return {ln.split()[0]: int(ln.split()[1]) for ln in out.stdout.splitlines()}
    return out.stdout


load = lambda name: json.load(open(os.path.join(GOLDEN, name)))


# ---- 1, 2: the reference's key and proof, the engine fixture -------------------------------------------------------------------
def test_the_references_key_and_golden_proof(exe):
    vk, rec = load("vk_k17.json"), load("yul_verdicts.json")["golden"]
    text = generate(exe, describe_json(vk))
    proof = bytes.fromhex(open(os.path.join(GOLDEN, "golden_proof_k17_evm.hex")).read().strip())
    ok, vm = yul_vm.run(text, proof)
    assert ok and rec["accepted"]
    assert [hex(h % yul_vm.R) for _, _, h in vm.keccak_log[:7]] == list(vk["golden_challenges"].values())
    calls, theirs = vm.precompile_calls, {int(k): v for k, v in rec["precompile_calls"].items()}
    print("precompile calls", calls, "the reference program's", theirs)
    assert calls[5] == 1 and calls[8] == 1
    assert calls[6] <= theirs[6] and calls[7] <= theirs[7]
    pos, mask = rec["flip"]
    bad = bytearray(proof)
    bad[pos] ^= mask
    assert yul_vm.run(text, bytes(bad))[0] is False and rec["flipped_accepted"] is False


def test_the_engine_fixture(exe):
    d = load("engine_proof_k17_evm.json")
    proof = bytes.fromhex(d["proof"])
    assert yul_vm.run(generate(exe, describe_json(d)), proof)[0] is True
    assert yul_vm.run(generate(exe, describe_json(load("vk_k17.json"))), proof)[0] is False


# ---- 3: every kind at the smallest shapes ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name, kind):
    """(proving key, advice sets, instance lists) of the kind at the shape: halo2_ref's keys and witnesses."""
    N, counts = KINDS[kind]
    if counts is None:
        pk, asgs = multi_cases.setup(name, N)
        return pk, [a.advice for a in asgs], [[] for _ in range(N)]
    made = multi_public_cases.lanes(name, counts)
    pk = public_cases.reference_key(name, made[0][0])
    return pk, [asg.advice for asg, _ in made], [list(vals) for _, vals in made]


def ref_verdict(vk, proof, instances, scheme):
    try:
        return halo2_ref.verify(vk, proof, instances, "evm", scheme)
    except ValueError:  # a value not below the modulus, a list the column cannot hold: halo2's error, no proof is accepted
        return False


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", SHAPES)
def test_every_kind_with_the_references_verdicts(exe, name, kind, scheme):
    pk, advs, instances = case(name, kind)
    vk, N = pk.vk, len(advs)
    counts = [len(v) for v in instances]
    proof = halo2_ref.create_proof(pk, advs, instances, ChaCha20Rng(SEED), "evm", scheme)
    text = generate(exe, describe_vk(vk, N, counts, scheme))
    ok, vm = yul_vm.run(text, yul_vm.calldata(instances, proof))
    assert ok is True and halo2_ref.verify(vk, proof, instances, "evm", scheme) is True
    assert (vm.precompile_calls[5], vm.precompile_calls[8]) == (1, 1)
    muts = yul_vm.mutations(vk.shape, N, scheme, instances, proof)
    assert len(muts) == (16 if any(counts) else 14)
    for what, lists, bad in muts:
        got = yul_vm.run(text, yul_vm.calldata(lists, bad))[0]
        assert got is False and ref_verdict(vk, bad, lists, scheme) is False, what
    for other in (N - 1, N + 1):  # the proof read under another circuit count
        if other == 0:
            continue
        lists = (instances + [[]])[:other]
        prog = generate(exe, describe_vk(vk, other, [len(v) for v in lists], scheme))
        assert yul_vm.run(prog, yul_vm.calldata(lists, proof))[0] is False and ref_verdict(vk, proof, lists, scheme) is False, other


# ---- 4: dialect, determinism, cost ------------------------------------------------------------------------------------------------
def all_descriptions():
    out = [describe_json(load("vk_k17.json")), describe_json(load("engine_proof_k17_evm.json"))]
    for name in SHAPES:
        for kind, (N, counts) in KINDS.items():
            vk = case(name, kind)[0].vk
            for scheme in ("gwc", "shplonk"):
                out.append(describe_vk(vk, N, counts or [0] * N, scheme))
    return out


def test_dialect_determinism_and_cost(exe):
    for desc in all_descriptions():
        text = generate(exe, desc)
        assert generate(exe, desc) == text
        assert text.startswith("//") and 'object "Runtime"' in text
        called, defined = yul_vm.called_names(text)
        assert called <= set(yul_vm.BUILTINS) | defined, called - set(yul_vm.BUILTINS) - defined
        assert "not" not in called and not (defined & set(yul_vm.BUILTINS))
        cost = generate(exe, desc, cost=True)
        assert cost == yul_vm.header_cost(text)
        # what a run does: the program is straight-line, so any calldata of the right length takes every call
        _, vm = yul_vm.run(text, bytes(cost["calldata_bytes"]))
        assert yul_vm.counted(vm) == {k: cost[k] for k in ("modexp", "ecadd", "ecmul", "pairing", "keccak_calls", "keccak_bytes")}
        assert cost["modexp"] == 1 and cost["pairing"] == 1


def test_a_kind_the_engine_does_not_have_is_refused(exe):
    vk = case("k18like", "one circuit")[0].vk
    for N, counts in ((1, [1]), (0, []), (2, [0])):  # a value without the column; no circuit; fewer counts than circuits
        out = subprocess.run([exe], input=describe_vk(vk, N, counts, "gwc"), capture_output=True, text=True)
        assert out.returncode == 2 and out.stdout == ""


# ---- 5: the generator under the sanitizers ------------------------------------------------------------------------------------------
def test_generator_under_address_and_undefined_sanitizers(exe, tmp_path):
    san = build(str(tmp_path / "evm_codegen_check_san"),
                ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"])
    for desc in all_descriptions():
        assert generate(san, desc) == generate(exe, desc)
        assert generate(san, desc, cost=True) == generate(exe, desc, cost=True)
