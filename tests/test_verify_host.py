"""csrc/pairing.h and csrc/verifier.h on the host (tests/verify_host_check.cpp, built here with hipcc; no GPU): the BN254 pairing's
laws, the reference's golden EVM proof accepted by a real pairing — under the tau-free check, with the SRS's s_g2 — with the Yul
verifier's challenges, and the same verdicts as the oracle verifier on oracle proofs of all four transcript x scheme combinations,
intact and tampered.  The point decoding is the product's own (csrc/g1_codec.hip.h, what verify_decode_kernel calls); the multi-scalar
sums, which the product does on the device, are the test binary's own host restatement."""
import json
import os
import shutil
import subprocess

import pytest

from zkoracle import plonk, prover, srs
from zkoracle.hashes import ChaCha20Rng
from prover_shapes import DRAW_SEED, SHAPES, random_shapes
import verify_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vhc") / "verify_host_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-x", "hip", "-I", os.path.join(ROOT, "webauthn-halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "verify_host_check.cpp"), "-o", out])
    return out


def run_job(exe, shape, kind, scheme, repr_, fixed, perm, proofs):
    lines = ["shape %d %d %d %d %d %d" % (shape.k, shape.num_advice, shape.num_lookup_advice, shape.num_fixed, shape.lookup_bits,
                                          shape.idle_gate_columns),
             "kind " + kind, "scheme " + scheme, "repr " + hex(repr_), "tau " + hex(srs.TAU)]
    lines += ["fixed %s %s" % (hex(p[0]), hex(p[1])) for p in fixed]
    lines += ["perm %s %s" % (hex(p[0]), hex(p[1])) for p in perm]
    lines += ["proof " + (p.hex() or "-") for p in proofs]
    out = subprocess.run([exe, "verify"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    res = []
    for ln in out.stdout.splitlines():
        t = ln.split()
        assert t[0] == "verdict"
        d = {"ok": t[1] == "1"}
        d.update({t[i]: t[i + 1] for i in range(2, len(t) - 1, 2)})
        if "terms" in t:  # |A| |B|: the sizes of the two KZG term lists
            d["terms"] = (int(t[t.index("terms") + 1]), int(t[t.index("terms") + 2]))
        res.append(d)
    assert len(res) == len(proofs)
    return res


def test_pairing_laws(exe):
    out = subprocess.run([exe, "pairing", hex(srs.TAU)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "pairing bad 0" in out.stdout, out.stdout + out.stderr


def golden():
    d = json.load(open(os.path.join(GOLD, "vk_k17.json")))
    shape = plonk.Shape(k=17, num_advice=4, num_lookup_advice=1, num_fixed=1, lookup_bits=16)
    pt = lambda p: (int(p[0], 16), int(p[1], 16))
    proof = bytes.fromhex(open(os.path.join(GOLD, "golden_proof_k17_evm.hex")).read().strip())
    return d, shape, [pt(p) for p in d["fixed_commitments"]], [pt(p) for p in d["permutation_commitments"]], int(d["transcript_repr"], 16), proof


def test_golden_proof_accepted_by_a_pairing(exe):
    d, shape, fixed, perm, repr_, proof = golden()
    flip = json.load(open(os.path.join(GOLD, "yul_verdicts.json")))["golden"]["flip"]
    bad = []
    for pos in (5, 0x1c0 + 40, 0x3c0 + 7, 0x3c0 + 32 * 20 + 31, 0x920 + 3, len(proof) - 1):  # test_oracle_verifier's positions
        b = bytearray(proof)
        b[pos] ^= 1
        bad.append(bytes(b))
    yul = bytearray(proof)
    yul[flip[0]] ^= flip[1]
    bad += [bytes(yul), proof[:-32], proof + bytes(32), b""]
    res = run_job(exe, shape, "evm", "gwc", repr_, fixed, perm, [proof] + bad)
    assert res[0]["ok"]
    for name, val in d["golden_challenges"].items():
        assert int(res[0][name], 16) == int(val, 16), name
    assert [r["ok"] for r in res[1:]] == [False] * len(bad)


@pytest.mark.parametrize("kind,scheme", vc.COMBOS)
@pytest.mark.parametrize("name", ["k19like", "k17like"])
def test_oracle_proofs_same_verdicts(exe, name, kind, scheme):
    pk, asg = vc.oracle_key(name)
    proof = vc.oracle_proof(pk, asg, kind, scheme)
    cases = [("intact", proof)] + vc.variants(proof, pk.shape, kind, scheme)
    vk = pk.vk
    res = run_job(exe, vk.shape, kind, scheme, vk.transcript_repr, vk.fixed_commitments, vk.permutation_commitments, [c[1] for c in cases])
    want = [plonk.verify(vk, c[1], kind, scheme) for c in cases]
    assert want[0]
    assert [r["ok"] for r in res] == want, [c[0] for c, r, w in zip(cases, res, want) if r["ok"] != w]
    ok, pf = plonk.verify(vk, proof, kind, scheme, return_detail=True)
    for name_ in ("theta", "beta", "gamma", "y", "x", "v", "u") + (("shplonk_y",) if scheme == "shplonk" else ()):
        assert int(res[0][name_], 16) == pf.challenges[name_], name_


def test_idle_gate_columns_shape(exe):
    pk, asg = vc.oracle_key("idle")
    for kind, scheme in (("evm", "gwc"), ("blake2b", "shplonk")):
        proof = vc.oracle_proof(pk, asg, kind, scheme)
        vk = pk.vk
        res = run_job(exe, vk.shape, kind, scheme, vk.transcript_repr, vk.fixed_commitments, vk.permutation_commitments,
                      [proof, proof[:-1] + bytes([proof[-1] ^ 4])])
        assert [r["ok"] for r in res] == [True, plonk.verify(vk, proof[:-1] + bytes([proof[-1] ^ 4]), kind, scheme)]


def oracle_case(name):
    """(oracle proving key, advice) of a CPU-tier case: the head of the shared random draw, manycols, an adversarial layout, the
    identity-commitment key."""
    if name.startswith("rand"):
        return vc.oracle_key(random_shapes(6, DRAW_SEED)[int(name[4:])])
    if name == "manycols":
        return vc.oracle_key(SHAPES["manycols"])
    if name == "adversarial":
        import adversarial_layout as adv
        sh = plonk.Shape(8, 3, 2, 2, 5)
        fixed, copies, advice = adv.build(sh, 1234)
        return prover.keygen(prover.Circuit(sh, fixed, copies, advice)), advice
    p, asg = vc.identity_assignment()
    return prover.keygen(prover.Circuit(vc.oracle_shape(p), asg.fixed, asg.copies, asg.advice)), asg


@pytest.mark.parametrize("name", ["rand%d" % i for i in range(6)] + ["manycols", "adversarial", "identity"])
def test_shape_sweep_same_verdicts(exe, name):
    """Oracle proofs of more column shapes, intact and tampered, all four combinations: verdicts and challenges equal to the oracle
    verifier's.  The wide shapes put more than 128 terms in a KZG term list — three or more per lane of the device's
    one-wave-per-sum kernel (csrc/verify.hip), which tests/test_gpu_verify_shapes.py runs on the same shapes."""
    pk, asg = oracle_case(name)
    advice = asg if isinstance(asg, list) else asg.advice
    vk = pk.vk
    if name == "identity":
        assert vk.fixed_commitments[1] is None and all(c is not None for i, c in enumerate(vk.fixed_commitments) if i != 1)
    fixed = [c if c is not None else (0, 0) for c in vk.fixed_commitments]  # the identity, as the engine writes it
    for kind, scheme in vc.COMBOS:
        proof = prover.create_proof(pk, advice, ChaCha20Rng(b"\x17" * 32), kind, scheme)
        cases = [("intact", proof)] + vc.variants(proof, vk.shape, kind, scheme, seed=sum(map(ord, name + kind + scheme)))
        res = run_job(exe, vk.shape, kind, scheme, vk.transcript_repr, fixed, vk.permutation_commitments, [c[1] for c in cases])
        want = [plonk.verify(vk, c[1], kind, scheme) for c in cases]
        assert want[0]
        assert [r["ok"] for r in res] == want, (kind, scheme, [c[0] for c, r, w in zip(cases, res, want) if r["ok"] != w])
        ok, pf = plonk.verify(vk, proof, kind, scheme, return_detail=True)
        for ch in ("theta", "beta", "gamma", "y", "x", "v", "u") + (("shplonk_y",) if scheme == "shplonk" else ()):
            assert int(res[0][ch], 16) == pf.challenges[ch], (kind, scheme, ch)
        if name in ("rand0", "manycols"):  # A = 45 / 36 gate columns
            assert res[0]["terms"][1] > 128, res[0]["terms"]
