"""zk_evm_verifier (csrc/evm_codegen.h behind the C ABI): the Yul program Engine.evm_verifier generates for a kind of proof, run in
the oracle's interpreter (tests/yul_vm.py), on DEVICE-made proofs with the EVM transcript - it accepts the intact proof, and on
every mutation of tests/yul_vm.py mutations and under another circuit count it says what eng.verify* says of the same bytes:
rejected.  Seed-0 SRS, so the interpreter's pairing stand-in applies; the updated-SRS case runs a true pairing (tests/pairing_ref.py).

  shapes   k19like (one column; the instance column joins a permutation chunk), k17like (with the instance column: a chunk of its
           own), wide (two lookups, two constants columns), idle (combined selectors q (2 - q) / q (1 - q))
  forms    prove, prove_public (9 values), prove_multi over 2 and 3 circuits, prove_multi_public (9 and 1 values), GWC and SHPLONK
  also     a verifying-only key gives the proving key's bytes; out = NULL gives the length; the refusals leave the outputs
           untouched; a program made before zk_srs_update rejects what the one made after it accepts; ecdsa_p256.generate_verifier
           and proving_server.generate_evm_verifier at degree 10 - a row handed to _config_for through ECDSA_CONFIG, the smallest
           at which the request path runs (tests/test_gpu_server_public_forms.py uses the same)"""
import ctypes
import json

import numpy as np
import pytest

import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
import multi_cases
import yul_vm
from multi_public_cases import engine_lanes, lanes
from public_cases import mont, params_of, shape_of

pytestmark = pytest.mark.gpu

SEED = b"\x5d" * 32
EVM = E.ZK_TRANSCRIPT_EVM
SCHEME = {"gwc": E.ZK_SCHEME_GWC, "shplonk": E.ZK_SCHEME_SHPLONK}
FORMS = {  # name: (circuits, instance counts or None = a key without the column)
    "prove": (1, None),
    "prove_public": (1, [9]),
    "prove_multi over 2": (2, None),
    "prove_multi over 3": (3, None),
    "prove_multi_public": (2, [9, 1]),
}


def resident(eng, name, form):
    """(key, advice sets, integer instance lists, halo2 shape) of the form at the shape, resident on `eng`."""
    N, counts = FORMS[form]
    if counts is None:
        pk, sets = multi_cases.engine_key(eng, name, multi_cases.witnesses(name, N))
        return pk, sets, [[] for _ in range(N)], shape_of(name, 0)
    made = lanes(name, counts)
    pk, sets, _ = engine_lanes(eng, name, made)
    return pk, sets, [list(vals) for _, vals in made], shape_of(name, 1)


def device_proof(eng, pk, sets, lists, public, scheme):
    mlists = [mont(v) if v else None for v in lists]
    if not public:
        return eng.prove(pk, sets[0], SEED, EVM, scheme) if len(sets) == 1 else eng.prove_multi(pk, sets, SEED, EVM, scheme)
    if len(sets) == 1:
        return eng.prove_public(pk, sets[0], mlists[0], SEED, EVM, scheme)
    return eng.prove_multi_public(pk, sets, mlists, SEED, EVM, scheme)


def engine_verdict(eng, pk, lists, public, proof, scheme):
    """eng.verify* on the same bytes.  A word not below r never reaches the engine - its lists are Montgomery images, which have no
    such value; proving_server answers "rejected" for it, and so does this."""
    if not public:
        return eng.verify_multi(pk, len(lists), proof, EVM, scheme)  # (one circuit: zk_verify)
    if any(v >= yul_vm.R for vals in lists for v in vals):
        return False
    return eng.verify_multi_public(pk, proof, [mont(v) if v else None for v in lists], EVM, scheme)


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["k19like", "k17like", "wide", "idle"])
def test_device_proofs_through_the_generated_program(name, form, scheme):
    eng = zk.Engine(0)
    try:
        pk, sets, lists, sh = resident(eng, name, form)
        N, public, s = len(sets), FORMS[form][1] is not None, SCHEME[scheme]
        counts = [len(v) for v in lists] if public else None
        proof = device_proof(eng, pk, sets, lists, public, s)
        text = eng.evm_verifier(pk, N, counts, s)
        ok, vm = yul_vm.run(text, yul_vm.calldata(lists, proof))
        assert ok is True and engine_verdict(eng, pk, lists, public, proof, s) is True
        assert yul_vm.counted(vm) == {k: v for k, v in eng.evm_verifier_cost(pk, N, counts, s).items() if k in yul_vm.counted(vm)}
        muts = yul_vm.mutations(sh, N, scheme, lists, proof)
        assert len(muts) == (16 if public else 14)
        for what, bad_lists, bad in muts:
            got = yul_vm.run(text, yul_vm.calldata(bad_lists, bad))[0]
            assert got is False and engine_verdict(eng, pk, bad_lists, public, bad, s) is False, what
        for other in (N - 1, N + 1):  # the proof read under another circuit count
            if other == 0:
                continue
            other_lists = (lists + [[]])[:other]
            prog = eng.evm_verifier(pk, other, [len(v) for v in other_lists] if public else None, s)
            assert yul_vm.run(prog, yul_vm.calldata(other_lists, proof))[0] is False
            assert engine_verdict(eng, pk, other_lists, public, proof, s) is False
    finally:
        eng.close()


def test_key_forms_and_buffer_forms():
    eng = zk.Engine(0)
    try:
        for name, form in (("k17like", "prove"), ("wide", "prove_multi_public")):
            pk, _, lists, _ = resident(eng, name, form)
            N, counts = FORMS[form]
            n_inst = 0 if counts is None else 1
            vk = eng.vk_from_parts(params_of(name, n_inst), *eng.vk_export(pk))
            for s in (E.ZK_SCHEME_DEFAULT, E.ZK_SCHEME_GWC, E.ZK_SCHEME_SHPLONK):
                text = eng.evm_verifier(pk, N, counts, s)
                assert eng.evm_verifier(vk, N, counts, s) == text
                assert eng.evm_verifier_cost(vk, N, counts, s) == eng.evm_verifier_cost(pk, N, counts, s) == yul_vm.header_cost(text)
                arr = None if counts is None else (ctypes.c_size_t * N)(*counts)
                ln = ctypes.c_size_t(0)
                assert eng.L.zk_evm_verifier(eng.ctx, pk, N, arr, s, None, 0, ctypes.byref(ln)) == 0 and ln.value == len(text.encode())
                buf = ctypes.create_string_buffer(b"\xa5" * (ln.value + 8), ln.value + 8)
                assert eng.L.zk_evm_verifier(eng.ctx, pk, N, arr, s, buf, ln.value, ctypes.byref(ln)) == 0
                assert buf.raw == text.encode() + b"\xa5" * 8
            assert eng.evm_verifier(pk, N, counts, E.ZK_SCHEME_DEFAULT) == eng.evm_verifier(pk, N, counts, E.ZK_SCHEME_GWC)
            assert eng.evm_verifier(pk, N, counts, E.ZK_SCHEME_SHPLONK) != eng.evm_verifier(pk, N, counts, E.ZK_SCHEME_GWC)
            if counts is None:  # NULL counts and all-zero counts are the same kind
                assert eng.evm_verifier(pk, N, [0] * N) == eng.evm_verifier(pk, N, None)
    finally:
        eng.close()


def test_errors_leave_the_outputs_untouched():
    eng = zk.Engine(0)
    try:
        L = eng.L
        fill = b"\x5a" * 64
        buf = ctypes.create_string_buffer(fill, 64)
        ln = ctypes.c_size_t(0)
        cost = E.EvmCostC(*([0x5a5a5a5a] * 8))
        sizes = lambda *v: (ctypes.c_size_t * len(v))(*v)

        def refused(code, ctx, pk, N, counts, scheme, with_len=True):
            ln.value = 77
            assert L.zk_evm_verifier(ctx, pk, N, counts, scheme, buf, 64, ctypes.byref(ln) if with_len else None) == code
            assert L.zk_evm_verifier_cost(ctx, pk, N, counts, scheme, ctypes.byref(cost)) == code
            assert buf.raw == fill and ln.value == 77 and all(getattr(cost, n) == 0x5a5a5a5a for n, _ in E.EvmCostC._fields_)

        # no SRS in the context: what zk_verify returns without one
        p = params_of("k17like", 0)
        asg = multi_cases.witnesses("k17like", 1)[0]
        other = zk.Engine(0)
        pk0, _ = multi_cases.engine_key(other, "k17like", [asg])
        vk_parts = other.vk_export(pk0)
        bare = eng.vk_from_parts(p, *vk_parts)
        ok = ctypes.c_int(0)
        want = L.zk_verify(eng.ctx, bare, EVM, E.ZK_SCHEME_GWC, bytes(64), 64, ctypes.byref(ok))
        assert want == -5
        refused(want, eng.ctx, bare, 1, None, E.ZK_SCHEME_GWC)
        other.close()

        public, _, _ = engine_lanes(eng, "k17like", lanes("k17like", [9]))  # (sets the SRS up: the verifying-only key now has one)
        plain = bare
        n = 1 << p.degree
        assert L.zk_evm_verifier(None, plain, 1, None, E.ZK_SCHEME_GWC, buf, 64, ctypes.byref(ln)) == -1 and buf.raw == fill
        assert L.zk_evm_verifier_cost(None, plain, 1, None, E.ZK_SCHEME_GWC, ctypes.byref(cost)) == -1
        assert L.zk_evm_verifier(eng.ctx, plain, 1, None, E.ZK_SCHEME_GWC, buf, 64, None) == -1 and buf.raw == fill
        assert L.zk_evm_verifier_cost(eng.ctx, plain, 1, None, E.ZK_SCHEME_GWC, None) == -1
        refused(-1, eng.ctx, plain, 0, None, E.ZK_SCHEME_GWC)
        refused(-1, eng.ctx, plain, E.ZK_PROVE_MULTI_MAX + 1, None, E.ZK_SCHEME_GWC)
        refused(-1, eng.ctx, plain, 1, sizes(1), E.ZK_SCHEME_GWC)          # a value on a key without the column
        refused(-1, eng.ctx, plain, 2, sizes(0, 3), E.ZK_SCHEME_GWC)
        refused(-1, eng.ctx, public, 1, sizes(n - 6), E.ZK_SCHEME_GWC)     # m > n - 7
        refused(-1, eng.ctx, public, 2, sizes(9, n - 6), E.ZK_SCHEME_GWC)
        refused(-1, eng.ctx, public, 1, sizes(9), 7)                       # an unknown scheme
        refused(-1, eng.ctx, 0xdead, 1, None, E.ZK_SCHEME_GWC)             # no such key
        assert len(eng.evm_verifier(public, 1, [n - 7])) > 0               # the column's last usable row is allowed
        assert L.zk_evm_verifier(eng.ctx, public, E.ZK_PROVE_MULTI_MAX, None, E.ZK_SCHEME_GWC, None, 0, ctypes.byref(ln)) == 0
        # a short buffer: the engine's usual code, with the length set
        text = eng.evm_verifier(plain, 1, None, E.ZK_SCHEME_GWC)
        big = ctypes.create_string_buffer(b"\x5a" * len(text), len(text))
        ln.value = 0
        assert L.zk_evm_verifier(eng.ctx, plain, 1, None, E.ZK_SCHEME_GWC, big, len(text) - 1, ctypes.byref(ln)) == -1
        assert ln.value == len(text) and big.raw == b"\x5a" * len(text)
    finally:
        eng.close()


def test_a_program_embeds_the_resident_srs():
    """k = 6: the program generated after zk_srs_update accepts a proof of a key made then; the one generated before rejects it.  The
    pairing is a true one: the interpreter's stand-in knows the seed-0 secret only."""
    eng = zk.Engine(0)
    try:
        name, asgs = "k18like", multi_cases.witnesses("k18like", 1)
        pk_before, _ = multi_cases.engine_key(eng, name, asgs)
        before = eng.evm_verifier(pk_before)
        eng.srs_update(b"\x77" * 32)
        p = params_of(name, 0)
        pk, sets = eng.keygen(p, np.stack([asgs[0].to_limbs(c) for c in asgs[0].fixed]), asgs[0].copies), []
        for col in asgs[0].advice:
            h = eng.poly(1 << p.degree)
            eng.upload_canonical(h, asgs[0].to_limbs(col))
            sets.append(h)
        proof = eng.prove(pk, sets, SEED, EVM)
        assert eng.verify(pk, proof, EVM) is True
        after = eng.evm_verifier(pk)
        assert after != before
        assert yul_vm.run(after, proof, true_pairing=True)[0] is True
        assert yul_vm.run(before, proof, true_pairing=True)[0] is False
        # the key differs too (its commitments are the new SRS's): the old program with the new key's constants still rejects,
        # because its s_g2 is the old one
        old_g2 = before[before.index("// e(rhs, g2)"):]
        swapped = after[:after.index("// e(rhs, g2)")] + old_g2
        assert yul_vm.run(swapped, proof, true_pairing=True)[0] is False
    finally:
        eng.close()


def requests(api, pkp, count):
    """`count` request bodies with ES256 signatures made here (plain secp256r1 arithmetic of the module itself)."""
    out = []
    for i in range(count):
        d, kk, z = 0x1234567 + 11 * i, 0x7654321 + 7 * i, int.from_bytes(bytes([0x21 + i]) * 32, "big") % api._N
        q, r = api._p256_mul(d, api._G), api._p256_mul(kk, api._G)[0] % api._N
        s = pow(kk, -1, api._N) * (z + r * d) % api._N
        vals = dict(zip(("pubkey_x", "pubkey_y", "r", "s", "msghash"), (list(v.to_bytes(32, "little")) for v in (q[0], q[1], r, s, z))))
        out.append(dict(vals, proving_key_path=pkp))
    return out


def test_server_and_generate_verifier(tmp_path, monkeypatch):
    api, srv = zk.ecdsa_p256, zk.proving_server
    api.shutdown()
    cfg = tmp_path / "ecdsa_circuit.config"
    cfg.write_text(json.dumps({"degree": 10, "num_advice": 3, "num_lookup_advice": 2, "num_fixed": 1, "lookup_bits": 8}) + "\n")
    monkeypatch.setenv("ECDSA_CONFIG", str(cfg))
    pkp, vkp, yul = str(tmp_path / "proving_key.pk"), str(tmp_path / "verifying_key.vk"), str(tmp_path / "verifier.yul")
    try:
        srv.setup(degree=10, proving_key_path=pkp, verifying_key_path=vkp, public=True)
        body = {"verifying_key_path": vkp, "valid_proof_hex": "", "deploy_code_path": "", "sol_code_path": "", "yul_code_path": yul}
        text = srv.generate_evm_verifier(json.dumps(body), degree=10, public=9)
        assert open(yul).read() == text == api.generate_verifier(vkp, 10, public=True)
        assert text != api.generate_verifier(vkp, 10, public=True, scheme=E.ZK_SCHEME_SHPLONK)
        assert yul_vm.header(text)["instances per circuit"] == "9"
        reqs = requests(api, pkp, 2)
        calldata = bytes.fromhex(srv.prove_evm(reqs[0], degree=10, rng_seed=bytes(32), public=True))
        words = lambda msg, key: api.public_inputs(bytes(msg["msghash"]), bytes(key["pubkey_x"]), bytes(key["pubkey_y"]))
        assert calldata[:288] == api.encode_calldata(words(reqs[0], reqs[0]), b"")
        assert yul_vm.run(text, calldata)[0] is True
        forged = api.encode_calldata(words(reqs[1], reqs[0]), calldata[288:])  # the same proof behind another msghash's limbs
        assert yul_vm.run(text, forged)[0] is False
        assert srv.verify_evm(json.dumps({"verifying_key_path": vkp, "proof": forged.hex()}), degree=10, public=9) == "rejected"
        two = api.generate_verifier(vkp, 10, n=2, public=True)
        assert yul_vm.header(two)["circuits"] == "2" and yul_vm.header(two)["instances per circuit"] == "9 9"
        for field in ("sol_code_path", "deploy_code_path"):
            with pytest.raises(ValueError, match="solc"):
                srv.generate_evm_verifier(dict(body, **{field: str(tmp_path / "x")}), degree=10, public=9)
    finally:
        api.shutdown()
