"""The plain-Python reference of zk_witness_check (tests/witness_ref.py) agrees with the other judges of "satisfied" this
repository has — adversarial_layout.check and the oracle's prover + verifier — and the C ABI / Python binding of the entry
point exist.  CPU only."""
import os
import re

import pytest

import webauthn_halo2_amd as zk
import witness_cases as C
import witness_ref as W
from prover_shapes import SHAPES
from zkoracle import plonk, prover
from zkoracle.field import R
from zkoracle.hashes import ChaCha20Rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["k19like", "k17like", "k18like", "wide", "idle"]


@pytest.mark.parametrize("name", NAMES)
def test_reference_accepts_satisfying_witnesses(name):
    """Both generators' witnesses are clean by the reference (adversarial_layout.check has accepted its own inside adv_case;
    that generator does not model idle gate columns, so `idle` is checked on circuit.synthesize alone)."""
    sh, fixed, copies, advice = C.synth_case(SHAPES[name])
    assert W.check(sh, fixed, copies, advice) == []
    if name != "idle":
        sh, fixed, copies, advice = C.adv_case(SHAPES[name], 7)
        assert W.check(sh, fixed, copies, advice) == []


def test_reference_reports_the_expected_neighbours_of_one_corrupted_cell():
    """One corrupted cell of a copy cycle: itself and its sigma-predecessor; one corrupted gate cell: the windows that hold it."""
    sh, fixed, copies, advice = C.adv_case(SHAPES["k17like"], 7)
    F = sh.num_fixed
    cyc = next(c for c in C.cycles(copies) if len(c) >= 5 and all(col >= F for col, _ in c))
    col, row = cyc[2]
    adv = [list(c) for c in advice]
    adv[col - F][row] = (adv[col - F][row] + 1) % R
    got = W.check(sh, fixed, copies, adv)
    copy_cells = [(f[1], f[2]) for f in got if f[0] == W.COPY]
    assert len(copy_cells) == 2 and (col, row) in copy_cells
    assert all((f[1], f[2]) in cyc and (f[3], f[4]) in cyc for f in got if f[0] == W.COPY)
    assert [f for f in got if f[0] == W.GATE] == W.gate_failures_around(sh, fixed, adv, col - F, row)
    assert not [f for f in got if f[0] in (W.LOOKUP, W.GATE_BLINDED)]


def test_reference_and_oracle_verifier_agree_on_unsatisfied():
    """Degree-5 shape, one planted failure of each kind a witness can have.  A broken gate and a broken copy go through the
    oracle's create_proof (the quotient fills the whole extended domain: the prover cannot notice) and plonk.verify rejects the
    proof; an off-table lookup input is refused by the prover itself, as halo2's is (Error::ConstraintSystemFailure)."""
    sh, fixed, copies, advice = C.synth_case(SHAPES["k19like"])
    pk = prover.keygen(prover.Circuit(sh, fixed, copies, advice))
    assert plonk.verify(pk.vk, prover.create_proof(pk, advice, ChaCha20Rng(bytes(32)), "evm"), "evm")
    F = sh.num_fixed
    in_cycle = {cell for c in C.cycles(copies) for cell in c}
    gate_row = next(r for r in range(0, sh.usable_rows - 3, 4) if fixed[sh.fx_sel[0]][r] and (F, r + 3) not in in_cycle)
    pair = next(c for c in C.cycles(copies) if len(c) == 2 and all(col >= F for col, _ in c))
    looked = next(r for r in range(sh.usable_rows) if fixed[sh.fx_qlookup][r])
    for kind, (row, value) in {W.GATE: (gate_row + 3, None), W.COPY: (pair[0][1], None), W.LOOKUP: (looked, 1 << 40)}.items():
        adv = [list(c) for c in advice]
        adv[0][row] = (adv[0][row] + 1) % R if value is None else value
        failures = W.check(sh, fixed, copies, adv)
        assert W.counts(failures)[kind] >= 1, kind
        if kind == W.LOOKUP:
            with pytest.raises(ValueError):
                prover.create_proof(pk, adv, ChaCha20Rng(bytes(32)), "evm")
        else:
            assert W.counts(failures)[W.LOOKUP] == 0
            assert not plonk.verify(pk.vk, prover.create_proof(pk, adv, ChaCha20Rng(bytes(32)), "evm"), "evm"), kind


def test_blinded_gate_rule():
    """A selector set where the gate would read a blinded row is a failure whatever the advice holds."""
    sh, fixed, copies, advice = C.synth_case(SHAPES["k17like"])
    fixed = [list(c) for c in fixed]
    fixed[sh.fx_sel[1]][sh.usable_rows - 2] = 1
    assert W.check(sh, fixed, copies, advice) == [(W.GATE_BLINDED, 1, sh.usable_rows - 2, 0, 0)]


def test_abi_declares_and_binds_witness_check():
    hdr = open(os.path.join(ROOT, "include", "zkmi355.h")).read()
    assert re.search(r"\bint zk_witness_check\(zk_ctx\* ctx, zk_pk pk, const zk_poly\* advice, size_t n_advice,\s*zk_witness_failure\* out, size_t cap,\s*uint64_t counts\[5\]\);", hdr)
    for name, v in (("ZK_FAIL_GATE", 1), ("ZK_FAIL_GATE_BLINDED", 2), ("ZK_FAIL_LOOKUP", 3), ("ZK_FAIL_COPY", 4)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr), name
        assert getattr(zk.engine, name) == v
    assert re.search(r"typedef struct \{ uint32_t kind, index, row, other_index, other_row, reserved; \} zk_witness_failure;", hdr)
    L = zk.load_library()
    assert L.zk_witness_check.argtypes is not None and len(L.zk_witness_check.argtypes) == 7
    assert callable(zk.Engine.witness_check)
    assert callable(zk.ecdsa_p256.mock_verify_advice) and issubclass(zk.ecdsa_p256.WitnessError, ValueError)
