"""ParamsKZG::downsize without a GPU: the tests' own g_to_lagrange reference (tests/g1_lagrange_ref.py) against the oracle's
tau-built SRS, and the four new entry points in the public header."""
import os
import re

import pytest

import g1_lagrange_ref as ref
from zkoracle import curve, srs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6])
def test_reference_g_to_lagrange_of_g_is_g_lagrange(k):
    assert ref.g_to_lagrange(srs.srs_points(k), k) == srs.srs_points(k, lagrange=True)


def test_reference_handles_degenerate_inputs():
    P = srs.g1_of_scalar(12345)
    assert ref.g_to_lagrange([None] * 8, 3) == [None] * 8
    assert ref.g_to_lagrange([P] * 8, 3) == [P] + [None] * 7  # [1/n] sum_j [w^-ij] P = P for i = 0, else the identity
    assert ref.g_to_lagrange([P, curve.neg(P)] * 4, 3)[0] is None
    assert ref.from_mont_limbs(ref.to_mont_limbs([P, None])) == [P, None]


def test_header_declares_the_downsize_entry_points():
    txt = open(os.path.join(ROOT, "include", "zkmi355.h")).read()
    for decl in (r"int zk_g_to_lagrange\(zk_ctx\* ctx, const uint64_t\* g[^,]*, uint32_t k, uint64_t\* out",
                 r"int zk_srs_downsize\(zk_ctx\* ctx, uint32_t k\)",
                 r"int zk_srs_read_downsize\(zk_ctx\* ctx, const uint8_t\* bytes, size_t len, int format, uint32_t k\)",
                 r"int zk_srs_check\(zk_ctx\* ctx, const uint8_t seed\[32\], uint32_t\* flags\)"):
        assert re.search(decl, txt), decl


def test_engine_and_api_expose_the_downsize():
    import webauthn_halo2_amd as zk
    from webauthn_halo2_amd import ecdsa_p256, proving_server

    for m in ("g_to_lagrange", "srs_downsize", "srs_read_downsize", "srs_check"):
        assert callable(getattr(zk.Engine, m))
    assert callable(ecdsa_p256.set_params_file)
    assert "params_path" in proving_server.setup.__code__.co_varnames
    L = zk.load_library()
    for s in ("zk_g_to_lagrange", "zk_srs_downsize", "zk_srs_read_downsize", "zk_srs_check"):
        assert hasattr(L, s)


def test_params_file_source_refuses_a_larger_degree(tmp_path):
    """gen_srs(degree) with a params file of smaller degree K raises ValueError before anything is built (halo2's downsize
    asserts k <= K) — checked on the file's header alone, no device needed."""
    from webauthn_halo2_amd import ecdsa_p256 as api

    f = tmp_path / "kzg_bn254_4.srs"
    f.write_bytes((4).to_bytes(4, "little") + bytes(16))
    assert api.params_file_degree(str(f)) == 4
    api.set_params_file(str(f), device=7)
    try:
        with pytest.raises(ValueError):
            api.gen_srs(5, device=7)
        assert 7 not in api._STATE or api._STATE[7]["eng"] is None
    finally:
        api.set_params_file(None, device=7)
        api._STATE.pop(7, None)
    with pytest.raises(FileNotFoundError):
        api.set_params_file(str(tmp_path / "missing.srs"), device=7)
