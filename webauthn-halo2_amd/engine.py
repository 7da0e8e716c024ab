"""ctypes binding of libzkmi355.so (include/zkmi355.h) — the only way Python
reaches the engine.  There is no CPU fallback: a missing library or a missing
gfx950 device raises `ZkError`.

Arrays are numpy uint64 with the Rust memory images (Fr/Fq: 4 LE limbs,
Montgomery; G1Affine: 8 limbs; G1 Jacobian: 12 limbs).
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

ZK_BASIS_MONOMIAL = 0
ZK_BASIS_LAGRANGE = 1
ZK_T_MSM, ZK_T_NTT, ZK_T_QUOTIENT, ZK_T_EVAL, ZK_T_MSM_ACCUM, ZK_T_MSM_COLUMNS, ZK_T_MSM_TAIL_MAIN, ZK_T_MSM_TAIL = 0, 1, 2, 3, 4, 5, 6, 7


ZK_TRANSCRIPT_BLAKE2B, ZK_TRANSCRIPT_EVM = 0, 1
ZK_SERDE_PROCESSED, ZK_SERDE_RAW_BYTES, ZK_SERDE_RAW_BYTES_UNCHECKED = 0, 1, 2
ZK_OPT_MSM_WINDOW, ZK_OPT_MSM_BATCH, ZK_OPT_NTT_MAX_RADIX_LOG2, ZK_OPT_GP_BATCH_INVERT, ZK_OPT_MSM_TAIL_STREAM = 1, 2, 3, 4, 5
ZK_OPT_MSM_TAIL_MAIN_ABOVE, ZK_OPT_BATCH_PASS_COLUMNS, ZK_OPT_XFORM_STREAM, ZK_OPT_MSM_STREAM, ZK_OPT_MSM_T1, ZK_OPT_STREAM_AUDIT = 6, 7, 8, 9, 10, 11
ZK_OPT_STREAM_PRIORITY, ZK_OPT_QUOTIENT_DOMAIN, ZK_OPT_ACTIVITY_HOLD = 12, 13, 14
ZK_VERIFY_INSTANCE_EVAL_AUTO, ZK_VERIFY_INSTANCE_EVAL_HOST, ZK_VERIFY_INSTANCE_EVAL_DEVICE = 0, 1, 2
ZK_SCHEME_DEFAULT, ZK_SCHEME_GWC, ZK_SCHEME_SHPLONK = 0, 1, 2
ZK_VERIFY_BATCH_MAX = 1024
ZK_PROVE_MULTI_MAX = 16
ZK_ES256_VALID, ZK_ES256_RANGE, ZK_ES256_OFF_CURVE, ZK_ES256_MISMATCH = 0, 1, 2, 3
ZK_ES256_BATCH_MAX = 16384
(ZK_WEBAUTHN_VALID, ZK_WEBAUTHN_RANGE, ZK_WEBAUTHN_OFF_CURVE, ZK_WEBAUTHN_MISMATCH, ZK_WEBAUTHN_SIZE, ZK_WEBAUTHN_AUTHDATA, ZK_WEBAUTHN_RPID,
 ZK_WEBAUTHN_FLAGS, ZK_WEBAUTHN_CLIENTDATA, ZK_WEBAUTHN_SIGNATURE_DER) = range(10)
ZK_WEBAUTHN_BATCH_MAX = ZK_ES256_BATCH_MAX
ZK_WEBAUTHN_AUTHDATA_MAX, ZK_WEBAUTHN_CLIENTDATA_MAX, ZK_WEBAUTHN_CHALLENGE_MAX, ZK_WEBAUTHN_ORIGIN_MAX = 1024, 4096, 64, 255
ZK_WEBAUTHN_CBOR, ZK_WEBAUTHN_CREDENTIAL, ZK_WEBAUTHN_COSE_KEY, ZK_WEBAUTHN_ATTESTATION = 10, 11, 12, 13  # zk_webauthn_register's own
ZK_WEBAUTHN_ATTOBJ_MAX = 8192
ZK_WEBAUTHN_ATT_IGNORE, ZK_WEBAUTHN_ATT_NONE_OR_SELF = 0, 1
ZK_WEBAUTHN_ATTESTED_NONE, ZK_WEBAUTHN_ATTESTED_SELF, ZK_WEBAUTHN_ATTESTED_NOT_JUDGED = 0, 1, 2
WEBAUTHN_REASON_NAMES = ("VALID", "RANGE", "OFF_CURVE", "MISMATCH", "SIZE", "AUTHDATA", "RPID", "FLAGS", "CLIENTDATA", "SIGNATURE_DER", "CBOR",
                         "CREDENTIAL", "COSE_KEY", "ATTESTATION")
ZK_PAIRING_VALID, ZK_PAIRING_RANGE, ZK_PAIRING_OFF_CURVE, ZK_PAIRING_MISMATCH = 0, 1, 2, 3
ZK_PAIRING_G2 = 4
ZK_PAIRING_BATCH_MAX = 4096
ZK_VERIFY_PAIRING_AUTO, ZK_VERIFY_PAIRING_HOST, ZK_VERIFY_PAIRING_DEVICE = 0, 1, 2
ZK_SRS_CHECK_POWERS, ZK_SRS_CHECK_LAGRANGE, ZK_SRS_CHECK_GENERATORS = 1, 2, 4
ZK_SRS_CONTRIB_SAME_SECRET, ZK_SRS_CONTRIB_LINKS, ZK_SRS_CONTRIB_NONTRIVIAL, ZK_SRS_CONTRIB_RESIDENT = 1, 2, 4, 8
ZK_SRS_CONTRIB_CHAINED = 16
ZK_SRS_CONTRIB_BATCH_MAX = 4096
ZK_FAIL_GATE, ZK_FAIL_GATE_BLINDED, ZK_FAIL_LOOKUP, ZK_FAIL_COPY = 1, 2, 3, 4
ZK_PK_FIXED_POLY, ZK_PK_SIGMA_POLY = 0, 1
(ZK_PK_PART_FIXED_COMMIT, ZK_PK_PART_SIGMA_COMMIT, ZK_PK_PART_FIXED_POLY, ZK_PK_PART_SIGMA_POLY, ZK_PK_PART_FIXED_COSET,
 ZK_PK_PART_SIGMA_COSET, ZK_PK_PART_L_COSET, ZK_PK_PART_SIGMA_LABEL, ZK_PK_PART_SIGMA_MAP) = range(1, 10)
ZK_PK_CHECK_COMMITMENTS, ZK_PK_CHECK_POLYS, ZK_PK_CHECK_COSETS, ZK_PK_CHECK_SIGMA, ZK_PK_CHECK_ALL, ZK_PK_CHECK_REPR = 1, 2, 4, 8, 15, 16
ZK_PLACEMENT_MAINS_OK, ZK_PLACEMENT_LONE_OK, ZK_PLACEMENT_PAIR_OK, ZK_PLACEMENT_LAYER1_OK, ZK_PLACEMENT_OK = 1, 2, 4, 8, 15
ZK_PLACEMENT_CALIBRATED, ZK_PLACEMENT_UNRESOLVED = 16, 32


def device_pci_bus_id(device=0):
    """PCI address of a device, e.g. '0000:c1:00.0' (zk_device_pci_bus_id)."""
    buf = ctypes.create_string_buffer(32)
    rc = load_library().zk_device_pci_bus_id(device, buf, len(buf))
    if rc:
        raise ZkError(rc, "zk_device_pci_bus_id")
    return buf.value.decode().lower()


def device_mem_info(device=0):
    """(free, total) bytes of a device's memory (zk_device_mem_info)."""
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = load_library().zk_device_mem_info(device, ctypes.byref(free), ctypes.byref(total))
    if rc:
        raise ZkError(rc, "zk_device_mem_info")
    return free.value, total.value


def stream_placement(device=0, calibrate=False) -> dict:
    """Which hardware queue each stream of the device's pool sits on, measured (zk_stream_placement; ~30 ms on an idle device).
    calibrate=True re-deals the pool from the measurement when it is not as the engine assumes and four classes were seen
    (only while no Engine of this process exists on the device).  Returns the report: n_queues (0 = unresolved), flags, the
    ZK_PLACEMENT_* bits by name, main_queue[8], role_queue[8][3] (tail, transform, MSM), spare_queue[8], rounds, streams,
    probe_ms.  ok = all four invariants hold.  A host calls it once per device at start-up, before its first Engine, and logs it."""
    r = PlacementC()
    rc = load_library().zk_stream_placement(device, 1 if calibrate else 0, ctypes.byref(r))
    if rc:
        raise ZkError(rc, "zk_stream_placement")
    f = r.flags
    return {"n_queues": r.n_queues, "flags": f, "ok": f & ZK_PLACEMENT_OK == ZK_PLACEMENT_OK,
            "mains_ok": bool(f & ZK_PLACEMENT_MAINS_OK), "lone_ok": bool(f & ZK_PLACEMENT_LONE_OK),
            "pair_ok": bool(f & ZK_PLACEMENT_PAIR_OK), "layer1_ok": bool(f & ZK_PLACEMENT_LAYER1_OK),
            "calibrated": bool(f & ZK_PLACEMENT_CALIBRATED), "unresolved": bool(f & ZK_PLACEMENT_UNRESOLVED),
            "main_queue": list(r.main_queue), "role_queue": [list(row) for row in r.role_queue], "spare_queue": list(r.spare_queue),
            "rounds": r.rounds, "streams": r.streams, "probe_ms": r.probe_ms}


class PinnedArray:
    """A numpy array over page-locked host memory (zk_host_alloc): the buffers a host hands to upload / upload_canonical.
    Keep the object alive while `a` is in use; free() (or garbage collection) returns the memory."""

    def __init__(self, shape, dtype=np.uint64):
        self.L = load_library()
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = self.L.zk_host_alloc(nbytes)
        if not self.ptr:
            raise ZkError(-2, "zk_host_alloc")
        self.a = np.frombuffer((ctypes.c_uint8 * nbytes).from_address(self.ptr), dtype=dtype).reshape(shape)

    def free(self):
        if self.ptr:
            self.a = None
            self.L.zk_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class CircuitParamsC(ctypes.Structure):
    _fields_ = [("k", ctypes.c_uint32), ("num_advice", ctypes.c_uint32), ("num_lookup_advice", ctypes.c_uint32),
                ("num_fixed", ctypes.c_uint32), ("lookup_bits", ctypes.c_uint32),
                ("num_idle_gate_columns", ctypes.c_uint32), ("num_instance_columns", ctypes.c_uint32)]


class WitnessFailureC(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("index", ctypes.c_uint32), ("row", ctypes.c_uint32), ("other_index", ctypes.c_uint32),
                ("other_row", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class PkFindingC(ctypes.Structure):
    _fields_ = [("part", ctypes.c_uint32), ("column", ctypes.c_uint32), ("index", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("count", ctypes.c_uint64)]


class SrsContributionC(ctypes.Structure):
    _fields_ = [("before_g1", ctypes.c_uint64 * 8), ("after_g1", ctypes.c_uint64 * 8), ("s_g1", ctypes.c_uint64 * 8),
                ("s_g2", ctypes.c_uint64 * 16)]


class WebauthnAssertionC(ctypes.Structure):
    _fields_ = [("authenticator_data", ctypes.c_char_p), ("authenticator_data_len", ctypes.c_size_t), ("client_data_json", ctypes.c_char_p),
                ("client_data_json_len", ctypes.c_size_t), ("signature", ctypes.c_char_p), ("signature_len", ctypes.c_size_t),
                ("pubkey_x", ctypes.c_uint8 * 32), ("pubkey_y", ctypes.c_uint8 * 32), ("challenge", ctypes.c_char_p),
                ("challenge_len", ctypes.c_size_t), ("origin", ctypes.c_char_p), ("origin_len", ctypes.c_size_t),
                ("rp_id_hash", ctypes.c_uint8 * 32), ("flags_required", ctypes.c_uint8), ("allow_cross_origin", ctypes.c_uint8)]


class WebauthnRegistrationC(ctypes.Structure):
    _fields_ = [("attestation_object", ctypes.c_char_p), ("attestation_object_len", ctypes.c_size_t), ("client_data_json", ctypes.c_char_p),
                ("client_data_json_len", ctypes.c_size_t), ("challenge", ctypes.c_char_p), ("challenge_len", ctypes.c_size_t),
                ("origin", ctypes.c_char_p), ("origin_len", ctypes.c_size_t), ("rp_id_hash", ctypes.c_uint8 * 32),
                ("flags_required", ctypes.c_uint8), ("allow_cross_origin", ctypes.c_uint8), ("attestation_policy", ctypes.c_uint8)]


class WebauthnCredentialC(ctypes.Structure):
    _fields_ = [("pubkey_x", ctypes.c_uint8 * 32), ("pubkey_y", ctypes.c_uint8 * 32), ("aaguid", ctypes.c_uint8 * 16),
                ("auth_data_off", ctypes.c_uint32), ("auth_data_len", ctypes.c_uint32), ("credential_id_off", ctypes.c_uint32),
                ("credential_id_len", ctypes.c_uint32), ("sign_count", ctypes.c_uint32), ("flags", ctypes.c_uint8),
                ("attestation", ctypes.c_uint8)]


class PlacementC(ctypes.Structure):
    _fields_ = [("n_queues", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("main_queue", ctypes.c_uint8 * 8),
                ("role_queue", (ctypes.c_uint8 * 3) * 8), ("spare_queue", ctypes.c_uint8 * 8), ("rounds", ctypes.c_uint32),
                ("streams", ctypes.c_uint32), ("probe_ms", ctypes.c_float)]


class CtxStreamsC(ctypes.Structure):
    _fields_ = [("slot", ctypes.c_int32), ("queue", ctypes.c_uint8 * 4), ("counts", ctypes.c_uint64 * 4)]


class ZkError(RuntimeError):
    def __init__(self, code, what, hip=0):
        self.code = code
        self.hip = hip
        super().__init__(f"{what}: zk error {code}" + (f" (hipError_t {hip})" if hip else ""))


def lib_path():
    # ZKMI355_LIB: an alternative build of the same library (A/B tuning variants, tools/ab_variants.sh)
    return os.environ.get("ZKMI355_LIB") or os.path.join(_HERE, "libzkmi355.so")


class EvmCostC(ctypes.Structure):  # zk_evm_cost
    _fields_ = [(n, ctypes.c_uint32) for n in ("calldata_bytes", "memory_bytes", "modexp", "ecadd", "ecmul", "pairing", "keccak_calls",
                                               "keccak_bytes")]


def load_library():
    """Load libzkmi355.so; raises if it has not been built (./build.sh)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise ZkError(-4, f"{p} is missing — run ./build.sh (no CPU fallback exists)")
    L = ctypes.CDLL(p)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    vp = ctypes.c_void_p
    sz = ctypes.c_size_t
    u32 = ctypes.c_uint32
    sig = {
        "zk_device_count": ([], ctypes.c_int),
        "zk_device_pci_bus_id": ([ctypes.c_int, ctypes.c_char_p, sz], ctypes.c_int),
        "zk_device_mem_info": ([ctypes.c_int, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
        "zk_host_alloc": ([sz], vp),
        "zk_host_free": ([vp], None),
        "zk_ctx_create": ([ctypes.c_int, ctypes.POINTER(vp)], ctypes.c_int),
        "zk_ctx_create_shared": ([vp, ctypes.POINTER(vp)], ctypes.c_int),
        "zk_ctx_destroy": ([vp], None),
        "zk_strerror": ([ctypes.c_int], ctypes.c_char_p),
        "zk_last_hip_error": ([vp], ctypes.c_int),
        "zk_sync": ([vp], ctypes.c_int),
        "zk_ctx_set_option": ([vp, ctypes.c_int, ctypes.c_int64], ctypes.c_int),
        "zk_msm_bn254": ([vp, u64p, u64p, sz, u64p], ctypes.c_int),
        "zk_msm_srs": ([vp, ctypes.c_int, u64p, sz, u64p], ctypes.c_int),
        "zk_ntt_bn254_fr": ([vp, u64p, u64p, u32], ctypes.c_int),
        "zk_srs_setup": ([vp, u32, ctypes.c_char_p], ctypes.c_int),
        "zk_srs_load": ([vp, u32, u64p, u64p], ctypes.c_int),
        "zk_srs_export": ([vp, ctypes.c_int, u64p, sz, sz], ctypes.c_int),
        "zk_srs_k": ([vp], ctypes.c_int),
        "zk_srs_msm_plan": ([vp, ctypes.POINTER(u32), ctypes.POINTER(u32)], ctypes.c_int),
        "zk_poly_alloc": ([vp, sz, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
        "zk_poly_free": ([vp, ctypes.c_uint64], ctypes.c_int),
        "zk_poly_detach": ([vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
        "zk_poly_attach": ([vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
        "zk_poly_discard": ([ctypes.c_uint64], ctypes.c_int),
        "zk_poly_len": ([vp, ctypes.c_uint64, ctypes.POINTER(sz)], ctypes.c_int),
        "zk_poly_upload": ([vp, ctypes.c_uint64, u64p, sz], ctypes.c_int),
        "zk_poly_download": ([vp, ctypes.c_uint64, u64p, sz], ctypes.c_int),
        "zk_poly_copy": ([vp, ctypes.c_uint64, ctypes.c_uint64], ctypes.c_int),
        "zk_commit": ([vp, ctypes.c_uint64, ctypes.c_int, u64p], ctypes.c_int),
        "zk_commit_batch": ([vp, ctypes.POINTER(ctypes.c_uint64), sz, ctypes.c_int, u64p], ctypes.c_int),
        "zk_lagrange_to_coeff": ([vp, ctypes.c_uint64], ctypes.c_int),
        "zk_coeff_to_lagrange": ([vp, ctypes.c_uint64], ctypes.c_int),
        "zk_coeff_to_extended": ([vp, ctypes.c_uint64, ctypes.c_uint64], ctypes.c_int),
        "zk_extended_to_coeff": ([vp, ctypes.c_uint64, sz], ctypes.c_int),
        "zk_eval": ([vp, ctypes.c_uint64, u64p, u64p], ctypes.c_int),
        "zk_last_kernel_ms": ([vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
        "zk_kate_division": ([vp, ctypes.c_uint64, u64p, ctypes.c_uint64], ctypes.c_int),
        "zk_timer_reset": ([vp], ctypes.c_int),
        "zk_timer_stats": ([vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
        "zk_clock_probe": ([vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
        "zk_audit_report": ([vp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p, sz], ctypes.c_int),
        "zk_keygen": ([vp, ctypes.POINTER(CircuitParamsC), u64p, sz, ctypes.POINTER(ctypes.c_uint32), sz,
                       ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
        "zk_pk_set_transcript_repr": ([vp, ctypes.c_uint64, u64p], ctypes.c_int),
        "zk_pk_free": ([vp, ctypes.c_uint64], ctypes.c_int),
        "zk_vk_export": ([vp, ctypes.c_uint64, u64p, u64p, u64p, ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
        "zk_proof_size": ([vp, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(sz)], ctypes.c_int),
        "zk_prove": ([vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), sz, ctypes.c_char_p, ctypes.c_int,
                      ctypes.c_int, ctypes.c_char_p, sz, ctypes.POINTER(sz)], ctypes.c_int),
        "zk_prove_public": ([vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), sz, u64p, sz, ctypes.c_char_p, ctypes.c_int,
                             ctypes.c_int, ctypes.c_char_p, sz, ctypes.POINTER(sz)], ctypes.c_int),
        "zk_verify_public": ([vp, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, u64p, sz, ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_int)],
                             ctypes.c_int),
        "zk_witness_check_public": ([vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), sz, ctypes.POINTER(WitnessFailureC), sz,
                                     ctypes.POINTER(ctypes.c_uint64), u64p, sz], ctypes.c_int),
        "zk_pk_num_instance_columns": ([vp, ctypes.c_uint64, ctypes.POINTER(u32)], ctypes.c_int),
        "zk_prove_batch": ([vp, ctypes.c_uint64, sz, ctypes.POINTER(ctypes.c_uint64), sz, ctypes.c_char_p, ctypes.c_int,
                            ctypes.c_int, ctypes.c_char_p, sz, ctypes.POINTER(sz)], ctypes.c_int),
        "zk_proof_size_multi": ([vp, ctypes.c_uint64, sz, ctypes.c_int, ctypes.c_int, ctypes.POINTER(sz)], ctypes.c_int),
        "zk_prove_multi": ([vp, ctypes.c_uint64, sz, ctypes.POINTER(ctypes.c_uint64), sz, ctypes.c_char_p, ctypes.c_int,
                            ctypes.c_int, ctypes.c_char_p, sz, ctypes.POINTER(sz)], ctypes.c_int),
        "zk_verify_multi": ([vp, ctypes.c_uint64, sz, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_int)],
                            ctypes.c_int),
        "zk_prove_batch_public": ([vp, ctypes.c_uint64, sz, ctypes.POINTER(ctypes.c_uint64), sz, ctypes.POINTER(u64p), ctypes.POINTER(sz),
                                   ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, sz, ctypes.POINTER(sz)], ctypes.c_int),
        "zk_prove_multi_public": ([vp, ctypes.c_uint64, sz, ctypes.POINTER(ctypes.c_uint64), sz, ctypes.POINTER(u64p), ctypes.POINTER(sz),
                                   ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, sz, ctypes.POINTER(sz)], ctypes.c_int),
        "zk_verify_batch_public": ([vp, ctypes.c_uint64, sz, ctypes.c_int, ctypes.c_int, ctypes.POINTER(u64p), ctypes.POINTER(sz),
                                    ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint8)], ctypes.c_int),
        "zk_verify_multi_public": ([vp, ctypes.c_uint64, sz, ctypes.c_int, ctypes.c_int, ctypes.POINTER(u64p), ctypes.POINTER(sz),
                                    ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
        "zk_verify_instance_eval_mode": ([vp, ctypes.c_int], ctypes.c_int),
        "zk_instance_eval": ([vp, u32, sz, ctypes.POINTER(u64p), ctypes.POINTER(sz), u64p, u64p, ctypes.POINTER(ctypes.c_uint8)], ctypes.c_int),
        "zk_es256_verify": ([vp, sz, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8)], ctypes.c_int),
        "zk_webauthn_verify": ([vp, sz, ctypes.POINTER(WebauthnAssertionC), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8),
                                ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(u32)], ctypes.c_int),
        "zk_webauthn_register": ([vp, sz, ctypes.POINTER(WebauthnRegistrationC), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8),
                                  ctypes.POINTER(WebauthnCredentialC)], ctypes.c_int),
        "zk_srs_write": ([vp, ctypes.c_int, vp, sz, ctypes.POINTER(sz)], ctypes.c_int),
        "zk_srs_read": ([vp, vp, sz, ctypes.c_int], ctypes.c_int),
        "zk_srs_set_g2": ([vp, u64p, u64p], ctypes.c_int),
        "zk_g_to_lagrange": ([vp, u64p, u32, u64p], ctypes.c_int),
        "zk_srs_downsize": ([vp, u32], ctypes.c_int),
        "zk_srs_read_downsize": ([vp, vp, sz, ctypes.c_int, u32], ctypes.c_int),
        "zk_srs_check": ([vp, ctypes.c_char_p, ctypes.POINTER(u32)], ctypes.c_int),
        "zk_srs_update": ([vp, ctypes.c_char_p, ctypes.POINTER(SrsContributionC)], ctypes.c_int),
        "zk_srs_contribution_check": ([vp, ctypes.POINTER(SrsContributionC), ctypes.POINTER(u32)], ctypes.c_int),
        "zk_vk_write": ([vp, ctypes.c_uint64, ctypes.c_int, vp, sz, ctypes.POINTER(sz)], ctypes.c_int),
        "zk_vk_load": ([vp, ctypes.c_uint64, vp, sz, ctypes.c_int, u64p], ctypes.c_int),
        "zk_pk_write": ([vp, ctypes.c_uint64, ctypes.c_int, vp, sz, ctypes.POINTER(sz)], ctypes.c_int),
        "zk_pk_read": ([vp, ctypes.POINTER(CircuitParamsC), vp, sz, ctypes.c_int, u64p, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
        "zk_pk_shape": ([vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
        "zk_quotient": ([vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), sz, ctypes.POINTER(ctypes.c_uint64), sz,
                         ctypes.POINTER(ctypes.c_uint64), sz, u64p, u64p, u64p, ctypes.c_int, ctypes.c_uint64], ctypes.c_int),
        "zk_poly_upload_canonical": ([vp, ctypes.c_uint64, u64p, sz], ctypes.c_int),
        "zk_poly_upload_range": ([vp, ctypes.c_uint64, sz, u64p, sz], ctypes.c_int),
        "zk_poly_copy_range": ([vp, ctypes.c_uint64, sz, ctypes.c_uint64, sz, sz], ctypes.c_int),
        "zk_poly_lincomb": ([vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), u64p, sz, u64p, sz], ctypes.c_int),
        "zk_lookup_permute": ([vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), sz, ctypes.POINTER(ctypes.c_uint64),
                               ctypes.POINTER(ctypes.c_uint64), sz], ctypes.c_int),
        "zk_lookup_product": ([vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), sz, ctypes.POINTER(ctypes.c_uint64),
                               ctypes.POINTER(ctypes.c_uint64), sz, u64p, u64p, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
        "zk_permutation_product": ([vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), sz, u64p, u64p,
                                    ctypes.POINTER(ctypes.c_uint64), sz], ctypes.c_int),
        "zk_permutation_product_public": ([vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), sz, ctypes.c_uint64, u64p, u64p,
                                           ctypes.POINTER(ctypes.c_uint64), sz], ctypes.c_int),
        "zk_quotient_multi": ([vp, ctypes.c_uint64, sz, ctypes.POINTER(ctypes.c_uint64), sz, ctypes.POINTER(ctypes.c_uint64),
                               ctypes.POINTER(ctypes.c_uint64), sz, ctypes.POINTER(ctypes.c_uint64), sz, u64p, u64p, u64p, ctypes.c_int,
                               ctypes.c_uint64], ctypes.c_int),
        "zk_eval_batch": ([vp, ctypes.POINTER(ctypes.c_uint64), u64p, sz, u64p], ctypes.c_int),
        "zk_pk_export_poly": ([vp, ctypes.c_uint64, ctypes.c_int, sz, ctypes.c_uint64], ctypes.c_int),
        "zk_random_poly": ([vp, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64], ctypes.c_int),
        "zk_vk_read": ([vp, ctypes.POINTER(CircuitParamsC), vp, sz, ctypes.c_int, u64p, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
        "zk_vk_from_parts": ([vp, ctypes.POINTER(CircuitParamsC), u64p, u64p, u64p, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
        "zk_verify": ([vp, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
        "zk_verify_batch": ([vp, ctypes.c_uint64, sz, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz),
                             ctypes.POINTER(ctypes.c_uint8)], ctypes.c_int),
        "zk_witness_check": ([vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), sz, ctypes.POINTER(WitnessFailureC), sz,
                              ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
        "zk_pk_check": ([vp, ctypes.c_uint64, ctypes.POINTER(u32), ctypes.POINTER(PkFindingC), sz, ctypes.POINTER(sz)], ctypes.c_int),
        "zk_stream_placement": ([ctypes.c_int, ctypes.c_int, ctypes.POINTER(PlacementC)], ctypes.c_int),
        "zk_ctx_stream_info": ([vp, ctypes.POINTER(CtxStreamsC)], ctypes.c_int),
        "zk_pairing_check_batch": ([vp, sz, u64p, u64p, u64p, u64p, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8)], ctypes.c_int),
        "zk_pairing_check_each": ([vp, sz, u64p, u64p, u64p, u64p, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8)], ctypes.c_int),
        "zk_srs_contribution_check_batch": ([vp, sz, ctypes.POINTER(SrsContributionC), ctypes.POINTER(u32)], ctypes.c_int),
        "zk_verify_pairing_mode": ([vp, ctypes.c_int], ctypes.c_int),
        "zk_verify_pairing_stats": ([vp, u64p], ctypes.c_int),
        "zk_evm_verifier": ([vp, ctypes.c_uint64, sz, ctypes.POINTER(sz), ctypes.c_int, ctypes.c_char_p, sz, ctypes.POINTER(sz)], ctypes.c_int),
        "zk_evm_verifier_cost": ([vp, ctypes.c_uint64, sz, ctypes.POINTER(sz), ctypes.c_int, ctypes.POINTER(EvmCostC)], ctypes.c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name, None)
        if fn is None:
            if name in ("zk_witness_check", "zk_pk_check", "zk_stream_placement", "zk_ctx_stream_info", "zk_proof_size_multi",
                        "zk_prove_multi", "zk_verify_multi", "zk_prove_public", "zk_verify_public", "zk_witness_check_public",
                        "zk_pk_num_instance_columns", "zk_prove_batch_public", "zk_prove_multi_public", "zk_verify_batch_public",
                        "zk_verify_multi_public", "zk_instance_eval", "zk_verify_instance_eval_mode", "zk_es256_verify",
                        "zk_pairing_check_batch", "zk_verify_pairing_mode", "zk_verify_pairing_stats", "zk_evm_verifier",
                        "zk_evm_verifier_cost", "zk_pairing_check_each", "zk_srs_contribution_check_batch", "zk_webauthn_verify",
                        "zk_webauthn_register") and os.environ.get("ZKMI355_LIB"):
                continue  # an earlier build of the library under A/B (tools/witness_check_time.py --ab-lib): calling it raises AttributeError
            raise ZkError(-4, f"{p} does not export {name} — rebuild it (./build.sh)")
        fn.argtypes = args
        fn.restype = res
    _LIB = L
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def _arr(a, cols):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size % cols:
        raise ValueError("bad array shape")
    return a.reshape(-1, cols)


def _lane_results(count):
    """The verdicts / reasons arrays of a call with one item per lane (an array of one where count is 0: the call then refuses
    it), and what turns them into ([bool verdicts], [int reasons]) after the call."""
    verdicts = (ctypes.c_uint8 * max(count, 1))()
    reasons = (ctypes.c_uint8 * max(count, 1))()
    return verdicts, reasons, lambda: ([bool(verdicts[j]) for j in range(count)], [int(reasons[j]) for j in range(count)])


def _pack_requests(ctype, dicts, strings, fixed32, scalars):
    """The `ctype` array of a sequence of dicts (it keeps their byte strings alive).  strings: the fields of variable length (a
    pointer and NAME_len; origin may be a str), fixed32: the fields of exactly 32 bytes, scalars: (name, default, int or bool)."""
    dicts = list(dicts)
    arr = (ctype * max(len(dicts), 1))()
    for c, q in zip(arr, dicts):
        for name in strings:
            v = q[name].encode() if name == "origin" and isinstance(q[name], str) else bytes(q[name])
            setattr(c, name, v)  # (the structure keeps the bytes object alive)
            setattr(c, name + "_len", len(v))
        for name in fixed32:
            v = bytes(q[name])
            if len(v) != 32:
                raise ValueError(name + ": 32 bytes")
            getattr(c, name)[:] = v
        for name, default, kind in scalars:
            setattr(c, name, int(kind(q.get(name, default))))
    arr.zk_count = len(dicts)  # (an empty list still makes an array of one: the call then refuses count = 0)
    return arr


class Poly:
    """Handle of a device-resident vector of Fr."""

    def __init__(self, eng, handle, n):
        self.eng, self.h, self.n = eng, handle, n

    def free(self):
        if self.h:
            self.eng._chk(self.eng.L.zk_poly_free(self.eng.ctx, self.h), "zk_poly_free")
            self.h = 0


class Engine:
    """One zk_ctx = one HIP device + stream."""

    def __init__(self, device=0, share_with=None):
        """share_with: another Engine on the same device whose resident SRS (bases + window tables) this one uses too
        (zk_ctx_create_shared) instead of loading its own copy."""
        self.L = load_library()
        ctx = ctypes.c_void_p()
        if share_with is not None:
            rc = self.L.zk_ctx_create_shared(share_with.ctx, ctypes.byref(ctx))
        else:
            rc = self.L.zk_ctx_create(device, ctypes.byref(ctx))
        if rc != 0:
            raise ZkError(rc, "zk_ctx_create: " + self.L.zk_strerror(rc).decode())
        self.ctx = ctx

    def close(self):
        if getattr(self, "ctx", None):
            self.L.zk_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise ZkError(rc, what + ": " + self.L.zk_strerror(rc).decode(), self.L.zk_last_hip_error(self.ctx))

    def set_option(self, option, value):
        self._chk(self.L.zk_ctx_set_option(self.ctx, option, value), "zk_ctx_set_option")

    # ---- fine-grained seam ----------------------------------------------------
    def msm_srs(self, scalars_mont, basis):
        """ParamsKZG::commit / commit_lagrange as a Rust host calls it: host scalars, resident basis."""
        s = _arr(scalars_mont, 4)
        out = np.zeros(12, dtype=np.uint64)
        self._chk(self.L.zk_msm_srs(self.ctx, basis, _p(s), s.shape[0], _p(out)), "zk_msm_srs")
        return out

    def msm(self, scalars_mont, bases_mont):
        s = _arr(scalars_mont, 4)
        b = _arr(bases_mont, 8)
        if s.shape[0] != b.shape[0]:
            raise ValueError("scalars / bases length mismatch")
        out = np.zeros(12, dtype=np.uint64)
        self._chk(self.L.zk_msm_bn254(self.ctx, _p(s), _p(b), s.shape[0], _p(out)), "zk_msm_bn254")
        return out

    def ntt(self, a_mont, omega_mont, log_n):
        a = _arr(a_mont, 4).copy()
        if a.shape[0] != (1 << log_n):
            raise ValueError("length != 2^log_n")
        w = np.ascontiguousarray(omega_mont, dtype=np.uint64).reshape(4)
        self._chk(self.L.zk_ntt_bn254_fr(self.ctx, _p(a), _p(w), log_n), "zk_ntt_bn254_fr")
        return a

    # ---- SRS ----------------------------------------------------------------------
    def srs_setup(self, k, seed=bytes(32)):
        if len(seed) != 32:
            raise ValueError("SRS seed must be 32 bytes")
        self._chk(self.L.zk_srs_setup(self.ctx, k, seed), "zk_srs_setup")

    def srs_load(self, k, g, g_lagrange):
        g, gl = _arr(g, 8), _arr(g_lagrange, 8)
        if g.shape[0] != (1 << k) or gl.shape[0] != (1 << k):
            raise ValueError("SRS arrays must hold 2^k points")
        self._chk(self.L.zk_srs_load(self.ctx, k, _p(g), _p(gl)), "zk_srs_load")

    def srs_msm_plan(self):
        c, w = ctypes.c_uint32(), ctypes.c_uint32()
        self._chk(self.L.zk_srs_msm_plan(self.ctx, ctypes.byref(c), ctypes.byref(w)), "zk_srs_msm_plan")
        return c.value, w.value

    def srs_export(self, basis, first, count):
        out = np.zeros((count, 8), dtype=np.uint64)
        self._chk(self.L.zk_srs_export(self.ctx, basis, _p(out), first, count), "zk_srs_export")
        return out

    # ---- the reference's files (ParamsKZG / VerifyingKey / ProvingKey images) ------------
    def _write(self, fn, what, *args):
        ln = ctypes.c_size_t()
        self._chk(fn(self.ctx, *args, None, 0, ctypes.byref(ln)), what)
        buf = np.empty(ln.value, dtype=np.uint8)
        self._chk(fn(self.ctx, *args, buf.ctypes.data, buf.size, ctypes.byref(ln)), what)
        return buf  # numpy uint8 (a k=19 proving key is 768 MiB: no bytes() copy unless the caller wants one)

    @staticmethod
    def _bytes_arg(data):
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        return a, a.ctypes.data, a.size

    def srs_write(self, fmt=ZK_SERDE_RAW_BYTES):
        return self._write(self.L.zk_srs_write, "zk_srs_write", fmt)

    def srs_read(self, data, fmt=ZK_SERDE_RAW_BYTES):
        keep, ptr, n = self._bytes_arg(data)
        self._chk(self.L.zk_srs_read(self.ctx, ptr, n, fmt), "zk_srs_read")

    def srs_set_g2(self, g2, s_g2):
        a, b = (np.ascontiguousarray(v, dtype=np.uint64).reshape(16) for v in (g2, s_g2))
        self._chk(self.L.zk_srs_set_g2(self.ctx, _p(a), _p(b)), "zk_srs_set_g2")

    # ---- an SRS without its secret: ParamsKZG::downsize and the structure check ----------------
    def g_to_lagrange(self, g, k):
        """halo2's g_to_lagrange on 2^k affine Montgomery points ((n, 8) uint64, identity (0, 0)): [1/n] iNTT over G1."""
        a = _arr(g, 8)
        if a.shape[0] != (1 << k):
            raise ValueError("g must hold 2^k points")
        out = np.zeros_like(a)
        self._chk(self.L.zk_g_to_lagrange(self.ctx, _p(a), k, _p(out)), "zk_g_to_lagrange")
        return out

    def srs_downsize(self, k):
        """ParamsKZG::downsize(k) of the resident SRS: the first 2^k points of g, g_lagrange rebuilt on the device."""
        self._chk(self.L.zk_srs_downsize(self.ctx, k), "zk_srs_downsize")

    def srs_read_downsize(self, data, k, fmt=ZK_SERDE_RAW_BYTES):
        """ParamsKZG::read_custom + downsize(k) of a params image of any degree K >= k."""
        keep, ptr, n = self._bytes_arg(data)
        self._chk(self.L.zk_srs_read_downsize(self.ctx, ptr, n, fmt, k), "zk_srs_read_downsize")

    def srs_check(self, seed=bytes(32)):
        """Randomized structure check of the resident SRS: the ZK_SRS_CHECK_* bits of the checks passed (7 = all)."""
        if len(seed) != 32:
            raise ValueError("check seed must be 32 bytes")
        f = ctypes.c_uint32()
        self._chk(self.L.zk_srs_check(self.ctx, bytes(seed), ctypes.byref(f)), "zk_srs_check")
        return f.value

    # ---- one ceremony contribution --------------------------------------------------------------
    CONTRIBUTION_FIELDS = ("before_g1", "after_g1", "s_g1", "s_g2")

    def srs_update(self, seed):
        """Multiplies the secret s = ChaCha20Rng(seed)'s first Fr into the resident SRS (tau -> s tau) and returns the receipt:
        a dict of uint64 limb arrays before_g1, after_g1, s_g1 (8 each) and s_g2 (16).  The caller draws the seed from the
        operating system and discards it."""
        if len(seed) != 32:
            raise ValueError("contribution seed must be 32 bytes")
        c = SrsContributionC()
        self._chk(self.L.zk_srs_update(self.ctx, bytes(seed), ctypes.byref(c)), "zk_srs_update")
        return {f: np.array(getattr(c, f), dtype=np.uint64) for f in self.CONTRIBUTION_FIELDS}

    def srs_contribution_check(self, contribution):
        """The ZK_SRS_CONTRIB_* bits a receipt passes (15 = all; RESIDENT: its after_g1 is this context's g[1])."""
        c = SrsContributionC()
        for f in self.CONTRIBUTION_FIELDS:
            a = np.ascontiguousarray(contribution[f], dtype=np.uint64).reshape(-1)
            if a.size != len(getattr(c, f)):
                raise ValueError("contribution field %s has the wrong length" % f)
            setattr(c, f, type(getattr(c, f))(*[int(x) for x in a]))
        flags = ctypes.c_uint32()
        self._chk(self.L.zk_srs_contribution_check(self.ctx, ctypes.byref(c), ctypes.byref(flags)), "zk_srs_contribution_check")
        return flags.value

    def srs_contribution_check_batch(self, contributions):
        """zk_srs_contribution_check_batch: the flag word of every receipt of a chain (oldest first) in one launch, one receipt per
        lane: srs_contribution_check's bits, plus ZK_SRS_CONTRIB_CHAINED where a receipt's before_g1 is the previous one's after_g1
        (always set for the first).  1 .. ZK_SRS_CONTRIB_BATCH_MAX receipts; needs no SRS.  -> [flag words]"""
        contributions = list(contributions)
        count = len(contributions)
        cs = (SrsContributionC * max(count, 1))()
        for c, contribution in zip(cs, contributions):
            for f in self.CONTRIBUTION_FIELDS:
                a = np.ascontiguousarray(contribution[f], dtype=np.uint64).reshape(-1)
                if a.size != len(getattr(c, f)):
                    raise ValueError("contribution field %s has the wrong length" % f)
                ctypes.memmove(getattr(c, f), a.ctypes.data, a.nbytes)
        flags = (ctypes.c_uint32 * max(count, 1))()
        self._chk(self.L.zk_srs_contribution_check_batch(self.ctx, count, cs, flags), "zk_srs_contribution_check_batch")
        return [int(flags[j]) for j in range(count)]

    def vk_write(self, pk, fmt=ZK_SERDE_RAW_BYTES):
        return self._write(self.L.zk_vk_write, "zk_vk_write", pk, fmt)

    def vk_load(self, pk, data, fmt=ZK_SERDE_RAW_BYTES, transcript_repr=None):
        keep, ptr, n = self._bytes_arg(data)
        t = None if transcript_repr is None else _p(np.ascontiguousarray(transcript_repr, dtype=np.uint64).reshape(4))
        self._chk(self.L.zk_vk_load(self.ctx, pk, ptr, n, fmt, t), "zk_vk_load")

    def pk_write(self, pk, fmt=ZK_SERDE_RAW_BYTES):
        return self._write(self.L.zk_pk_write, "zk_pk_write", pk, fmt)

    def pk_read(self, params, data, fmt=ZK_SERDE_RAW_BYTES, transcript_repr=None):
        cp = self._params_c(params)
        keep, ptr, n = self._bytes_arg(data)
        t = None if transcript_repr is None else _p(np.ascontiguousarray(transcript_repr, dtype=np.uint64).reshape(4))
        h = ctypes.c_uint64()
        self._chk(self.L.zk_pk_read(self.ctx, ctypes.byref(cp), ptr, n, fmt, t, ctypes.byref(h)), "zk_pk_read")
        return h.value

    # ---- resident polynomials ---------------------------------------------------
    def poly(self, n, data=None):
        h = ctypes.c_uint64()
        self._chk(self.L.zk_poly_alloc(self.ctx, n, ctypes.byref(h)), "zk_poly_alloc")
        p = Poly(self, h.value, n)
        if data is not None:
            self.upload(p, data)
        return p

    def upload(self, p, data):
        d = _arr(data, 4)
        self._chk(self.L.zk_poly_upload(self.ctx, p.h, _p(d), d.shape[0]), "zk_poly_upload")

    def download(self, p, n=None):
        n = p.n if n is None else n
        out = np.zeros((n, 4), dtype=np.uint64)
        self._chk(self.L.zk_poly_download(self.ctx, p.h, _p(out), n), "zk_poly_download")
        return out

    def copy(self, dst, src):
        self._chk(self.L.zk_poly_copy(self.ctx, dst.h, src.h), "zk_poly_copy")

    def commit(self, p, basis):
        out = np.zeros(8, dtype=np.uint64)
        self._chk(self.L.zk_commit(self.ctx, p.h, basis, _p(out)), "zk_commit")
        return out

    def commit_batch(self, polys, basis):
        hs = (ctypes.c_uint64 * len(polys))(*[p.h for p in polys])
        out = np.zeros((len(polys), 8), dtype=np.uint64)
        self._chk(self.L.zk_commit_batch(self.ctx, hs, len(polys), basis, _p(out)), "zk_commit_batch")
        return out

    def lagrange_to_coeff(self, p):
        self._chk(self.L.zk_lagrange_to_coeff(self.ctx, p.h), "zk_lagrange_to_coeff")

    def coeff_to_lagrange(self, p):
        self._chk(self.L.zk_coeff_to_lagrange(self.ctx, p.h), "zk_coeff_to_lagrange")

    def coeff_to_extended(self, src, dst):
        self._chk(self.L.zk_coeff_to_extended(self.ctx, src.h, dst.h), "zk_coeff_to_extended")

    def extended_to_coeff(self, ext, n_out):
        self._chk(self.L.zk_extended_to_coeff(self.ctx, ext.h, n_out), "zk_extended_to_coeff")

    def eval(self, p, x_mont):
        x = np.ascontiguousarray(x_mont, dtype=np.uint64).reshape(4)
        out = np.zeros(4, dtype=np.uint64)
        self._chk(self.L.zk_eval(self.ctx, p.h, _p(x), _p(out)), "zk_eval")
        return out

    def poly_detach(self, p):
        """Take a resident vector out of this engine for another one on the same device -> (token, n); see poly_attach."""
        t = ctypes.c_uint64()
        self._chk(self.L.zk_poly_detach(self.ctx, p.h, ctypes.byref(t)), "zk_poly_detach")
        p.h = 0
        return t.value, p.n

    def poly_attach(self, detached):
        """Adopt a vector another engine detached (no copy) -> Poly of this engine."""
        token, n = detached
        h = ctypes.c_uint64()
        self._chk(self.L.zk_poly_attach(self.ctx, token, ctypes.byref(h)), "zk_poly_attach")
        return Poly(self, h.value, n)

    def poly_discard(self, detached):
        """Free a detached vector that will not be attached after all (error paths of a staged load)."""
        self._chk(self.L.zk_poly_discard(detached[0]), "zk_poly_discard")

    def kate_division(self, p, z_mont, q=None):
        """arithmetic::kate_division: q = (p - p(z)) / (X - z), same length as p (top coefficient 0); in place by default."""
        z = np.ascontiguousarray(z_mont, dtype=np.uint64).reshape(4)
        self._chk(self.L.zk_kate_division(self.ctx, p.h, _p(z), (q or p).h), "zk_kate_division")

    def upload_canonical(self, p, data):
        d = _arr(data, 4)
        self._chk(self.L.zk_poly_upload_canonical(self.ctx, p.h, _p(d), d.shape[0]), "zk_poly_upload_canonical")

    # ---- the provers between the commitments (phase-level ABI: the host keeps transcript, RNG and blinding) --------------
    @staticmethod
    def _handles(polys):
        return (ctypes.c_uint64 * max(len(polys), 1))(*[p.h for p in polys])

    @staticmethod
    def _fr(v):
        return _p(np.ascontiguousarray(v, dtype=np.uint64).reshape(4))

    def _outputs(self, count, n):
        out = []
        try:
            for _ in range(count):
                out.append(self.poly(n))
        except ZkError:
            self._drop(out)
            raise
        return out

    @staticmethod
    def _drop(polys):
        for p in polys:
            p.free()

    def lookup_permute(self, pk, advice):
        """zk_lookup_permute: (a', s') of every lookup of the key -> two lists of new Polys the caller frees; rows 0 .. n - 8 are
        written, the 7 rows behind them are the host's blinding (upload_range).  ZkError -6: an input is not in the table."""
        sh = self.pk_shape(pk)
        n, nl = 1 << sh["k"], sh["n_lookups"]
        out = self._outputs(2 * nl, n)
        a, s = out[:nl], out[nl:]
        rc = self.L.zk_lookup_permute(self.ctx, pk, self._handles(advice), len(advice), self._handles(a), self._handles(s), nl)
        if rc:
            self._drop(out)
        self._chk(rc, "zk_lookup_permute")
        return a, s

    def lookup_product(self, pk, advice, permuted_input, permuted_table, beta, gamma):
        """zk_lookup_product: the grand product zL of every lookup (rows 0 .. n - 7) -> list of new Polys the caller frees;
        beta, gamma: Montgomery images."""
        if len(permuted_input) != len(permuted_table):
            raise ValueError("one permuted table per permuted input")
        n = 1 << self.pk_shape(pk)["k"]
        z = self._outputs(len(permuted_input), n)
        rc = self.L.zk_lookup_product(self.ctx, pk, self._handles(advice), len(advice), self._handles(permuted_input),
                                      self._handles(permuted_table), len(permuted_input), self._fr(beta), self._fr(gamma), self._handles(z))
        if rc:
            self._drop(z)
        self._chk(rc, "zk_lookup_product")
        return z

    def permutation_product(self, pk, advice, beta, gamma):
        """zk_permutation_product: the permutation argument's grand products, one per chunk (rows 0 .. n - 7) -> list of new
        Polys the caller frees."""
        sh = self.pk_shape(pk)
        z = self._outputs(sh["n_chunks"], 1 << sh["k"])
        rc = self.L.zk_permutation_product(self.ctx, pk, self._handles(advice), len(advice), self._fr(beta), self._fr(gamma),
                                           self._handles(z), len(z))
        if rc:
            self._drop(z)
        self._chk(rc, "zk_permutation_product")
        return z

    def permutation_product_public(self, pk, advice, instance, beta, gamma, z_out=None):
        """zk_permutation_product_public: permutation_product for a key with the instance column; `instance`: the resident column
        (public inputs in rows 0 .. m - 1, zero behind them), None for a key without one -> list of new Polys the caller frees,
        or z_out (one Poly per chunk) where the caller brings the outputs."""
        sh = self.pk_shape(pk)
        z = self._outputs(sh["n_chunks"], 1 << sh["k"]) if z_out is None else list(z_out)
        rc = self.L.zk_permutation_product_public(self.ctx, pk, self._handles(advice), len(advice), instance.h if instance is not None else 0,
                                                  self._fr(beta), self._fr(gamma), self._handles(z), len(z))
        if rc and z_out is None:
            self._drop(z)
        self._chk(rc, "zk_permutation_product_public")
        return z

    def quotient_multi(self, pk, advice_ext, instance_ext, perm_z_ext, lookup_ext, beta, gamma, y, out_ext, divide=True):
        """zk_quotient_multi: ONE h over len(advice_ext) circuits.  Per circuit: advice_ext[c] its advice cosets, perm_z_ext[c] its
        z cosets, lookup_ext[c] its (a', s', zL) triples, instance_ext[c] its instance coset (instance_ext None: a key without the
        column)."""
        N = len(advice_ext)
        flat = lambda sets: [p for one in sets for p in one]
        lk = [p for one in lookup_ext for trip in one for p in trip]
        self._chk(self.L.zk_quotient_multi(self.ctx, pk, N, self._handles(flat(advice_ext)), len(advice_ext[0]) if N else 0,
                                           None if instance_ext is None else self._handles(instance_ext),
                                           self._handles(flat(perm_z_ext)), len(perm_z_ext[0]) if N else 0, self._handles(lk),
                                           len(lookup_ext[0]) if N else 0, self._fr(beta), self._fr(gamma), self._fr(y),
                                           1 if divide else 0, out_ext.h), "zk_quotient_multi")

    def eval_batch(self, polys, points_mont):
        """zk_eval_batch: polys[i] at points_mont[i] (count, 4) -> (count, 4) Montgomery images, each what eval gives for its pair."""
        x = _arr(points_mont, 4)
        if x.shape[0] != len(polys):
            raise ValueError("one point per polynomial")
        out = np.zeros((len(polys), 4), dtype=np.uint64)
        self._chk(self.L.zk_eval_batch(self.ctx, self._handles(polys), _p(x), len(polys), _p(out)), "zk_eval_batch")
        return out

    def poly_lincomb(self, out, ins, coeffs, sub_low=None):
        """zk_poly_lincomb: out = sum_j coeffs[j] * ins[j] - (sub_low[0] + sub_low[1] X + ..); coeffs (count, 4), sub_low (n_low <= 8, 4),
        Montgomery images."""
        c = _arr(coeffs, 4)
        if c.shape[0] != len(ins):
            raise ValueError("one coefficient per input")
        low = None if sub_low is None else _arr(sub_low, 4)
        n_low = 0 if low is None else low.shape[0]
        self._chk(self.L.zk_poly_lincomb(self.ctx, out.h, self._handles(ins), _p(c), len(ins), _p(low) if n_low else None, n_low),
                  "zk_poly_lincomb")

    def random_poly(self, key, first_block, out):
        """zk_random_poly: out[i] = the Fr::random of ChaCha20 block first_block + i under the 32-byte `key`."""
        if len(key) != 32:
            raise ValueError("ChaCha20 key must be 32 bytes")
        self._chk(self.L.zk_random_poly(self.ctx, bytes(key), first_block, out.h), "zk_random_poly")

    def pk_export_poly(self, pk, which, index, dst):
        """zk_pk_export_poly: coefficient form of the key's fixed column (ZK_PK_FIXED_POLY, query order) or sigma (ZK_PK_SIGMA_POLY)
        number `index` into dst."""
        self._chk(self.L.zk_pk_export_poly(self.ctx, pk, which, index, dst.h), "zk_pk_export_poly")

    def upload_range(self, p, first, data):
        """zk_poly_upload_range: rows [first, first + len(data)) of p from the host (Montgomery images)."""
        d = _arr(data, 4)
        self._chk(self.L.zk_poly_upload_range(self.ctx, p.h, first, _p(d) if d.shape[0] else None, d.shape[0]), "zk_poly_upload_range")

    def copy_range(self, dst, dst_first, src, src_first, count):
        """zk_poly_copy_range: dst[dst_first ..] = src[src_first .. src_first + count)."""
        self._chk(self.L.zk_poly_copy_range(self.ctx, dst.h, dst_first, src.h, src_first, count), "zk_poly_copy_range")

    # ---- keygen / create_proof -------------------------------------------------------
    def keygen(self, params, fixed_canonical, copies):
        """params: circuit.CircuitParams; fixed_canonical: (n_fix, n, 4) uint64 canonical limbs;
        copies: iterable of ((perm_col, row), (perm_col, row)); the instance column of a shape that has one is the last
        permutation column."""
        cp = self._params_c(params)
        fx = np.ascontiguousarray(fixed_canonical, dtype=np.uint64)
        if fx.ndim != 3 or fx.shape[1:] != (1 << params.degree, 4):
            raise ValueError("fixed_canonical must have shape (n_fixed_columns, 2^degree, 4)")
        cps = np.ascontiguousarray(np.array([[a[0], a[1], b[0], b[1]] for a, b in copies], dtype=np.uint32).reshape(-1, 4))
        h = ctypes.c_uint64()
        self._chk(self.L.zk_keygen(self.ctx, ctypes.byref(cp), _p(fx), fx.shape[0],
                                   cps.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), cps.shape[0], ctypes.byref(h)), "zk_keygen")
        return h.value

    def pk_shape(self, pk):
        out = (ctypes.c_uint32 * 8)()
        self._chk(self.L.zk_pk_shape(self.ctx, pk, out), "zk_pk_shape")
        return dict(zip(("k", "ext_k", "n_advice", "n_fixed", "n_perm", "n_chunks", "n_lookups", "n_h"), out))

    def quotient(self, pk, advice_ext, perm_z_ext, lookup_ext, beta, gamma, y, out_ext, divide=True):
        """Evaluator::evaluate_h (+ divide_by_vanishing_poly) over resident extended cosets; lookup_ext: (a', s', zL) per lookup."""
        arr = lambda ps: (ctypes.c_uint64 * max(len(ps), 1))(*[p.h for p in ps])
        flat = [p for trip in lookup_ext for p in trip]
        f = lambda v: _p(np.ascontiguousarray(v, dtype=np.uint64).reshape(4))
        self._chk(self.L.zk_quotient(self.ctx, pk, arr(advice_ext), len(advice_ext), arr(perm_z_ext), len(perm_z_ext), arr(flat),
                                     len(lookup_ext), f(beta), f(gamma), f(y), 1 if divide else 0, out_ext.h), "zk_quotient")

    def pk_set_transcript_repr(self, pk, repr_mont):
        t = np.ascontiguousarray(repr_mont, dtype=np.uint64).reshape(4)
        self._chk(self.L.zk_pk_set_transcript_repr(self.ctx, pk, _p(t)), "zk_pk_set_transcript_repr")

    def pk_free(self, pk):
        self._chk(self.L.zk_pk_free(self.ctx, pk), "zk_pk_free")

    def vk_export(self, pk):
        counts = (ctypes.c_uint32 * 2)()
        self._chk(self.L.zk_vk_export(self.ctx, pk, None, None, None, counts), "zk_vk_export")
        fc = np.zeros((counts[0], 8), dtype=np.uint64)
        pc = np.zeros((counts[1], 8), dtype=np.uint64)
        tr = np.zeros(4, dtype=np.uint64)
        self._chk(self.L.zk_vk_export(self.ctx, pk, _p(fc), _p(pc), _p(tr), counts), "zk_vk_export")
        return fc, pc, tr

    def prove(self, pk, advice_polys, seed=bytes(32), transcript=ZK_TRANSCRIPT_BLAKE2B, scheme=ZK_SCHEME_DEFAULT):
        if len(seed) != 32:
            raise ValueError("rng seed must be 32 bytes")
        hs = (ctypes.c_uint64 * len(advice_polys))(*[p.h for p in advice_polys])
        ln = ctypes.c_size_t()
        self._chk(self.L.zk_proof_size(self.ctx, pk, transcript, scheme, ctypes.byref(ln)), "zk_proof_size")
        buf = ctypes.create_string_buffer(ln.value)
        self._chk(self.L.zk_prove(self.ctx, pk, hs, len(advice_polys), seed, transcript, scheme, buf, len(buf),
                                  ctypes.byref(ln)), "zk_prove")
        return buf.raw[:ln.value]

    @staticmethod
    def _instance_arg(instance_mont):
        """(n, 4) uint64 Montgomery images (or None / empty) -> (array kept alive, pointer or None, count)"""
        a = np.zeros((0, 4), dtype=np.uint64) if instance_mont is None else _arr(instance_mont, 4)
        return a, (_p(a) if a.shape[0] else None), a.shape[0]

    def pk_num_instance_columns(self, pk):
        out = ctypes.c_uint32()
        self._chk(self.L.zk_pk_num_instance_columns(self.ctx, pk, ctypes.byref(out)), "zk_pk_num_instance_columns")
        return out.value

    def prove_public(self, pk, advice_polys, instance_mont, seed=bytes(32), transcript=ZK_TRANSCRIPT_BLAKE2B, scheme=ZK_SCHEME_DEFAULT):
        """zk_prove_public: create_proof with the circuit's public inputs - `instance_mont` (m, 4) uint64 Montgomery images, the first
        m rows of the key's instance column.  A key without the column takes none and gives prove()'s bytes."""
        if len(seed) != 32:
            raise ValueError("rng seed must be 32 bytes")
        hs = (ctypes.c_uint64 * len(advice_polys))(*[p.h for p in advice_polys])
        keep, iptr, ni = self._instance_arg(instance_mont)
        ln = ctypes.c_size_t()
        self._chk(self.L.zk_proof_size(self.ctx, pk, transcript, scheme, ctypes.byref(ln)), "zk_proof_size")
        buf = ctypes.create_string_buffer(ln.value)
        self._chk(self.L.zk_prove_public(self.ctx, pk, hs, len(advice_polys), iptr, ni, seed, transcript, scheme, buf, len(buf),
                                         ctypes.byref(ln)), "zk_prove_public")
        return buf.raw[:ln.value]

    def verify_public(self, pk, proof, instance_mont, transcript, scheme=ZK_SCHEME_DEFAULT) -> bool:
        """zk_verify_public: verify_proof with the public inputs (full or verifying-only key).  Wrong values: False."""
        proof = bytes(proof)
        keep, iptr, ni = self._instance_arg(instance_mont)
        ok = ctypes.c_int(0)
        self._chk(self.L.zk_verify_public(self.ctx, pk, transcript, scheme, iptr, ni, proof, len(proof), ctypes.byref(ok)), "zk_verify_public")
        return bool(ok.value)

    def witness_check_public(self, pk, advice_polys, instance_mont, cap=64):
        """zk_witness_check_public: witness_check() with the instance column's values; the column is the last permutation column."""
        hs = (ctypes.c_uint64 * max(len(advice_polys), 1))(*[p.h for p in advice_polys])
        keep, iptr, ni = self._instance_arg(instance_mont)
        out = (WitnessFailureC * cap)() if cap else None
        counts = (ctypes.c_uint64 * 5)()
        self._chk(self.L.zk_witness_check_public(self.ctx, pk, hs, len(advice_polys), out, cap, counts, iptr, ni), "zk_witness_check_public")
        m = min(cap, int(counts[0]))
        return [int(v) for v in counts], [(f.kind, f.index, f.row, f.other_index, f.other_row) for f in out[:m]] if m else []

    def prove_batch(self, pk, advice_sets, seeds, transcript=ZK_TRANSCRIPT_BLAKE2B, scheme=ZK_SCHEME_DEFAULT):
        """zk_prove_batch: len(advice_sets) independent proofs of one key in lock-step.  advice_sets[j]: proof j's advice
        columns (resident Polys); seeds[j]: its 32-byte RNG seed.  Returns the proofs, each byte-identical to
        prove(pk, advice_sets[j], seeds[j], ...)."""
        B = len(advice_sets)
        if B == 0 or len(seeds) != B or any(len(sd) != 32 for sd in seeds):
            raise ValueError("one 32-byte rng seed per proof")
        na = len(advice_sets[0])
        if any(len(a) != na for a in advice_sets):
            raise ValueError("every proof of a batch has the key's number of advice columns")
        hs = (ctypes.c_uint64 * (B * na))(*[p.h for a in advice_sets for p in a])
        ln = ctypes.c_size_t()
        self._chk(self.L.zk_proof_size(self.ctx, pk, transcript, scheme, ctypes.byref(ln)), "zk_proof_size")
        stride = ln.value
        buf = ctypes.create_string_buffer(stride * B)
        self._chk(self.L.zk_prove_batch(self.ctx, pk, B, hs, na, b"".join(bytes(sd) for sd in seeds), transcript, scheme, buf, stride,
                                        ctypes.byref(ln)), "zk_prove_batch")
        return [buf.raw[j * stride:j * stride + ln.value] for j in range(B)]

    @staticmethod
    def _instance_lists_arg(lists, count):
        """`count` instance lists (each (m, 4) uint64 Montgomery images, None or empty) -> (arrays kept alive, pointer array or None,
        length array or None).  lists None: both NULL - every list empty, for a key without the column."""
        if lists is None:
            return [], None, None
        if len(lists) != count:
            raise ValueError("one instance list per proof / circuit")
        arrs = [np.zeros((0, 4), dtype=np.uint64) if l is None else _arr(l, 4) for l in lists]
        u64p = ctypes.POINTER(ctypes.c_uint64)
        ptrs = (u64p * count)(*[_p(a) if a.shape[0] else ctypes.cast(None, u64p) for a in arrs])
        lens = (ctypes.c_size_t * count)(*[a.shape[0] for a in arrs])
        return arrs, ptrs, lens

    def prove_batch_public(self, pk, advice_sets, instance_lists, seeds, transcript=ZK_TRANSCRIPT_BLAKE2B, scheme=ZK_SCHEME_DEFAULT):
        """zk_prove_batch_public: prove_batch with instance_lists[j] the public inputs of proof j (lists may differ in length; None
        for a key without the column).  Proof j is byte-identical to prove_public(pk, advice_sets[j], instance_lists[j], seeds[j])."""
        B = len(advice_sets)
        if B == 0 or len(seeds) != B or any(len(sd) != 32 for sd in seeds):
            raise ValueError("one 32-byte rng seed per proof")
        na = len(advice_sets[0])
        if any(len(a) != na for a in advice_sets):
            raise ValueError("every proof of a batch has the key's number of advice columns")
        hs = (ctypes.c_uint64 * (B * na))(*[p.h for a in advice_sets for p in a])
        keep, iptrs, ilens = self._instance_lists_arg(instance_lists, B)
        ln = ctypes.c_size_t()
        self._chk(self.L.zk_proof_size(self.ctx, pk, transcript, scheme, ctypes.byref(ln)), "zk_proof_size")
        stride = ln.value
        buf = ctypes.create_string_buffer(stride * B)
        self._chk(self.L.zk_prove_batch_public(self.ctx, pk, B, hs, na, iptrs, ilens, b"".join(bytes(sd) for sd in seeds), transcript, scheme,
                                               buf, stride, ctypes.byref(ln)), "zk_prove_batch_public")
        return [buf.raw[j * stride:j * stride + ln.value] for j in range(B)]

    def prove_multi_public(self, pk, advice_sets, instance_lists, seed=bytes(32), transcript=ZK_TRANSCRIPT_BLAKE2B, scheme=ZK_SCHEME_DEFAULT):
        """zk_prove_multi_public: prove_multi with instance_lists[c] the public inputs of circuit c (halo2's create_proof with several
        circuits and their instances).  One circuit gives prove_public()'s bytes."""
        N = len(advice_sets)
        if len(seed) != 32:
            raise ValueError("rng seed must be 32 bytes")
        na = len(advice_sets[0]) if N else 0
        if any(len(a) != na for a in advice_sets):
            raise ValueError("every circuit has the key's number of advice columns")
        hs = (ctypes.c_uint64 * max(N * na, 1))(*[p.h for a in advice_sets for p in a])
        keep, iptrs, ilens = self._instance_lists_arg(instance_lists, N)
        ln = ctypes.c_size_t()
        self._chk(self.L.zk_proof_size_multi(self.ctx, pk, N, transcript, scheme, ctypes.byref(ln)), "zk_proof_size_multi")
        buf = ctypes.create_string_buffer(ln.value)
        self._chk(self.L.zk_prove_multi_public(self.ctx, pk, N, hs, na, iptrs, ilens, seed, transcript, scheme, buf, len(buf), ctypes.byref(ln)),
                  "zk_prove_multi_public")
        return buf.raw[:ln.value]

    def verify_multi_public(self, pk, proof, instance_lists, transcript, scheme=ZK_SCHEME_DEFAULT) -> bool:
        """zk_verify_multi_public: verify_proof of one proof over len(instance_lists) circuits with their public inputs."""
        proof = bytes(proof)
        N = len(instance_lists)
        keep, iptrs, ilens = self._instance_lists_arg(instance_lists, N)
        ok = ctypes.c_int(0)
        self._chk(self.L.zk_verify_multi_public(self.ctx, pk, N, transcript, scheme, iptrs, ilens, proof, len(proof), ctypes.byref(ok)),
                  "zk_verify_multi_public")
        return bool(ok.value)

    def verify_batch_public(self, pk, proofs, instance_lists, transcript, scheme=ZK_SCHEME_DEFAULT):
        """zk_verify_batch_public: one verdict per proof, each what verify_public(pk, proofs[j], instance_lists[j]) says (batches above
        ZK_VERIFY_BATCH_MAX are split).  instance_lists None: a key without the column."""
        proofs = [bytes(p) for p in proofs]
        if instance_lists is not None and len(instance_lists) != len(proofs):
            raise ValueError("one instance list per proof")
        out = []
        for lo in range(0, len(proofs), ZK_VERIFY_BATCH_MAX):
            part = proofs[lo:lo + ZK_VERIFY_BATCH_MAX]
            keep, iptrs, ilens = self._instance_lists_arg(None if instance_lists is None else instance_lists[lo:lo + len(part)], len(part))
            ptrs = (ctypes.c_char_p * len(part))(*part)
            lens = (ctypes.c_size_t * len(part))(*[len(p) for p in part])
            v = (ctypes.c_uint8 * len(part))()
            self._chk(self.L.zk_verify_batch_public(self.ctx, pk, len(part), transcript, scheme, iptrs, ilens, ptrs, lens, v), "zk_verify_batch_public")
            out.extend(bool(x) for x in v)
        return out

    def set_verify_instance_eval(self, mode):
        """zk_verify_instance_eval_mode: where verify_batch_public / verify_multi_public evaluate inst(x) - 0 auto (the host), 1 host,
        2 device.  Same verdicts."""
        self._chk(self.L.zk_verify_instance_eval_mode(self.ctx, mode), "zk_verify_instance_eval_mode")

    def instance_eval(self, k, instance_lists, xs_mont):
        """zk_instance_eval: inst(x) of len(instance_lists) (list, point) pairs over the domain of 2^k rows, on the device ->
        ((count, 4) uint64 Montgomery values, [on_domain flags]).  Lists that are the SAME object are uploaded once."""
        count = len(instance_lists)
        xs = _arr(xs_mont, 4)
        if xs.shape[0] != count:
            raise ValueError("one point per list")
        same = {}
        arrs = []
        for l in instance_lists:
            a = same.get(id(l))
            if a is None:
                a = same[id(l)] = np.zeros((0, 4), dtype=np.uint64) if l is None else _arr(l, 4)
            arrs.append(a)
        u64p = ctypes.POINTER(ctypes.c_uint64)
        ptrs = (u64p * max(count, 1))(*[_p(a) if a.shape[0] else ctypes.cast(None, u64p) for a in arrs])
        lens = (ctypes.c_size_t * max(count, 1))(*[a.shape[0] for a in arrs])
        out = np.zeros((count, 4), dtype=np.uint64)
        flags = (ctypes.c_uint8 * max(count, 1))()
        self._chk(self.L.zk_instance_eval(self.ctx, k, count, ptrs, lens, _p(xs), _p(out), flags), "zk_instance_eval")
        return out, [bool(flags[j]) for j in range(count)]

    def es256_verify(self, sigs):
        """zk_es256_verify: secp256r1 ECDSA verification of len(sigs) // 160 requests in one launch, one signature per lane.  sigs:
        the records back to back (bytes), each pubkey_x || pubkey_y || r || s || msghash as 32 little-endian bytes - or a sequence
        of such 160-byte records.  -> ([bool verdicts], [ZK_ES256_* reasons]); a bad signature is a verdict, not an error."""
        if not isinstance(sigs, (bytes, bytearray, memoryview)):
            sigs = b"".join(bytes(r) for r in sigs)
        sigs = bytes(sigs)
        if len(sigs) % 160:
            raise ValueError("a record is 160 bytes")
        count = len(sigs) // 160
        verdicts, reasons, unpack = _lane_results(count)
        self._chk(self.L.zk_es256_verify(self.ctx, count, sigs, verdicts, reasons), "zk_es256_verify")
        return unpack()

    def webauthn_verify(self, assertions):
        """zk_webauthn_verify: the relying party's check of WebAuthn assertions in two launches, one assertion per lane - both hashes,
        the rules for authenticatorData and clientDataJSON, the DER parse, then zk_es256_verify's rule over the record it assembled.
        assertions: a sequence of dicts with authenticator_data, client_data_json, signature (DER), pubkey_x, pubkey_y (32 BIG-endian
        bytes each), challenge (the raw bytes issued), origin (str or bytes), rp_id_hash (32 bytes) and, optionally, flags_required
        (default 0x01, UP) and allow_cross_origin (default False).  -> ([bool verdicts], [ZK_WEBAUTHN_* reasons], [160-byte records],
        [signature counters]); a bad assertion is a verdict, not an error.  A caller that makes the same call again (a measurement)
        passes webauthn_pack's result instead and skips the marshalling."""
        arr = assertions if isinstance(assertions, ctypes.Array) else self.webauthn_pack(assertions)
        count = len(arr) if getattr(arr, "zk_count", 1) else 0
        verdicts, reasons, unpack = _lane_results(count)
        records = (ctypes.c_uint8 * (160 * max(count, 1)))()
        counts = (ctypes.c_uint32 * max(count, 1))()
        self._chk(self.L.zk_webauthn_verify(self.ctx, count, arr, verdicts, reasons, records, counts), "zk_webauthn_verify")
        raw = bytes(records)
        return unpack() + ([raw[160 * j:160 * j + 160] for j in range(count)], [int(counts[j]) for j in range(count)])

    @staticmethod
    def webauthn_pack(assertions):
        """The zk_webauthn_assertion array of webauthn_verify's dicts (it keeps their byte strings alive)."""
        return _pack_requests(WebauthnAssertionC, assertions, ("authenticator_data", "client_data_json", "signature", "challenge", "origin"),
                              ("pubkey_x", "pubkey_y", "rp_id_hash"), (("flags_required", 0x01, int), ("allow_cross_origin", False, bool)))

    def webauthn_register(self, registrations):
        """zk_webauthn_register: the relying party's check of WebAuthn registrations in two launches, one per lane - the CBOR walk of
        the attestationObject, the authData and attested-credential-data rules, the COSE key template, the client-data rule with
        webauthn.create, the key's curve test and, under policy ZK_WEBAUTHN_ATT_NONE_OR_SELF, the statement (a packed self
        attestation is verified with the credential's own key).  registrations: a sequence of dicts with attestation_object,
        client_data_json, challenge (the raw bytes issued), origin (str or bytes), rp_id_hash (32 bytes) and, optionally,
        flags_required (default 0x01, UP), allow_cross_origin (default False) and attestation_policy (default
        ZK_WEBAUTHN_ATT_IGNORE).  -> [(ok, ZK_WEBAUTHN_* reason, credential dict or None)]: pubkey_x, pubkey_y (32 BIG-endian bytes,
        what webauthn_verify takes), aaguid, credential_id, auth_data (both cut out of the object), sign_count, flags, attestation
        (ZK_WEBAUTHN_ATTESTED_*).  A bad registration is a verdict, not an error.  A caller that makes the same call again (a
        measurement) passes webauthn_register_pack's result instead and skips the marshalling."""
        arr = registrations if isinstance(registrations, ctypes.Array) else self.webauthn_register_pack(registrations)
        count = len(arr) if getattr(arr, "zk_count", 1) else 0
        verdicts, reasons, unpack = _lane_results(count)
        creds = (WebauthnCredentialC * max(count, 1))()
        self._chk(self.L.zk_webauthn_register(self.ctx, count, arr, verdicts, reasons, creds), "zk_webauthn_register")
        out = []
        for j, (ok, reason) in enumerate(zip(*unpack())):
            cred = None
            if ok:
                c, obj = creds[j], arr.zk_objects[j]  # (reading the c_char_p field back would stop at the first zero byte)
                cred = {"pubkey_x": bytes(c.pubkey_x), "pubkey_y": bytes(c.pubkey_y), "aaguid": bytes(c.aaguid),
                        "credential_id": obj[c.credential_id_off:c.credential_id_off + c.credential_id_len],
                        "auth_data": obj[c.auth_data_off:c.auth_data_off + c.auth_data_len], "auth_data_off": int(c.auth_data_off),
                        "auth_data_len": int(c.auth_data_len), "credential_id_off": int(c.credential_id_off),
                        "credential_id_len": int(c.credential_id_len), "sign_count": int(c.sign_count), "flags": int(c.flags),
                        "attestation": int(c.attestation)}
            out.append((ok, reason, cred))
        return out

    @staticmethod
    def webauthn_register_pack(registrations):
        """The zk_webauthn_registration array of webauthn_register's dicts (it keeps their byte strings alive)."""
        registrations = list(registrations)
        arr = _pack_requests(WebauthnRegistrationC, registrations, ("attestation_object", "client_data_json", "challenge", "origin"), ("rp_id_hash",),
                             (("flags_required", 0x01, int), ("allow_cross_origin", False, bool), ("attestation_policy", ZK_WEBAUTHN_ATT_IGNORE, int)))
        arr.zk_objects = [bytes(q["attestation_object"]) for q in registrations]  # the offsets of a credential count within these
        return arr

    def pairing_check_batch(self, a, b, g2=None, s_g2=None):
        """zk_pairing_check_batch: e(a_i, s_g2) = e(b_i, g2) for every pair in one launch, one check per lane.  a, b: (count, 8)
        uint64 affine Montgomery points ((0, 0): the identity); g2, s_g2: 16-word Montgomery images as set_g2 takes them, or both
        None for the resident SRS's pair.  -> ([bool verdicts], [ZK_PAIRING_* reasons]); a bad pair is a verdict, not an error."""
        a, b = _arr(a, 8), _arr(b, 8)
        if a.shape[0] != b.shape[0]:
            raise ValueError("one b per a")
        count = a.shape[0]
        u64p = ctypes.POINTER(ctypes.c_uint64)
        gp = [ctypes.cast(None, u64p) if g is None else _p(np.ascontiguousarray(g, dtype=np.uint64).reshape(16)) for g in (g2, s_g2)]
        verdicts, reasons, unpack = _lane_results(count)
        self._chk(self.L.zk_pairing_check_batch(self.ctx, count, _p(a), _p(b), gp[0], gp[1], verdicts, reasons), "zk_pairing_check_batch")
        return unpack()

    def pairing_check_each(self, a, b, q, g2=None):
        """zk_pairing_check_each: e(a_i, q_i) = e(b_i, g2) with a G2 point per item, one check per lane; every lane tests and walks
        its own q_i.  a, b: (count, 8) uint64 affine Montgomery points; q: (count, 16) Montgomery images as set_g2 takes them; g2: one
        such image, or None for the resident SRS's.  -> ([bool verdicts], [ZK_PAIRING_* reasons]; ZK_PAIRING_G2: q_i not a proper
        point); a bad item is a verdict, not an error."""
        a, b, q = _arr(a, 8), _arr(b, 8), _arr(q, 16)
        if a.shape[0] != b.shape[0] or a.shape[0] != q.shape[0]:
            raise ValueError("one b and one q per a")
        count = a.shape[0]
        gp = ctypes.cast(None, ctypes.POINTER(ctypes.c_uint64)) if g2 is None else _p(np.ascontiguousarray(g2, dtype=np.uint64).reshape(16))
        verdicts, reasons, unpack = _lane_results(count)
        self._chk(self.L.zk_pairing_check_each(self.ctx, count, _p(a), _p(b), _p(q), gp, verdicts, reasons), "zk_pairing_check_each")
        return unpack()

    def verify_pairing_mode(self, mode):
        """zk_verify_pairing_mode: how verify_batch / verify_batch_public settle a failing fold of two or more proofs - 0 auto (the
        host), 1 host (bisection), 2 device (one launch of the device pairing over the whole set).  Same verdicts."""
        self._chk(self.L.zk_verify_pairing_mode(self.ctx, mode), "zk_verify_pairing_mode")

    def verify_pairing_stats(self):
        """zk_verify_pairing_stats -> (host pairing checks, device-checked pairs) of this engine's verify calls since it was made"""
        out = (ctypes.c_uint64 * 2)()
        self._chk(self.L.zk_verify_pairing_stats(self.ctx, out), "zk_verify_pairing_stats")
        return int(out[0]), int(out[1])

    def proof_size_multi(self, pk, n_circuits, transcript=ZK_TRANSCRIPT_BLAKE2B, scheme=ZK_SCHEME_DEFAULT):
        ln = ctypes.c_size_t()
        self._chk(self.L.zk_proof_size_multi(self.ctx, pk, n_circuits, transcript, scheme, ctypes.byref(ln)), "zk_proof_size_multi")
        return ln.value

    def prove_multi(self, pk, advice_sets, seed=bytes(32), transcript=ZK_TRANSCRIPT_BLAKE2B, scheme=ZK_SCHEME_DEFAULT):
        """zk_prove_multi: ONE proof over len(advice_sets) circuits of one key (halo2's create_proof with several circuits): one
        transcript, one RNG stream from `seed`, one quotient, one multi-open.  advice_sets[c]: circuit c's advice columns
        (resident Polys).  One circuit gives prove()'s bytes."""
        N = len(advice_sets)
        if len(seed) != 32:
            raise ValueError("rng seed must be 32 bytes")
        na = len(advice_sets[0]) if N else 0
        if any(len(a) != na for a in advice_sets):
            raise ValueError("every circuit has the key's number of advice columns")
        hs = (ctypes.c_uint64 * max(N * na, 1))(*[p.h for a in advice_sets for p in a])
        ln = ctypes.c_size_t()
        self._chk(self.L.zk_proof_size_multi(self.ctx, pk, N, transcript, scheme, ctypes.byref(ln)), "zk_proof_size_multi")
        buf = ctypes.create_string_buffer(ln.value)
        self._chk(self.L.zk_prove_multi(self.ctx, pk, N, hs, na, seed, transcript, scheme, buf, len(buf), ctypes.byref(ln)), "zk_prove_multi")
        return buf.raw[:ln.value]

    def verify_multi(self, pk, n_circuits, proof, transcript, scheme=ZK_SCHEME_DEFAULT) -> bool:
        """zk_verify_multi: verify_proof of one proof over n_circuits circuits (full or verifying-only key)."""
        proof = bytes(proof)
        ok = ctypes.c_int(0)
        self._chk(self.L.zk_verify_multi(self.ctx, pk, n_circuits, transcript, scheme, proof, len(proof), ctypes.byref(ok)), "zk_verify_multi")
        return bool(ok.value)

    def witness_check(self, pk, advice_polys, cap=64):
        """MockProver::verify of resident advice columns against a resident key (zk_witness_check) -> (counts, failures):
        counts[kind] = failures of each ZK_FAIL_* kind (counts[0] their sum); failures = the first min(cap, counts[0]) of them
        in ascending (kind, index, row) order as (kind, index, row, other_index, other_row) tuples.  A violated circuit is a
        verdict, not an error; nothing is proved and nothing a proof is made of changes."""
        hs = (ctypes.c_uint64 * max(len(advice_polys), 1))(*[p.h for p in advice_polys])
        out = (WitnessFailureC * cap)() if cap else None
        counts = (ctypes.c_uint64 * 5)()
        self._chk(self.L.zk_witness_check(self.ctx, pk, hs, len(advice_polys), out, cap, counts), "zk_witness_check")
        m = min(cap, int(counts[0]))
        return [int(v) for v in counts], [(f.kind, f.index, f.row, f.other_index, f.other_row) for f in out[:m]] if m else []

    def pk_check(self, pk, cap=64):
        """The audit of a resident proving key (zk_pk_check) -> (flags, findings): flags = ZK_PK_CHECK_* bits (flags & ZK_PK_CHECK_ALL
        == ZK_PK_CHECK_ALL: the key is what keygen would have made of its own values); findings = the first min(cap, total) of
        one (part, column, index, count) tuple per ZK_PK_PART_* and column with a mismatch - its lowest index and how many - in
        ascending (part, column) order.  A broken key is a verdict, not an error; the key and every proof byte are unchanged."""
        out = (PkFindingC * cap)() if cap else None
        flags, total = ctypes.c_uint32(0), ctypes.c_size_t(0)
        self._chk(self.L.zk_pk_check(self.ctx, pk, ctypes.byref(flags), out, cap, ctypes.byref(total)), "zk_pk_check")
        m = min(cap, total.value)
        return flags.value, [(f.part, f.column, f.index, int(f.count)) for f in out[:m]] if m else []

    # ---- verify_proof ----------------------------------------------------------------------------------
    @staticmethod
    def _params_c(params):
        return CircuitParamsC(params.degree, params.num_advice, params.num_lookup_advice, params.num_fixed, params.lookup_bits,
                              getattr(params, "idle_gate_columns", 0), getattr(params, "num_instance_columns", 0))

    def vk_read(self, params, data, fmt=ZK_SERDE_RAW_BYTES, transcript_repr=None):
        """VerifyingKey::read: a verifying-only key (commitments + transcript_repr, no prover state) from a zk_vk_write image."""
        cp = self._params_c(params)
        keep, ptr, n = self._bytes_arg(data)
        t = None if transcript_repr is None else _p(np.ascontiguousarray(transcript_repr, dtype=np.uint64).reshape(4))
        h = ctypes.c_uint64()
        self._chk(self.L.zk_vk_read(self.ctx, ctypes.byref(cp), ptr, n, fmt, t, ctypes.byref(h)), "zk_vk_read")
        return h.value

    def vk_from_parts(self, params, fixed_commitments, perm_commitments, transcript_repr=None):
        """The inverse of vk_export: a verifying-only key from affine Montgomery commitments ((n, 8) uint64 each)."""
        from .circuit import Layout

        cp = self._params_c(params)
        fc, pc = _arr(fixed_commitments, 8), _arr(perm_commitments, 8)
        lay = Layout(params)  # (the C entry point reads exactly the shape's counts)
        if fc.shape[0] != lay.n_fix or pc.shape[0] != len(lay.perm_cols):
            raise ZkError(-1, f"zk_vk_from_parts: the shape has {lay.n_fix} fixed and {len(lay.perm_cols)} permutation commitments")
        t = None if transcript_repr is None else _p(np.ascontiguousarray(transcript_repr, dtype=np.uint64).reshape(4))
        h = ctypes.c_uint64()
        self._chk(self.L.zk_vk_from_parts(self.ctx, ctypes.byref(cp), _p(fc), _p(pc), t, ctypes.byref(h)), "zk_vk_from_parts")
        return h.value

    def verify(self, pk, proof, transcript, scheme=ZK_SCHEME_DEFAULT) -> bool:
        """plonk::verify_proof with the KZG pairing check against the resident SRS (zk_verify)."""
        proof = bytes(proof)
        ok = ctypes.c_int(0)
        self._chk(self.L.zk_verify(self.ctx, pk, transcript, scheme, proof, len(proof), ctypes.byref(ok)), "zk_verify")
        return bool(ok.value)

    @staticmethod
    def _evm_counts(n_circuits, n_instances):
        if n_instances is None:
            return None
        if len(n_instances) != n_circuits:
            raise ValueError("one instance count per circuit")
        return (ctypes.c_size_t * max(n_circuits, 1))(*[int(m) for m in n_instances])

    def evm_verifier(self, pk, n_circuits=1, n_instances=None, scheme=ZK_SCHEME_DEFAULT) -> str:
        """zk_evm_verifier: the text of the Yul program that verifies, on the EVM, ONE proof of `pk` (full or verifying-only) over
        n_circuits circuits with n_instances[c] public inputs in circuit c (None: none), made with the EVM transcript and `scheme`
        (default GWC) under the resident SRS.  Its calldata is ecdsa_p256.encode_calldata's: all instances, then the proof."""
        counts = self._evm_counts(n_circuits, n_instances)
        ln = ctypes.c_size_t()
        self._chk(self.L.zk_evm_verifier(self.ctx, pk, n_circuits, counts, scheme, None, 0, ctypes.byref(ln)), "zk_evm_verifier")
        buf = ctypes.create_string_buffer(ln.value)
        self._chk(self.L.zk_evm_verifier(self.ctx, pk, n_circuits, counts, scheme, buf, len(buf), ctypes.byref(ln)), "zk_evm_verifier")
        return buf.raw[:ln.value].decode("ascii")

    def evm_verifier_cost(self, pk, n_circuits=1, n_instances=None, scheme=ZK_SCHEME_DEFAULT) -> dict:
        """zk_evm_verifier_cost: that program's calldata length, memory top, precompile calls (modexp, ecadd, ecmul, pairing) and
        keccak256 calls / hashed bytes, counted where it is generated."""
        out = EvmCostC()
        self._chk(self.L.zk_evm_verifier_cost(self.ctx, pk, n_circuits, self._evm_counts(n_circuits, n_instances), scheme, ctypes.byref(out)),
                  "zk_evm_verifier_cost")
        return {n: int(getattr(out, n)) for n, _ in EvmCostC._fields_}

    def verify_batch(self, pk, proofs, transcript, scheme=ZK_SCHEME_DEFAULT):
        """zk_verify_batch: one verdict per proof, each what verify() says of it (batches above ZK_VERIFY_BATCH_MAX are split)."""
        proofs = [bytes(p) for p in proofs]
        out = []
        for lo in range(0, len(proofs), ZK_VERIFY_BATCH_MAX):
            part = proofs[lo:lo + ZK_VERIFY_BATCH_MAX]
            ptrs = (ctypes.c_char_p * len(part))(*part)
            lens = (ctypes.c_size_t * len(part))(*[len(p) for p in part])
            v = (ctypes.c_uint8 * len(part))()
            self._chk(self.L.zk_verify_batch(self.ctx, pk, len(part), transcript, scheme, ptrs, lens, v), "zk_verify_batch")
            out.extend(bool(x) for x in v)
        return out

    def proof_size(self, pk, transcript=ZK_TRANSCRIPT_BLAKE2B, scheme=ZK_SCHEME_DEFAULT):
        ln = ctypes.c_size_t()
        self._chk(self.L.zk_proof_size(self.ctx, pk, transcript, scheme, ctypes.byref(ln)), "zk_proof_size")
        return ln.value

    def sync(self):
        self._chk(self.L.zk_sync(self.ctx), "zk_sync")

    def timer_reset(self):
        self._chk(self.L.zk_timer_reset(self.ctx), "zk_timer_reset")

    def timer_stats(self, which):
        t, n = ctypes.c_double(), ctypes.c_uint64()
        self._chk(self.L.zk_timer_stats(self.ctx, which, ctypes.byref(t), ctypes.byref(n)), "zk_timer_stats")
        return t.value, n.value

    def audit_report(self):
        """(ordering checks made, violations, description of the first violation) of ZK_OPT_STREAM_AUDIT (zk_audit_report)."""
        counts = (ctypes.c_uint64 * 2)()
        msg = ctypes.create_string_buffer(600)
        self._chk(self.L.zk_audit_report(self.ctx, counts, msg, len(msg)), "zk_audit_report")
        return int(counts[0]), int(counts[1]), msg.value.decode(errors="replace")

    def stream_info(self):
        """This context's streams (zk_ctx_stream_info): its slot in the device's pool (-1: its own streams), the class of its
        main / tail / transform / MSM stream as stream_placement last measured them (255: not measured yet), and four counts
        since creation: MSM passes with the tail on the main / on the tail stream, proofs that took the transform / the MSM stream."""
        r = CtxStreamsC()
        self._chk(self.L.zk_ctx_stream_info(self.ctx, ctypes.byref(r)), "zk_ctx_stream_info")
        return {"slot": r.slot, "queue": list(r.queue), "counts": list(r.counts)}

    def clock_probe(self, millis=100):
        """(shader-clock ticks, 100 MHz ticks, dependent multiply-adds issued) over ~`millis` ms of one spinning wave (zk_clock_probe)."""
        out = (ctypes.c_uint64 * 4)()
        self._chk(self.L.zk_clock_probe(self.ctx, millis, out), "zk_clock_probe")
        return int(out[0]), int(out[1]), int(out[2])

    def last_ms(self, which):
        v = ctypes.c_float()
        self._chk(self.L.zk_last_kernel_ms(self.ctx, which, ctypes.byref(v)), "zk_last_kernel_ms")
        return v.value
