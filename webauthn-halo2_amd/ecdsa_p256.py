"""Host-side mirror of the reference's proving API (halo2-circuits/src/ecc/ecdsa_p256.rs) on top of
the resident engine.

    download_keys(degree, proving_key_path, verifying_key_path)        ecdsa_p256.rs:256-272
    create_proof_from_advice(advice_columns, ..., transcript)          the engine's real input: the advice
                                                                       columns `ECDSACircuit::synthesize`
                                                                       (ecdsa_p256.rs:117-206) leaves behind
    mock_verify_advice(advice_columns, proving_key_path, degree)       MockProver::run(..).verify() of such columns
                                                                       (test_secp256r1_ecdsa, ecdsa_p256.rs:209-248)
    generate_proof_synthetic / generate_proof_evm_synthetic            request-shaped stand-ins for
                                                                       generate_proof (:379-427) / _evm (:329-377)

What the scope of this repository imposes, stated where a caller will read it:

  * The reference re-reads the SRS and the proving key from disk on EVERY request
    (ecdsa_p256.rs:338-343); here `gen_srs` and the key stay resident on the device
     — the path arguments select a cached, resident key.
  * The secp256r1 witness generation (`ECDSACircuit::synthesize`) needs the Rust halo2-ecc chips and stays
    on the host side of the real integration.  The product entry point is therefore
    `create_proof_from_advice`: it takes advice columns and proves them.
  * The request-shaped functions carry `_synthetic` in their name because the circuit they prove is the
    SAME-SHAPE SYNTHETIC circuit of `circuit.synthesize`, not the secp256r1 verification circuit: a proof
    from them says nothing about the signature inside the SNARK.  They do check the ES256 signature on the
    host first (plain secp256r1 ECDSA verification of (r, s) over msg_hash under the public key) and refuse
    an invalid request, so that, unlike a bare seed-hash, an invalid signature or arbitrary bytes never
    yields a verifying proof.  The reference's `generate_proof*` names are deliberately NOT exported.
  * `verify` / `verify_evm` (ecdsa_p256.rs:429-469) check a proof against the resident `gen_srs(degree)` with a real
    pairing (zk_verify): the verifying key file is read once into a cached verifying-only key (re-read when the file
    changes), the proof points are decoded and the check's multi-scalar sums made on the device, the pairing on the host.
    `verify_batch` sends many proofs of one key through one zk_verify_batch call.
  * PUBLIC INPUTS are an extension: the reference circuit has none (`num_instance = vec![]`), so its proofs are bound neither
    to the message hash nor to the account's key.  `download_keys(public=True)` makes the key of the same shape with ONE instance
    column; `create_proof_from_advice` / `verify` / `verify_evm` / `mock_verify_advice` take `instances` (canonical integers),
    the `_synthetic` request functions with public=True expose msghash, pubkey_x and pubkey_y as `public_inputs` gives them,
    and `encode_calldata` lays instances and proof out as snark-verifier's verifier contracts read them.  The rule is
    [RECALLED] (include/zkmi355.h "public inputs").
"""
import base64
import dataclasses
import hashlib
import os
import queue
import threading
import time

import numpy as np

from . import circuit
from .engine import (ZK_PK_CHECK_ALL, ZK_SCHEME_DEFAULT, ZK_SCHEME_GWC, ZK_SCHEME_SHPLONK, ZK_SERDE_RAW_BYTES, ZK_SRS_CONTRIB_LINKS,
                     ZK_SRS_CONTRIB_BATCH_MAX, ZK_SRS_CONTRIB_CHAINED, ZK_SRS_CONTRIB_NONTRIVIAL, ZK_SRS_CONTRIB_RESIDENT,
                     ZK_SRS_CONTRIB_SAME_SECRET, ZK_TRANSCRIPT_BLAKE2B,
                     ZK_ES256_BATCH_MAX, ZK_TRANSCRIPT_EVM, Engine, ZkError, stream_placement)
from .engine import (WEBAUTHN_REASON_NAMES, ZK_WEBAUTHN_AUTHDATA, ZK_WEBAUTHN_AUTHDATA_MAX, ZK_WEBAUTHN_BATCH_MAX, ZK_WEBAUTHN_CHALLENGE_MAX,
                     ZK_WEBAUTHN_CLIENTDATA, ZK_WEBAUTHN_CLIENTDATA_MAX, ZK_WEBAUTHN_FLAGS, ZK_WEBAUTHN_MISMATCH, ZK_WEBAUTHN_OFF_CURVE,
                     ZK_WEBAUTHN_ORIGIN_MAX, ZK_WEBAUTHN_RANGE, ZK_WEBAUTHN_RPID, ZK_WEBAUTHN_SIGNATURE_DER, ZK_WEBAUTHN_SIZE, ZK_WEBAUTHN_VALID,
                     ZK_WEBAUTHN_ATT_IGNORE, ZK_WEBAUTHN_ATT_NONE_OR_SELF, ZK_WEBAUTHN_ATTESTATION, ZK_WEBAUTHN_ATTESTED_NONE,
                     ZK_WEBAUTHN_ATTESTED_NOT_JUDGED, ZK_WEBAUTHN_ATTESTED_SELF, ZK_WEBAUTHN_ATTOBJ_MAX, ZK_WEBAUTHN_CBOR, ZK_WEBAUTHN_COSE_KEY,
                     ZK_WEBAUTHN_CREDENTIAL)

# (device) -> {"eng": Engine, "k": int, "keys": {path: (params, pk_handle)}, "slots": {columns: [[Poly]]},
#              "extra": [{"eng": Engine sharing the first one's SRS, "keys": {path: pk_handle}, "slots": {..}}], "free": Queue of pipeline indices}
_STATE = {}
_SLOTS_LOCK = threading.Lock()
_STATE_LOCK = threading.RLock()  # set-up / tear-down of a device's resident state (gen_srs with a new degree, shutdown)
# Proof pipelines per device = requests proved CONCURRENTLY on it (the reference: one Rocket worker thread per request,
# proving-server/src/main.rs:457-472).  Each is a context of its own (own key, own workspace, shared SRS and window tables).
# Four is the measured optimum for the server's default shape since round 5: 143 / 184 / 208 / 224 / 208 proofs/s at k = 17 with
# 1 / 2 / 3 / 4 / 6 (tools/inflight_k17.py, profiles/r5_k17_inflight.txt; round 4: 144 / 195 / 173 / 183), and what k = 19 batches
# want too (batch.py, bench.py).  A request that arrives alone still proves alone: pipeline 0 is taken first.
PIPELINES_PER_DEVICE = 4
_MAX_SLOT_SETS = 4  # parked request-slot sets per column count: the server's usual number of requests in flight per device
# Resident bytes per pipeline by degree (tools/mem_footprint.py: SRS + window tables are shared, every pipeline keeps its own
# key, prover workspace and three MSM lanes), plus the request-slot sets it may park (_MAX_SLOT_SETS advice sets of 32 B x n)
_PIPELINE_BYTES = {17: 2.0 * 2**30, 18: 3.2 * 2**30, 19: 5.3 * 2**30, 20: 10.5 * 2**30, 21: 21.0 * 2**30}


def pipelines_for(degree: int, device: int = 0) -> int:
    """How many pipelines a device gets at this degree: PIPELINES_PER_DEVICE, fewer when they would not leave a quarter of the
    device's FREE memory to everything else (another process's contexts, lock-step members: 1.4 GiB each at k = 19)."""
    from .engine import device_mem_info

    want = max(1, PIPELINES_PER_DEVICE)
    per = _PIPELINE_BYTES.get(degree, _PIPELINE_BYTES[21] * (1 << max(0, degree - 21)) if degree > 21 else _PIPELINE_BYTES[17])
    per += _MAX_SLOT_SETS * 32 * (1 << degree)
    try:
        free, _ = device_mem_info(device)
    except Exception:
        return want
    return max(1, min(want, int(0.75 * free // per)))


def _config_for(degree: int) -> circuit.CircuitParams:
    """The reference reads ECDSA_CONFIG / src/configs/ecdsa_circuit.config (ecdsa_p256.rs:95-100);
    the rows BASELINE.json names are built in, anything else comes from $ECDSA_CONFIG."""
    path = os.environ.get("ECDSA_CONFIG")
    if path and os.path.exists(path):
        p = circuit.CircuitParams.from_json(open(path).read().strip().splitlines()[0])
        if p.degree == degree:
            return p
    if degree == 19:
        return circuit.K19
    if degree == 17:
        return circuit.K17
    raise ValueError(f"no circuit config for degree {degree}; set ECDSA_CONFIG")


def _drain(st):
    """Take every pipeline of a device out of its free queue: returns once no request holds one (requests in flight finish
    first — their `finally` puts the index back into THIS queue object), so contexts can be closed without a use after close."""
    q = st.get("free")
    if q is None:
        return
    for _ in range(1 + len(st["extra"])):
        q.get()
    st["free"] = None


class _Hold:
    """Every pipeline of a device taken out of its free queue for the duration of a `with` block (requests in flight finish
    first, new ones wait): a key can be freed and replaced without a request proving under it.  The indices go back into the
    same queue object, pipeline 0 on top."""

    def __init__(self, st):
        self.q, self.n = st.get("free"), 1 + len(st["extra"])

    def __enter__(self):
        if self.q is not None:
            for _ in range(self.n):
                self.q.get()
        return self

    def __exit__(self, *exc):
        if self.q is not None:
            for i in range(self.n - 1, -1, -1):
                self.q.put(i)
        return False


# (device) -> absolute path of the ParamsKZG file (RawBytes, as Params::write writes it) whose SRS gen_srs downsizes; a device
# without an entry uses the seed-0 setup.  The source is explicit: no $PARAMS_DIR lookup.
_PARAMS_FILES = {}


def set_params_file(path, device: int = 0):
    """The SRS source of `device`: a trusted-setup ParamsKZG file of any degree K (the caller ships the ceremony's largest), or
    None for halo2-base's seed-0 setup (the default).  From now on gen_srs(degree) on the device reads the file and downsizes
    it to `degree` (ParamsKZG::read + downsize) — ValueError when degree > K.  A new source takes effect like a new degree: at
    the next gen_srs the device's keys and verifying keys are freed and its pipelines rebuilt on the new SRS."""
    with _STATE_LOCK:
        if path is None:
            _PARAMS_FILES.pop(device, None)
            return
        path = os.path.abspath(path)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"Unable to open params file: {path}")
        _PARAMS_FILES[device] = path


def _source_tag(device):
    """The identity of the device's SRS source: None (seed-0 setup) or (path, mtime, size) of its params file, as _resident_vk
    keys its files."""
    path = _PARAMS_FILES.get(device)
    if path is None:
        return None
    try:
        stt = os.stat(path)
    except OSError as e:
        raise FileNotFoundError(f"Unable to open params file: {path}") from e
    return (path, stt.st_mtime_ns, stt.st_size)


def params_file_degree(path) -> int:
    """K of a ParamsKZG file: its first four bytes, u32 little-endian."""
    with open(path, "rb") as f:
        head = f.read(4)
    if len(head) != 4:
        raise ValueError(f"{path}: not a ParamsKZG file")
    return int.from_bytes(head, "little")


def gen_srs(degree: int, device: int = 0) -> Engine:
    """halo2-base `gen_srs(k)`, kept resident: ParamsKZG::setup(k, ChaCha20Rng::from_seed([0; 32])), or — after
    set_params_file(path) — ParamsKZG::read(path) + downsize(k)."""
    with _STATE_LOCK:
        return _gen_srs_locked(degree, device)


def _gen_srs_locked(degree, device):
    st = _STATE.setdefault(device, {"eng": None, "k": None, "src": None, "keys": {}, "slots": {}, "extra": [], "free": None})
    src = _source_tag(device)
    if src is not None and degree > params_file_degree(src[0]):
        # halo2's downsize asserts k <= self.k; nothing resident changes
        raise ValueError(f"degree {degree} is larger than the params file's ({params_file_degree(src[0])}): {src[0]}")
    if st["eng"] is None:
        st["eng"] = Engine(device)
    if st["k"] != degree or st.get("src") != src:
        _drain(st)  # requests still proving under the old SRS hold a pipeline: wait for them before anything is closed
        for _, pk in st["keys"].values():
            st["eng"].pk_free(pk)
        st["keys"].clear()
        for vk in st.get("vks", {}).values():  # verifying keys of the old degree's shape
            st["eng"].pk_free(vk)
        st["vks"] = {}
        with _SLOTS_LOCK:
            for sets in st["slots"].values():
                for polys in sets:
                    for h in polys:
                        h.free()
            st["slots"].clear()
        for m in st["extra"]:  # the further pipelines saw the old SRS: they go with it
            m["eng"].close()
        st["extra"] = []
        st["k"] = None  # (until the new SRS is resident: a failed read leaves the device to be set up again by the next call)
        if src is None:
            st["eng"].srs_setup(degree, bytes(32))
        else:
            with open(src[0], "rb") as f:
                data = f.read()
            st["eng"].srs_read_downsize(data, degree)
        st["k"], st["src"] = degree, src
        st["extra"] = [{"eng": Engine(device, share_with=st["eng"]), "keys": {}, "slots": {}} for _ in range(pipelines_for(degree, device) - 1)]
        st["free"] = queue.LifoQueue()
        for i in range(len(st["extra"]), -1, -1):  # pipeline 0 (the first context) on top: a lone request takes it
            st["free"].put(i)
    return st["eng"]


_RECEIPT_POINTS = (("before_g1", 8), ("after_g1", 8), ("s_g1", 8), ("s_g2", 16))
_CONTRIB_CHAIN = ZK_SRS_CONTRIB_SAME_SECRET | ZK_SRS_CONTRIB_LINKS | ZK_SRS_CONTRIB_NONTRIVIAL

# Where check_contributions checks a chain's receipts: one host check per receipt (zk_srs_contribution_check), or the chain in
# launches of up to ZK_SRS_CONTRIB_BATCH_MAX receipts, one per lane (zk_srs_contribution_check_batch).  A process-wide setting like
# set_verify_pairing's.  "auto" is the host for chains shorter than _CONTRIBUTION_AUTO_DEVICE_FROM receipts and the device from there
# on: the smallest count of tools/contribution_chain_rate.py's table (docs/experiments.md, 2026-10-20) at which the device median lies
# below the host median by more than either cell's min-to-median spread; at 1 and 8 receipts the host is ahead.  Same verdicts.
_CONTRIBUTION_CHECK = "auto"
_CONTRIBUTION_CHECK_MODES = ("auto", "host", "device")
_CONTRIBUTION_AUTO_DEVICE_FROM = 64


def set_contribution_check(mode: str):
    """Where check_contributions checks the receipts of a chain: "host" (one check per receipt), "device" (the chain in launches
    of up to 4096 receipts) or "auto" (the host below 64 receipts, the device from 64 on).  The verdict is the same."""
    global _CONTRIBUTION_CHECK
    if mode not in _CONTRIBUTION_CHECK_MODES:
        raise ValueError('contribution check: "host", "device" or "auto"')
    _CONTRIBUTION_CHECK = mode


def contribution_check() -> str:
    return _CONTRIBUTION_CHECK


def _contribution_route(n_receipts: int) -> str:
    """"host" or "device": where a chain of n_receipts is checked under the current setting"""
    if _CONTRIBUTION_CHECK != "auto":
        return _CONTRIBUTION_CHECK
    return "device" if n_receipts >= _CONTRIBUTION_AUTO_DEVICE_FROM else "host"


def _sha256_file(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def _receipt_points(receipt):
    """the four points of a receipt as the uint64 limb arrays Engine.srs_contribution_check takes"""
    out = {}
    for name, words in _RECEIPT_POINTS:
        raw = bytes.fromhex(receipt[name])
        if len(raw) != 8 * words:
            raise ValueError(f"receipt field {name}: {len(raw)} bytes, not {8 * words}")
        out[name] = np.frombuffer(raw, dtype="<u8").astype(np.uint64)
    return out


def contribute_params(src_path, dst_path, seed: bytes, device: int = 0, degree=None) -> dict:
    """One ceremony contribution: reads the ParamsKZG file `src_path` (RawBytes) — or, with src_path=None, runs the seed-0 setup
    of `degree` —, multiplies the secret drawn from `seed` into it (zk_srs_update: tau -> s tau) and writes the result to
    `dst_path` as a RawBytes params file, which set_params_file and the Rust host's ParamsKZG::read both take.  The seed is 32
    bytes from the operating system (os.urandom(32)) that the caller uses for this one call and discards: who keeps it keeps s.

    Nothing is written unless the new SRS passes the structure check (srs_check == 7) and its receipt all four contribution
    checks; ValueError otherwise.  Also ValueError for dst_path == src_path, a seed that is not 32 bytes, or no source at all;
    FileNotFoundError for a missing source — all before a device is touched.  The call uses a context of its own: the
    device's resident server state is not disturbed.

    Returns the receipt, a JSON-able dict:
        before_g1, after_g1, s_g1   hex of the 64-byte affine Montgomery images (g[1] before and after the step, [s] G1)
        s_g2                        hex of the 128-byte image of [s] G2 (x.c0 || x.c1 || y.c0 || y.c1)
        k                           the degree of both files
        src_sha256, dst_sha256      sha256 of the two files (src_sha256 is None for the seed-0 setup)
    A third party checks a chain of them with check_contributions."""
    if not isinstance(seed, (bytes, bytearray)) or len(seed) != 32:
        raise ValueError("contribution seed must be 32 bytes")
    if dst_path is None:
        raise ValueError("no destination path")
    if src_path is None:
        if degree is None:
            raise ValueError("no source: give src_path or degree")
    else:
        if os.path.abspath(src_path) == os.path.abspath(dst_path) or (os.path.exists(dst_path) and os.path.samefile(src_path, dst_path)):
            raise ValueError("dst_path is src_path: a contribution never overwrites its source")
        if not os.path.isfile(src_path):
            raise FileNotFoundError(f"Unable to open params file: {src_path}")
        if degree is not None and degree != params_file_degree(src_path):
            raise ValueError(f"degree {degree} is not the params file's ({params_file_degree(src_path)}): {src_path}")
    eng = Engine(device)
    try:
        if src_path is None:
            eng.srs_setup(degree, bytes(32))
        else:
            with open(src_path, "rb") as f:
                eng.srs_read(f.read())
        rec = eng.srs_update(bytes(seed))
        if eng.srs_check(os.urandom(32)) != 7:
            raise ValueError("the updated SRS fails the structure check")
        if eng.srs_contribution_check(rec) != _CONTRIB_CHAIN | ZK_SRS_CONTRIB_RESIDENT:
            raise ValueError("the contribution's receipt fails its check")
        k = eng.L.zk_srs_k(eng.ctx)
        image = eng.srs_write(ZK_SERDE_RAW_BYTES)
    finally:
        eng.close()
    tmp = dst_path + ".partial"
    with open(tmp, "wb") as f:
        f.write(memoryview(image))
    os.replace(tmp, dst_path)
    receipt = {name: rec[name].astype("<u8").tobytes().hex() for name, _ in _RECEIPT_POINTS}
    receipt.update(k=k, src_sha256=None if src_path is None else _sha256_file(src_path), dst_sha256=_sha256_file(dst_path))
    return receipt


def check_contributions(params_path, receipts, device: int = 0) -> bool:
    """Checks a params file against the chain of receipts that led to it (oldest first): every receipt shows
    SAME_SECRET | LINKS | NONTRIVIAL, each before_g1 is the previous receipt's after_g1, the last after_g1 is g[1] of the file
    (RESIDENT), and the file passes the structure check (srs_check == 7).  Then the file's secret is the chain's starting one
    times every contributor's.  False for an empty chain or a file that cannot be read as RawBytes params.  The receipts are
    checked one by one on the host or in launches of up to 4096 on the device (set_contribution_check); the verdict is the same."""
    from .engine import ZkError

    receipts = list(receipts)
    if not receipts or not os.path.isfile(params_path):
        return False
    try:
        points = [_receipt_points(r) for r in receipts]
    except (KeyError, TypeError, ValueError):
        return False
    for prev, cur in zip(points, points[1:]):
        if prev["after_g1"].tobytes() != cur["before_g1"].tobytes():
            return False
    eng = Engine(device)
    try:
        with open(params_path, "rb") as f:
            try:
                eng.srs_read(f.read())
            except ZkError:
                return False
        if _contribution_route(len(points)) == "device":
            for at in range(0, len(points), ZK_SRS_CONTRIB_BATCH_MAX):
                chunk = points[at:at + ZK_SRS_CONTRIB_BATCH_MAX]
                for i, flags in enumerate(eng.srs_contribution_check_batch(chunk), at):
                    # (a chunk's first receipt is CHAINED by rule: the links across chunks are the byte comparison above)
                    want = _CONTRIB_CHAIN | ZK_SRS_CONTRIB_CHAINED | (ZK_SRS_CONTRIB_RESIDENT if i == len(points) - 1 else 0)
                    if flags & want != want:
                        return False
        else:
            for i, pts in enumerate(points):
                want = _CONTRIB_CHAIN | (ZK_SRS_CONTRIB_RESIDENT if i == len(points) - 1 else 0)
                if eng.srs_contribution_check(pts) & want != want:
                    return False
        return eng.srs_check(os.urandom(32)) == 7  # fresh weights: a file cannot be made to fit a known check
    finally:
        eng.close()


def shutdown(device=None):
    """Release the resident state (every pipeline's context, keys and request slots) of `device`, or of all devices."""
    with _STATE_LOCK:
        with _ES256_LOCK:  # the signature check's own context
            for d in ([device] if device is not None else list(_ES256_ENGINES)):
                eng = _ES256_ENGINES.pop(d, None)
                if eng is not None:
                    eng.close()
        for d in ([device] if device is not None else list(_STATE)):
            st = _STATE.get(d)
            if not st:
                continue
            _drain(st)  # (a request that arrives from now on finds no queue: "no resident state")
            _STATE.pop(d, None)
            st["k"] = None
            for m in st["extra"][::-1]:
                m["eng"].close()
            if st["eng"] is not None:
                st["eng"].close()


class PlacementError(ValueError):
    """The streams of a device's pool do not sit on the hardware queues the engine deals them for (check_placement,
    proving_server.setup(check_placement=True)): `report` is what engine.stream_placement measured.  Proofs are right either
    way; four pipelines are slower."""

    def __init__(self, report):
        self.report = report
        super().__init__(f"stream placement not as assumed: {report['n_queues']} queue classes, flags {report['flags']:#x}, "
                         f"main streams on {report['main_queue']}")


def check_placement(device=0, calibrate=True):
    """engine.stream_placement of `device`, once at start-up: returns the report when all four invariants hold, raises
    PlacementError otherwise.  calibrate=True lets the engine re-deal its pool first - only while the device has no resident
    engine of this module yet (a pool in use is measured, never re-dealt: the device's pipelines are held meanwhile, and the
    4 ms for which the engine still counts the last request's context as active are waited out)."""
    with _STATE_LOCK:
        st = _STATE.get(device)
        if not (st and st["eng"] is not None):
            report = stream_placement(device, calibrate)
        else:
            with _Hold(st):
                for attempt in range(8):
                    try:
                        report = stream_placement(device, False)
                        break
                    except ZkError as e:
                        if e.code != -5 or attempt == 7:  # ZK_ESTATE: a context enqueued an MSM pass within the last 4 ms
                            raise
                        time.sleep(0.004)
    if not report["ok"]:
        raise PlacementError(report)
    return report


def _pipeline(st, i):
    """(engine, {key name: pk handle}, request slots) of pipeline i of a device: 0 is the first context."""
    if i == 0:
        return st["eng"], {name: v[1] for name, v in st["keys"].items()}, st["slots"]
    m = st["extra"][i - 1]
    return m["eng"], m["keys"], m["slots"]


class ProvingKeyError(ValueError):
    """A proving key failed its audit (download_keys(check=True), proving_server.setup(check_keys=True)): `flags` and `findings`
    are what Engine.pk_check returned - which part, column and index of the key is not what keygen makes of the key's own
    values."""

    def __init__(self, flags, findings):
        self.flags, self.findings = flags, findings
        super().__init__(f"proving key fails its audit: flags {flags:#x}, first findings {findings[:4]}")


def check_keys(proving_key_path, degree, device=0, cap=64):
    """Engine.pk_check of the resident key registered under `proving_key_path` -> (flags, findings)."""
    with _STATE_LOCK:
        eng, _, pk = _resident_key(proving_key_path, degree, device)
        with _Hold(_STATE[device]):  # (the audit borrows the key's idle workspace: no request proves under it meanwhile)
            return eng.pk_check(pk, cap)


def _audit_or_raise(eng, pk):
    flags, findings = eng.pk_check(pk)
    if flags & ZK_PK_CHECK_ALL != ZK_PK_CHECK_ALL:
        raise ProvingKeyError(flags, findings)


def public_inputs(msg_hash: bytes, pubkey_x: bytes, pubkey_y: bytes, limb_bits: int = 88, num_limbs: int = 3):
    """The instance column of a circuit with public inputs: msghash, pubkey_x, pubkey_y (32 little-endian bytes each, as the
    requests carry them), each as num_limbs limbs of limb_bits bits, least significant first - nine values with the config's
    88-bit limbs (how halo2-ecc's CRT integers are exposed)."""
    mask = (1 << limb_bits) - 1
    out = []
    for v in (msg_hash, pubkey_x, pubkey_y):
        x = int.from_bytes(bytes(v), "little")
        if x >> (limb_bits * num_limbs):
            raise ValueError("value does not fit the limbs")
        out += [(x >> (limb_bits * i)) & mask for i in range(num_limbs)]
    return out


def encode_calldata(instances, proof: bytes) -> bytes:
    """snark-verifier's `encode_calldata`: the instances as 32-byte big-endian words, then the proof - what a generated verifier
    contract takes as its calldata."""
    return b"".join(int(v).to_bytes(32, "big") for v in instances) + bytes(proof)


def _mont_limbs(instances):
    vals = [int(v) for v in instances]
    if any(not 0 <= v < circuit.R for v in vals):
        raise ValueError("an instance value is not below the scalar modulus")
    return circuit.Assignment.to_mont_limbs(vals)


def download_keys(degree: int, proving_key_path=None, verifying_key_path=None, device: int = 0, check: bool = False,
                  public: bool = False):
    """keygen_vk + keygen_pk for the ECDSA-shape circuit.  The proving key stays on the device
    (registered under `proving_key_path`; a key already registered under that name is freed first); the
    verifying key is written to `verifying_key_path` if given, as the reference writes it
    (`vk.to_bytes(SerdeFormat::RawBytes)`, ecdsa_p256.rs:266-270: the VerifyingKey::write image of zk_vk_write).
    check=True: the new resident key goes through Engine.pk_check, and so does - when `proving_key_path` names an existing
    ProvingKey file (RawBytes, what the reference reads on every request, ecdsa_p256.rs:338-343) - the key of that file, read
    beside it and freed again; a key that fails raises ProvingKeyError (a file zk_pk_read itself refuses raises ZkError).
    public=True: the circuit with public inputs - one instance column, its first 3 x num_limbs rows copy-constrained to the
    cells that hold msghash, pubkey_x and pubkey_y (public_inputs); proofs of such a key need `instances`."""
    p = _config_for(degree)
    if public:
        p = dataclasses.replace(p, num_instance_columns=1)
    # structure only: fixed columns and copy constraints
    asg = circuit.synthesize(p, 0, n_public=3 * p.num_limbs if p.num_instance_columns else 0)
    fixed = np.stack([asg.to_limbs(c) for c in asg.fixed])
    with _STATE_LOCK:  # (one set-up / tear-down of a device's state at a time)
        eng = _gen_srs_locked(degree, device)
        st = _STATE[device]
        keys = st["keys"]
        name = proving_key_path or "<default>"
        # /setup called again while requests are proving: they finish under the old key first — the pipelines are held while the
        # resident key (GBs at k = 17 / 19) is freed and replaced, not leaked and not pulled from under a proof
        with _Hold(st):
            if name in keys:
                eng.pk_free(keys.pop(name)[1])
            pk = eng.keygen(p, fixed, asg.copies)
            keys[name] = (p, pk)
            for m in st["extra"]:  # every further pipeline of the device holds the key too (its own workspace comes with it)
                if name in m["keys"]:
                    m["eng"].pk_free(m["keys"].pop(name))
                m["keys"][name] = m["eng"].keygen(p, fixed, asg.copies)
            if check:
                _audit_or_raise(eng, pk)
                if proving_key_path and os.path.isfile(proving_key_path):
                    with open(proving_key_path, "rb") as f:
                        data = f.read()
                    from_file = eng.pk_read(p, data, ZK_SERDE_RAW_BYTES)
                    try:
                        _audit_or_raise(eng, from_file)
                    finally:
                        eng.pk_free(from_file)
        if verifying_key_path:
            with open(verifying_key_path, "wb") as f:
                f.write(eng.vk_write(pk).tobytes())
    return pk


def _resident_key(proving_key_path, degree, device):
    eng = gen_srs(degree, device)
    keys = _STATE[device]["keys"]
    key = proving_key_path or "<default>"
    if key not in keys:
        # the reference panics with "Unable to open proving key file" (ecdsa_p256.rs:340)
        raise FileNotFoundError(f"Unable to open proving key file: {proving_key_path} (call download_keys first)")
    return (eng,) + keys[key]


class WitnessError(ValueError):
    """The advice columns do not satisfy the circuit (create_proof_from_advice(check=True)): `counts` and `failures` are what
    Engine.witness_check returned — which gate row, lookup row or copied cell is wrong."""

    def __init__(self, counts, failures):
        self.counts, self.failures = counts, failures
        super().__init__(f"witness violates the circuit: {counts[0]} failure(s), first {failures[:4]}")


def create_proof_from_advice(advice_columns, proving_key_path, degree, transcript=ZK_TRANSCRIPT_BLAKE2B, device=0,
                             rng_seed=None, check=False, instances=None) -> bytes:
    """create_proof over host-synthesized advice columns — what an unchanged Rust host hands the engine
    after `ECDSACircuit::synthesize`.  `advice_columns`: sequence of (n, 4) uint64 arrays of canonical
    little-endian limbs, one per advice column of the key's shape.  check=True: the columns go through
    Engine.witness_check first and a violated circuit raises WitnessError instead of being proved.
    instances: the public inputs (canonical integers) of a key made with public=True - Engine.prove_public; None: no instances,
    which a key with the column refuses (ZkError -1: halo2's InvalidInstances)."""
    inst = None if instances is None else _mont_limbs(instances)
    return _with_pipeline(advice_columns, proving_key_path, degree, device,
                          lambda st, eng, pk, slots, cols, n: _prove_on(st, eng, pk, slots, cols, n, degree, transcript, rng_seed, check, inst))


def create_proof_multi_from_advice(advice_sets, proving_key_path, degree, transcript=ZK_TRANSCRIPT_BLAKE2B, device=0, rng_seed=None,
                                   check=False, instances=None) -> bytes:
    """create_proof(&params, &pk, &[c_0 .. c_{N-1}], &[&[]; N], ..): ONE proof over the N = len(advice_sets) circuits whose
    host-synthesized advice columns are given (Engine.prove_multi: one transcript, one RNG stream, one quotient, one multi-open)
    — an extension: the reference proves one circuit per call.  advice_sets[c]: circuit c's columns as
    create_proof_from_advice takes them.  check=True: every circuit goes through Engine.witness_check first; WitnessError
    carries the index of the first violated circuit in `.circuit`.  The verifier must expect the same N (verify_multi).
    instances: one list of public inputs (canonical integers) per circuit, for a key made with public=True -
    Engine.prove_multi_public; None: no instances, which a key with the column refuses."""
    advice_sets = [list(a) for a in advice_sets]
    if not advice_sets or any(len(a) != len(advice_sets[0]) for a in advice_sets):
        raise ValueError("every circuit brings the key's number of advice columns")
    if instances is not None and len(instances) != len(advice_sets):
        raise ValueError("one instance list per circuit")
    insts = None if instances is None else [_mont_limbs(l) for l in instances]
    per = len(advice_sets[0])

    def run(st, eng, pk, slots, cols, n):
        def prove(sets):
            if check:
                for c, polys in enumerate(sets):
                    counts, failures = eng.witness_check(pk, polys) if insts is None else eng.witness_check_public(pk, polys, insts[c])
                    if counts[0]:
                        err = WitnessError(counts, failures)
                        err.circuit = c
                        raise err
            seed = rng_seed if rng_seed is not None else os.urandom(32)
            return eng.prove_multi(pk, sets, seed, transcript) if insts is None else eng.prove_multi_public(pk, sets, insts, seed, transcript)

        def take(c, sets):  # a set of request slots per circuit, nested so that each is handed back on every way out
            if c == len(advice_sets):
                return prove(sets)
            return _on_slots(st, eng, slots, cols[c * per:(c + 1) * per], n, degree, lambda polys: take(c + 1, sets + [polys]))

        return take(0, [])

    return _with_pipeline([col for a in advice_sets for col in a], proving_key_path, degree, device, run)


def mock_verify_advice(advice_columns, proving_key_path, degree, device=0, cap=64, instances=None):
    """`MockProver::run(degree, &circuit, vec![]).verify()` — the body of the reference's test_secp256r1_ecdsa
    (ecdsa_p256.rs:209-248) — for a host that brings its own advice columns: the resident key and a pipeline's request slots
    exactly as create_proof_from_advice takes them.  Returns the first `cap` failures as (kind, index, row, other_index,
    other_row) tuples of engine.ZK_FAIL_*; the empty list is MockProver's Ok(()).  instances: the public inputs of a key made
    with public=True (`MockProver::run(degree, &circuit, vec![instances])`)."""
    inst = None if instances is None else _mont_limbs(instances)
    check = lambda eng, pk, polys: eng.witness_check(pk, polys, cap) if inst is None else eng.witness_check_public(pk, polys, inst, cap)
    return _with_pipeline(advice_columns, proving_key_path, degree, device,
                          lambda st, eng, pk, slots, cols, n: _on_slots(st, eng, slots, cols, n, degree,
                                                                        lambda polys: check(eng, pk, polys)[1]))


def _with_pipeline(advice_columns, proving_key_path, degree, device, fn):
    """fn(st, eng, pk, slots, cols, n) on a free pipeline of the device, with the advice columns validated."""
    _resident_key(proving_key_path, degree, device)  # (raises for an unknown key)
    n = 1 << degree
    cols = []
    for col in advice_columns:
        col = np.ascontiguousarray(col, dtype=np.uint64)
        if col.shape != (n, 4):
            raise ValueError("an advice column must be an (n, 4) array of canonical limbs")
        cols.append(col)
    # a pipeline of the device for this request: concurrent requests prove side by side (PIPELINES_PER_DEVICE), further ones wait
    st = _STATE[device]
    q = st["free"]  # THIS queue object gets the index back, whatever happens to the device's state meanwhile (_drain waits on it)
    if q is None or st["k"] != degree:
        raise RuntimeError("the device's resident state was released or replaced while this request was being set up")
    while True:
        try:
            which = q.get(timeout=0.05)
            break
        except queue.Empty:  # every pipeline is busy — or the device's state went away while we waited (its queue is drained for good)
            if st["free"] is not q:
                raise RuntimeError("the device's resident state was released or replaced while this request was waiting")
    try:
        eng, pks, slots = _pipeline(st, which)
        name = proving_key_path or "<default>"
        if st["k"] != degree or name not in pks:  # gen_srs(another degree) ran between the key lookup above and here
            raise FileNotFoundError(f"Unable to open proving key file: {proving_key_path} (the resident key was replaced)")
        return fn(st, eng, pks[name], slots, cols, n)
    finally:
        q.put(which)


def _prove_on(st, eng, pk, slots, cols, n, degree, transcript, rng_seed, check=False, inst=None):
    def run(polys):
        if check:
            counts, failures = eng.witness_check(pk, polys) if inst is None else eng.witness_check_public(pk, polys, inst)
            if counts[0]:
                raise WitnessError(counts, failures)
        seed = rng_seed if rng_seed is not None else os.urandom(32)  # the reference draws from OsRng (ecdsa_p256.rs:362)
        return eng.prove(pk, polys, seed, transcript) if inst is None else eng.prove_public(pk, polys, inst, seed, transcript)

    return _on_slots(st, eng, slots, cols, n, degree, run)


def _on_slots(st, eng, slots, cols, n, degree, fn):
    """fn(polys) with the columns uploaded into a set of the pipeline's request slots."""
    # request slots: the columns' device buffers are kept between requests (a hipFree per request would wait for the whole
    # device, i.e. for every other request in flight on it); concurrent requests each take a set of their own
    with _SLOTS_LOCK:
        free = slots.setdefault(len(cols), [])
        polys = free.pop() if free else None
    if polys is None:
        polys = []
        try:
            for _ in cols:
                polys.append(eng.poly(n))
        except Exception:  # a partial allocation must not leak the handles already made
            for h in polys:
                h.free()
            raise
    try:
        for h, col in zip(polys, cols):
            eng.upload_canonical(h, col)
        return fn(polys)
    finally:
        with _SLOTS_LOCK:
            keep = slots.setdefault(len(cols), [])
            # at most _MAX_SLOT_SETS parked sets per column count (a set is GBs at k = 19 with many columns): more
            # concurrent requests than that allocate and free their own
            if st["k"] == degree and len(keep) < _MAX_SLOT_SETS:  # (`st` as captured at entry: shutdown() may have dropped _STATE[device])
                keep.append(polys)
            else:  # the SRS was replaced meanwhile (these buffers belong to the old size), or enough sets are parked
                for h in polys:
                    h.free()


# ---- ES256 (secp256r1 ECDSA) request validation, host side -------------------------------------------
_P = 0xFFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF
_N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
_B = 0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B
_G = (0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296,
      0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5)


def _p256_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % _P == 0:
            return None
        lam = 3 * (a[0] * a[0] - 1) * pow(2 * a[1], -1, _P) % _P  # a = -3
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, _P) % _P
    x = (lam * lam - a[0] - b[0]) % _P
    return x, (lam * (a[0] - x) - a[1]) % _P


def _p256_mul(k, pt):
    acc = None
    while k:
        if k & 1:
            acc = _p256_add(acc, pt)
        pt = _p256_add(pt, pt)
        k >>= 1
    return acc


def _p256_key_reason(x, y):
    """The key's own tests, what ZK_ES256_ / ZK_WEBAUTHN_RANGE and _OFF_CURVE mean for it: x, y below p, then on the curve
    (Secp256r1Affine::from_xy is None off it).  -> the failing one's code, or 0 (_VALID)."""
    if x >= _P or y >= _P:
        return ZK_WEBAUTHN_RANGE
    return ZK_WEBAUTHN_OFF_CURVE if (y * y - (x * x * x - 3 * x + _B)) % _P else ZK_WEBAUTHN_VALID


def es256_verify(pubkey_x: bytes, pubkey_y: bytes, r: bytes, s: bytes, msg_hash: bytes) -> bool:
    """Plain secp256r1 ECDSA verification of the request, all five fields 32 little-endian bytes as the web
    client posts them (web-demo/src/pages/index.tsx:285-293; `Fp::from_bytes` / `Fq::from_bytes` at
    ecdsa_p256.rs:345-352 reject non-canonical encodings — so does this)."""
    x, y = int.from_bytes(pubkey_x, "little"), int.from_bytes(pubkey_y, "little")
    ri, si, z = int.from_bytes(r, "little"), int.from_bytes(s, "little"), int.from_bytes(msg_hash, "little")
    if _p256_key_reason(x, y) or z >= _N or not (0 < ri < _N) or not (0 < si < _N):
        return False
    w = pow(si, -1, _N)
    pt = _p256_add(_p256_mul(z * w % _N, _G), _p256_mul(ri * w % _N, (x, y)))
    return pt is not None and pt[0] % _N == ri


# ---- the same check on the device (opt-in) --------------------------------------------------------------
# es256_verify above is affine Python with one modular inversion per point operation and runs under the GIL: the threads of
# proving_server.prove_batch and the bodies of prove_multi pay for it one after another.  zk_es256_verify (csrc/es256.hip) checks
# up to 16 384 requests in one launch, one signature per lane.  Which of the two the prover entry points use is a process-wide
# setting; the default is the host, exactly the path above (tools/es256_rate.py measures both; a later change may flip it).
_SIGNATURE_CHECK = "host"
_REFUSED = "invalid ES256 signature (or non-canonical field encoding): request refused"
_ES256_ENGINES = {}  # device -> an Engine of its own for the check (no SRS, no key), used under _ES256_LOCK: contexts are not thread-safe
_ES256_LOCK = threading.Lock()


def set_signature_check(mode: str):
    """Where _prove_synthetic, proving_server.prove_multi and prove_batch check a request's ES256 signature: "host" (es256_verify,
    the default) or "device" (es256_verify_many: all bodies of a call in one zk_es256_verify launch before any proof starts).
    The same requests are refused with the same ValueError either way."""
    global _SIGNATURE_CHECK
    if mode not in ("host", "device"):
        raise ValueError('signature check: "host" or "device"')
    _SIGNATURE_CHECK = mode


def signature_check() -> str:
    return _SIGNATURE_CHECK


def _es256_record(q):
    """The 160-byte record of a request: a (pubkey_x, pubkey_y, r, s, msg_hash) tuple (es256_verify's argument order) or a parsed
    request body (proving_server.parse_request)."""
    if isinstance(q, dict):
        q = (q["pubkey_x"], q["pubkey_y"], q["r"], q["s"], q["msghash"])
    if len(q) != 5 or any(len(v) != 32 for v in q):
        raise ValueError("a request is five fields of 32 little-endian bytes")
    return b"".join(bytes(v) for v in q)


def _on_check_engine(device, items, cap, call):
    """The results of call(engine, chunk) over the chunks of at most `cap` items, joined in order: the device's check engine is made
    on first use, and the lock is held for the whole walk."""
    out = []
    with _ES256_LOCK:
        eng = _ES256_ENGINES.get(device)
        if eng is None:
            eng = _ES256_ENGINES[device] = Engine(device)
        for lo in range(0, len(items), cap):
            out += call(eng, items[lo:lo + cap])
    return out


def es256_verify_many(requests, device: int = 0):
    """es256_verify of every request on the device, in one zk_es256_verify call per ZK_ES256_BATCH_MAX requests -> [bool], in order.
    requests: (pubkey_x, pubkey_y, r, s, msg_hash) tuples, or parsed request bodies."""
    return _on_check_engine(device, [_es256_record(q) for q in requests], ZK_ES256_BATCH_MAX, lambda eng, recs: eng.es256_verify(b"".join(recs))[0])


def _check_route(items, device, many, one):
    """The items' results by the route set_signature_check names: one(item) each on the host, or many(items, device)."""
    items = list(items)
    if _SIGNATURE_CHECK == "device":
        return many(items, device)
    return [one(q) for q in items]


def _signature_ok(pubkey_x, pubkey_y, r, s, msg_hash, device):
    if _SIGNATURE_CHECK == "device":
        return es256_verify_many([(pubkey_x, pubkey_y, r, s, msg_hash)], device)[0]
    return es256_verify(pubkey_x, pubkey_y, r, s, msg_hash)


# ---- the WebAuthn assertion check: msghash made HERE from the assertion, not taken from the client ---------------------------
# What the web client does before it posts a ProveRequestBody (web-demo/src/pages/index.tsx:172-197, 237-250, 285-293: both hashes,
# the ASN.1 parse, the reversal to little-endian) and what a relying party must check of clientDataJSON and authenticatorData, as
# one rule with one reason code per request (include/zkmi355.h, zk_webauthn_verify; csrc/webauthn.hip.h states it in full).
# webauthn_verify is the host route in Python, webauthn_verify_many the device route; set_signature_check chooses, as for ES256.
def _der_integer(sig, pos):
    if pos + 2 > len(sig) or sig[pos] != 0x02:
        return None
    n = sig[pos + 1]
    if not 1 <= n <= 33 or pos + 2 + n > len(sig):
        return None
    body = sig[pos + 2:pos + 2 + n]
    if body[0] & 0x80 or (n > 1 and body[0] == 0 and not body[1] & 0x80) or (n == 33 and body[0] != 0):
        return None
    return int.from_bytes(body, "big"), pos + 2 + n


def webauthn_der_signature(sig: bytes):
    """(r, s) of the strict DER of ECDSA-Sig-Value (short-form lengths, exact, non-negative minimal INTEGERs below 2^256), or None."""
    if not 8 <= len(sig) <= 72 or sig[0] != 0x30 or sig[1] != len(sig) - 2:
        return None
    a = _der_integer(sig, 2)
    b = a and _der_integer(sig, a[1])
    if not b or b[1] != len(sig):
        return None
    return a[0], b[0]


def webauthn_expected_prefix(challenge: bytes, origin, typ: bytes = b"webauthn.get") -> bytes:
    """E of the client-data rule: what a conforming client's clientDataJSON for this challenge and origin starts with.  typ:
    b"webauthn.get" for an assertion, b"webauthn.create" for a registration."""
    origin = origin.encode() if isinstance(origin, str) else bytes(origin)
    return (b'{"type":"' + typ + b'","challenge":"' + base64.urlsafe_b64encode(bytes(challenge)).rstrip(b"=") + b'","origin":"' + origin
            + b'","crossOrigin":')


def _client_data_ok(cd, challenge, origin, allow_cross_origin, typ=b"webauthn.get"):
    e = webauthn_expected_prefix(challenge, origin, typ)
    if not cd.startswith(e):
        return False
    rest = cd[len(e):]
    word = b"true" if rest.startswith(b"true") else b"false" if rest.startswith(b"false") else None
    if word is None or rest[len(word):len(word) + 1] not in (b",", b"}") or not cd.endswith(b"}"):
        return False
    return word == b"false" or bool(allow_cross_origin)


def _auth_data_reason(ad, rp_id_hash, flags_required):
    """The AUTHDATA, RPID and FLAGS steps of both ceremonies over authData -> the first failing one's code, or 0 (_VALID)."""
    if len(ad) < 37:
        return ZK_WEBAUTHN_AUTHDATA
    if ad[:32] != bytes(rp_id_hash):
        return ZK_WEBAUTHN_RPID
    return ZK_WEBAUTHN_FLAGS if ad[32] & flags_required != flags_required else ZK_WEBAUTHN_VALID


def webauthn_verify(authenticator_data, client_data_json, signature, pubkey_x, pubkey_y, challenge, origin, rp_id_hash, flags_required=0x01,
                    allow_cross_origin=False):
    """The relying party's check of one assertion on the host: zk_webauthn_verify's rule in Python (hashlib, the DER and prefix
    rules, es256_verify).  pubkey_x, pubkey_y: 32 BIG-endian bytes (COSE's -2 / -3).  -> (ok, reason, record, sign_count): reason an
    engine.ZK_WEBAUTHN_* code, the FIRST failing test; record the 160 bytes pubkey_x || pubkey_y || r || s || msghash, little-endian
    fields (what the provers take), all zero for a request refused before the curve."""
    ad, cd, sig = bytes(authenticator_data), bytes(client_data_json), bytes(signature)
    origin_b = origin.encode() if isinstance(origin, str) else bytes(origin)
    zero = bytes(160)
    if (len(ad) > ZK_WEBAUTHN_AUTHDATA_MAX or len(cd) > ZK_WEBAUTHN_CLIENTDATA_MAX or not 8 <= len(sig) <= 72
            or not 1 <= len(challenge) <= ZK_WEBAUTHN_CHALLENGE_MAX or len(origin_b) > ZK_WEBAUTHN_ORIGIN_MAX):
        return False, ZK_WEBAUTHN_SIZE, zero, 0
    reason = _auth_data_reason(ad, rp_id_hash, flags_required)
    count = 0 if reason == ZK_WEBAUTHN_AUTHDATA else int.from_bytes(ad[33:37], "big")
    if reason:
        return False, reason, zero, count
    if not _client_data_ok(cd, challenge, origin_b, allow_cross_origin):
        return False, ZK_WEBAUTHN_CLIENTDATA, zero, count
    rs = webauthn_der_signature(sig)
    if rs is None:
        return False, ZK_WEBAUTHN_SIGNATURE_DER, zero, count
    z = hashlib.sha256(ad + hashlib.sha256(cd).digest()).digest()
    x, y = int.from_bytes(pubkey_x, "big"), int.from_bytes(pubkey_y, "big")
    fields = (bytes(pubkey_x)[::-1], bytes(pubkey_y)[::-1], rs[0].to_bytes(32, "little"), rs[1].to_bytes(32, "little"), z[::-1])
    record = b"".join(fields)
    key = _p256_key_reason(x, y)  # (RANGE covers the key, the digest and the signature together, before the curve)
    if key == ZK_WEBAUTHN_RANGE or int.from_bytes(z, "big") >= _N or not 0 < rs[0] < _N or not 0 < rs[1] < _N:
        return False, ZK_WEBAUTHN_RANGE, record, count
    if key:
        return False, key, record, count
    ok = es256_verify(*fields)
    return ok, ZK_WEBAUTHN_VALID if ok else ZK_WEBAUTHN_MISMATCH, record, count


def webauthn_verify_many(assertions, device: int = 0):
    """webauthn_verify of every assertion on the device, in one zk_webauthn_verify call per ZK_WEBAUTHN_BATCH_MAX of them ->
    [(ok, reason, record, sign_count)], in order.  assertions: dicts as Engine.webauthn_verify takes them."""
    return _on_check_engine(device, list(assertions), ZK_WEBAUTHN_BATCH_MAX, lambda eng, chunk: zip(*eng.webauthn_verify(chunk)))


def webauthn_check(assertions, device: int = 0):
    """[(ok, reason, record, sign_count)] of the assertions by the route set_signature_check names: one webauthn_verify each on the
    host, or all of them in one launch on the device."""
    return _check_route(assertions, device, webauthn_verify_many, lambda q: webauthn_verify(
        q["authenticator_data"], q["client_data_json"], q["signature"], q["pubkey_x"], q["pubkey_y"], q["challenge"], q["origin"], q["rp_id_hash"],
        q.get("flags_required", 0x01), q.get("allow_cross_origin", False)))


# ---- the WebAuthn registration check: where the key of an assertion came from --------------------------------------------------
# The other ceremony (navigator.credentials.create): the attestationObject's CBOR, authData's attested credential data, the COSE key
# in it, clientDataJSON of type webauthn.create and, if asked for, the statement - one rule with one reason code per request
# (include/zkmi355.h, zk_webauthn_register; csrc/webauthn_register.hip.h states it in full).  webauthn_register is the host route in
# Python, webauthn_register_many the device route; set_signature_check chooses.  The CBOR below is the header's: heads are read, items
# are skipped with one counter of items still owed, nothing is decoded.
def _cbor_head(b, pos):
    """(major, argument, position behind the head) of the head at b[pos:], or None where it is not well-formed and in shortest form."""
    if pos >= len(b):
        return None
    major, ai = b[pos] >> 5, b[pos] & 31
    pos += 1
    if ai < 24:
        return major, ai, pos
    if ai > 27:
        return None  # 28 .. 30 reserved; 31 indefinite lengths and `break`
    width = 1 << (ai - 24)
    if len(b) - pos < width:
        return None
    val = int.from_bytes(b[pos:pos + width], "big")
    pos += width
    if major == 7:
        return (major, val, pos) if ai != 24 or val >= 32 else None  # (25 .. 27: a float, any bits)
    return (major, val, pos) if val >= (24, 1 << 8, 1 << 16, 1 << 32)[ai - 24] else None


def _cbor_skip(b, pos):
    """The position behind the data item at b[pos:], or None where it is not well-formed."""
    owed = 1
    while owed:
        head = _cbor_head(b, pos)
        if head is None:
            return None
        major, val, pos = head
        owed -= 1
        if 2 <= major <= 5 and val > len(b) - pos:
            return None  # more bytes, items or pairs than bytes left
        if major in (2, 3):
            pos += val
        else:
            owed += {4: val, 5: 2 * val, 6: 1}.get(major, 0)
    return pos


def _attestation_object(o):
    """(fmt, attStmt item, offset of authData, authData) of the accepted encoding, or None."""
    head = _cbor_head(o, 0)
    if head is None or head[:2] != (5, 3) or o[head[2]:head[2] + 4] != b"\x63fmt":
        return None
    head = _cbor_head(o, head[2] + 4)
    if head is None or head[0] != 3 or head[1] > len(o) - head[2]:
        return None
    fmt, pos = o[head[2]:head[2] + head[1]], head[2] + head[1]
    if o[pos:pos + 8] != b"\x67attStmt" or o[pos + 8:pos + 9] == b"" or o[pos + 8] >> 5 != 5:
        return None
    end = _cbor_skip(o, pos + 8)
    if end is None or o[end:end + 9] != b"\x68authData":
        return None
    stmt = o[pos + 8:end]
    head = _cbor_head(o, end + 9)
    if head is None or head[0] != 2 or head[2] + head[1] != len(o):
        return None
    return fmt, stmt, head[2], o[head[2]:]


_COSE_HEAD, _COSE_Y = bytes.fromhex("a5010203262001215820"), bytes.fromhex("225820")


def webauthn_register(attestation_object, client_data_json, challenge, origin, rp_id_hash, flags_required=0x01, allow_cross_origin=False,
                      attestation_policy=ZK_WEBAUTHN_ATT_IGNORE):
    """The relying party's check of one registration on the host: zk_webauthn_register's rule in Python.  -> (ok, reason, credential):
    reason an engine.ZK_WEBAUTHN_* code, the FIRST failing test; credential None unless ok, else what Engine.webauthn_register
    gives (pubkey_x, pubkey_y: 32 BIG-endian bytes, what webauthn_verify takes)."""
    o, cd = bytes(attestation_object), bytes(client_data_json)
    origin_b = origin.encode() if isinstance(origin, str) else bytes(origin)
    if attestation_policy not in (ZK_WEBAUTHN_ATT_IGNORE, ZK_WEBAUTHN_ATT_NONE_OR_SELF):
        raise ValueError("attestation policy: ZK_WEBAUTHN_ATT_IGNORE or ZK_WEBAUTHN_ATT_NONE_OR_SELF")

    def refused(reason):
        return False, reason, None

    if (not 1 <= len(o) <= ZK_WEBAUTHN_ATTOBJ_MAX or len(cd) > ZK_WEBAUTHN_CLIENTDATA_MAX or not 1 <= len(challenge) <= ZK_WEBAUTHN_CHALLENGE_MAX
            or len(origin_b) > ZK_WEBAUTHN_ORIGIN_MAX):
        return refused(ZK_WEBAUTHN_SIZE)
    parts = _attestation_object(o)
    if parts is None:
        return refused(ZK_WEBAUTHN_CBOR)
    fmt, stmt, ad_off, ad = parts
    reason = _auth_data_reason(ad, rp_id_hash, flags_required)
    if reason:
        return refused(reason)
    flags = ad[32]
    id_len = int.from_bytes(ad[53:55], "big")
    if not flags & 0x40 or len(ad) < 55 or not 1 <= id_len <= 1023 or len(ad) - 55 < id_len:
        return refused(ZK_WEBAUTHN_CREDENTIAL)
    key_off = 55 + id_len
    pos = _cbor_skip(ad, key_off)
    if pos is None:
        return refused(ZK_WEBAUTHN_CREDENTIAL)
    key = ad[key_off:pos]
    if flags & 0x80:  # ED: exactly one map of extensions
        pos = _cbor_skip(ad, pos) if pos < len(ad) and ad[pos] >> 5 == 5 else None
    if pos != len(ad):
        return refused(ZK_WEBAUTHN_CREDENTIAL)
    if len(key) != 77 or key[:10] != _COSE_HEAD or key[42:45] != _COSE_Y:
        return refused(ZK_WEBAUTHN_COSE_KEY)
    if not _client_data_ok(cd, challenge, origin_b, allow_cross_origin, b"webauthn.create"):
        return refused(ZK_WEBAUTHN_CLIENTDATA)
    xb, yb = key[10:42], key[45:77]
    reason = _p256_key_reason(int.from_bytes(xb, "big"), int.from_bytes(yb, "big"))
    if reason:
        return refused(reason)
    attestation = ZK_WEBAUTHN_ATTESTED_NOT_JUDGED
    if attestation_policy == ZK_WEBAUTHN_ATT_NONE_OR_SELF:
        if fmt == b"none" and stmt == b"\xa0":
            attestation = ZK_WEBAUTHN_ATTESTED_NONE
        elif fmt == b"packed" and stmt[:10] == b"\xa2\x63alg\x26\x63sig":
            head = _cbor_head(stmt, 10)
            if head is None or head[0] != 2 or head[2] + head[1] != len(stmt):
                return refused(ZK_WEBAUTHN_ATTESTATION)
            attestation = ZK_WEBAUTHN_ATTESTED_SELF
            rs = webauthn_der_signature(stmt[head[2]:])
            if rs is None:
                return refused(ZK_WEBAUTHN_SIGNATURE_DER)
            z = hashlib.sha256(ad + hashlib.sha256(cd).digest()).digest()
            if int.from_bytes(z, "big") >= _N or not 0 < rs[0] < _N or not 0 < rs[1] < _N:
                return refused(ZK_WEBAUTHN_RANGE)
            if not es256_verify(xb[::-1], yb[::-1], rs[0].to_bytes(32, "little"), rs[1].to_bytes(32, "little"), z[::-1]):
                return refused(ZK_WEBAUTHN_MISMATCH)
        else:
            return refused(ZK_WEBAUTHN_ATTESTATION)
    return True, ZK_WEBAUTHN_VALID, {
        "pubkey_x": xb, "pubkey_y": yb, "aaguid": ad[37:53], "credential_id": ad[55:key_off], "auth_data": ad, "auth_data_off": ad_off,
        "auth_data_len": len(ad), "credential_id_off": ad_off + 55, "credential_id_len": id_len, "sign_count": int.from_bytes(ad[33:37], "big"),
        "flags": flags, "attestation": attestation}


def webauthn_register_many(registrations, device: int = 0):
    """webauthn_register of every registration on the device, in one zk_webauthn_register call per ZK_WEBAUTHN_BATCH_MAX of them ->
    [(ok, reason, credential or None)], in order.  registrations: dicts as Engine.webauthn_register takes them."""
    return _on_check_engine(device, list(registrations), ZK_WEBAUTHN_BATCH_MAX, lambda eng, chunk: eng.webauthn_register(chunk))


def webauthn_register_check(registrations, device: int = 0):
    """[(ok, reason, credential or None)] of the registrations by the route set_signature_check names: one webauthn_register each on
    the host, or all of them in one launch on the device."""
    return _check_route(registrations, device, webauthn_register_many, lambda q: webauthn_register(
        q["attestation_object"], q["client_data_json"], q["challenge"], q["origin"], q["rp_id_hash"], q.get("flags_required", 0x01),
        q.get("allow_cross_origin", False), q.get("attestation_policy", ZK_WEBAUTHN_ATT_IGNORE)))


def _witness_seed(pubkey_x, pubkey_y, r, s, msg_hash) -> int:
    return int.from_bytes(hashlib.sha256(bytes(pubkey_x) + bytes(pubkey_y) + bytes(r) + bytes(s) + bytes(msg_hash)).digest()[:8], "little")


def _prove_synthetic(pubkey_x, pubkey_y, r, s, msg_hash, proving_key_path, degree, transcript, device, rng_seed, check=False, public=False,
                     signature_ok=None):
    """signature_ok: the verdict of a check the caller already made for this request (proving_server.prove_batch under
    set_signature_check("device") checks all its requests in one launch); None: checked here."""
    for name, v in (("pubkey_x", pubkey_x), ("pubkey_y", pubkey_y), ("r", r), ("s", s), ("msg_hash", msg_hash)):
        if len(v) != 32:
            raise ValueError(f"{name} must be 32 little-endian bytes")  # the reference takes &[u8; 32]
    if signature_ok is None:
        signature_ok = _signature_ok(pubkey_x, pubkey_y, r, s, msg_hash, device)
    if not signature_ok:
        # the real circuit would be unsatisfiable; never let such a request come back with a verifying proof
        raise ValueError(_REFUSED)
    _, p, _ = _resident_key(proving_key_path, degree, device)
    if bool(p.num_instance_columns) != bool(public):
        raise ValueError("the resident key was made %s public inputs (download_keys(public=...))" % ("with" if p.num_instance_columns else "without"))
    vals = public_inputs(msg_hash, pubkey_x, pubkey_y, p.limb_bits, p.num_limbs) if public else None
    asg = circuit.synthesize(p, _witness_seed(pubkey_x, pubkey_y, r, s, msg_hash), n_public=len(vals) if public else 0, public_values=vals)
    return create_proof_from_advice([asg.to_limbs(col) for col in asg.advice], proving_key_path, degree, transcript, device, rng_seed,
                                    check, vals)


def generate_proof_synthetic(pubkey_x, pubkey_y, r, s, msg_hash, proving_key_path, degree, device=0, rng_seed=None, check=False,
                             public=False) -> bytes:
    """Request shape of `generate_proof` (Blake2b + SHPLONK, the /prove endpoint, proving-server/src/main.rs:65-79)
    over the SYNTHETIC same-shape circuit — see the module docstring.  check: create_proof_from_advice's.  public=True (a key of
    download_keys(public=True)): the proof's public inputs are public_inputs(msg_hash, pubkey_x, pubkey_y)."""
    return _prove_synthetic(pubkey_x, pubkey_y, r, s, msg_hash, proving_key_path, degree, ZK_TRANSCRIPT_BLAKE2B, device, rng_seed, check, public)


def generate_proof_evm_synthetic(pubkey_x, pubkey_y, r, s, msg_hash, proving_key_path, degree, device=0, rng_seed=None, check=False,
                                 public=False) -> bytes:
    """Request shape of `generate_proof_evm` (Keccak EvmTranscript + GWC, the /prove_evm endpoint,
    proving-server/src/main.rs:49-63) over the SYNTHETIC same-shape circuit — see the module docstring.  check:
    create_proof_from_advice's; public: generate_proof_synthetic's."""
    return _prove_synthetic(pubkey_x, pubkey_y, r, s, msg_hash, proving_key_path, degree, ZK_TRANSCRIPT_EVM, device, rng_seed, check, public)


# ---- verify / verify_evm (ecdsa_p256.rs:429-469) -----------------------------------------------------------------------------

# How a verifying context settles a batch whose folded pairing check fails (zk_verify_pairing_mode): by halving on the host, or by
# one launch of the device pairing over the whole set (csrc/pairing.hip).  A process-wide setting like the signature check's,
# applied to every context _resident_vk hands out; "auto" is the host (tools/verify_bad_rate.py measures both).  Same verdicts.
_VERIFY_PAIRING = "auto"
_VERIFY_PAIRING_MODES = {"auto": 0, "host": 1, "device": 2}


def set_verify_pairing(mode: str):
    """Where verify_batch (and proving_server.verify_batch behind it) finds the verdicts of a batch with failing proofs: "host"
    (bisection, up to 2 B - 1 host pairings), "device" (one launch) or "auto" (the host).  The verdicts are the same."""
    global _VERIFY_PAIRING
    if mode not in _VERIFY_PAIRING_MODES:
        raise ValueError('verify pairing: "host", "device" or "auto"')
    _VERIFY_PAIRING = mode


def verify_pairing() -> str:
    return _VERIFY_PAIRING


def _resident_vk(degree, verifying_key_path, device, public=False):
    """(engine, verifying-only key) for the file: VerifyingKey::read::<_, ECDSACircuit<Fr>> (ecdsa_p256.rs:431-435) once per file
    version, cached with the device's resident state (the key is a few kB: commitments and transcript_repr).  public: the file is
    the key of a circuit with public inputs (the file itself does not say: the shape comes from the circuit's configure)."""
    with _STATE_LOCK:
        eng = _gen_srs_locked(degree, device)
        st = _STATE[device]
        vks = st.setdefault("vks", {})
        try:
            stt = os.stat(verifying_key_path)
        except OSError as e:  # the reference panics with "Unable to open verifying key file" (ecdsa_p256.rs:432)
            raise FileNotFoundError(f"Unable to open verifying key file: {verifying_key_path}") from e
        tag = (os.path.abspath(verifying_key_path), stt.st_mtime_ns, stt.st_size, bool(public))
        if tag not in vks:
            for old in [t for t in vks if t[0] == tag[0] and t[3] == tag[3]]:
                eng.pk_free(vks.pop(old))
            with open(verifying_key_path, "rb") as f:
                data = f.read()
            p = _config_for(degree)
            vks[tag] = eng.vk_read(dataclasses.replace(p, num_instance_columns=1) if public else p, data)
        eng.verify_pairing_mode(_VERIFY_PAIRING_MODES[_VERIFY_PAIRING])
        return eng, vks[tag]


def _verify(degree, proof, verifying_key_path, device, instances, transcript, scheme):
    eng, vk = _resident_vk(degree, verifying_key_path, device, instances is not None)
    if instances is None:
        return eng.verify(vk, bytes(proof), transcript, scheme)
    return eng.verify_public(vk, bytes(proof), _mont_limbs(instances), transcript, scheme)


def verify(degree: int, proof: bytes, verifying_key_path: str, device: int = 0, instances=None) -> bool:
    """`verify` (ecdsa_p256.rs:429-447): Blake2b transcript + SHPLONK against gen_srs(degree); no instances, as the reference -
    or, for the key of a circuit with public inputs, `instances` (canonical integers): wrong values are a rejected proof."""
    return _verify(degree, proof, verifying_key_path, device, instances, ZK_TRANSCRIPT_BLAKE2B, ZK_SCHEME_SHPLONK)


def verify_evm(degree: int, proof: bytes, verifying_key_path: str, device: int = 0, instances=None) -> bool:
    """`verify_evm` (ecdsa_p256.rs:449-469): Keccak EvmTranscript + GWC against gen_srs(degree); `instances` as verify's."""
    return _verify(degree, proof, verifying_key_path, device, instances, ZK_TRANSCRIPT_EVM, ZK_SCHEME_GWC)


def verify_batch(degree: int, proofs, verifying_key_path: str, evm: bool, device: int = 0, instances=None):
    """Many proofs of one verifying key in one zk_verify_batch call: one verdict per proof, each what verify / verify_evm
    says of it.  instances: one list of public inputs (canonical integers) per proof, for the key of a circuit with public
    inputs - zk_verify_batch_public; None: no instances."""
    eng, vk = _resident_vk(degree, verifying_key_path, device, instances is not None)
    t, s = (ZK_TRANSCRIPT_EVM, ZK_SCHEME_GWC) if evm else (ZK_TRANSCRIPT_BLAKE2B, ZK_SCHEME_SHPLONK)
    if instances is None:
        return eng.verify_batch(vk, [bytes(p) for p in proofs], t, s)
    return eng.verify_batch_public(vk, [bytes(p) for p in proofs], [_mont_limbs(l) for l in instances], t, s)


def verify_multi(degree: int, proof: bytes, verifying_key_path: str, n: int, evm: bool, device: int = 0, instances=None) -> bool:
    """verify_proof of ONE proof over n circuits (create_proof_multi_from_advice; halo2: n instance slices, snark-verifier:
    `Config::kzg().with_num_proof(n)`) under the reference's two pairings: evm = Keccak EvmTranscript + GWC, else Blake2b +
    SHPLONK.  An extension: the reference verifies one circuit per proof.  A proof over another number of circuits is rejected.
    instances: one list of public inputs per circuit (n of them), for the key of a circuit with public inputs -
    zk_verify_multi_public; None: no instances."""
    eng, vk = _resident_vk(degree, verifying_key_path, device, instances is not None)
    t, s = (ZK_TRANSCRIPT_EVM, ZK_SCHEME_GWC) if evm else (ZK_TRANSCRIPT_BLAKE2B, ZK_SCHEME_SHPLONK)
    if instances is None:
        return eng.verify_multi(vk, n, bytes(proof), t, s)
    if len(instances) != n:
        raise ValueError("one instance list per circuit")
    return eng.verify_multi_public(vk, bytes(proof), [_mont_limbs(l) for l in instances], t, s)


def generate_verifier(verifying_key_path: str, degree: int, n: int = 1, public: bool = False, scheme=None, device: int = 0) -> str:
    """`generate_verifier` (ecdsa_p256.rs:275-327), the Yul half: the text of the EVM verifier of the proofs of the key in the file
    under gen_srs(degree) - of ONE proof over n circuits (n = 1: generate_proof_evm's; above: create_proof_multi_from_advice's with
    the EVM transcript), with the nine values of public_inputs per circuit when public (the key of a circuit with public inputs).
    scheme: ZK_SCHEME_GWC (None: the EVM transcript's default, GWC) or ZK_SCHEME_SHPLONK.  The program's calldata is
    encode_calldata's: every circuit's instance words in circuit order, then the proof.  The reference then compiles the text with
    solc, runs the bytecode on revm against a valid proof and rewrites the text as Solidity; the engine carries no solc and stops
    at the text - nobody has compiled it or run it on an EVM (the suite runs it in an interpreter of the Yul subset it uses)."""
    eng, vk = _resident_vk(degree, verifying_key_path, device, public)
    p = _config_for(degree)
    counts = [3 * p.num_limbs] * n if public else None
    return eng.evm_verifier(vk, n, counts, ZK_SCHEME_DEFAULT if scheme is None else scheme)
