"""JSON-in / hex-out request contract of the reference's proving server, on the resident engine.

Mirrors the proving and verifying endpoints of proving-server/src/main.rs (the Rocket server itself is out of scope —
SURVEY.md §2 #9 — only its request/response contract is reproduced so that a batch of recorded requests can
be replayed against the engine):

    struct ProveRequestBody { r, s, pubkey_x, pubkey_y, msghash: [u8; 32], proving_key_path: String }
                                                                       proving-server/src/main.rs:39-47
    POST /prove_evm  -> hex::encode(generate_proof_evm(..., DEGREE))   main.rs:49-63
    POST /prove      -> hex::encode(generate_proof(..., DEGREE))       main.rs:65-79
    POST /setup      -> download_keys(DEGREE, "./keys/proving_key.pk", "./keys/verifying_key.vk")   main.rs:29-37
    struct VerifyRequestBody { verifying_key_path: String, proof: String }      main.rs:409-413
    POST /verify     -> verify(DEGREE, hex::decode(proof)?, path) ? "verified" : "rejected"      main.rs:415-425
    POST /verify_evm -> verify_evm(DEGREE, hex::decode(proof)?, path) ? "verified" : "rejected"  main.rs:427-439
    struct GenerateEVMVerifierRequestBody { verifying_key_path, valid_proof_hex, deploy_code_path, sol_code_path, yul_code_path }
    POST /generate_evm_verifier -> the Yul text of generate_verifier(path, DEGREE, ..), written to yul_code_path   main.rs:376-409
                                   (the Solidity rewrite and the deployment bytecode need solc: not made here)
    const DEGREE: u32 = 17                                             main.rs:17

The five byte arrays are LITTLE-endian, as the web client builds them (web-demo/src/pages/index.tsx:285-293:
big-endian WebAuthn values reversed before the POST).  serde rejects a body whose arrays are not exactly 32
integers in 0..=255; so does `parse_request`.

The proofs are those of `ecdsa_p256.generate_proof*_synthetic` (the same-shape synthetic circuit, ES256
signature checked on the host — see that module's docstring for what that does and does not mean).
"""
import base64
import hashlib
import json
import re
import threading

from . import ecdsa_p256

DEGREE = 17  # proving-server/src/main.rs:17
FIELDS = ("r", "s", "pubkey_x", "pubkey_y", "msghash")


def parse_request(body):
    """ProveRequestBody from a JSON string / dict: five [u8; 32] arrays + proving_key_path."""
    if isinstance(body, (str, bytes, bytearray)):
        body = json.loads(body)
    if not isinstance(body, dict):
        raise ValueError("request body must be a JSON object")
    out = {}
    for f in FIELDS:
        v = body.get(f)
        if not isinstance(v, list) or len(v) != 32 or not all(isinstance(b, int) and not isinstance(b, bool) and 0 <= b <= 255 for b in v):
            raise ValueError(f"{f}: expected an array of 32 integers in 0..=255")  # serde: invalid length / invalid value
        out[f] = bytes(v)
    path = body.get("proving_key_path")
    if not isinstance(path, str):
        raise ValueError("proving_key_path: expected a string")
    out["proving_key_path"] = path
    return out


def setup(device=0, degree=DEGREE, proving_key_path="./keys/proving_key.pk", verifying_key_path=None, params_path=None, check_keys=False,
          check_placement=False, public=False):
    """POST /setup (and the server's start-up keygen, main.rs:451-456).  The proving key stays resident on
    `device`, registered under `proving_key_path` (the name later requests carry); the verifying key is
    written only when a path is given (the reference writes ./keys/verifying_key.vk).  `params_path`: a trusted-setup
    ParamsKZG file of degree >= `degree`, made the device's SRS source (ecdsa_p256.set_params_file) before keygen; None keeps
    the device's current source (the seed-0 setup unless one was set).  The seed-0 setup's secret is public — anybody can forge
    proofs under it —, so a deployment passes a ceremony file, or one with its own secret multiplied in
    (ecdsa_p256.contribute_params writes such a file, check_contributions checks its receipts).  check_keys=True: download_keys(check=True) - the key is
    audited (ecdsa_p256.ProvingKeyError names the part, column and index of a key that is not what keygen makes).
    check_placement=True: before anything is made resident the device's stream placement is measured
    (ecdsa_p256.check_placement: re-dealt if need be while the device has no engine yet, measured only when it has) and
    ecdsa_p256.PlacementError raised if the pipelines would share hardware queues; the report is returned instead of "Done".
    public=True: the key of the circuit with public inputs (download_keys(public=True)), for prove*(public=True)."""
    report = ecdsa_p256.check_placement(device, calibrate=True) if check_placement else None
    if params_path is not None:
        ecdsa_p256.set_params_file(params_path, device)
    ecdsa_p256.download_keys(degree, proving_key_path, verifying_key_path, device, check=check_keys, public=public)
    return report if check_placement else "Done"


def _prove(body, evm, device, degree, rng_seed, check=False, public=False, signature_ok=None):
    """check=True: the request's advice columns go through the witness check first (ecdsa_p256.WitnessError instead of a proof
    no verifier accepts).  public=True (an extension; the key of setup(public=True)): the proof is bound to the request's msghash
    and public key - the answer is the hex of ecdsa_p256.encode_calldata: the nine instance words, then the proof."""
    q = parse_request(body)
    if signature_ok is None:
        fn = ecdsa_p256.generate_proof_evm_synthetic if evm else ecdsa_p256.generate_proof_synthetic
        proof = fn(q["pubkey_x"], q["pubkey_y"], q["r"], q["s"], q["msghash"], q["proving_key_path"], degree, device, rng_seed, check, public)
    else:  # prove_batch under the device check: this request's signature went through the batch's one launch already
        transcript = ecdsa_p256.ZK_TRANSCRIPT_EVM if evm else ecdsa_p256.ZK_TRANSCRIPT_BLAKE2B
        proof = ecdsa_p256._prove_synthetic(q["pubkey_x"], q["pubkey_y"], q["r"], q["s"], q["msghash"], q["proving_key_path"], degree, transcript,
                                            device, rng_seed, check, public, signature_ok=signature_ok)
    if public:
        _, p, _ = ecdsa_p256._resident_key(q["proving_key_path"], degree, device)
        proof = ecdsa_p256.encode_calldata(ecdsa_p256.public_inputs(q["msghash"], q["pubkey_x"], q["pubkey_y"], p.limb_bits, p.num_limbs), proof)
    return proof.hex()  # hex::encode: lowercase, no prefix


def prove_evm(body, device=0, degree=DEGREE, rng_seed=None, check=False, public=False) -> str:
    """POST /prove_evm: Keccak EvmTranscript + GWC; the hex string the web client puts into userOp.signature."""
    return _prove(body, True, device, degree, rng_seed, check, public)


def prove(body, device=0, degree=DEGREE, rng_seed=None, check=False, public=False) -> str:
    """POST /prove: Blake2b + SHPLONK."""
    return _prove(body, False, device, degree, rng_seed, check, public)


def prove_batch(bodies, evm=True, devices=(0,), degree=DEGREE, public=False):
    """A recorded batch of requests over several GPUs: request i goes to devices[i % len(devices)], and every device proves
    `ecdsa_p256.PIPELINES_PER_DEVICE` of its requests side by side — one host thread per request in flight (the reference:
    one Rocket worker thread per request, main.rs:457-472).  Every device must have been `setup`.  Returns the hex proofs in
    request order; a failed request yields its exception.  public: prove's - every answer carries its nine instance words.
    Under ecdsa_p256.set_signature_check("device") the signatures of ALL requests are checked in one launch on devices[0] before any
    proof starts (a body that does not parse is left to its own slot's error)."""
    bodies = list(bodies)
    out = [None] * len(bodies)
    checked = [None] * len(bodies)
    if ecdsa_p256.signature_check() == "device":
        checked, _ = _each_body(bodies, lambda i, b: parse_request(b), lambda parsed: ecdsa_p256.es256_verify_many([q for _, q in parsed], devices[0]),
                                lambda q, ok: ok)
    _prove_slots(bodies, checked, out, evm, devices, degree, public)
    return out


def _each_body(bodies, parse, check_all, finish):
    """The walk of the batch entry points: parse(i, body) each, check_all([(i, parsed)]) - ONE call over all that parsed, which
    gives a verdict each -, finish(parsed, verdict) each.  -> (results, errors), a slot per body in both: a body whose parse raised,
    or whose finish raised a ValueError, has its exception in errors and None in results, and leaves the others alone."""
    results, errors = [None] * len(bodies), [None] * len(bodies)
    parsed = []
    for i, b in enumerate(bodies):
        try:
            parsed.append((i, parse(i, b)))
        except Exception as e:
            errors[i] = e
    if parsed:
        for (i, q), verdict in zip(parsed, check_all(parsed)):
            try:
                results[i] = finish(q, verdict)
            except ValueError as e:
                errors[i] = e
    return results, errors


def _prove_slots(bodies, checked, out, evm, devices, degree, public):
    """prove_batch's threads: out[i] = the hex proof of bodies[i] or its exception; a slot that already holds something is left."""
    per = max(1, ecdsa_p256.PIPELINES_PER_DEVICE)
    workers = len(devices) * per

    def work(q):
        for i in range(q, len(bodies), workers):
            if out[i] is not None:
                continue
            try:
                out[i] = _prove(bodies[i], evm, devices[q % len(devices)], degree, None, False, public, checked[i])
            except Exception as e:  # the reference answers 500 for that request and keeps serving
                out[i] = e

    ths = [threading.Thread(target=work, args=(q,)) for q in range(workers)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()


# ---- an extension the reference server does not have: the assertion itself in, msghash made here ---------------------------------
# The reference's web client hashes clientDataJSON and authenticatorData, parses the ASN.1 signature, reverses everything and posts
# the five arrays (web-demo/src/pages/index.tsx:172-197, 237-250, 285-293); the server then has to trust the client for the hash and
# for the challenge, origin and relying party inside it.  These entry points take what the authenticator returned, check it against
# what THIS server issued and expects (ecdsa_p256.webauthn_verify / zk_webauthn_verify), and build the classic request from the
# record that check assembled - so the answer is byte for byte what prove / prove_evm / prove_batch give for the body an honest web
# client would have posted.

_B64URL = re.compile(r"[A-Za-z0-9_-]*")
ASSERTION_FIELDS = ("authenticator_data", "client_data_json", "signature")


def _b64url_fields(body, names):
    """(the body as a dict, {name: bytes}) of a JSON string / dict whose members `names` are base64url strings without padding."""
    if isinstance(body, (str, bytes, bytearray)):
        body = json.loads(body)
    if not isinstance(body, dict):
        raise ValueError("request body must be a JSON object")
    out = {}
    for f in names:
        v = body.get(f)
        if not isinstance(v, str) or not _B64URL.fullmatch(v) or len(v) % 4 == 1:
            raise ValueError(f"{f}: expected a base64url string without padding")
        out[f] = base64.urlsafe_b64decode(v + "=" * (-len(v) % 4))
    return body, out


def parse_assertion(body):
    """An assertion body from a JSON string / dict: authenticator_data, client_data_json, signature as base64url strings without
    padding (as @simplewebauthn/browser delivers response.authenticatorData, .clientDataJSON, .signature), pubkey_x, pubkey_y as
    [u8; 32] LITTLE-endian arrays (ProveRequestBody's), proving_key_path."""
    body, out = _b64url_fields(body, ASSERTION_FIELDS)
    for f in ("pubkey_x", "pubkey_y"):
        v = body.get(f)
        if not isinstance(v, list) or len(v) != 32 or not all(isinstance(b, int) and not isinstance(b, bool) and 0 <= b <= 255 for b in v):
            raise ValueError(f"{f}: expected an array of 32 integers in 0..=255")
        out[f] = bytes(v)
    path = body.get("proving_key_path")
    if not isinstance(path, str):
        raise ValueError("proving_key_path: expected a string")
    out["proving_key_path"] = path
    return out


def _expected(expected_challenge, origin, rp_id, require_uv, allow_cross_origin):
    """What this server expects of either ceremony, as the fields ecdsa_p256.webauthn_check / webauthn_register_check take."""
    rp_id = rp_id.encode() if isinstance(rp_id, str) else bytes(rp_id)
    return {"challenge": bytes(expected_challenge), "origin": origin, "rp_id_hash": hashlib.sha256(rp_id).digest(),
            "flags_required": 0x05 if require_uv else 0x01, "allow_cross_origin": bool(allow_cross_origin)}


def _expectation(q, expected_challenge, origin, rp_id, require_uv, allow_cross_origin):
    """The assertion of a parsed body with what this server expects of it, as ecdsa_p256.webauthn_check takes it."""
    return {"authenticator_data": q["authenticator_data"], "client_data_json": q["client_data_json"], "signature": q["signature"],
            "pubkey_x": q["pubkey_x"][::-1], "pubkey_y": q["pubkey_y"][::-1],
            **_expected(expected_challenge, origin, rp_id, require_uv, allow_cross_origin)}


def _classic_body(q, verdict):
    """The ProveRequestBody an honest web client would have posted for an accepted assertion, from the record the check assembled;
    ValueError naming the reason for a refused one."""
    ok, reason, record, _ = verdict
    if not ok:
        raise ValueError("WebAuthn assertion refused: %s" % ecdsa_p256.WEBAUTHN_REASON_NAMES[reason])
    f = [list(record[32 * i:32 * i + 32]) for i in range(5)]
    return {"pubkey_x": f[0], "pubkey_y": f[1], "r": f[2], "s": f[3], "msghash": f[4], "proving_key_path": q["proving_key_path"]}


def _prove_assertion(body, evm, expected_challenge, origin, rp_id, require_uv, allow_cross_origin, device, degree, rng_seed, check, public):
    q = parse_assertion(body)
    verdict = ecdsa_p256.webauthn_check([_expectation(q, expected_challenge, origin, rp_id, require_uv, allow_cross_origin)], device)[0]
    return _prove(_classic_body(q, verdict), evm, device, degree, rng_seed, check, public, signature_ok=True)


def prove_assertion(body, expected_challenge, origin, rp_id, require_uv=False, allow_cross_origin=False, device=0, degree=DEGREE, rng_seed=None,
                    check=False, public=False) -> str:
    """prove for an assertion body (parse_assertion): the assertion is checked against expected_challenge (the raw bytes this server
    issued), origin and rp_id (rpIdHash = SHA-256(rp_id) is made here; UP is required, UV too with require_uv), msghash comes out of
    that check, and the answer is prove's for the classic body.  A refused assertion is a ValueError naming the first failing test."""
    return _prove_assertion(body, False, expected_challenge, origin, rp_id, require_uv, allow_cross_origin, device, degree, rng_seed, check, public)


def prove_assertion_evm(body, expected_challenge, origin, rp_id, require_uv=False, allow_cross_origin=False, device=0, degree=DEGREE,
                        rng_seed=None, check=False, public=False) -> str:
    """prove_evm for an assertion body: prove_assertion's with the Keccak EvmTranscript + GWC."""
    return _prove_assertion(body, True, expected_challenge, origin, rp_id, require_uv, allow_cross_origin, device, degree, rng_seed, check, public)


def prove_assertions_batch(bodies, expected_challenges, origin, rp_id, require_uv=False, allow_cross_origin=False, evm=True, devices=(0,),
                           degree=DEGREE, public=False):
    """prove_batch for assertion bodies; expected_challenges: one per body.  All assertions are checked before any proof starts -
    under ecdsa_p256.set_signature_check("device") in ONE launch on devices[0].  Returns the hex proofs in request order; a body that
    does not parse, or an assertion that is refused, yields its exception in its own slot and leaves the others alone."""
    bodies, expected_challenges = list(bodies), list(expected_challenges)
    if len(expected_challenges) != len(bodies):
        raise ValueError("one expected challenge per body")
    classic, out = _each_body(
        bodies, lambda i, b: parse_assertion(b),
        lambda parsed: ecdsa_p256.webauthn_check([_expectation(q, expected_challenges[i], origin, rp_id, require_uv, allow_cross_origin)
                                                  for i, q in parsed], devices[0]),
        _classic_body)
    _prove_slots(classic, [True] * len(bodies), out, evm, devices, degree, public)
    return out


# ---- the other ceremony: a registration in, the credential to store out ----------------------------------------------------------
# Where the pubkey_x / pubkey_y of every body above come from: navigator.credentials.create returns an attestationObject whose
# authData holds the credential id and the COSE key.  register_credential checks it against what THIS server issued and expects
# (ecdsa_p256.webauthn_register / zk_webauthn_register) and answers with what to store; the key arrays are the LITTLE-endian ones
# parse_request / parse_assertion take, so a stored credential drops into a prove body.  No proof is made here.
REGISTRATION_FIELDS = ("attestation_object", "client_data_json")
_ATTESTATION_POLICY = {"ignore": ecdsa_p256.ZK_WEBAUTHN_ATT_IGNORE, "none-or-self": ecdsa_p256.ZK_WEBAUTHN_ATT_NONE_OR_SELF}
_ATTESTATION_NAME = {ecdsa_p256.ZK_WEBAUTHN_ATTESTED_NONE: "none", ecdsa_p256.ZK_WEBAUTHN_ATTESTED_SELF: "self",
                     ecdsa_p256.ZK_WEBAUTHN_ATTESTED_NOT_JUDGED: "not-judged"}


def parse_registration(body):
    """A registration body from a JSON string / dict: attestation_object and client_data_json as base64url strings without padding
    (AuthenticatorAttestationResponse's attestationObject and clientDataJSON after toJSON())."""
    return _b64url_fields(body, REGISTRATION_FIELDS)[1]


def _registration(q, expected_challenge, origin, rp_id, require_uv, allow_cross_origin, attestation):
    """The registration of a parsed body with what this server expects of it, as ecdsa_p256.webauthn_register_check takes it."""
    if attestation not in _ATTESTATION_POLICY:
        raise ValueError('attestation: "ignore" or "none-or-self"')
    return {"attestation_object": q["attestation_object"], "client_data_json": q["client_data_json"],
            "attestation_policy": _ATTESTATION_POLICY[attestation], **_expected(expected_challenge, origin, rp_id, require_uv, allow_cross_origin)}


def _stored_credential(verdict):
    """What to store for an accepted registration; ValueError naming the reason for a refused one."""
    ok, reason, cred = verdict
    if not ok:
        raise ValueError("WebAuthn registration refused: %s" % ecdsa_p256.WEBAUTHN_REASON_NAMES[reason])
    return {"credential_id": cred["credential_id"].hex(), "pubkey_x": list(cred["pubkey_x"][::-1]), "pubkey_y": list(cred["pubkey_y"][::-1]),
            "aaguid": cred["aaguid"].hex(), "sign_count": cred["sign_count"], "flags": cred["flags"],
            "attestation": _ATTESTATION_NAME[cred["attestation"]]}


def register_credential(body, expected_challenge, origin, rp_id, require_uv=False, allow_cross_origin=False, attestation="ignore", device=0):
    """The credential of a registration body (parse_registration), checked against expected_challenge (the raw bytes this server
    issued), origin and rp_id (rpIdHash = SHA-256(rp_id) is made here; UP is required, UV too with require_uv).  attestation:
    "ignore" (the statement only has to be well-formed) or "none-or-self".  -> {"credential_id": hex, "pubkey_x", "pubkey_y": 32
    integers each, LITTLE-endian as parse_request / parse_assertion take them, "aaguid": hex, "sign_count", "flags", "attestation":
    "none" | "self" | "not-judged"}.  A refused registration is a ValueError naming the first failing test."""
    q = _registration(parse_registration(body), expected_challenge, origin, rp_id, require_uv, allow_cross_origin, attestation)
    return _stored_credential(ecdsa_p256.webauthn_register_check([q], device)[0])


def register_credentials_batch(bodies, expected_challenges, origin, rp_id, require_uv=False, allow_cross_origin=False, attestation="ignore",
                               device=0):
    """register_credential for many bodies (an enrolment wave, an imported credential store); expected_challenges: one per body.
    Under ecdsa_p256.set_signature_check("device") all of them are checked in ONE launch.  Returns one slot per body: the credential,
    or the exception of a body that does not parse or a registration that is refused, which leaves the others alone."""
    bodies, expected_challenges = list(bodies), list(expected_challenges)
    if len(expected_challenges) != len(bodies):
        raise ValueError("one expected challenge per body")
    stored, errors = _each_body(
        bodies, lambda i, b: _registration(parse_registration(b), expected_challenges[i], origin, rp_id, require_uv, allow_cross_origin, attestation),
        lambda parsed: ecdsa_p256.webauthn_register_check([q for _, q in parsed], device), lambda q, verdict: _stored_credential(verdict))
    return [cred if e is None else e for cred, e in zip(stored, errors)]


_HEX = re.compile(r"[0-9a-fA-F]*")


def parse_verify_request(body):
    """VerifyRequestBody from a JSON string / dict -> (verifying_key_path, proof bytes).  The proof hex is decoded as strictly as
    `hex::decode`: even length, hex digits only (either case), no 0x prefix, no whitespace — otherwise ValueError, where the
    reference answers with its FromHexError."""
    if isinstance(body, (str, bytes, bytearray)):
        body = json.loads(body)
    if not isinstance(body, dict):
        raise ValueError("request body must be a JSON object")
    path, proof = body.get("verifying_key_path"), body.get("proof")
    if not isinstance(path, str):
        raise ValueError("verifying_key_path: expected a string")
    if not isinstance(proof, str):
        raise ValueError("proof: expected a string")
    if len(proof) % 2:
        raise ValueError("proof: odd number of hex digits")  # FromHexError::OddLength
    if not _HEX.fullmatch(proof):
        raise ValueError("proof: invalid hex character")  # FromHexError::InvalidHexCharacter
    return path, bytes.fromhex(proof)


def _split_calldata(proof, public):
    """(instances or None, proof): `public` leading 32-byte big-endian words of ecdsa_p256.encode_calldata's layout split off."""
    if not public:
        return None, proof
    if len(proof) < 32 * public:
        raise ValueError("proof: shorter than its instance words")
    return [int.from_bytes(proof[32 * i:32 * i + 32], "big") for i in range(public)], proof[32 * public:]


def _verify(body, fn, device, degree, public):
    path, proof = parse_verify_request(body)
    instances, proof = _split_calldata(proof, public)
    if instances is not None and any(v >= ecdsa_p256.circuit.R for v in instances):
        return "rejected"  # (a generated verifier contract reverts on a non-canonical instance word)
    return "verified" if fn(degree, proof, path, device, instances) else "rejected"


def verify(body, device=0, degree=DEGREE, public=0) -> str:
    """POST /verify: Blake2b + SHPLONK; "verified" or "rejected".  public: how many leading instance words the proof string
    carries (prove(public=True) answers with nine), for the verifying key of a circuit with public inputs."""
    return _verify(body, ecdsa_p256.verify, device, degree, public)


def verify_evm(body, device=0, degree=DEGREE, public=0) -> str:
    """POST /verify_evm: Keccak EvmTranscript + GWC; "verified" or "rejected".  public: verify's."""
    return _verify(body, ecdsa_p256.verify_evm, device, degree, public)


def verify_batch(bodies, evm=True, device=0, degree=DEGREE, public=0):
    """A recorded batch of verify requests: the proofs of each verifying key go through ONE zk_verify_batch call.  Returns
    "verified" / "rejected" per request, in request order; a malformed request yields its exception.  public: verify's - every
    proof string carries that many leading instance words, and the batch goes through zk_verify_batch_public."""
    out = [None] * len(bodies)
    by_key = {}
    for i, b in enumerate(bodies):
        try:
            path, proof = parse_verify_request(b)
            instances, proof = _split_calldata(proof, public)
        except ValueError as e:
            out[i] = e
            continue
        if instances is not None and any(v >= ecdsa_p256.circuit.R for v in instances):
            out[i] = "rejected"  # (a generated verifier contract reverts on a non-canonical instance word)
            continue
        by_key.setdefault(path, []).append((i, proof, instances))
    for path, items in by_key.items():
        try:
            verdicts = ecdsa_p256.verify_batch(degree, [it[1] for it in items], path, evm, device,
                                               [it[2] for it in items] if public else None)
        except Exception as e:  # (an unreadable key file: every request of that key fails)
            for it in items:
                out[it[0]] = e
            continue
        for it, ok in zip(items, verdicts):
            out[it[0]] = "verified" if ok else "rejected"
    return out


# ---- extensions the reference server does not have: ONE proof over several requests -----------------------------------------
# halo2's create_proof takes a slice of circuits; N signatures under one key then share one transcript, one quotient, one opening
# proof and — on chain — one pairing.  The reference's endpoints prove one request per call; these two keep its JSON contract
# (a list of the existing request bodies in, one hex proof out) for a host that aggregates.

def prove_multi(bodies, evm=True, device=0, degree=DEGREE, rng_seed=None, check=False, public=False) -> str:
    """A list of ProveRequestBody (JSON strings / dicts, all naming ONE proving key) -> the hex of ONE proof over all of them, in
    list order (ecdsa_p256.create_proof_multi_from_advice).  Each body passes the ES256 check first; one refused body refuses
    the call.  The proof verifies with verify_multi and the same count only.  public=True (the key of setup(public=True)): circuit
    c is bound to request c's msghash and public key; the answer is the hex of ecdsa_p256.encode_calldata over ALL circuits' instance
    words in circuit order (nine per circuit), then the proof."""
    reqs = [parse_request(b) for b in bodies]
    if not reqs:
        raise ValueError("at least one request")
    path = reqs[0]["proving_key_path"]
    if any(q["proving_key_path"] != path for q in reqs):
        raise ValueError("proving_key_path: the requests of one proof name one key")
    if ecdsa_p256.signature_check() == "device":  # all bodies in one launch
        verdicts = ecdsa_p256.es256_verify_many(reqs, device)
    else:
        verdicts = (ecdsa_p256.es256_verify(q["pubkey_x"], q["pubkey_y"], q["r"], q["s"], q["msghash"]) for q in reqs)
    for i, ok in enumerate(verdicts):
        if not ok:
            raise ValueError(f"request {i}: invalid ES256 signature (or non-canonical field encoding): request refused")
    _, p, _ = ecdsa_p256._resident_key(path, degree, device)
    if bool(p.num_instance_columns) != bool(public):
        raise ValueError("the resident key was made %s public inputs (setup(public=...))" % ("with" if p.num_instance_columns else "without"))
    sets, lists = [], []
    for q in reqs:
        vals = ecdsa_p256.public_inputs(q["msghash"], q["pubkey_x"], q["pubkey_y"], p.limb_bits, p.num_limbs) if public else None
        asg = ecdsa_p256.circuit.synthesize(p, ecdsa_p256._witness_seed(q["pubkey_x"], q["pubkey_y"], q["r"], q["s"], q["msghash"]),
                                            n_public=len(vals) if public else 0, public_values=vals)
        sets.append([asg.to_limbs(col) for col in asg.advice])
        lists.append(vals)
    transcript = ecdsa_p256.ZK_TRANSCRIPT_EVM if evm else ecdsa_p256.ZK_TRANSCRIPT_BLAKE2B
    proof = ecdsa_p256.create_proof_multi_from_advice(sets, path, degree, transcript, device, rng_seed, check, lists if public else None)
    if public:
        proof = ecdsa_p256.encode_calldata([v for vals in lists for v in vals], proof)
    return proof.hex()


def verify_multi(body, evm=True, device=0, degree=DEGREE, public=0) -> str:
    """VerifyRequestBody plus "num_proof": the number of requests the proof covers -> "verified" or "rejected".  public: how many
    instance words EACH circuit has (prove_multi(public=True): nine); the proof string then starts with num_proof x public words, in
    circuit order."""
    path, proof = parse_verify_request(body)
    if isinstance(body, (str, bytes, bytearray)):
        body = json.loads(body)
    n = body.get("num_proof")
    if not isinstance(n, int) or isinstance(n, bool) or n < 1:
        raise ValueError("num_proof: expected a positive integer")
    if not public:
        return "verified" if ecdsa_p256.verify_multi(degree, proof, path, n, evm, device) else "rejected"
    words, proof = _split_calldata(proof, n * public)
    if any(v >= ecdsa_p256.circuit.R for v in words):
        return "rejected"  # (a generated verifier contract reverts on a non-canonical instance word)
    lists = [words[c * public:(c + 1) * public] for c in range(n)]
    return "verified" if ecdsa_p256.verify_multi(degree, proof, path, n, evm, device, lists) else "rejected"


def generate_evm_verifier(body, device=0, degree=DEGREE, public=0, n=1) -> str:
    """POST /generate_evm_verifier: GenerateEVMVerifierRequestBody (JSON string / dict) -> the Yul text of the EVM verifier of the
    proofs of the verifying key in `verifying_key_path` (ecdsa_p256.generate_verifier), written to `yul_code_path` and returned.
    public: the key is that of the circuit with public inputs (setup(public=True)) - every circuit carries its nine instance words;
    n: the program verifies ONE proof over n requests (prove_multi's).  The reference also compiles the text with solc into
    deployment bytecode (`deploy_code_path`), runs it on revm against `valid_proof_hex` and rewrites the text as Solidity
    (`sol_code_path`); the engine carries no solc, so a non-empty `sol_code_path` or `deploy_code_path` is a ValueError, and
    `valid_proof_hex` is not read."""
    if isinstance(body, (str, bytes, bytearray)):
        body = json.loads(body)
    if not isinstance(body, dict):
        raise ValueError("request body must be a JSON object")
    path, yul_path = body.get("verifying_key_path"), body.get("yul_code_path")
    if not isinstance(path, str):
        raise ValueError("verifying_key_path: expected a string")
    if not isinstance(yul_path, str) or not yul_path:
        raise ValueError("yul_code_path: expected a file name")
    for f in ("sol_code_path", "deploy_code_path"):
        if body.get(f):
            raise ValueError(f"{f}: the Solidity rewrite and the deployment bytecode need solc, which the engine does not carry; "
                             "leave it empty and compile the Yul text elsewhere")
    text = ecdsa_p256.generate_verifier(path, degree, n, bool(public), None, device)
    with open(yul_path, "w") as f:
        f.write(text)
    return text
