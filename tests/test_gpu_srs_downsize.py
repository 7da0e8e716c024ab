"""ParamsKZG::downsize on an MI355X: zk_g_to_lagrange (the G1 inverse NTT of csrc/g1_ntt.hip) against the Python reference on
arbitrary and degenerate points, zk_srs_downsize / zk_srs_read_downsize against the seed setup of the smaller degree, the
failure rules, keys and shared contexts, zk_srs_check on good and broken SRS, and the server's params-file source."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

import g1_lagrange_ref as ref
import webauthn_halo2_amd as zk
from webauthn_halo2_amd import engine as E
from zkoracle import curve, field as F, serde, srs

pytestmark = pytest.mark.gpu
FMTS = [E.ZK_SERDE_PROCESSED, E.ZK_SERDE_RAW_BYTES, E.ZK_SERDE_RAW_BYTES_UNCHECKED]
ALL = E.ZK_SRS_CHECK_POWERS | E.ZK_SRS_CHECK_LAGRANGE | E.ZK_SRS_CHECK_GENERATORS
SEED1 = bytes(range(32))
FIX = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fullsize_proofs.json")))
KIND = {"evm": E.ZK_TRANSCRIPT_EVM, "blake2b": E.ZK_TRANSCRIPT_BLAKE2B}


def G(s):
    return srs.g1_of_scalar(s)


def inputs(kind, k, rnd):
    n = 1 << k
    if kind == "random":
        return [G(rnd.randrange(1, F.R)) for _ in range(n)]
    if kind == "identity":
        return [None] * n
    if kind == "repeated":
        return [G(rnd.randrange(1, F.R))] * n
    if kind == "single":
        pts = [None] * n
        pts[rnd.randrange(n)] = G(rnd.randrange(1, F.R))
        return pts
    if kind == "opposite":
        P = G(rnd.randrange(1, F.R))
        return [P if i % 2 == 0 else curve.neg(P) for i in range(n)]
    # "meet": butterflies meet a + (-a) and a + a: inputs in bit-reversed order pair equal / opposite points at every stage
    P, Q = G(rnd.randrange(1, F.R)), G(rnd.randrange(1, F.R))
    return [[P, curve.neg(P), P, Q][i % 4] if i < n // 2 else [P, P, curve.neg(Q), Q][i % 4] for i in range(n)]


@pytest.mark.parametrize("kind", ["random", "identity", "repeated", "single", "opposite", "meet"])
def test_g_to_lagrange_equals_the_reference(engine, kind):
    rnd = random.Random(hash(kind) & 0xFFFF)
    for k in range(1, 9):
        pts = inputs(kind, k, rnd)
        got = ref.from_mont_limbs(engine.g_to_lagrange(ref.to_mont_limbs(pts), k))
        assert got == ref.g_to_lagrange(pts, k), (kind, k)
        if kind == "repeated":
            assert got == [pts[0]] + [None] * ((1 << k) - 1)


def test_g_to_lagrange_refuses_points_off_the_curve(engine):
    a = ref.to_mont_limbs([G(5), G(7), None, G(9)])
    bad = a.copy()
    bad[1, 0] ^= 1
    with pytest.raises(zk.ZkError) as e:
        engine.g_to_lagrange(bad, 2)
    assert e.value.code == -1
    assert engine.L.zk_g_to_lagrange(engine.ctx, E._p(a), 0, E._p(a.copy())) == -1  # k = 0
    assert ref.from_mont_limbs(engine.g_to_lagrange(a, 2)) == ref.g_to_lagrange(ref.from_mont_limbs(a), 2)


PAIRS = [(10, 4), (12, 9), (14, 13), (16, 16), (19, 17), (21, 17), (21, 19)]
_images = {}


def setup_image(k, seed, fmt):
    key = (k, seed, fmt)
    if key not in _images:
        if len(_images) > 6:
            _images.clear()
        e = zk.Engine(0)
        e.srs_setup(k, seed)
        _images[key] = e.srs_write(fmt).tobytes()
        e.close()
    return _images[key]


@pytest.mark.parametrize("K,k", PAIRS)
@pytest.mark.parametrize("seed", [bytes(32), SEED1], ids=["seed0", "seed1"])
def test_downsize_equals_setup(K, k, seed):
    eng = zk.Engine(0)
    eng.srs_setup(K, seed)
    eng.srs_downsize(k)
    assert eng.srs_check(b"\x01" * 32) == ALL
    for fmt in FMTS:
        assert eng.srs_write(fmt).tobytes() == setup_image(k, seed, fmt), (K, k, fmt)
    eng.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_read_downsize(fmt):
    K, k = 12, 9
    img = setup_image(K, bytes(32), fmt)
    eng = zk.Engine(0)
    eng.srs_read_downsize(img, k, fmt)
    assert eng.srs_write(fmt).tobytes() == setup_image(k, bytes(32), fmt)
    assert eng.srs_check() == ALL
    with pytest.raises(zk.ZkError) as e:
        eng.srs_read_downsize(img, K + 1, fmt)
    assert e.value.code == -1
    # malformed images: the verdict is zk_srs_read's on the same bytes, and a refusal leaves the resident SRS and its keys alone
    p = zk.circuit.CircuitParams(degree=9, num_advice=1, num_lookup_advice=1, num_fixed=1, lookup_bits=8)
    asg = zk.circuit.synthesize(p, 9)
    pk = eng.keygen(p, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
    h = eng.poly(1 << 9)
    eng.upload_canonical(h, asg.to_limbs(asg.advice[0]))
    proof = eng.prove(pk, [h], b"\x09" * 32, E.ZK_TRANSCRIPT_EVM)
    before = eng.srs_write(E.ZK_SERDE_RAW_BYTES).tobytes()
    gs = 32 if fmt == E.ZK_SERDE_PROCESSED else 64
    N = 1 << K
    g2s = 64 if fmt == E.ZK_SERDE_PROCESSED else 128
    cases = []  # (image, the code the oracle's codec expects of both readers: its verdict on the altered element alone)

    def expected(parse, element):
        try:
            parse(element, fmt)
            return 0
        except ValueError:
            return -1

    bad = bytearray(img)
    off = 4 + ((1 << k) + 3) * gs
    bad[off + 1] ^= 1  # a point of g beyond 2^k
    cases.append((bytes(bad), expected(serde.g1_parse, bytes(bad[off:off + gs]))))
    bad = bytearray(img)
    off = 4 + (N + 17) * gs
    bad[off + 1] ^= 1  # a point of the g_lagrange section
    cases.append((bytes(bad), expected(serde.g1_parse, bytes(bad[off:off + gs]))))
    bad = bytearray(img)
    off = 4 + 2 * N * gs + g2s
    bad[off + 1] ^= 1  # s_g2
    cases.append((bytes(bad), expected(serde.g2_parse, bytes(bad[off:off + g2s]))))
    cases.append((img[:-1], -1))  # wrong length
    if fmt != E.ZK_SERDE_PROCESSED:  # (a flipped bit of a compressed x may land on another point: there the oracle alone decides)
        assert [c[1] for c in cases] == ([0, 0, 0, -1] if fmt == E.ZK_SERDE_RAW_BYTES_UNCHECKED else [-1] * 4)
    other = zk.Engine(0)
    for b, oracle_code in cases:
        try:
            other.srs_read(b, fmt)
            want = 0
        except zk.ZkError as e:
            want = e.code
        try:
            eng.srs_read_downsize(b, k, fmt)
            got = 0
        except zk.ZkError as e:
            got = e.code
        assert got == want == oracle_code
        if got:
            assert eng.srs_write(E.ZK_SERDE_RAW_BYTES).tobytes() == before
            assert eng.prove(pk, [h], b"\x09" * 32, E.ZK_TRANSCRIPT_EVM) == proof
        else:  # (an unchecked image: both accept it; restore the good SRS for the next case)
            eng.srs_read_downsize(img, k, fmt)
            eng.pk_free(pk)
            pk = eng.keygen(p, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
    other.close()
    h.free()
    eng.pk_free(pk)
    eng.close()


def test_wrong_lagrange_section_is_found_and_rebuilt():
    K = 10
    img = bytearray(setup_image(K, bytes(32), E.ZK_SERDE_RAW_BYTES))
    N = 1 << K
    img[4 + N * 64:4 + 2 * N * 64] = img[4:4 + N * 64]  # g_lagrange := g
    eng = zk.Engine(0)
    eng.srs_read(bytes(img))
    f = eng.srs_check()
    assert not f & E.ZK_SRS_CHECK_LAGRANGE and f & E.ZK_SRS_CHECK_POWERS
    eng.srs_read_downsize(bytes(img), K)
    assert eng.srs_check() == ALL
    assert eng.srs_write().tobytes() == setup_image(K, bytes(32), E.ZK_SERDE_RAW_BYTES)
    eng.close()


def prove_k17(eng, name, pk, p):
    fx = FIX[name]
    asg = zk.circuit.synthesize(p, fx["witness_seed"], worst_case=fx["worst_case"])
    polys = []
    for col in asg.advice:
        h = eng.poly(1 << 17)
        eng.upload_canonical(h, asg.to_limbs(col))
        polys.append(h)
    proof = eng.prove(pk, polys, bytes.fromhex(fx["rng_seed"]), KIND[fx["transcript"]])
    for h in polys:
        h.free()
    return proof


@pytest.mark.parametrize("route", ["downsize", "read_downsize"])
def test_fullsize_proofs_under_a_downsized_srs(route):
    eng = zk.Engine(0)
    if route == "downsize":
        eng.srs_setup(19)
        eng.srs_downsize(17)
    else:
        eng.srs_read_downsize(setup_image(19, bytes(32), E.ZK_SERDE_RAW_BYTES), 17)
    assert eng.srs_check(b"\x02" * 32) == ALL
    names = [n for n in sorted(FIX) if FIX[n]["degree"] == 17]
    fx = FIX[names[0]]
    p = zk.circuit.CircuitParams(degree=17, num_advice=fx["num_advice"], num_lookup_advice=fx["num_lookup_advice"],
                                 num_fixed=fx["num_fixed"], lookup_bits=fx["lookup_bits"])
    asg = zk.circuit.synthesize(p, 0)
    pk = eng.keygen(p, np.stack([asg.to_limbs(c) for c in asg.fixed]), asg.copies)
    for name in names:
        proof = prove_k17(eng, name, pk, p)
        assert hashlib.sha256(proof).hexdigest() == FIX[name]["sha256"], name
        scheme = E.ZK_SCHEME_GWC if FIX[name]["transcript"] == "evm" else E.ZK_SCHEME_SHPLONK
        assert eng.verify(pk, proof, KIND[FIX[name]["transcript"]], scheme)
    eng.pk_free(pk)
    eng.close()


def test_keys_and_shared_contexts():
    k = 10
    p = zk.circuit.CircuitParams(degree=k, num_advice=1, num_lookup_advice=1, num_fixed=1, lookup_bits=9)
    asg = zk.circuit.synthesize(p, 3)
    fixed = np.stack([asg.to_limbs(c) for c in asg.fixed])
    eng = zk.Engine(0)
    eng.srs_setup(12, SEED1)
    eng.srs_downsize(k)
    assert eng.srs_check() == ALL
    pk_old = eng.keygen(p, fixed, asg.copies)
    early = zk.Engine(0, share_with=eng)
    pk_early = early.keygen(p, fixed, asg.copies)

    def prove(e, pk):
        h = e.poly(1 << k)
        e.upload_canonical(h, asg.to_limbs(asg.advice[0]))
        out = e.prove(pk, [h], b"\x33" * 32, E.ZK_TRANSCRIPT_EVM)
        h.free()
        return out

    want = prove(eng, pk_old)
    with pytest.raises(zk.ZkError) as ex:
        eng.srs_downsize(k + 1)  # k > zk_srs_k
    assert ex.value.code == -1
    assert prove(eng, pk_old) == want  # (a refused downsize changes nothing)
    eng.srs_downsize(k)  # k == zk_srs_k recomputes: a new SRS, the same bytes
    with pytest.raises(zk.ZkError) as ex:
        prove(eng, pk_old)
    assert ex.value.code == -5
    assert prove(early, pk_early) == want  # shared before the call: the old SRS and its key still prove
    late = zk.Engine(0, share_with=eng)
    assert late.srs_write().tobytes() == eng.srs_write().tobytes()
    pk_late = late.keygen(p, fixed, asg.copies)
    assert prove(late, pk_late) == want
    pk_new = eng.keygen(p, fixed, asg.copies)
    assert prove(eng, pk_new) == want
    for e, pk in ((eng, pk_old), (eng, pk_new), (early, pk_early), (late, pk_late)):
        e.pk_free(pk)
    late.close()
    early.close()
    eng.close()
    fresh = zk.Engine(0)
    with pytest.raises(zk.ZkError) as ex:
        fresh.srs_downsize(4)
    assert ex.value.code == -5
    with pytest.raises(zk.ZkError) as ex:
        fresh.srs_check()
    assert ex.value.code == -5
    fresh.close()


def g2_words(pt):
    """G2 affine ((x0, x1), (y0, y1)) ints -> the 16-word Montgomery image zk_srs_set_g2 takes"""
    words = []
    for c in (pt[0][0], pt[0][1], pt[1][0], pt[1][1]):
        m = c * (1 << 256) % F.P
        words += [(m >> (64 * q)) & 0xFFFFFFFFFFFFFFFF for q in range(4)]
    return np.array(words, dtype=np.uint64)


def test_check_flags_on_broken_srs(engine):
    for k in (1, 2, 5, 10, 13):
        engine.srs_setup(k)
        assert engine.srs_check(bytes([k]) * 32) == ALL, k
    k = 6
    n = 1 << k
    engine.srs_setup(k, SEED1)
    g, gl = engine.srs_export(0, 0, n), engine.srs_export(1, 0, n)
    img = engine.srs_write().tobytes()
    g2, s_g2 = (np.frombuffer(img[4 + 2 * n * 64 + 128 * q:4 + 2 * n * 64 + 128 * (q + 1)], dtype=np.uint64).copy() for q in range(2))

    def load(a, b, s=s_g2, t=g2):
        engine.srs_load(k, a, b)
        engine.srs_set_g2(t, s)
        return engine.srs_check()

    assert load(g, gl) == ALL
    bad = g.copy()
    bad[5] = ref.to_mont_limbs([G(777)])[0]
    assert not load(bad, gl) & E.ZK_SRS_CHECK_POWERS
    bad = gl.copy()
    bad[9] = ref.to_mont_limbs([G(777)])[0]
    assert not load(g, bad) & E.ZK_SRS_CHECK_LAGRANGE
    s2 = ref_g2_from_words(s_g2)
    assert not load(g, gl, s=g2_words(curve.g2_add(s2, s2))) & E.ZK_SRS_CHECK_POWERS
    assert not load(gl, g) & E.ZK_SRS_CHECK_LAGRANGE
    # every point times the same scalar m: the structure holds, the generators do not
    m = 0x1234567
    gm = ref.to_mont_limbs([curve.mul(pt, m) for pt in ref.from_mont_limbs(g)])
    glm = ref.to_mont_limbs([curve.mul(pt, m) for pt in ref.from_mont_limbs(gl)])
    f = load(gm, glm, s=g2_words(curve.g2_mul(s2, m)), t=g2_words(curve.g2_mul(ref_g2_from_words(g2), m)))
    assert f == E.ZK_SRS_CHECK_POWERS | E.ZK_SRS_CHECK_LAGRANGE
    engine.srs_load(k, g, gl)  # no G2 half: ZK_ESTATE
    with pytest.raises(zk.ZkError) as ex:
        engine.srs_check()
    assert ex.value.code == -5


def ref_g2_from_words(w):
    rinv = F.inv(1 << 256, F.P)
    c = [sum(int(w[4 * q + i]) << (64 * i) for i in range(4)) * rinv % F.P for q in range(4)]
    return ((c[0], c[1]), (c[2], c[3]))


def es256_request():
    from webauthn_halo2_amd import ecdsa_p256 as api

    d, kk, z = 0x1234567, 0x7654321, 0xABCDEF
    q, r = api._p256_mul(d, api._G), api._p256_mul(kk, api._G)[0] % api._N
    sig_s = pow(kk, -1, api._N) * (z + r * d) % api._N
    return [v.to_bytes(32, "little") for v in (q[0], q[1], r, sig_s, z)]


def test_server_params_file_source(tmp_path):
    from webauthn_halo2_amd import ecdsa_p256 as api, proving_server as srv

    req = es256_request()
    body = {"pubkey_x": list(req[0]), "pubkey_y": list(req[1]), "r": list(req[2]), "s": list(req[3]), "msghash": list(req[4])}
    pkp, vkp = str(tmp_path / "proving_key.pk"), str(tmp_path / "verifying_key.vk")
    b = dict(body, proving_key_path=pkp)
    vbody = lambda path, proof: json.dumps({"verifying_key_path": path, "proof": proof})
    f0, f1 = tmp_path / "kzg_bn254_19.srs", tmp_path / "kzg_bn254_19_other.srs"
    f0.write_bytes(setup_image(19, bytes(32), E.ZK_SERDE_RAW_BYTES))
    f1.write_bytes(setup_image(19, SEED1, E.ZK_SERDE_RAW_BYTES))
    api.shutdown()
    try:
        srv.setup(0, 17, pkp, vkp)  # the default source: the seed-0 setup
        want_evm, want = srv.prove_evm(b, rng_seed=bytes(32)), srv.prove(b, rng_seed=bytes(32))
        srv.setup(0, 17, pkp, vkp, params_path=str(f0))
        assert api._STATE[0]["src"][0] == str(f0)
        assert srv.prove_evm(b, rng_seed=bytes(32)) == want_evm and srv.prove(b, rng_seed=bytes(32)) == want
        assert srv.verify(vbody(vkp, want)) == "verified" and srv.verify_evm(vbody(vkp, want_evm)) == "verified"
        with pytest.raises(ValueError):
            api.gen_srs(20)
        # another ceremony: its proofs verify under it, and not under the seed-0 source
        vk1 = str(tmp_path / "verifying_key_1.vk")
        srv.setup(0, 17, pkp, vk1, params_path=str(f1))
        assert api._STATE[0]["eng"].srs_check() == ALL
        other = srv.prove_evm(b, rng_seed=bytes(32))
        assert other != want_evm
        assert srv.verify_evm(vbody(vk1, other)) == "verified"
        api.set_params_file(None)
        with pytest.raises(FileNotFoundError):  # the keys went with the source
            srv.prove_evm(b, rng_seed=bytes(32))
        assert srv.verify_evm(vbody(vk1, other)) == "rejected"
        srv.setup(0, 17, pkp, None)
        assert srv.prove_evm(b, rng_seed=bytes(32)) == want_evm
    finally:
        api.set_params_file(None)
        api.shutdown()
