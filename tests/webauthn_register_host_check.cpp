// webauthn_register_host_check.cpp — csrc/webauthn_register.hip.h's portable form and its packing of a batch on the CPU: a
// stand-alone program (its own main, nothing of the library linked, no GPU touched), built by tests/test_webauthn_register_ref.py with
//   hipcc -x hip --offload-arch=gfx950 --cuda-host-only -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I webauthn-halo2_amd/csrc
// and run as a child process.
//
//   webauthn_register_host_check <cases.bin> <results.bin>
//
// cases.bin: the file tests/webauthn_register_cases.py write_case_file makes.  Every case runs TWICE.  Packed: all registrations
// of the file go through webauthn_register_pack - the function the library packs with - at once, the image it returns is copied
// into an allocation of exactly its length, and the rule runs through the descriptors and offsets of that image, as a lane does
// (the neighbours' bytes follow each string); a registration outside the caps must come out of the packer as not live and gets
// SIZE.  Exact: every string copied into an allocation of exactly its length, so that one byte read past an end is the
// sanitizer's to report.  The two runs must agree.  Then one small batch of its own checks the packer's arithmetic (packer_case).
// results.bin: MAGIC_OUT, the count; per registration webauthn_register_check_one's reason (1 byte) and the credential (104
// bytes), over a comb table of G this program builds with p256_comb_window.
#include "webauthn_host_io.h"
#include "webauthn_register.hip.h"
using namespace zk;

static const uint32_t MAGIC_IN = 0x57415231u, MAGIC_OUT = 0x5741524Fu;

struct Result {
    uint8_t reason;
    WebauthnCredential cred;
    bool operator==(const Result& o) const { return reason == o.reason && !memcmp(&cred, &o.cred, sizeof cred); }
};

// a request whose strings are exact allocations; `part`: attestationObject, clientDataJSON, challenge, origin
static zk_webauthn_registration request(const uint8_t* const part[4], const uint32_t len[4], const uint8_t* fixed) {
    zk_webauthn_registration q;
    memset(&q, 0, sizeof q);
    q.attestation_object = exact(part[0], len[0]), q.attestation_object_len = len[0];
    q.client_data_json = exact(part[1], len[1]), q.client_data_json_len = len[1];
    q.challenge = exact(part[2], len[2]), q.challenge_len = len[2];
    q.origin = (const char*)exact(part[3], len[3]), q.origin_len = len[3];
    memcpy(q.rp_id_hash, fixed, 32);
    q.flags_required = fixed[32];
    q.allow_cross_origin = fixed[33];
    q.attestation_policy = fixed[34];
    return q;
}

static void release(zk_webauthn_registration& q) {
    for (const void* p : {(const void*)q.attestation_object, (const void*)q.client_data_json, (const void*)q.challenge, (const void*)q.origin}) free((void*)p);
}

static bool size_ok(const zk_webauthn_registration& q) {
    return webauthn_register_size_ok(q.attestation_object_len, q.client_data_json_len, q.challenge_len, q.origin_len);
}

// the exact run: E as the library builds it, only for a request inside the caps (the buffer is sized for those)
static Result run_exact(const zk_webauthn_registration& q, const P256Affine* table) {
    uint8_t* e = (uint8_t*)malloc(WEBAUTHN_CREATE_PREFIX_MAX);
    uint32_t e_len = 0;
    if (size_ok(q)) {
        e_len = webauthn_expected_prefix(q.challenge, q.challenge_len, q.origin, q.origin_len, e, true);
        uint8_t* cut = exact(e, e_len);
        free(e);
        e = cut;
    }
    uint8_t* rp = exact(q.rp_id_hash, 32);
    Result r;
    memset(&r.cred, 0xEE, sizeof r.cred);
    r.reason = webauthn_register_check_one(q.attestation_object, q.attestation_object_len, q.client_data_json, q.client_data_json_len, q.challenge_len,
                                           q.origin_len, e, e_len, rp, q.flags_required, q.allow_cross_origin != 0, q.attestation_policy, table, &r.cred);
    free(rp);
    free(e);
    return r;
}

// the packed run of a whole batch: results[i] for every request, through the image of webauthn_register_pack
static std::vector<Result> run_packed(const std::vector<zk_webauthn_registration>& reqs, const P256Affine* table) {
    const WebauthnImage im = webauthn_register_pack(reqs.data(), reqs.size());
    check_image<WebauthnRegisterDesc>(im, {{&WebauthnRegisterDesc::obj_off, &WebauthnRegisterDesc::obj_len},
                                           {&WebauthnRegisterDesc::cd_off, &WebauthnRegisterDesc::cd_len},
                                           {&WebauthnRegisterDesc::e_off, &WebauthnRegisterDesc::e_len}});
    std::vector<Result> res(reqs.size());
    for (Result& r : res) {  // what the library gives a request without a lane
        memset(&r.cred, 0, sizeof r.cred);
        r.reason = ZK_WEBAUTHN_SIZE;
    }
    size_t j = 0;
    for (size_t i = 0; i < reqs.size(); i++) {
        const bool is_live = j < im.live.size() && im.live[j] == i;
        EXPECT(is_live == size_ok(reqs[i]), "request %zu is %s in the image, the size rule says otherwise", i, is_live ? "live" : "not live");
        j += is_live;
    }
    EXPECT(j == im.live.size(), "the image names %zu live requests, %zu of them are requests of the batch in ascending order", im.live.size(), j);
    uint8_t* image = exact(im.bytes.data(), im.bytes.size());
    const uint8_t* blob = image + im.live.size() * sizeof(WebauthnRegisterDesc);
    for (j = 0; j < im.live.size(); j++) {
        WebauthnRegisterDesc d;
        memcpy(&d, image + j * sizeof(WebauthnRegisterDesc), sizeof d);
        const zk_webauthn_registration& q = reqs[im.live[j]];
        Result& r = res[im.live[j]];
        r.reason = webauthn_register_check_one(blob + d.obj_off, d.obj_len, blob + d.cd_off, d.cd_len, q.challenge_len, q.origin_len, blob + d.e_off, d.e_len,
                                               d.rp_id_hash, d.flags_required, d.allow_cross_origin != 0, d.policy, table, &r.cred);
    }
    free(image);
    return res;
}

// The smallest batch that can go wrong in the packer: three requests, the middle one outside a cap, the outer ones with an empty
// clientDataJSON and a one-byte challenge
static void packer_case(const P256Affine* table) {
    static const uint8_t obj[3] = {0xA3, 0x63, 0x66}, challenge[1] = {0xA5}, fixed[35] = {0};
    std::vector<uint8_t> wide(ZK_WEBAUTHN_CHALLENGE_MAX + 1, 0x5A);
    const uint8_t* part[4] = {obj, obj, challenge, (const uint8_t*)"https://rp.example"};
    const uint8_t* part_wide[4] = {obj, obj, wide.data(), part[3]};
    const uint32_t inside[4] = {3, 0, 1, 18}, outside[4] = {3, 0, ZK_WEBAUTHN_CHALLENGE_MAX + 1, 18};
    std::vector<zk_webauthn_registration> reqs = {request(part, inside, fixed), request(part_wide, outside, fixed), request(part, inside, fixed)};
    const WebauthnImage im = webauthn_register_pack(reqs.data(), reqs.size());
    EXPECT(im.live == (std::vector<uint32_t>{0, 2}), "packer case: the live requests are not {0, 2}");
    // the sum of the parts, written out: two descriptors; per live request the object, no clientDataJSON and E, whose length is
    // the 39 + 12 + 16 literal bytes, 2 characters of a one-byte challenge and the origin
    const size_t e_len = 39 + 2 + 12 + 18 + 16;
    EXPECT(im.bytes.size() == 2 * sizeof(WebauthnRegisterDesc) + 2 * (3 + 0 + e_len), "packer case: the image has %zu bytes", im.bytes.size());
    const std::vector<Result> res = run_packed(reqs, table);  // (checks every offset + length against the image)
    EXPECT(res[1].reason == ZK_WEBAUTHN_SIZE && res[0] == run_exact(reqs[0], table) && res[2] == run_exact(reqs[2], table) && res[0] == res[2],
           "packer case: the packed results differ from the exact ones");
    for (zk_webauthn_registration& q : reqs) release(q);
}

int main(int argc, char** argv) {
    PROGRAM = "webauthn_register_host_check";
    if (argc != 3) {
        fprintf(stderr, "usage: webauthn_register_host_check cases.bin results.bin\n");
        return 2;
    }
    const std::vector<uint8_t> raw = slurp(argv[1]);
    Reader rd{raw};
    if (rd.u32() != MAGIC_IN) {
        fprintf(stderr, "webauthn_register_host_check: malformed case file\n");
        return 2;
    }
    const uint32_t n = rd.u32();
    const std::vector<P256Affine> table = comb_table();
    std::vector<zk_webauthn_registration> reqs;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t len[4];
        for (int k = 0; k < 4; k++) len[k] = rd.u32();
        const uint8_t* fixed = rd.take(35);  // rpIdHash, flags_required, allow_cross_origin, policy
        const uint8_t* part[4];
        for (int k = 0; k < 4; k++) part[k] = rd.take(len[k]);
        reqs.push_back(request(part, len, fixed));
    }
    rd.done();
    std::vector<uint8_t> out;
    put_u32(out, MAGIC_OUT);
    put_u32(out, n);
    const std::vector<Result> packed = run_packed(reqs, table.data());
    for (uint32_t i = 0; i < n; i++) {
        const Result r = run_exact(reqs[i], table.data());
        EXPECT(r == packed[i], "case %u gives reason %u packed and %u in exact allocations", i, packed[i].reason, r.reason);
        out.push_back(r.reason);
        out.insert(out.end(), (const uint8_t*)&r.cred, (const uint8_t*)&r.cred + sizeof r.cred);
        release(reqs[i]);
    }
    packer_case(table.data());
    write_results(argv[2], out);
    printf("webauthn_register_host_check: %u registrations, each twice\n", n);
    return 0;
}
