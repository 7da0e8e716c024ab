// webauthn_host_check.cpp — csrc/webauthn.hip.h's portable forms and its packing of a batch on the CPU: a stand-alone program (its
// own main, nothing of the library linked, no GPU touched), built by tests/test_webauthn_ref.py with
//   hipcc -x hip --offload-arch=gfx950 --cuda-host-only -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I webauthn-halo2_amd/csrc
// and run as a child process.
//
//   webauthn_host_check <cases.bin> <results.bin>
//
// cases.bin: the file tests/webauthn_cases.py write_case_file makes (assertions, then messages for the hash alone).  Every
// assertion runs TWICE.  Exact: every byte string, E included, in an allocation of exactly its length, so that a read past its end
// is the sanitizer's to report.  Packed: all assertions of the file go through webauthn_pack - the function the library packs
// with - at once, the image it returns is copied into an allocation of exactly its length, and the rule runs through the
// descriptors and offsets of that image, as a lane does; an assertion outside the caps must come out of the packer as not live
// and gets SIZE.  The two runs must agree.  Then one small batch of its own checks the packer's arithmetic (packer_case).
// results.bin: MAGIC_OUT, the two counts; per assertion webauthn_check_one's reason (1 byte), the counter (4, little-endian) and
// the record (160), over a comb table of G this program builds with p256_comb_window; per message the 32 bytes of sha256_two.
#include "webauthn_host_io.h"
using namespace zk;

static const uint32_t MAGIC_IN = 0x57414331u, MAGIC_OUT = 0x5741434Fu;

struct Result {
    uint8_t reason;
    uint32_t sign_count;
    uint8_t record[160];
    bool operator==(const Result& o) const { return reason == o.reason && sign_count == o.sign_count && !memcmp(record, o.record, 160); }
};

// a request whose strings are exact allocations (the caller frees them through the request)
static zk_webauthn_assertion request(const uint8_t* const part[5], const uint32_t len[5], const uint8_t* fixed) {
    zk_webauthn_assertion q;
    memset(&q, 0, sizeof q);
    q.authenticator_data = exact(part[0], len[0]), q.authenticator_data_len = len[0];
    q.client_data_json = exact(part[1], len[1]), q.client_data_json_len = len[1];
    q.signature = exact(part[2], len[2]), q.signature_len = len[2];
    q.challenge = exact(part[3], len[3]), q.challenge_len = len[3];
    q.origin = (const char*)exact(part[4], len[4]), q.origin_len = len[4];
    memcpy(q.pubkey_x, fixed, 32);
    memcpy(q.pubkey_y, fixed + 32, 32);
    memcpy(q.rp_id_hash, fixed + 64, 32);
    q.flags_required = fixed[96];
    q.allow_cross_origin = fixed[97];
    return q;
}

static void release(zk_webauthn_assertion& q) {
    for (const void* p : {(const void*)q.authenticator_data, (const void*)q.client_data_json, (const void*)q.signature, (const void*)q.challenge,
                          (const void*)q.origin})
        free((void*)p);
}

static bool size_ok(const zk_webauthn_assertion& q) {
    return webauthn_size_ok(q.authenticator_data_len, q.client_data_json_len, q.signature_len, q.challenge_len, q.origin_len);
}

// the exact run: E as the library builds it, only for a request inside the caps (the buffer is sized for those)
static Result run_exact(const zk_webauthn_assertion& q, const P256Affine* table) {
    uint8_t* e = (uint8_t*)malloc(WEBAUTHN_PREFIX_MAX);
    uint32_t e_len = 0;
    if (size_ok(q)) {
        e_len = webauthn_expected_prefix(q.challenge, q.challenge_len, q.origin, q.origin_len, e);
        uint8_t* cut = exact(e, e_len);
        free(e);
        e = cut;
    }
    uint8_t *x = exact(q.pubkey_x, 32), *y = exact(q.pubkey_y, 32), *rp = exact(q.rp_id_hash, 32);
    uint8_t* record = (uint8_t*)malloc(160);
    memset(record, 0xEE, 160);
    Result r;
    r.sign_count = 0xEEEEEEEEu;
    r.reason = webauthn_check_one(q.authenticator_data, q.authenticator_data_len, q.client_data_json, q.client_data_json_len, q.signature, q.signature_len,
                                  q.challenge_len, q.origin_len, e, e_len, x, y, rp, q.flags_required, q.allow_cross_origin != 0, table, record, &r.sign_count);
    memcpy(r.record, record, 160);
    for (uint8_t* p : {record, x, y, rp, e}) free(p);
    return r;
}

// the packed run of a whole batch: results[i] for every request, through the image of webauthn_pack
static std::vector<Result> run_packed(const std::vector<zk_webauthn_assertion>& reqs, const P256Affine* table) {
    const WebauthnImage im = webauthn_pack(reqs.data(), reqs.size());
    check_image<WebauthnDesc>(im, {{&WebauthnDesc::ad_off, &WebauthnDesc::ad_len},
                                   {&WebauthnDesc::cd_off, &WebauthnDesc::cd_len},
                                   {&WebauthnDesc::sig_off, &WebauthnDesc::sig_len},
                                   {&WebauthnDesc::e_off, &WebauthnDesc::e_len}});
    std::vector<Result> res(reqs.size());
    for (Result& r : res) {  // what the library gives a request without a lane
        memset(&r, 0, sizeof r);
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
    const uint8_t* blob = image + im.live.size() * sizeof(WebauthnDesc);
    for (j = 0; j < im.live.size(); j++) {
        WebauthnDesc d;
        memcpy(&d, image + j * sizeof(WebauthnDesc), sizeof d);
        const zk_webauthn_assertion& q = reqs[im.live[j]];
        Result& r = res[im.live[j]];
        r.reason = webauthn_check_one(blob + d.ad_off, d.ad_len, blob + d.cd_off, d.cd_len, blob + d.sig_off, d.sig_len, q.challenge_len, q.origin_len,
                                      blob + d.e_off, d.e_len, d.x, d.y, d.rp_id_hash, d.flags_required, d.allow_cross_origin != 0, table, r.record,
                                      &r.sign_count);
    }
    free(image);
    return res;
}

// The smallest batch that can go wrong in the packer: three requests, the middle one outside a cap, the outer ones with an empty
// clientDataJSON and a one-byte challenge
static void packer_case(const P256Affine* table) {
    static const uint8_t ad[37] = {0}, sig[8] = {0x30, 0x06, 0x02, 0x01, 0x01, 0x02, 0x01, 0x01}, challenge[1] = {0xA5}, fixed[98] = {0};
    const uint8_t* part[5] = {ad, ad, sig, challenge, (const uint8_t*)"https://rp.example"};
    const uint32_t inside[5] = {37, 0, 8, 1, 18}, outside[5] = {37, 0, 8, ZK_WEBAUTHN_CHALLENGE_MAX + 1, 18};
    std::vector<uint8_t> wide(ZK_WEBAUTHN_CHALLENGE_MAX + 1, 0x5A);
    const uint8_t* part_wide[5] = {ad, ad, sig, wide.data(), part[4]};
    std::vector<zk_webauthn_assertion> reqs = {request(part, inside, fixed), request(part_wide, outside, fixed), request(part, inside, fixed)};
    const WebauthnImage im = webauthn_pack(reqs.data(), reqs.size());
    EXPECT(im.live == (std::vector<uint32_t>{0, 2}), "packer case: the live requests are not {0, 2}");
    // the sum of the parts, written out: two descriptors; per live request authData, no clientDataJSON, the signature and E, whose
    // length is the 36 + 12 + 16 literal bytes, 2 characters of a one-byte challenge and the origin
    const size_t e_len = 36 + 2 + 12 + 18 + 16;
    EXPECT(im.bytes.size() == 2 * sizeof(WebauthnDesc) + 2 * (37 + 0 + 8 + e_len), "packer case: the image has %zu bytes", im.bytes.size());
    const std::vector<Result> res = run_packed(reqs, table);  // (checks every offset + length against the image)
    EXPECT(res[1].reason == ZK_WEBAUTHN_SIZE && res[0] == run_exact(reqs[0], table) && res[2] == run_exact(reqs[2], table) && res[0] == res[2],
           "packer case: the packed results differ from the exact ones");
    for (zk_webauthn_assertion& q : reqs) release(q);
}

int main(int argc, char** argv) {
    PROGRAM = "webauthn_host_check";
    if (argc != 3) {
        fprintf(stderr, "usage: webauthn_host_check cases.bin results.bin\n");
        return 2;
    }
    const std::vector<uint8_t> raw = slurp(argv[1]);
    Reader rd{raw};
    if (rd.u32() != MAGIC_IN) {
        fprintf(stderr, "webauthn_host_check: malformed case file\n");
        return 2;
    }
    const uint32_t n = rd.u32(), n_msgs = rd.u32();
    const std::vector<P256Affine> table = comb_table();
    std::vector<zk_webauthn_assertion> reqs;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t len[5];
        for (int k = 0; k < 5; k++) len[k] = rd.u32();
        const uint8_t* fixed = rd.take(98);  // x, y, rpIdHash, flags_required, allow_cross_origin
        const uint8_t* part[5];
        for (int k = 0; k < 5; k++) part[k] = rd.take(len[k]);
        reqs.push_back(request(part, len, fixed));
    }
    std::vector<uint8_t> out;
    put_u32(out, MAGIC_OUT);
    put_u32(out, n);
    put_u32(out, n_msgs);
    const std::vector<Result> packed = run_packed(reqs, table.data());
    for (uint32_t i = 0; i < n; i++) {
        const Result r = run_exact(reqs[i], table.data());
        EXPECT(r == packed[i], "case %u gives reason %u in exact allocations and %u packed", i, r.reason, packed[i].reason);
        out.push_back(r.reason);
        put_u32(out, r.sign_count);
        out.insert(out.end(), r.record, r.record + 160);
        release(reqs[i]);
    }
    for (uint32_t i = 0; i < n_msgs; i++) {
        const uint32_t l0 = rd.u32(), l1 = rd.u32();
        uint8_t* p0 = exact(rd.take(l0), l0);
        uint8_t* p1 = exact(rd.take(l1), l1);
        uint32_t h[8];
        uint8_t digest[32];
        sha256_two(p0, l0, p1, l1, h);
        sha256_put(h, digest);
        out.insert(out.end(), digest, digest + 32);
        free(p0);
        free(p1);
    }
    rd.done();
    packer_case(table.data());
    write_results(argv[2], out);
    printf("webauthn_host_check: %u assertions, each twice, %u messages\n", n, n_msgs);
    return 0;
}
