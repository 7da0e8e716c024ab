// webauthn_host_check.cpp — csrc/webauthn.hip.h's portable forms on the CPU: a stand-alone program (its own main, nothing of the
// library linked, no GPU touched), built by tests/test_webauthn_ref.py with
//   hipcc -x hip --offload-arch=gfx950 --cuda-host-only -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I webauthn-halo2_amd/csrc
// and run as a child process.
//
//   webauthn_host_check <cases.bin> <results.bin>
//
// cases.bin: the file tests/webauthn_cases.py write_case_file makes (assertions, then messages for the hash alone).  Every byte
// string is copied into an allocation of exactly its length before it is used, so that a read past its end is the sanitizer's to
// report.  results.bin: MAGIC_OUT, the two counts; per assertion webauthn_check_one's reason (1 byte), the counter (4, little-endian)
// and the record (160), over a comb table of G this program builds with p256_comb_window; per message the 32 bytes of sha256_two.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "webauthn.hip.h"
using namespace zk;

static const uint32_t MAGIC_IN = 0x57414331u, MAGIC_OUT = 0x5741434Fu;

static std::vector<uint8_t> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "webauthn_host_check: cannot open %s\n", path);
        exit(2);
    }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

struct Reader {
    const std::vector<uint8_t>& v;
    size_t pos = 0;
    void need(size_t n) const {
        if (v.size() - pos < n) {
            fprintf(stderr, "webauthn_host_check: the case file ends early\n");
            exit(2);
        }
    }
    uint32_t u32() {
        need(4);
        const uint32_t x = (uint32_t)v[pos] | ((uint32_t)v[pos + 1] << 8) | ((uint32_t)v[pos + 2] << 16) | ((uint32_t)v[pos + 3] << 24);
        pos += 4;
        return x;
    }
    // an allocation of exactly n bytes (never null: a zero-length string still has an address)
    uint8_t* bytes(size_t n) {
        need(n);
        uint8_t* p = (uint8_t*)malloc(n ? n : 1);
        if (n) memcpy(p, &v[pos], n);
        pos += n;
        return p;
    }
};

static void put_u32(std::vector<uint8_t>& out, uint32_t x) {
    for (int j = 0; j < 4; j++) out.push_back((uint8_t)(x >> (8 * j)));
}

int main(int argc, char** argv) {
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
    std::vector<P256Affine> table(P256_COMB_POINTS);
    for (int win = 0; win < P256_COMB_WINDOWS; win++) {
        P256LocalStore st;
        p256_comb_window(win, st, &table[(size_t)win * P256_COMB_ENTRIES]);
    }
    std::vector<uint8_t> out;
    put_u32(out, MAGIC_OUT);
    put_u32(out, n);
    put_u32(out, n_msgs);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t len[5];
        for (int k = 0; k < 5; k++) len[k] = rd.u32();
        uint8_t* fixed = rd.bytes(98);  // x, y, rpIdHash, flags_required, allow_cross_origin
        uint8_t* part[5];
        for (int k = 0; k < 5; k++) part[k] = rd.bytes(len[k]);
        uint8_t* record = (uint8_t*)malloc(160);
        memset(record, 0xEE, 160);
        uint32_t sign_count = 0xEEEEEEEEu;
        // E as the library builds it: only for a request inside the caps (the buffer is sized for those)
        uint8_t* e = (uint8_t*)malloc(WEBAUTHN_PREFIX_MAX);
        uint32_t e_len = 0;
        if (webauthn_size_ok(len[0], len[1], len[2], len[3], len[4])) {
            e_len = webauthn_expected_prefix(part[3], len[3], (const char*)part[4], len[4], e);
            uint8_t* exact = (uint8_t*)malloc(e_len);
            memcpy(exact, e, e_len);
            free(e);
            e = exact;
        }
        const uint8_t reason = webauthn_check_one(part[0], len[0], part[1], len[1], part[2], len[2], len[3], len[4], e, e_len, fixed, fixed + 32, fixed + 64,
                                                  fixed[96], fixed[97] != 0, table.data(), record, &sign_count);
        out.push_back(reason);
        put_u32(out, sign_count);
        out.insert(out.end(), record, record + 160);
        free(e);
        free(record);
        free(fixed);
        for (int k = 0; k < 5; k++) free(part[k]);
    }
    for (uint32_t i = 0; i < n_msgs; i++) {
        const uint32_t l0 = rd.u32(), l1 = rd.u32();
        uint8_t* p0 = rd.bytes(l0);
        uint8_t* p1 = rd.bytes(l1);
        uint32_t h[8];
        uint8_t digest[32];
        sha256_two(p0, l0, p1, l1, h);
        sha256_put(h, digest);
        out.insert(out.end(), digest, digest + 32);
        free(p0);
        free(p1);
    }
    if (rd.pos != raw.size()) {
        fprintf(stderr, "webauthn_host_check: %zu bytes left over in the case file\n", raw.size() - rd.pos);
        return 2;
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f)) {
        fprintf(stderr, "webauthn_host_check: cannot write %s\n", argv[2]);
        return 2;
    }
    printf("webauthn_host_check: %u assertions, %u messages\n", n, n_msgs);
    return 0;
}
