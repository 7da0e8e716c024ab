// webauthn_register_host_check.cpp — csrc/webauthn_register.hip.h's portable form on the CPU: a stand-alone program (its own main,
// nothing of the library linked, no GPU touched), built by tests/test_webauthn_register_ref.py with
//   hipcc -x hip --offload-arch=gfx950 --cuda-host-only -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I webauthn-halo2_amd/csrc
// and run as a child process.
//
//   webauthn_register_host_check <cases.bin> <results.bin>
//
// cases.bin: the file tests/webauthn_register_cases.py write_case_file makes.  Every case runs TWICE: once with its byte strings
// where they lie in one buffer that holds them back to back (as the library packs them: the neighbours' bytes follow each string),
// and once with every string copied into an allocation of exactly its length, so that one byte read past an end is the
// sanitizer's to report.  The two runs must agree.  results.bin: MAGIC_OUT, the count; per registration
// webauthn_register_check_one's reason (1 byte) and the credential (104 bytes), over a comb table of G this program builds with
// p256_comb_window.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "webauthn_register.hip.h"
using namespace zk;

static const uint32_t MAGIC_IN = 0x57415231u, MAGIC_OUT = 0x5741524Fu;

static std::vector<uint8_t> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "webauthn_register_host_check: cannot open %s\n", path);
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
            fprintf(stderr, "webauthn_register_host_check: the case file ends early\n");
            exit(2);
        }
    }
    uint32_t u32() {
        need(4);
        const uint32_t x = (uint32_t)v[pos] | ((uint32_t)v[pos + 1] << 8) | ((uint32_t)v[pos + 2] << 16) | ((uint32_t)v[pos + 3] << 24);
        pos += 4;
        return x;
    }
    const uint8_t* take(size_t n) {
        need(n);
        const uint8_t* p = v.data() + pos;
        pos += n;
        return p;
    }
};

// an allocation of exactly n bytes (never null: a zero-length string still has an address)
static uint8_t* exact(const uint8_t* p, size_t n) {
    uint8_t* q = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(q, p, n);
    return q;
}

// one run of the rule; `part`: attestationObject, clientDataJSON, challenge, origin
static uint8_t run(const uint8_t* const part[4], const uint32_t len[4], const uint8_t* fixed, const P256Affine* table, WebauthnCredential* cred) {
    memset(cred, 0xEE, sizeof *cred);
    // E as the library builds it: only for a request inside the caps (the buffer is sized for those)
    uint8_t* e = (uint8_t*)malloc(WEBAUTHN_CREATE_PREFIX_MAX);
    uint32_t e_len = 0;
    if (webauthn_register_size_ok(len[0], len[1], len[2], len[3])) {
        e_len = webauthn_expected_prefix(part[2], len[2], (const char*)part[3], len[3], e, true);
        uint8_t* cut = exact(e, e_len);
        free(e);
        e = cut;
    }
    uint8_t* rp = exact(fixed, 32);
    const uint8_t reason = webauthn_register_check_one(part[0], len[0], part[1], len[1], len[2], len[3], e, e_len, rp, fixed[32], fixed[33] != 0, fixed[34],
                                                       table, cred);
    free(rp);
    free(e);
    return reason;
}

int main(int argc, char** argv) {
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
    std::vector<P256Affine> table(P256_COMB_POINTS);
    for (int win = 0; win < P256_COMB_WINDOWS; win++) {
        P256LocalStore st;
        p256_comb_window(win, st, &table[(size_t)win * P256_COMB_ENTRIES]);
    }
    std::vector<uint8_t> out;
    for (int j = 0; j < 4; j++) out.push_back((uint8_t)(MAGIC_OUT >> (8 * j)));
    for (int j = 0; j < 4; j++) out.push_back((uint8_t)(n >> (8 * j)));
    for (uint32_t i = 0; i < n; i++) {
        uint32_t len[4];
        for (int k = 0; k < 4; k++) len[k] = rd.u32();
        const uint8_t* fixed = rd.take(35);  // rpIdHash, flags_required, allow_cross_origin, policy
        const uint8_t* packed[4];
        uint8_t* alone[4];
        for (int k = 0; k < 4; k++) {
            packed[k] = rd.take(len[k]);
            alone[k] = exact(packed[k], len[k]);
        }
        WebauthnCredential a, b;
        const uint8_t reason = run(packed, len, fixed, table.data(), &a);
        const uint8_t again = run(alone, len, fixed, table.data(), &b);
        for (int k = 0; k < 4; k++) free(alone[k]);
        if (reason != again || memcmp(&a, &b, sizeof a)) {
            fprintf(stderr, "webauthn_register_host_check: case %u gives reason %u packed and %u in exact allocations\n", i, reason, again);
            return 1;
        }
        out.push_back(reason);
        out.insert(out.end(), (const uint8_t*)&a, (const uint8_t*)&a + sizeof a);
    }
    if (rd.pos != raw.size()) {
        fprintf(stderr, "webauthn_register_host_check: %zu bytes left over in the case file\n", raw.size() - rd.pos);
        return 2;
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f)) {
        fprintf(stderr, "webauthn_register_host_check: cannot write %s\n", argv[2]);
        return 2;
    }
    printf("webauthn_register_host_check: %u registrations, each twice\n", n);
    return 0;
}
