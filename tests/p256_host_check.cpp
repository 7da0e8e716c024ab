// p256_host_check.cpp — csrc/p256.hip.h's portable forms on the CPU: a stand-alone program (its own main, nothing of the
// library linked, no GPU touched), built by tests/test_es256_ref.py with
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I webauthn-halo2_amd/csrc
// and run as a child process.
//
//   p256_host_check <cases.bin> <results.bin> <signatures.bin> <reasons.bin>
//
// cases.bin: the case file of tests/p256_cases.py (field, point and x-compare cases); results.bin: MAGIC_OUT, n, OUT_WORDS, 1 and one
// result record per case.  signatures.bin: records of 160 bytes; reasons.bin: p256_verify_one's reason code per record, over a comb
// table of G this program builds with p256_comb_window.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "p256_check_ops.h"
using namespace zk;
using namespace p256check;

static std::vector<uint8_t> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "p256_host_check: cannot open %s\n", path);
        exit(2);
    }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}
static void spill(const char* path, const void* p, size_t n, const void* head = nullptr, size_t head_n = 0) {
    FILE* f = fopen(path, "wb");
    if (!f || (head_n && fwrite(head, 1, head_n, f) != head_n) || fwrite(p, 1, n, f) != n || fclose(f)) {
        fprintf(stderr, "p256_host_check: cannot write %s\n", path);
        exit(2);
    }
}

int main(int argc, char** argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: p256_host_check cases.bin results.bin signatures.bin reasons.bin\n");
        return 2;
    }
    const std::vector<uint8_t> raw = slurp(argv[1]);
    if (raw.size() < 16) return 2;
    std::vector<uint32_t> w(raw.size() / 4);
    for (size_t i = 0; i < w.size(); i++)
        w[i] = (uint32_t)raw[4 * i] | ((uint32_t)raw[4 * i + 1] << 8) | ((uint32_t)raw[4 * i + 2] << 16) | ((uint32_t)raw[4 * i + 3] << 24);
    const uint32_t n = w[1];
    if (w[0] != MAGIC_IN || w[2] != REC_WORDS || w.size() != 4 + (size_t)n * REC_WORDS) {
        fprintf(stderr, "p256_host_check: malformed case file\n");
        return 2;
    }
    std::vector<uint32_t> out((size_t)n * OUT_WORDS, 0xffffffffu);
    for (uint32_t i = 0; i < n; i++) run_case(&w[4 + (size_t)i * REC_WORDS], &out[(size_t)i * OUT_WORDS]);
    const uint32_t head[4] = {MAGIC_OUT, n, OUT_WORDS, 1};
    spill(argv[2], out.data(), out.size() * 4, head, sizeof head);

    std::vector<P256Affine> table(P256_COMB_POINTS);
    for (int win = 0; win < P256_COMB_WINDOWS; win++) {
        P256LocalStore st;
        p256_comb_window(win, st, &table[(size_t)win * P256_COMB_ENTRIES]);
    }
    const std::vector<uint8_t> sigs = slurp(argv[3]);
    if (sigs.size() % 160) {
        fprintf(stderr, "p256_host_check: the signature file is not a whole number of records\n");
        return 2;
    }
    std::vector<uint8_t> reasons(sigs.size() / 160);
    for (size_t i = 0; i < reasons.size(); i++) reasons[i] = p256_verify_one(&sigs[160 * i], table.data());
    spill(argv[4], reasons.data(), reasons.size());
    printf("p256_host_check: %u cases, %zu signatures\n", n, reasons.size());
    return 0;
}
