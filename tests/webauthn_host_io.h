// webauthn_host_io.h — what the two stand-alone CPU programs of the WebAuthn rules share (webauthn_host_check.cpp,
// webauthn_register_host_check.cpp): the reader of a case file, exact allocations, the comb table of G, the result file.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <utility>
#include <vector>

#include "../include/zkmi355.h"  // (first: the rule headers define the same constants where this one is absent)
#include "webauthn.hip.h"

static const char* PROGRAM = "webauthn host check";  // set by main: the name in front of every message

static std::vector<uint8_t> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "%s: cannot open %s\n", PROGRAM, path);
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
            fprintf(stderr, "%s: the case file ends early\n", PROGRAM);
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
    void done() const {
        if (pos != v.size()) {
            fprintf(stderr, "%s: %zu bytes left over in the case file\n", PROGRAM, v.size() - pos);
            exit(2);
        }
    }
};

// an allocation of exactly n bytes (never null: a zero-length string still has an address), so that one byte read past its end
// is the sanitizer's to report
static uint8_t* exact(const void* p, size_t n) {
    uint8_t* q = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(q, p, n);
    return q;
}

static void put_u32(std::vector<uint8_t>& out, uint32_t x) {
    for (int j = 0; j < 4; j++) out.push_back((uint8_t)(x >> (8 * j)));
}

static std::vector<zk::P256Affine> comb_table() {
    std::vector<zk::P256Affine> table(zk::P256_COMB_POINTS);
    for (int win = 0; win < zk::P256_COMB_WINDOWS; win++) {
        zk::P256LocalStore st;
        zk::p256_comb_window(win, st, &table[(size_t)win * zk::P256_COMB_ENTRIES]);
    }
    return table;
}

static void write_results(const char* path, const std::vector<uint8_t>& out) {
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f)) {
        fprintf(stderr, "%s: cannot write %s\n", PROGRAM, path);
        exit(2);
    }
}

// a failed expectation of the program itself ends it with status 1
#define EXPECT(cond, ...)                       \
    do {                                        \
        if (!(cond)) {                          \
            fprintf(stderr, "%s: ", PROGRAM);   \
            fprintf(stderr, __VA_ARGS__);       \
            fprintf(stderr, "\n");              \
            exit(1);                            \
        }                                       \
    } while (0)

// What must hold of any image (csrc/webauthn.hip.h WebauthnImage) with descriptors Desc; `strings` names the (offset, length)
// members of a descriptor's strings in the order they are packed.  Every string lies inside the blob, the strings lie back to back in descriptor order,
// and the image's length is the sum of its parts: the descriptors and every string
template <class Desc>
static void check_image(const zk::WebauthnImage& im, std::initializer_list<std::pair<uint32_t Desc::*, uint32_t Desc::*>> strings) {
    const size_t n = im.live.size(), desc_bytes = n * sizeof(Desc);
    EXPECT(im.bytes.size() >= desc_bytes, "the image is shorter than its descriptors");
    const size_t blob = im.bytes.size() - desc_bytes;
    size_t at = 0;
    for (size_t j = 0; j < n; j++) {
        Desc d;
        memcpy(&d, im.bytes.data() + j * sizeof(Desc), sizeof d);
        for (const auto& s : strings) {
            const size_t off = d.*s.first, len = d.*s.second;
            EXPECT(off <= blob && len <= blob - off, "descriptor %zu: %zu + %zu lies outside the blob of %zu bytes", j, off, len, blob);
            EXPECT(off == at, "descriptor %zu: a string starts at %zu, the one before it ended at %zu", j, off, at);
            at += len;
        }
    }
    EXPECT(at == blob, "the image holds %zu blob bytes, its strings add up to %zu", blob, at);
}
