// Host check of csrc/srs_update.h (tests/test_srs_update_host.py builds and drives it; no device is opened).  One answer per
// line of standard input:
//   receipt <hex of a zk_srs_contribution's 320 bytes>     ->  flags <SAME_SECRET | LINKS | NONTRIVIAL word>
//   g2mul <hex of a 128-byte G2 image> <s, canonical hex>  ->  g2 <hex of the image of [s] of it>
//   make <hex of before_g1's 64 bytes> <hex of after_g1's> <s, canonical hex>  ->  receipt <hex of the 320 bytes>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "srs_update.h"

using namespace zk;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v(s.size() / 2);
    for (size_t i = 0; i < v.size(); i++) v[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return v;
}
static std::string hex(const uint8_t* p, size_t n) {
    std::string s;
    char b[3];
    for (size_t i = 0; i < n; i++) {
        snprintf(b, sizeof b, "%02x", p[i]);
        s += b;
    }
    return s;
}
static Fr fr_from_hex(const std::string& h) {  // canonical big-endian hex -> Montgomery
    Fr c = Fr::zero();
    const std::string s = h.substr(0, 2) == "0x" ? h.substr(2) : h;
    for (size_t i = 0; i < s.size() && i < 64; i++) {
        const int d = (int)std::stoul(s.substr(s.size() - 1 - i, 1), nullptr, 16);
        c.v[i / 8] |= (uint32_t)d << (4 * (i % 8));
    }
    return fe_to_mont(c);
}

int main() {
    static_assert(sizeof(zk_srs_contribution) == 320, "the receipt is four packed point images");
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, a, b, c;
        in >> op >> a >> b >> c;
        if (op == "receipt") {
            const std::vector<uint8_t> raw = unhex(a);
            if (raw.size() != sizeof(zk_srs_contribution)) return 2;
            zk_srs_contribution r;
            memcpy(&r, raw.data(), sizeof r);
            printf("flags %u\n", srs_contribution_flags(r));
        } else if (op == "g2mul") {
            const std::vector<uint8_t> raw = unhex(a);
            if (raw.size() != 128) return 2;
            uint8_t out[128];
            srs_update_s_g2(raw.data(), fr_from_hex(b), out);
            printf("g2 %s\n", hex(out, 128).c_str());
        } else if (op == "make") {
            const std::vector<uint8_t> p = unhex(a), q = unhex(b);
            if (p.size() != 64 || q.size() != 64) return 2;
            uint64_t w[8];
            memcpy(w, p.data(), 64);
            const G1Affine before = g1_from_words(w);
            memcpy(w, q.data(), 64);
            const G1Affine after = g1_from_words(w);
            zk_srs_contribution r;
            srs_contribution_make(before, after, fr_from_hex(c), &r);
            printf("receipt %s\n", hex((const uint8_t*)&r, sizeof r).c_str());
        } else if (!op.empty()) {
            return 2;
        }
    }
    return 0;
}
