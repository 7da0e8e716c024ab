// Host check of csrc/serde_host.h and the codec under it, csrc/g1_codec.hip.h (tests/test_serde_host.py builds and drives it, once
// more under the sanitizers; no device is opened).  The functions are the ones the codec kernels call: this is a CPU run of what
// they run.  One answer per line of standard input; <fmt> is a ZK_SERDE_* number, points travel as hex:
//   sqrtexp                            ->  the compile-time (p + 1) / 4, 64 hex digits
//   ptb <hex of 32 bytes>              ->  point <hex of x || y big-endian> | refuse     (a proof point of the Blake2b transcript)
//   pte <hex of 64 bytes>              ->  point <hex of x || y big-endian> | refuse     (a proof point of the EVM transcript)
//   frr <0 | 1: big-endian> <hex of 32 bytes>  ->  value <hex, big-endian> | refuse      (verifier::fr_read)
//   g1r <fmt> <hex of 32 / 64 bytes>   ->  admit <hex of the 64-byte Montgomery image> | refuse       (host_g1_read)
//   g2r <fmt> <hex of 64 / 128 bytes>  ->  admit <hex of the 128-byte Montgomery image> | refuse      (host_g2_read)
//   g1w <fmt> <hex of the 64-byte image>   ->  bytes <hex>                                            (host_g1_write)
//   g2w <fmt> <hex of the 128-byte image>  ->  bytes <hex>                                            (host_g2_write)
//   in <len> <n> <n> ..        ->  per take its offset into the buffer or -1, then "pos <pos>"       (In; n = max: SIZE_MAX)
//   out <cap | null> <n> ..    ->  per take its offset or -1, then "pos <pos> real <0 | 1>"          (Out; null: size only)
//   be32 <value>               ->  bytes <hex of put_be32> back <get_be32 of them>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "serde_host.h"
#include "verifier.h"

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
static size_t count_of(const std::string& t) { return t == "max" ? SIZE_MAX : (size_t)std::stoull(t); }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, a, b;
        in >> op;
        if (op == "g1r" || op == "g2r" || op == "g1w" || op == "g2w") {
            int fmt;
            in >> fmt >> a;
            // the element sits at the very end of an exactly sized allocation: a read past it is a heap overflow a sanitizer sees
            const std::vector<uint8_t> v = unhex(a);
            const bool g1 = op[1] == '1';
            if (op[2] == 'r') {
                if (v.size() != (g1 ? g1_size(fmt) : g2_size(fmt))) return 2;
                if (g1) {
                    G1Affine p;
                    if (host_g1_read(v.data(), fmt, &p))
                        printf("admit %s\n", hex((const uint8_t*)&p, 64).c_str());
                    else
                        printf("refuse\n");
                } else {
                    std::vector<uint8_t> raw(128);
                    if (host_g2_read(v.data(), fmt, raw.data()))
                        printf("admit %s\n", hex(raw.data(), 128).c_str());
                    else
                        printf("refuse\n");
                }
            } else {
                if (v.size() != (g1 ? 64u : 128u)) return 2;
                std::vector<uint8_t> out(g1 ? g1_size(fmt) : g2_size(fmt));
                if (g1) {
                    G1Affine p;
                    memcpy(&p, v.data(), 64);
                    host_g1_write(p, fmt, out.data());
                } else {
                    host_g2_write(v.data(), fmt, out.data());
                }
                printf("bytes %s\n", hex(out.data(), out.size()).c_str());
            }
        } else if (op == "sqrtexp") {
            for (int i = 7; i >= 0; i--) printf("%08x", FqSqrt::EXP[i]);
            printf("\n");
        } else if (op == "ptb" || op == "pte") {
            in >> a;
            const std::vector<uint8_t> v = unhex(a);  // (exactly sized, as above)
            if (v.size() != (op == "ptb" ? 32u : 64u)) return 2;
            G1Affine p;
            uint8_t xy[64];
            // as verify_decode_kernel: the codec's answer, and the verifier's own rule that a proof holds no identity
            if (!(op == "ptb" ? g1_decompress(v.data(), &p) == G1_POINT : g1_read_evm(v.data(), &p))) {
                printf("refuse\n");
            } else {
                g1_write_evm(p, xy);
                printf("point %s\n", hex(xy, 64).c_str());
            }
        } else if (op == "frr") {
            int be;
            in >> be >> a;
            const std::vector<uint8_t> v = unhex(a);
            if (v.size() != 32u) return 2;
            Fr s;
            uint8_t out[32];
            if (!verifier::fr_read(v.data(), be != 0, &s)) {
                printf("refuse\n");
            } else {
                fe_to_bytes(fe_from_mont(s), true, out);
                printf("value %s\n", hex(out, 32).c_str());
            }
        } else if (op == "in") {
            size_t len;
            in >> len;
            const std::vector<uint8_t> buf(len ? len : 1);
            In r{buf.data(), len};
            while (in >> a) {
                const uint8_t* p = r.take(count_of(a));
                printf("%lld ", p ? (long long)(p - buf.data()) : -1LL);
            }
            printf("pos %zu\n", r.pos);
        } else if (op == "out") {
            in >> a;
            std::vector<uint8_t> buf(a == "null" ? 0 : std::stoull(a));
            Out w(a == "null" ? nullptr : buf.data(), buf.size());
            if (a != "null" && buf.empty()) return 2;
            while (in >> b) {
                const uint8_t* p = w.take(count_of(b));
                printf("%lld ", p ? (long long)(p - buf.data()) : -1LL);
            }
            printf("pos %zu real %d\n", w.pos, w.real ? 1 : 0);
        } else if (op == "be32") {
            in >> a;
            uint8_t w[4];
            put_be32(w, (uint32_t)std::stoul(a));
            printf("bytes %s back %u\n", hex(w, 4).c_str(), get_be32(w));
        } else if (!op.empty()) {
            return 2;
        }
    }
    return 0;
}
