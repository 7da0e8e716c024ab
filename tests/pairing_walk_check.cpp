// Host check of the G2-per-lane half of csrc/pairing.h (tests/test_pairing_walk.py builds and drives it; no device is opened).
// The functions a lane of pairing_check_each_kernel and contribution_check_kernel runs are compiled here for the host.  One answer
// per line of input:
//   walk <hex of P's 64 bytes> <hex of Q's 128-byte image>
//       ->  walk <hex of the 384 bytes of final_exponentiation_chain(miller_loop_walk<1>(Q; P))>   (the fixed side left out)
//   each <hex of a> <hex of b> <hex of q> <hex of g2>  ->  each <pairing_check_walk's reason> <pairing_check(a, b, g2, q), or -1 for an improper q>
//   g2proper <hex of a 128-byte G2 image>  ->  proper <g2_is_proper> <g2_is_proper_lane>
//   receipt <hex of before_g1> <hex of after_g1> <hex of s_g1> <hex of s_g2>
//       ->  receipt <srs_contribution_flags> <contribution_check_lanes against the generator's table>
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
static G1Affine g1_of(const std::vector<uint8_t>& raw) {
    G1Affine p;
    memcpy(p.x.v, raw.data(), 32);
    memcpy(p.y.v, raw.data() + 32, 32);
    return p;
}

int main() {
    std::string line;
    std::vector<PairingTable> gen(1), tab(1);
    const G2A none{f2_zero(), f2_zero(), true};
    pairing_table_make(g2_generator(), none, gen.data());
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, s0, s1, s2, s3;
        in >> op >> s0 >> s1 >> s2 >> s3;
        if (op == "walk") {
            const std::vector<uint8_t> rp = unhex(s0), rq = unhex(s1);
            if (rp.size() != 64 || rq.size() != 128) return 2;
            const G1Affine P = g1_of(rp), O{Fq::zero(), Fq::zero()};
            Fq12 f;
            miller_loop_walk<1>(g2_from_raw(rq.data()), &P, &O, gen[0], &f);
            const Fq12 e = final_exponentiation_chain(f, gen[0].gamma);
            const uint8_t* b = (const uint8_t*)&e;
            printf("walk ");
            for (size_t i = 0; i < sizeof(Fq12); i++) printf("%02x", b[i]);
            printf("\n");
        } else if (op == "each") {
            const std::vector<uint8_t> ra = unhex(s0), rb = unhex(s1), rq = unhex(s2), rg = unhex(s3);
            if (ra.size() != 64 || rb.size() != 64 || rq.size() != 128 || rg.size() != 128) return 2;
            const G2A q = g2_from_raw(rq.data()), g2 = g2_from_raw(rg.data());
            pairing_table_make(g2, none, tab.data());
            printf("each %d %d\n", (int)pairing_check_walk(g1_of(ra), g1_of(rb), q, tab[0]), g2_is_proper(q) ? (int)pairing_check(g1_of(ra), g1_of(rb), g2, q) : -1);
        } else if (op == "g2proper") {
            const std::vector<uint8_t> rg = unhex(s0);
            if (rg.size() != 128) return 2;
            const G2A q = g2_from_raw(rg.data());
            printf("proper %d %d\n", (int)g2_is_proper(q), (int)g2_is_proper_lane(q));
        } else if (op == "receipt") {
            const std::vector<uint8_t> r0 = unhex(s0), r1 = unhex(s1), r2 = unhex(s2), r3 = unhex(s3);
            if (r0.size() != 64 || r1.size() != 64 || r2.size() != 64 || r3.size() != 128) return 2;
            zk_srs_contribution c;
            memcpy(c.before_g1, r0.data(), 64);
            memcpy(c.after_g1, r1.data(), 64);
            memcpy(c.s_g1, r2.data(), 64);
            memcpy(c.s_g2, r3.data(), 128);
            printf("receipt %u %u\n", srs_contribution_flags(c), contribution_check_lanes(g1_of(r0), g1_of(r1), g1_of(r2), g2_from_raw(r3.data()), gen[0]));
        } else if (!op.empty()) {
            return 2;
        }
    }
    return 0;
}
