// Host check of the shared host / device half of csrc/pairing.h (tests/test_pairing_lines.py builds and drives it; no device is
// opened).  The functions a lane of pairing_check_kernel runs are compiled here for the host.  One answer per line of input:
//   check <hex of a's 64 bytes> <hex of b's> <hex of g2's 128-byte image> <hex of s_g2's>
//       ->  check <m> <e> <host> <reason>
//           m: miller_loop_lines over the prepared table equals multi_miller_loop limb for limb
//           e: final_exponentiation_chain of that value equals final_exponentiation of it limb for limb
//           host: pairing_check's verdict; reason: pairing_check_lines' ZK_PAIRING_* value
//   steps <hex of a 128-byte G2 image>  ->  steps <PAIRING_STEPS> <steps a walk by hand takes> <popcount of the low word of 6u + 2>
//   g2proper <hex of a 128-byte G2 image>  ->  proper <0 | 1>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "pairing.h"

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
    std::vector<PairingTable> tab(1);
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, sa, sb, sg, ss;
        in >> op >> sa >> sb >> sg >> ss;
        if (op == "check") {
            const std::vector<uint8_t> ra = unhex(sa), rb = unhex(sb), rg = unhex(sg), rs = unhex(ss);
            if (ra.size() != 64 || rb.size() != 64 || rg.size() != 128 || rs.size() != 128) return 2;
            const G1Affine a = g1_of(ra), b = g1_of(rb);
            const G2A g2 = g2_from_raw(rg.data()), s_g2 = g2_from_raw(rs.data());
            pairing_table_make(g2, s_g2, tab.data());
            G1Affine P[2] = {a, b};
            P[1].y = fe_neg(b.y);
            const G2A Q[2] = {s_g2, g2};
            const Fq12 want = multi_miller_loop(P, Q, 2), got = miller_loop_lines(P[0], P[1], tab[0]);
            const Fq12 e_want = final_exponentiation(got), e_got = final_exponentiation_chain(got, tab[0].gamma);
            printf("check %d %d %d %d\n", memcmp(&want, &got, sizeof(Fq12)) == 0, memcmp(&e_want, &e_got, sizeof(Fq12)) == 0,
                   (int)pairing_check(a, b, g2, s_g2), (int)pairing_check_lines(a, b, tab[0]));
        } else if (op == "steps") {
            const std::vector<uint8_t> rg = unhex(sa);
            if (rg.size() != 128) return 2;
            // the walk as multi_miller_loop takes it, counted here without the table
            G2A T = g2_from_raw(rg.data());
            const G2A q = T;
            int n = 0;
            for (int b = 63; b >= 0; b--) {
                pairing_step_line(T, T);
                n++;
                if ((SIX_U_PLUS_2_LO >> b) & 1) {
                    pairing_step_line(T, q);
                    n++;
                }
            }
            n += 2;  // the two Frobenius lines
            std::vector<PairingLine> walk(PAIRING_STEPS + 1);
            memset((void*)walk.data(), 0xEE, walk.size() * sizeof(PairingLine));
            pairing_prepare(q, walk.data());
            const uint8_t* guard = (const uint8_t*)&walk[PAIRING_STEPS];
            bool untouched = true;
            for (size_t i = 0; i < sizeof(PairingLine); i++) untouched = untouched && guard[i] == 0xEE;
            if (!untouched) return 3;
            printf("steps %d %d %d\n", PAIRING_STEPS, n, __builtin_popcountll(SIX_U_PLUS_2_LO));
        } else if (op == "g2proper") {
            const std::vector<uint8_t> rg = unhex(sa);
            if (rg.size() != 128) return 2;
            printf("proper %d\n", (int)g2_is_proper(g2_from_raw(rg.data())));
        } else if (!op.empty()) {
            return 2;
        }
    }
    return 0;
}
