// Host check of csrc/evm_codegen.h (tests/test_evm_codegen.py builds and drives it; no GPU, no library): reads the description of
// one kind of proof on stdin and prints the Yul program generated for it, or — with --cost — the program's static cost as
// "name value" lines.
//
//   evm_codegen_check [--cost] < description
//
// description, one item per line (canonical hex):
//   shape <k> <advice> <lookup advice> <fixed> <lookup bits> <idle gate columns> <instance columns>
//   scheme gwc | shplonk
//   repr <transcript_repr>
//   fixed <x> <y>            one per fixed commitment, in order
//   perm <x> <y>             one per permutation commitment, in order
//   tau <s>                  g2 = the generator, s_g2 = [s] g2;  or both of
//   g2 <x.c0> <x.c1> <y.c0> <y.c1>   and   s_g2 <x.c0> <x.c1> <y.c0> <y.c1>
//   circuits <N>
//   instances <m_0> .. <m_{N-1}>     (absent: none)
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>

#include "evm_codegen.h"

using namespace zk;

template <class F>
static F from_hex(const std::string& h) {  // canonical big-endian hex -> Montgomery
    F c = F::zero();
    const std::string s = h.substr(0, 2) == "0x" ? h.substr(2) : h;
    for (size_t i = 0; i < s.size() && i < 64; i++) {
        const int d = (int)std::stoul(s.substr(s.size() - 1 - i, 1), nullptr, 16);
        c.v[i / 8] |= (uint32_t)d << (4 * (i % 8));
    }
    return fe_to_mont(c);
}

static G2A read_g2(std::istringstream& is) {
    std::string a, b, c, d;
    is >> a >> b >> c >> d;
    return G2A{{from_hex<Fq>(a), from_hex<Fq>(b)}, {from_hex<Fq>(c), from_hex<Fq>(d)}, false};
}

int main(int argc, char** argv) {
    const bool cost_only = argc >= 2 && !strcmp(argv[1], "--cost");
    evmgen::Desc d;
    d.params = zk_circuit_params{};
    d.transcript_repr = Fr::zero();
    d.g2 = g2_generator();
    d.s_g2 = d.g2;
    std::vector<uint32_t> ms;
    std::string line, tok;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        tok.clear();
        is >> tok;
        if (tok == "shape") {
            is >> d.params.k >> d.params.num_advice >> d.params.num_lookup_advice >> d.params.num_fixed >> d.params.lookup_bits >>
                d.params.num_idle_gate_columns >> d.params.num_instance_columns;
        } else if (tok == "scheme") {
            is >> tok;
            d.shplonk = tok == "shplonk";
        } else if (tok == "repr") {
            is >> tok;
            d.transcript_repr = from_hex<Fr>(tok);
        } else if (tok == "fixed" || tok == "perm") {
            std::string x, y;
            is >> x >> y;
            G1Affine p;
            p.x = from_hex<Fq>(x);
            p.y = from_hex<Fq>(y);
            (tok == "fixed" ? d.fixed : d.perm).push_back(p);
        } else if (tok == "tau") {
            is >> tok;
            d.g2 = g2_generator();
            d.s_g2 = g2_mul(d.g2, from_hex<Fr>(tok));
        } else if (tok == "g2") {
            d.g2 = read_g2(is);
        } else if (tok == "s_g2") {
            d.s_g2 = read_g2(is);
        } else if (tok == "circuits") {
            is >> d.n_circuits;
        } else if (tok == "instances") {
            uint32_t m;
            while (is >> m) ms.push_back(m);
        }
    }
    d.n_instances = ms.empty() ? std::vector<uint32_t>(d.n_circuits, 0) : ms;
    std::string text;
    evmgen::evm_verifier_cost cost;
    if (!evmgen::generate(d, &text, &cost)) {
        fprintf(stderr, "evm_codegen_check: the description is not of a kind this engine has\n");
        return 2;
    }
    if (cost_only) {
        printf("calldata_bytes %u\nmemory_bytes %u\nmodexp %u\necadd %u\necmul %u\npairing %u\nkeccak_calls %u\nkeccak_bytes %u\n", cost.calldata_bytes,
               cost.memory_bytes, cost.modexp, cost.ecadd, cost.ecmul, cost.pairing, cost.keccak_calls, cost.keccak_bytes);
    } else {
        fwrite(text.data(), 1, text.size(), stdout);
    }
    return 0;
}
