// Host check of public inputs (tests/test_public_host.py builds and drives it): csrc/verifier.h with the instance values absorbed and
// inst(x) as the instance column's evaluation, and csrc/vkrepr.h + csrc/pk.h rendering the vk digest of a shape with the column.
// tests/verify_host_check.cpp's job reader, point decoding, host sums and pairing as they stand; the shape line's missing seventh
// number (instance columns) and the instance values come from the command line.
//
//   public_host_check verify <n_instance_columns> <file of instance values, one hex per line> < job    one verdict per proof line
//   public_host_check repr <n_instance_columns> < job      transcript_repr of the job's shape and commitments (format: tests/test_verify_host.py)
#include <fstream>

#include "pairing.h"
#include "verifier.h"
#include "vkrepr.h"

static uint32_t g_instance_columns = 0;
static std::vector<zk::Fr> g_instance;
static const zk_circuit_params& with_instance_column(zk_circuit_params& cp) {
    cp.num_instance_columns = g_instance_columns;
    return cp;
}
#define init(cp) init(with_instance_column(cp))
#define prepare(lay, repr, pl, proof, pts, out) prepare(lay, repr, pl, proof, pts, out, g_instance.data(), g_instance.size())
#define main verify_host_check_main
#include "verify_host_check.cpp"
#undef main
#undef prepare
#undef init

static int run_repr() {
    zk_circuit_params cp{};
    std::vector<G1Affine> fixed, perm;
    std::string line, tok;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        is >> tok;
        if (tok == "shape") is >> cp.k >> cp.num_advice >> cp.num_lookup_advice >> cp.num_fixed >> cp.lookup_bits >> cp.num_idle_gate_columns;
        else if (tok == "fixed" || tok == "perm") {
            std::string x, y;
            is >> x >> y;
            G1Affine p;
            p.x = from_hex<Fq>(x);
            p.y = from_hex<Fq>(y);
            (tok == "fixed" ? fixed : perm).push_back(p);
        }
    }
    cp.num_instance_columns = g_instance_columns;
    Layout lay;
    if (!lay.init(cp) || fixed.size() != lay.n_fix || perm.size() != lay.perm_cols.size()) {
        printf("bad shape\n");
        return 2;
    }
    printf("repr %s perm_cols %zu chunks %u\n", to_hex(vkrepr::transcript_repr(lay, fixed, perm)).c_str(), lay.perm_cols.size(), lay.n_chunks);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3) g_instance_columns = (uint32_t)atoi(argv[2]);
    if (argc >= 3 && !strcmp(argv[1], "repr")) return run_repr();
    if (argc >= 4 && !strcmp(argv[1], "verify")) {
        std::ifstream f(argv[3]);
        std::string h;
        while (f >> h) g_instance.push_back(from_hex<Fr>(h));
        return run_verify();
    }
    fprintf(stderr, "usage: public_host_check verify <n_instance_columns> <instance file> < job | repr <n_instance_columns> < job\n");
    return 2;
}
