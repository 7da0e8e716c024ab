// Host check of csrc/verifier.h with ONE instance list PER CIRCUIT (the host half of zk_verify_multi_public and, with one circuit, of
// zk_verify_batch_public; tests/test_verify_public_forms_host.py builds and drives it): tests/verify_host_check.cpp's job reader,
// point decoding, host sums and pairing as they stand; the circuit count, the instance column and the lists come from the command
// line.  Every proof is prepared TWICE - verifier::prepare_lists computing inst(x) itself, and again with the values handed in
// (verifier::challenge_x, then verifier::instance_eval per list, as a caller that evaluates elsewhere would) - and the two must
// agree in their verdict, their challenges and their term lists, or the program fails.
//
//   verify_public_forms_host_check <n_circuits> <file: one line per circuit, its values in hex, or "-"> < job
//   one verdict per proof line of the job (format: tests/test_verify_host.py)
#include <fstream>

#include "pairing.h"
#include "verifier.h"

static uint32_t g_circuits = 1;
static std::vector<std::vector<zk::Fr>> g_lists;
static int g_mismatch = 0;
static const zk_circuit_params& with_instance_column(zk_circuit_params& cp) {
    cp.num_instance_columns = 1;
    return cp;
}

static bool same_terms(const std::vector<zk::verifier::Term>& a, const std::vector<zk::verifier::Term>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].base != b[i].base || memcmp(&a[i].s, &b[i].s, sizeof(zk::Fr)) != 0) return false;
    return true;
}

// (shplonk_y is set under SHPLONK only: the fields every proof sets are compared)
static bool same_challenges(const zk::verifier::Challenges& a, const zk::verifier::Challenges& b) {
    const zk::Fr* fa[] = {&a.theta, &a.beta, &a.gamma, &a.y, &a.x, &a.v, &a.u};
    const zk::Fr* fb[] = {&b.theta, &b.beta, &b.gamma, &b.y, &b.x, &b.v, &b.u};
    for (int i = 0; i < 7; i++)
        if (memcmp(fa[i], fb[i], sizeof(zk::Fr)) != 0) return false;
    return true;
}

static bool prepare_both(const Layout& lay, const zk::Fr& repr, const zk::verifier::ProofLayout& pl, const uint8_t* proof, const G1Affine* pts,
                         zk::verifier::Prepared* out) {
    using namespace zk;
    std::vector<verifier::InstanceList> lists;
    for (const auto& l : g_lists) lists.push_back(verifier::InstanceList{l.data(), l.size()});
    const bool ok = verifier::prepare_lists(lay, repr, pl, proof, pts, out, lists.data(), lists.size());
    // the same with inst(x) computed outside
    const Fr x = verifier::challenge_x(lay, repr, pl, pts, lists.data(), lists.size());
    Fr xn = x;
    for (uint32_t i = 0; i < lay.k; i++) xn = fe_sqr(xn);
    const Fr c = fe_mul(fe_sub(xn, Fr::one()), fe_inv_fast(fr_from_u64(lay.n)));
    std::vector<Fr> vals(lists.size());
    std::vector<uint8_t> on_domain(lists.size(), 0);
    for (size_t l = 0; l < lists.size(); l++) on_domain[l] = verifier::instance_eval(lay, lists[l].vals, lists[l].n, x, c, &vals[l]) ? 0 : 1;
    const verifier::InstanceEvals given{vals.data(), on_domain.data()};
    verifier::Prepared other;
    const bool ok2 = verifier::prepare_lists(lay, repr, pl, proof, pts, &other, lists.data(), lists.size(), &given);
    if (ok != ok2 || (ok && (!same_terms(out->a, other.a) || !same_terms(out->b, other.b) || !same_challenges(out->ch, other.ch)))) {
        g_mismatch++;
        fprintf(stderr, "the form that takes inst(x) disagrees with the one that computes it\n");
    }
    return ok;
}

#define init(cp) init(with_instance_column(cp))
#define proof_layout(lay, evm, shplonk) proof_layout(lay, evm, shplonk, g_circuits)
#define prepare(lay, repr, pl, proof, pts, out) prepare_for_check(lay, repr, pl, proof, pts, out)
namespace zk {
namespace verifier {
static bool prepare_for_check(const Layout& lay, const Fr& repr, const ProofLayout& pl, const uint8_t* proof, const G1Affine* pts, Prepared* out) {
    return prepare_both(lay, repr, pl, proof, pts, out);
}
}  // namespace verifier
}  // namespace zk
#define main verify_host_check_main
#include "verify_host_check.cpp"
#undef main
#undef prepare
#undef proof_layout
#undef init

int main(int argc, char** argv) {
    if (argc < 3 || atoi(argv[1]) < 1) {
        fprintf(stderr, "usage: verify_public_forms_host_check <n_circuits> <lists file> < job\n");
        return 2;
    }
    g_circuits = (uint32_t)atoi(argv[1]);
    std::ifstream f(argv[2]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream is(line);
        std::string h;
        std::vector<zk::Fr> l;
        while (is >> h)
            if (h != "-") l.push_back(from_hex<Fr>(h));
        g_lists.push_back(l);
    }
    if (g_lists.size() != g_circuits) {
        fprintf(stderr, "%zu lists for %u circuits\n", g_lists.size(), g_circuits);
        return 2;
    }
    const int rc = run_verify();
    return rc ? rc : (g_mismatch ? 3 : 0);
}
