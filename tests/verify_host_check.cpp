// Host check of csrc/pairing.h and csrc/verifier.h (tests/test_verify_host.py builds and drives it).  The proof-point decoding is
// the product's own (csrc/g1_codec.hip.h): a CPU run of what verify_decode_kernel runs.  The multi-scalar sums the product does on
// the device are restated here in their plainest host form — test code only: the product has no CPU path.
//
//   verify_host_check pairing <tau hex>     bilinearity / order / non-degeneracy, and e([tau]G1, G2) = e(G1, [tau]G2)
//   verify_host_check verify < job          one verdict per proof line of the job (format: tests/test_verify_host.py)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "pairing.h"
#include "verifier.h"

using namespace zk;

template <class F>
static F from_hex(const std::string& h) {  // canonical big-endian hex -> Montgomery
    F c = F::zero();
    std::string s = h.substr(0, 2) == "0x" ? h.substr(2) : h;
    for (size_t i = 0; i < s.size(); i++) {
        const int d = (int)std::stoul(s.substr(s.size() - 1 - i, 1), nullptr, 16);
        c.v[i / 8] |= (uint32_t)d << (4 * (i % 8));
    }
    return fe_to_mont(c);
}
template <class F>
static std::string to_hex(const F& m) {
    const F c = fe_from_mont(m);
    char buf[80];
    char* p = buf;
    p += sprintf(p, "0x");
    for (int w = 7; w >= 0; w--) p += sprintf(p, "%08x", c.v[w]);
    return buf;
}

static G1Affine to_affine(const G1X& p) {
    G1Affine r;
    if (p.is_identity()) {
        r.x = Fq::zero();
        r.y = Fq::zero();
        return r;
    }
    r.x = fe_mul(p.x, fe_inv_fast(p.zz));
    r.y = fe_mul(p.y, fe_inv_fast(p.zzz));
    return r;
}
static G1X g1_mul(const G1Affine& b, const Fr& s_mont) {  // naive double-and-add
    const Fr s = fe_from_mont(s_mont);
    G1X acc = G1X::identity();
    if (affine_is_identity(b)) return acc;
    for (int i = 255; i >= 0; i--) {
        acc = g1x_dbl(acc);
        if ((s.v[i >> 5] >> (i & 31)) & 1) g1x_add_affine(acc, b.x, b.y);
    }
    return acc;
}
static G1Affine msm(const std::vector<verifier::Term>& t, const std::vector<G1Affine>& bases) {
    G1X acc = G1X::identity();
    for (const auto& x : t) g1x_add(acc, g1_mul(bases[x.base], x.s));
    return to_affine(acc);
}
static G1Affine g1_gen() {
    G1Affine g;
    g.x = fq_small(1);
    g.y = fq_small(2);
    return g;
}

// one proof point, exactly as verify_decode_kernel decodes it: the product's codec, and the caller's rule that a proof holds no identity
static bool decode_point(const uint8_t* b, bool evm, G1Affine* out) { return evm ? g1_read_evm(b, out) : g1_decompress(b, out) == G1_POINT; }

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v(s.size() / 2);
    for (size_t i = 0; i < v.size(); i++) v[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return v;
}

static int run_pairing(const std::string& tau_hex) {
    int bad = 0;
    const G1Affine P = g1_gen();
    const G2A Q = g2_generator();
    ChaCha20Rng rng((const uint8_t*)"verify_host_check pairing seed!!");
    for (int it = 0; it < 2; it++) {
        const Fr a = rng.next_fr(), b = rng.next_fr();
        const Fq12 lhs = pairing(to_affine(g1_mul(P, a)), g2_mul(Q, b));
        const Fq12 rhs = pairing(to_affine(g1_mul(P, fe_mul(a, b))), Q);
        if (memcmp(&lhs, &rhs, sizeof(Fq12)) != 0) bad++, printf("bilinearity failed\n");
    }
    const Fq12 e = pairing(P, Q);
    if (f12_is_one(e)) bad++, printf("degenerate\n");
    {  // e^r = 1
        uint32_t rw[8];
        for (int i = 0; i < 8; i++) rw[i] = FrParams::P[i];
        Fq12 acc = f12_one();
        for (int i = 255; i >= 0; i--) {
            acc = f12_sqr(acc);
            if ((rw[i >> 5] >> (i & 31)) & 1) acc = f12_mul(acc, e);
        }
        if (!f12_is_one(acc)) bad++, printf("order != r\n");
    }
    G1Affine nP = P;
    nP.y = fe_neg(P.y);
    if (!f12_is_one(f12_mul(pairing(nP, Q), e))) bad++, printf("e(-P, Q) e(P, Q) != 1\n");
    const Fr tau = from_hex<Fr>(tau_hex);
    const G1Affine tP = to_affine(g1_mul(P, tau));
    const G2A tQ = g2_mul(Q, tau);
    if (!pairing_check(tP, P, Q, Q)) {
        // e(tP, Q) e(-P, Q) = 1 is false unless tau = 1: expected
    } else {
        bad++, printf("pairing_check accepted a wrong pair\n");
    }
    if (!pairing_check(P, tP, Q, tQ)) bad++, printf("e(G1, [tau]G2) != e([tau]G1, G2)\n");
    if (!pairing_check(tP, to_affine(g1_mul(P, fe_sqr(tau))), Q, tQ)) bad++, printf("e([tau]G1, [tau]G2) != e([tau^2]G1, G2)\n");
    G1Affine O;
    O.x = Fq::zero();
    O.y = Fq::zero();
    if (!pairing_check(O, O, Q, tQ)) bad++, printf("identity pair rejected\n");
    printf("pairing bad %d\n", bad);
    return bad ? 1 : 0;
}

static int run_verify() {
    zk_circuit_params cp{};
    std::string kind, scheme, tok;
    Fr repr;
    Fr tau;
    std::vector<G1Affine> fixed, perm;
    std::vector<std::string> proofs;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        is >> tok;
        if (tok == "shape") is >> cp.k >> cp.num_advice >> cp.num_lookup_advice >> cp.num_fixed >> cp.lookup_bits >> cp.num_idle_gate_columns;
        else if (tok == "kind") is >> kind;
        else if (tok == "scheme") is >> scheme;
        else if (tok == "repr") { is >> tok; repr = from_hex<Fr>(tok); }
        else if (tok == "tau") { is >> tok; tau = from_hex<Fr>(tok); }
        else if (tok == "fixed" || tok == "perm") {
            std::string x, y;
            is >> x >> y;
            G1Affine p;
            p.x = from_hex<Fq>(x);
            p.y = from_hex<Fq>(y);
            (tok == "fixed" ? fixed : perm).push_back(p);
        } else if (tok == "proof") {
            std::string h;
            is >> h;
            proofs.push_back(h == "-" ? "" : h);
        }
    }
    Layout lay;
    if (!lay.init(cp)) {
        printf("bad shape\n");
        return 2;
    }
    const bool evm = kind == "evm", shplonk = scheme == "shplonk";
    const verifier::ProofLayout pl = verifier::proof_layout(lay, evm, shplonk);
    const G2A g2 = g2_generator(), s_g2 = g2_mul(g2, tau);
    for (const std::string& ph : proofs) {
        const std::vector<uint8_t> proof = unhex(ph);
        int ok = 0;
        verifier::Prepared pr;
        bool prepared = false;
        if (proof.size() == pl.len) {
            std::vector<G1Affine> bases(pl.n_bases());
            bool pts_ok = true;
            for (uint32_t i = 0; i < pl.n_points; i++) pts_ok = pts_ok && decode_point(proof.data() + pl.point_off[i], evm, &bases[i]);
            if (pts_ok && verifier::prepare(lay, repr, pl, proof.data(), bases.data(), &pr)) {
                prepared = true;
                for (uint32_t i = 0; i < pl.n_fix; i++) bases[pl.base_fix() + i] = fixed[i];
                for (uint32_t i = 0; i < pl.n_perm; i++) bases[pl.base_perm() + i] = perm[i];
                bases[pl.base_g0()] = g1_gen();
                ok = pairing_check(msm(pr.a, bases), msm(pr.b, bases), g2, s_g2) ? 1 : 0;
            }
        }
        printf("verdict %d", ok);
        if (prepared) {
            const verifier::Challenges& c = pr.ch;
            printf(" theta %s beta %s gamma %s y %s x %s v %s u %s", to_hex(c.theta).c_str(), to_hex(c.beta).c_str(), to_hex(c.gamma).c_str(),
                   to_hex(c.y).c_str(), to_hex(c.x).c_str(), to_hex(c.v).c_str(), to_hex(c.u).c_str());
            if (shplonk) printf(" shplonk_y %s", to_hex(c.shplonk_y).c_str());
            printf(" terms %zu %zu", pr.a.size(), pr.b.size());
        }
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "pairing")) return run_pairing(argv[2]);
    if (argc >= 2 && !strcmp(argv[1], "verify")) return run_verify();
    fprintf(stderr, "usage: verify_host_check pairing <tau> | verify < job\n");
    return 2;
}
