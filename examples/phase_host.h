// phase_host.h — what the phase-level example hosts share (prove_host_phases.cpp: one circuit, the reference's shape;
// prove_host_phases_multi.cpp: N circuits and public inputs): the call counter, the small helpers over the C ABI, and the two
// multi-open provers (ProverGWC, ProverSHPLONK) over a query list — host-side field arithmetic from the engine's host headers, the
// device work through zk_poly_lincomb / zk_kate_division / zk_commit_batch.  Nothing of the engine's prover is used.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../include/zkmi355.h"
#include "../webauthn-halo2_amd/csrc/transcript.h"

using namespace zk;

static const char* prog = "phase_host";  // set by main: the prefix of every message
static zk_ctx* ctx = nullptr;
static size_t abi_calls = 0;  // every call of the engine's ABI goes through CHECK

static std::vector<uint8_t> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "%s: cannot open %s\n", prog, path);
        exit(2);
    }
    fseek(f, 0, SEEK_END);
    const long len = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> buf((size_t)len);
    if (len && fread(buf.data(), 1, (size_t)len, f) != (size_t)len) {
        fprintf(stderr, "%s: short read of %s\n", prog, path);
        exit(2);
    }
    fclose(f);
    return buf;
}

#define CHECK(call)                                                                                                      \
    do {                                                                                                                 \
        abi_calls++;                                                                                                     \
        const int rc_ = (call);                                                                                          \
        if (rc_ != ZK_OK) {                                                                                              \
            fprintf(stderr, "%s: %s failed: %d (%s)\n", prog, #call, rc_, zk_strerror(rc_));                             \
            exit(1);                                                                                                     \
        }                                                                                                                \
    } while (0)

static const uint64_t* limbs(const Fr& a) { return reinterpret_cast<const uint64_t*>(a.v); }
static zk_poly alloc(size_t n) {
    zk_poly p = 0;
    CHECK(zk_poly_alloc(ctx, n, &p));
    return p;
}
// commits `polys` and writes the points to the transcript, in order
static void commit_write(Transcript& tr, const std::vector<zk_poly>& polys, int basis) {
    std::vector<G1Affine> pts(polys.size());
    CHECK(zk_commit_batch(ctx, polys.data(), polys.size(), basis, reinterpret_cast<uint64_t*>(pts.data())));
    for (const G1Affine& p : pts)
        if (!tr.write_point(p)) {
            fprintf(stderr, "%s: a commitment is the identity\n", prog);
            exit(1);
        }
}
static bool parse_seed(const char* hex, uint8_t seed[32]) {
    if (strlen(hex) != 64) return false;
    for (int i = 0; i < 32; i++) {
        unsigned v;
        if (sscanf(hex + 2 * i, "%2x", &v) != 1) return false;
        seed[i] = (uint8_t)v;
    }
    return true;
}

// an opened value: polynomial (coefficient form, n coefficients), rotation, p(x w^rot)
struct Q {
    zk_poly poly;
    int rot;
    Fr eval;
};
// x w^r over the domain of 2^k rows
struct Rotations {
    Fr omega, omega_inv;
    explicit Rotations(uint32_t k) : omega(fr_omega(k)), omega_inv(fe_inv(fr_omega(k))) {}
    Fr operator()(const Fr& x, int r) const { return fe_mul(x, fe_pow_u64(r >= 0 ? omega : omega_inv, (uint64_t)(r >= 0 ? r : -r))); }
};

// the multi-open over `queries` (the prover's order) at x: its challenges are squeezed from `tr`, its commitments written to it
static void multi_open(Transcript& tr, const std::vector<Q>& queries, const Fr& x, size_t n, const Rotations& xrot, bool shplonk) {
    // ---- ProverGWC: one witness polynomial per distinct rotation
    if (!shplonk) {
        const Fr v = tr.squeeze();
        std::vector<std::pair<int, std::vector<Q>>> sets;
        for (const Q& q : queries) {
            bool found = false;
            for (auto& s : sets)
                if (s.first == q.rot) {
                    s.second.push_back(q);
                    found = true;
                    break;
                }
            if (!found) sets.push_back({q.rot, {q}});
        }
        std::vector<zk_poly> wit;
        for (auto& s : sets) {
            // (sum_i v^i p_i(X) - sum_i v^i e_i) / (X - x w^rot).  A polynomial opened twice in one set (none here) would appear twice.
            std::vector<zk_poly> in;
            std::vector<Fr> c;
            Fr pv = Fr::one(), eb = Fr::zero();
            for (const Q& q : s.second) {
                in.push_back(q.poly);
                c.push_back(pv);
                eb = fe_add(eb, fe_mul(pv, q.eval));
                pv = fe_mul(pv, v);
            }
            zk_poly w = alloc(n);
            CHECK(zk_poly_lincomb(ctx, w, in.data(), reinterpret_cast<const uint64_t*>(c.data()), in.size(), limbs(eb), 1));
            const Fr pt = xrot(x, s.first);
            CHECK(zk_kate_division(ctx, w, limbs(pt), w));
            wit.push_back(w);
        }
        commit_write(tr, wit, ZK_BASIS_MONOMIAL);
    } else {
        // ---- 7'. multi-open (ProverSHPLONK): polynomials grouped by their set of rotations; h(X) = sum_i v^i (sum_j y^j (P_ij - R_ij)) / Z_i
        struct CR {
            zk_poly poly;
            std::vector<int> rots;
            std::vector<Fr> evals;
        };
        std::vector<CR> com;
        for (const Q& q : queries) {
            size_t at = com.size();
            for (size_t i = 0; i < com.size(); i++)
                if (com[i].poly == q.poly) at = i;
            if (at == com.size()) com.push_back(CR{q.poly, {}, {}});
            com[at].rots.push_back(q.rot);
            com[at].evals.push_back(q.eval);
        }
        auto canon_less = [&](int ra, int rb) {  // BTreeSet<Fr>: the points ordered by their canonical integer value
            const Fr a = fe_from_mont(xrot(x, ra)), b = fe_from_mont(xrot(x, rb));
            for (int i = 7; i >= 0; i--)
                if (a.v[i] != b.v[i]) return a.v[i] < b.v[i];
            return false;
        };
        struct RS {
            std::vector<int> rots;
            std::vector<size_t> coms;
        };
        std::vector<RS> rsets;
        std::vector<int> all_rots;
        for (size_t ci = 0; ci < com.size(); ci++) {
            CR& cr = com[ci];
            std::vector<size_t> order(cr.rots.size());
            for (size_t i = 0; i < order.size(); i++) order[i] = i;
            std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return canon_less(cr.rots[a], cr.rots[b]); });
            std::vector<int> r2;
            std::vector<Fr> e2;
            for (size_t i : order) {
                r2.push_back(cr.rots[i]);
                e2.push_back(cr.evals[i]);
            }
            cr.rots = r2;
            cr.evals = e2;
            for (int r : cr.rots)
                if (std::find(all_rots.begin(), all_rots.end(), r) == all_rots.end()) all_rots.push_back(r);
            size_t hit = rsets.size();
            for (size_t si = 0; si < rsets.size(); si++)
                if (rsets[si].rots == cr.rots) hit = si;
            if (hit == rsets.size()) rsets.push_back(RS{cr.rots, {}});
            rsets[hit].coms.push_back(ci);
        }
        std::sort(all_rots.begin(), all_rots.end(), canon_less);
        const Fr yc = tr.squeeze(), v = tr.squeeze();
        // the Lagrange basis over a set's points as coefficient vectors, one inversion for all denominators (lagrange_interpolate)
        auto lagrange_basis = [&](const std::vector<Fr>& pts) {
            const size_t m = pts.size();
            std::vector<std::vector<Fr>> basis(m);
            std::vector<Fr> den(m, Fr::one());
            for (size_t j = 0; j < m; j++) {
                std::vector<Fr> num(1, Fr::one());
                for (size_t i = 0; i < m; i++) {
                    if (i == j) continue;
                    std::vector<Fr> nn(num.size() + 1, Fr::zero());
                    for (size_t t = 0; t < num.size(); t++) {
                        nn[t + 1] = fe_add(nn[t + 1], num[t]);
                        nn[t] = fe_sub(nn[t], fe_mul(pts[i], num[t]));
                    }
                    num.swap(nn);
                    den[j] = fe_mul(den[j], fe_sub(pts[j], pts[i]));
                }
                basis[j] = num;
            }
            for (size_t j = 0; j < m; j++) {
                const Fr dj = fe_inv(den[j]);
                for (Fr& cf : basis[j]) cf = fe_mul(cf, dj);
            }
            return basis;
        };
        std::vector<std::vector<Fr>> low(com.size());  // every polynomial's remainder over its set's points
        std::vector<zk_poly> sbuf;
        for (RS& rs : rsets) {
            std::vector<Fr> pts;
            for (int r : rs.rots) pts.push_back(xrot(x, r));
            const std::vector<std::vector<Fr>> basis = lagrange_basis(pts);
            std::vector<zk_poly> in;
            std::vector<Fr> c, rsum(pts.size(), Fr::zero());
            Fr py = Fr::one();
            for (size_t ci : rs.coms) {
                std::vector<Fr>& lo = low[ci];
                lo.assign(pts.size(), Fr::zero());
                for (size_t j = 0; j < pts.size(); j++)
                    for (size_t t = 0; t < pts.size(); t++) lo[t] = fe_add(lo[t], fe_mul(basis[j][t], com[ci].evals[j]));
                in.push_back(com[ci].poly);
                c.push_back(py);
                for (size_t t = 0; t < pts.size(); t++) rsum[t] = fe_add(rsum[t], fe_mul(py, lo[t]));
                py = fe_mul(py, yc);
            }
            zk_poly sb = alloc(n);
            CHECK(zk_poly_lincomb(ctx, sb, in.data(), reinterpret_cast<const uint64_t*>(c.data()), in.size(),
                                  reinterpret_cast<const uint64_t*>(rsum.data()), rsum.size()));
            for (const Fr& pt : pts) CHECK(zk_kate_division(ctx, sb, limbs(pt), sb));  // exact: the numerator vanishes on the set
            sbuf.push_back(sb);
        }
        zk_poly hx = alloc(n);
        {
            std::vector<Fr> c;
            Fr pv = Fr::one();
            for (size_t si = 0; si < rsets.size(); si++) {
                c.push_back(pv);
                pv = fe_mul(pv, v);
            }
            CHECK(zk_poly_lincomb(ctx, hx, sbuf.data(), reinterpret_cast<const uint64_t*>(c.data()), sbuf.size(), nullptr, 0));
        }
        commit_write(tr, {hx}, ZK_BASIS_MONOMIAL);
        const Fr u = tr.squeeze();
        // L(X) = sum_i v^i z_i(u) sum_j y^j (P_ij(X) - R_ij(u)) - Z_T(u) h(X);  the proof's last point commits to L(X) / ((X - u) z_0(u))
        auto vanishing_eval = [&](const std::vector<Fr>& pts, const Fr& at) {
            Fr acc = Fr::one();
            for (const Fr& p : pts) acc = fe_mul(acc, fe_sub(at, p));
            return acc;
        };
        std::vector<zk_poly> in;
        std::vector<Fr> c, z_diffs;
        Fr sub = Fr::zero(), pv = Fr::one();
        for (RS& rs : rsets) {
            std::vector<Fr> diffs;
            for (int r : all_rots)
                if (std::find(rs.rots.begin(), rs.rots.end(), r) == rs.rots.end()) diffs.push_back(xrot(x, r));
            const Fr zi = vanishing_eval(diffs, u);
            z_diffs.push_back(zi);
            Fr py = Fr::one();
            for (size_t ci : rs.coms) {
                const Fr coef = fe_mul(fe_mul(pv, zi), py);
                in.push_back(com[ci].poly);
                c.push_back(coef);
                Fr ru = Fr::zero();  // R_ij(u)
                for (size_t t = low[ci].size(); t-- > 0;) ru = fe_add(fe_mul(ru, u), low[ci][t]);
                sub = fe_add(sub, fe_mul(coef, ru));
                py = fe_mul(py, yc);
            }
            pv = fe_mul(pv, v);
        }
        std::vector<Fr> all_pts;
        for (int r : all_rots) all_pts.push_back(xrot(x, r));
        in.push_back(hx);
        c.push_back(fe_neg(vanishing_eval(all_pts, u)));
        zk_poly lx = alloc(n), fin = alloc(n);
        CHECK(zk_poly_lincomb(ctx, lx, in.data(), reinterpret_cast<const uint64_t*>(c.data()), in.size(), limbs(sub), 1));
        CHECK(zk_kate_division(ctx, lx, limbs(u), lx));
        const Fr zinv = fe_inv(z_diffs[0]);
        CHECK(zk_poly_lincomb(ctx, fin, &lx, limbs(zinv), 1, nullptr, 0));
        commit_write(tr, {fin}, ZK_BASIS_MONOMIAL);
    }
}
