// verifier.h — the host half of plonk::verify_proof for the circuit family of this engine (zk_verify / zk_verify_batch).
//
// Restates halo2_proofs' verifier (plonk/verifier.rs, the permutation / lookup / vanishing verifiers, KZG multi-open
// `poly/kzg/multiopen/{gwc,shplonk}/verifier.rs`) the way the repository's pinned verifier does: the proof is read in the
// prover's order, the challenges are squeezed from the same transcripts (transcript.h), the expected quotient value is the
// y-Horner of the gate, permutation and lookup expressions at x divided by x^n - 1, and the multi-open reduces everything
// to one KZG check e(A, [s]G2) = e(B, G2).  What leaves this file is that check as two lists of (scalar, base) terms — the
// bases are the proof's points, the key's commitments and g[0] — which the device sums (verify.hip).  A proof that fails
// before that point (non-canonical scalar, a zero where the verifier divides) is rejected here.
//
// Proof points are decoded before this runs (they depend on the bytes only): `pts` holds them in transcript order, affine
// Montgomery, already checked (canonical, on the curve, not the identity).  Host code only: it compiles without a device.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "pk.h"
#include "transcript.h"

namespace zk {
namespace verifier {

struct Term {
    Fr s;           // Montgomery
    uint32_t base;  // [0, n_points): the proof's points; then fixed commitments, permutation commitments, g[0] (ProofLayout)
};

// where everything sits in a proof of one key / transcript / scheme
struct ProofLayout {
    bool evm = false, shplonk = false;
    uint32_t nc = 1;                   // circuits the proof covers (zk_verify_multi; 1: a proof of zk_prove)
    size_t point_size = 0, len = 0;
    std::vector<uint32_t> point_off;   // byte offset of each point, transcript order
    uint32_t n_points = 0;             // = point_off.size()
    uint32_t n_fix = 0, n_perm = 0;
    uint32_t base_fix() const { return n_points; }
    uint32_t base_perm() const { return n_points + n_fix; }
    uint32_t base_g0() const { return n_points + n_fix + n_perm; }
    uint32_t n_bases() const { return base_g0() + 1; }
};

// one opened value: commitment (a base index, or H for the quotient pieces combined with powers of x^n), rotation, eval index
static constexpr uint32_t KEY_H = 0xffffffffu;
struct Query {
    uint32_t key;
    int rot;
    uint32_t eval;
};

// One proof over nc circuits of one key [RECALLED: halo2's create_proof / verify_proof over `circuits: &[C]`; restated by
// tests/halo2_ref.py]: every per-circuit group of a phase is written for circuit 0, then circuit 1, ...; what belongs to the key
// or to the proof (fixed / sigma evaluations, random polynomial, h pieces, the opening) is written once.  The per-circuit
// groups below hold circuit 0's index; circuit c's is that plus c times the group's stride (`*_of`).  nc = 1: a proof of zk_prove.
// point indices in transcript order
struct PointIdx {
    uint32_t adv, lk_perm, perm_z, lk_z, random, h, opening;
    uint32_t s_adv, s_lk_perm, s_perm_z, s_lk_z;  // strides per circuit
    uint32_t adv_of(uint32_t c) const { return adv + c * s_adv; }
    uint32_t lk_perm_of(uint32_t c) const { return lk_perm + c * s_lk_perm; }
    uint32_t perm_z_of(uint32_t c) const { return perm_z + c * s_perm_z; }
    uint32_t lk_z_of(uint32_t c) const { return lk_z + c * s_lk_z; }
};
inline PointIdx point_idx(const Layout& lay, uint32_t nc = 1) {
    PointIdx p;
    p.s_adv = lay.n_adv;
    p.s_lk_perm = 2 * lay.n_lookups;              // (a', s') per lookup
    p.s_perm_z = lay.n_chunks;
    p.s_lk_z = lay.n_lookups;
    p.adv = 0;
    p.lk_perm = nc * p.s_adv;
    p.perm_z = p.lk_perm + nc * p.s_lk_perm;
    p.lk_z = p.perm_z + nc * p.s_perm_z;
    p.random = p.lk_z + nc * p.s_lk_z;
    p.h = p.random + 1;
    p.opening = p.h + lay.n_h;
    return p;
}
// scalar indices (evaluations) in transcript order
struct EvalIdx {
    uint32_t adv, fix, random, sigma, perm, lookup, count;
    uint32_t s_adv, s_perm, s_lookup;  // strides per circuit
    uint32_t adv_of(uint32_t c) const { return adv + c * s_adv; }
    uint32_t perm_of(uint32_t c) const { return perm + c * s_perm; }
    uint32_t lookup_of(uint32_t c) const { return lookup + c * s_lookup; }
};
inline EvalIdx eval_idx(const Layout& lay, uint32_t nc = 1) {
    EvalIdx e;
    e.s_adv = (uint32_t)lay.advice_queries.size();
    e.s_perm = 3 * lay.n_chunks - 1;  // (z, z_next, z_last) per chunk, the last chunk without z_last
    e.s_lookup = 5 * lay.n_lookups;
    e.adv = 0;
    e.fix = nc * e.s_adv;
    e.random = e.fix + lay.n_fix;
    e.sigma = e.random + 1;
    e.perm = e.sigma + (uint32_t)lay.perm_cols.size();
    e.lookup = e.perm + nc * e.s_perm;
    e.count = e.lookup + nc * e.s_lookup;
    return e;
}

// the verifier's queries in halo2's order (the pinned verifier's build_queries, then h and the random polynomial)
inline std::vector<Query> build_queries(const Layout& lay, const ProofLayout& pl) {
    const uint32_t nc = pl.nc;
    const PointIdx P = point_idx(lay, nc);
    const EvalIdx E = eval_idx(lay, nc);
    std::vector<Query> q;
    for (uint32_t c = 0; c < nc; c++) {  // every circuit's own openings, circuit by circuit; then what the circuits share
        for (uint32_t i = 0; i < lay.advice_queries.size(); i++)
            q.push_back({P.adv_of(c) + lay.advice_queries[i].first, lay.advice_queries[i].second, E.adv_of(c) + i});
        for (uint32_t i = 0; i < lay.n_chunks; i++) {
            q.push_back({P.perm_z_of(c) + i, 0, E.perm_of(c) + 3 * i});
            q.push_back({P.perm_z_of(c) + i, 1, E.perm_of(c) + 3 * i + 1});
        }
        for (int i = (int)lay.n_chunks - 2; i >= 0; i--) q.push_back({P.perm_z_of(c) + i, lay.last_rot, E.perm_of(c) + 3 * i + 2});
        for (uint32_t l = 0; l < lay.n_lookups; l++) {
            const uint32_t e = E.lookup_of(c) + 5 * l;  // z, z_next, a', a'(w^-1 x), s'
            q.push_back({P.lk_z_of(c) + l, 0, e});
            q.push_back({P.lk_perm_of(c) + 2 * l, 0, e + 2});
            q.push_back({P.lk_perm_of(c) + 2 * l + 1, 0, e + 4});
            q.push_back({P.lk_perm_of(c) + 2 * l, -1, e + 3});
            q.push_back({P.lk_z_of(c) + l, 1, e + 1});
        }
    }
    for (uint32_t f = 0; f < lay.n_fix; f++) q.push_back({pl.base_fix() + f, 0, E.fix + f});
    for (uint32_t i = 0; i < lay.perm_cols.size(); i++) q.push_back({pl.base_perm() + i, 0, E.sigma + i});
    q.push_back({KEY_H, 0, E.count});  // the expected h(x): an extra value, appended to the evaluations
    q.push_back({P.random, 0, E.random});
    return q;
}

// GWC: the distinct rotations in order of first appearance
inline std::vector<int> gwc_rotations(const std::vector<Query>& qs) {
    std::vector<int> rots;
    for (const Query& q : qs)
        if (std::find(rots.begin(), rots.end(), q.rot) == rots.end()) rots.push_back(q.rot);
    return rots;
}

// SHPLONK: the commitments by rotation set.  Commitments with their rotations in order of first appearance; the sets (each sorted)
// in order of first appearance, each with its commitments in that order; all_rots: the distinct rotations by first appearance
struct RSet {
    std::vector<int> rots;  // sorted
    std::vector<uint32_t> keys;
};
inline std::vector<RSet> shplonk_sets(const std::vector<Query>& qs, std::vector<int>* all_rots) {
    struct ComRots {
        uint32_t key;
        std::vector<int> rots;
    };
    std::vector<ComRots> cr;
    all_rots->clear();
    for (const Query& q : qs) {
        if (std::find(all_rots->begin(), all_rots->end(), q.rot) == all_rots->end()) all_rots->push_back(q.rot);
        auto it = std::find_if(cr.begin(), cr.end(), [&](const ComRots& c2) { return c2.key == q.key; });
        if (it == cr.end()) cr.push_back({q.key, {q.rot}});
        else if (std::find(it->rots.begin(), it->rots.end(), q.rot) == it->rots.end()) it->rots.push_back(q.rot);
    }
    std::vector<RSet> rs;
    for (ComRots& c2 : cr) {
        std::sort(c2.rots.begin(), c2.rots.end());
        auto it = std::find_if(rs.begin(), rs.end(), [&](const RSet& r) { return r.rots == c2.rots; });
        if (it == rs.end()) rs.push_back({c2.rots, {c2.key}});
        else it->keys.push_back(c2.key);
    }
    return rs;
}

inline ProofLayout proof_layout(const Layout& lay, bool evm, bool shplonk, uint32_t nc = 1) {
    ProofLayout pl;
    pl.nc = nc;
    pl.evm = evm;
    pl.shplonk = shplonk;
    pl.point_size = evm ? 64 : 32;
    pl.n_fix = lay.n_fix;
    pl.n_perm = (uint32_t)lay.perm_cols.size();
    const PointIdx P = point_idx(lay, nc);
    const EvalIdx E = eval_idx(lay, nc);
    size_t off = 0;
    auto pts = [&](uint32_t n) {
        for (uint32_t i = 0; i < n; i++) {
            pl.point_off.push_back((uint32_t)off);
            off += pl.point_size;
        }
    };
    pts(P.opening);  // every commitment before the evaluations
    off += 32 * (size_t)E.count;
    pl.n_points = P.opening;  // (provisional: the opening points follow)
    if (shplonk) {
        pts(2);
    } else {
        ProofLayout tmp = pl;
        pts((uint32_t)gwc_rotations(build_queries(lay, tmp)).size());
    }
    pl.n_points = (uint32_t)pl.point_off.size();
    pl.len = off;
    return pl;
}

inline bool fr_read(const uint8_t* b, bool big_endian, Fr* out_mont) {
    const Fr c = fe_from_bytes<FrParams>(b, big_endian);
    if (!c.below_modulus()) return false;  // r itself is refused with everything above it
    *out_mont = fe_to_mont(c);
    return true;
}

inline Fr fr_delta_host() { return fe_pow_u64(fr_from_u64(7), 1ull << 28); }  // 7^(2^28), the permutation coset generator

struct Challenges {
    Fr theta, beta, gamma, y, x, v, u, shplonk_y;
};

struct Prepared {
    std::vector<Term> a, b;
    Challenges ch;
};

// a product of terms that shares bases: one term per base (zero scalars kept out)
inline void merge_terms(std::vector<Term>& t) {
    std::stable_sort(t.begin(), t.end(), [](const Term& x, const Term& y) { return x.base < y.base; });
    std::vector<Term> out;
    for (const Term& x : t) {
        if (!out.empty() && out.back().base == x.base) out.back().s = fe_add(out.back().s, x.s);
        else out.push_back(x);
    }
    t.clear();
    for (const Term& x : out)
        if (!x.s.is_zero()) t.push_back(x);
}

// inst(x) = sum_i v_i l_i(x), l_i(x) = w^i (x^n - 1) / (n (x - w^i)): the instance column's evaluation, which no proof carries
// (halo2 with KZG: QUERY_INSTANCE = false).  One batch inversion; false: x is one of the w^i
inline bool instance_eval(const Layout& lay, const Fr* inst, size_t n_inst, const Fr& x, const Fr& xn1_over_n, Fr* out) {
    *out = Fr::zero();
    if (!n_inst) return true;
    const Fr w = fr_omega(lay.k);
    std::vector<Fr> den(n_inst), inv(n_inst), wi(n_inst);
    Fr cur = Fr::one();
    for (size_t i = 0; i < n_inst; i++) {
        wi[i] = cur;
        den[i] = fe_sub(x, cur);
        cur = fe_mul(cur, w);
    }
    if (!fr_batch_invert(den.data(), inv.data(), (uint32_t)n_inst)) return false;
    Fr acc = Fr::zero();
    for (size_t i = 0; i < n_inst; i++) acc = fe_add(acc, fe_mul(inst[i], fe_mul(wi[i], inv[i])));
    *out = fe_mul(acc, xn1_over_n);
    return true;
}

// the instance lists of one proof (Montgomery values, each at most lay.usable: the caller's check).  ONE list per circuit, in
// circuit order (pl.nc of them) — or exactly one list for the whole proof, the form the single-list prepare() at the end of this file passes on.  All
// of them are absorbed behind transcript_repr in list order, before any commitment (neither their number nor their lengths are
// hashed); circuit c's permutation terms use the evaluation of list c (of the one list, where there is one)
struct InstanceList {
    const Fr* vals;
    size_t n;
};
// inst(x) of every list computed elsewhere (zk_instance_eval's kernel, verify.hip): x[i] of list i, and on_domain[i] != 0 where x is
// one of that list's w^j — the case in which instance_eval returns false, and so does prepare
struct InstanceEvals {
    const Fr* x;
    const uint8_t* on_domain;
};

// the transcript of a proof from its first word to the challenge x (the points' bytes only: no evaluation is read)
inline void absorb_to_x(const Layout& lay, const Fr& transcript_repr, uint32_t nc, const G1Affine* pts, const InstanceList* lists, size_t n_lists,
                        Transcript* tr, Challenges* ch, uint32_t* np_out) {
    tr->common_scalar(transcript_repr);
    for (size_t l = 0; l < n_lists; l++)
        for (size_t i = 0; i < lists[l].n; i++) tr->common_scalar(lists[l].vals[i]);  // (the counts are not hashed)
    uint32_t np = 0;
    auto absorb_points = [&](uint32_t n) {
        for (uint32_t i = 0; i < n; i++) tr->common_point(pts[np++]);
    };
    absorb_points(nc * lay.n_adv);
    ch->theta = tr->squeeze();
    absorb_points(nc * 2 * lay.n_lookups);
    ch->beta = tr->squeeze();
    ch->gamma = tr->squeeze();
    absorb_points(nc * (lay.n_chunks + lay.n_lookups) + 1);
    ch->y = tr->squeeze();
    absorb_points(lay.n_h);
    ch->x = tr->squeeze();
    *np_out = np;
}
// the challenge x of a proof alone: what a caller needs to have inst(x) computed elsewhere before it calls prepare_lists()
inline Fr challenge_x(const Layout& lay, const Fr& transcript_repr, const ProofLayout& pl, const G1Affine* pts, const InstanceList* lists,
                      size_t n_lists) {
    EvmTranscript evm;
    Blake2bTranscript b2;
    Challenges ch;
    uint32_t np;
    absorb_to_x(lay, transcript_repr, pl.nc, pts, lists, n_lists, pl.evm ? (Transcript*)&evm : (Transcript*)&b2, &ch, &np);
    return ch.x;
}

// false: the proof is rejected before the pairing (non-canonical scalar, an inverse of zero).  Otherwise `out` holds the two
// term lists of the KZG check.  proof.len == pl.len is the caller's check.  lists / n_lists: see InstanceList (n_lists is 0, 1 or
// pl.nc).  given: the lists' inst(x) from elsewhere (n_lists of them), or null: computed here by instance_eval — the same term lists
inline bool prepare_lists(const Layout& lay, const Fr& transcript_repr, const ProofLayout& pl, const uint8_t* proof, const G1Affine* pts,
                          Prepared* out, const InstanceList* lists, size_t n_lists, const InstanceEvals* given = nullptr) {
    if (n_lists > 1 && n_lists != pl.nc) return false;
    EvmTranscript evm;
    Blake2bTranscript b2;
    Transcript* tr = pl.evm ? (Transcript*)&evm : (Transcript*)&b2;
    const uint32_t nc = pl.nc;
    const PointIdx P = point_idx(lay, nc);
    const EvalIdx E = eval_idx(lay, nc);
    Challenges& ch = out->ch;
    uint32_t np = 0;
    absorb_to_x(lay, transcript_repr, nc, pts, lists, n_lists, tr, &ch, &np);
    std::vector<Fr> ev(E.count + 1);
    const size_t ev_off = (size_t)P.opening * pl.point_size;
    for (uint32_t i = 0; i < E.count; i++) {
        if (!fr_read(proof + ev_off + 32 * (size_t)i, pl.evm, &ev[i])) return false;
        tr->common_scalar(ev[i]);
    }

    // ---- expected h(x) (the pinned verifier's expected_h_eval) ----
    const Fr one = Fr::one(), x = ch.x, y = ch.y, beta = ch.beta, gamma = ch.gamma;
    const Fr w = fr_omega(lay.k);
    Fr xn = x;
    for (uint32_t i = 0; i < lay.k; i++) xn = fe_sqr(xn);
    const Fr xn1 = fe_sub(xn, one);
    if (xn1.is_zero()) return false;
    const Fr c = fe_mul(xn1, fe_inv_fast(fr_from_u64(lay.n)));
    const Fr w_inv = fe_inv_fast(w);
    bool zero_div = false;
    auto L = [&](int i) {  // l_i(x) = w^i (x^n - 1) / (n (x - w^i)), i may be negative
        Fr wi = one;
        const Fr step = i >= 0 ? w : w_inv;
        for (int t = 0; t < (i >= 0 ? i : -i); t++) wi = fe_mul(wi, step);
        const Fr d = fe_sub(x, wi);
        if (d.is_zero()) zero_div = true;
        return fe_mul(fe_mul(wi, c), fe_inv_fast(d));
    };
    const Fr l0 = L(0), l_last = L(-(int)(BLINDING_FACTORS + 1));
    Fr l_blind = Fr::zero();
    for (int i = 1; i <= (int)BLINDING_FACTORS; i++) l_blind = fe_add(l_blind, L(-i));
    if (zero_div) return false;
    const Fr active = fe_sub(fe_sub(one, l_last), l_blind);
    std::vector<Fr> inst_xs(std::max<size_t>(n_lists, 1), Fr::zero());  // inst(x) per list
    if (lay.n_inst)
        for (size_t l = 0; l < n_lists; l++) {
            if (given) {
                if (given->on_domain[l]) return false;
                inst_xs[l] = given->x[l];
            } else if (!instance_eval(lay, lists[l].vals, lists[l].n, x, c, &inst_xs[l])) {
                return false;
            }
        }
    auto fix = [&](uint32_t f) { return ev[E.fix + f]; };
    const Fr delta = fr_delta_host();
    std::vector<Fr> exprs;  // the nc x T expressions of the y-Horner chain: circuit 0's, then circuit 1's, ...
    for (uint32_t circ = 0; circ < nc; circ++) {
        const Fr inst_x = inst_xs[n_lists > 1 ? circ : 0];
        auto adv = [&](uint32_t col, int rot) {
            for (uint32_t i = 0; i < lay.advice_queries.size(); i++)
                if (lay.advice_queries[i].first == col && lay.advice_queries[i].second == rot) return ev[E.adv_of(circ) + i];
            return Fr::zero();
        };
        for (uint32_t j = 0; j < lay.n_gate; j++) {
            const Fr a = adv(j, 0), b = adv(j, 1), cc = adv(j, 2), d = adv(j, 3);
            const uint32_t col = lay.gate_sel[j] & 0xffffffu, form = lay.gate_sel[j] >> 24;
            const Fr q = fix(col);
            Fr sel = q;
            if (form) sel = fe_mul(q, fe_sub(fr_from_u64(form == 1 ? 2 : 1), q));
            exprs.push_back(fe_mul(sel, fe_sub(fe_add(a, fe_mul(b, cc)), d)));
        }
        auto col_eval = [&](const Col& col) { return col.type == COL_FIXED ? fix(col.idx) : col.type == COL_INSTANCE ? inst_x : adv(col.idx, 0); };
        auto pe = [&](uint32_t i, uint32_t which) { return ev[E.perm_of(circ) + 3 * i + which]; };
        exprs.push_back(fe_mul(l0, fe_sub(one, pe(0, 0))));
        const Fr zl = pe(lay.n_chunks - 1, 0);
        exprs.push_back(fe_mul(l_last, fe_sub(fe_sqr(zl), zl)));
        for (uint32_t i = 1; i < lay.n_chunks; i++) exprs.push_back(fe_mul(l0, fe_sub(pe(i, 0), pe(i - 1, 2))));
        Fr cur_base = fe_mul(beta, x);  // beta x delta^(i chunk_len)
        for (uint32_t i = 0; i < lay.n_chunks; i++) {
            const uint32_t lo = i * lay.chunk_len, hi = std::min<uint32_t>(lo + lay.chunk_len, (uint32_t)lay.perm_cols.size());
            Fr left = pe(i, 1), right = pe(i, 0), cur = cur_base;
            for (uint32_t t = lo; t < hi; t++) {
                const Fr ce = col_eval(lay.perm_cols[t]);
                left = fe_mul(left, fe_add(fe_add(ce, fe_mul(beta, ev[E.sigma + t])), gamma));
                right = fe_mul(right, fe_add(fe_add(ce, cur), gamma));
                cur = fe_mul(cur, delta);
            }
            cur_base = cur;
            exprs.push_back(fe_mul(active, fe_sub(left, right)));
        }
        for (uint32_t l = 0; l < lay.n_lookups; l++) {
            const Fr* le = &ev[E.lookup_of(circ) + 5 * l];
            const Fr z = le[0], zn = le[1], ap = le[2], ap_inv = le[3], sp = le[4];
            const Fr inp = lay.single ? fe_mul(fix(lay.fx_qlookup), adv(0, 0)) : adv(lay.n_gate + l, 0);
            const Fr tab = fix(lay.fx_table);
            exprs.push_back(fe_mul(l0, fe_sub(one, z)));
            exprs.push_back(fe_mul(l_last, fe_sub(fe_sqr(z), z)));
            const Fr left = fe_mul(fe_mul(zn, fe_add(ap, beta)), fe_add(sp, gamma));
            const Fr right = fe_mul(fe_mul(z, fe_add(inp, beta)), fe_add(tab, gamma));
            exprs.push_back(fe_mul(active, fe_sub(left, right)));
            exprs.push_back(fe_mul(l0, fe_sub(ap, sp)));
            exprs.push_back(fe_mul(fe_mul(active, fe_sub(ap, sp)), fe_sub(ap, ap_inv)));
        }
    }
    Fr acc = Fr::zero();
    for (const Fr& e : exprs) acc = fe_add(fe_mul(acc, y), e);
    ev[E.count] = fe_mul(acc, fe_inv_fast(xn1));  // expected h(x)

    // ---- multi-open ----
    const std::vector<Query> qs = build_queries(lay, pl);
    std::vector<Fr> xn_pow(lay.n_h);
    xn_pow[0] = one;
    for (uint32_t i = 1; i < lay.n_h; i++) xn_pow[i] = fe_mul(xn_pow[i - 1], xn);
    auto point_of = [&](int rot) {  // x w^rot
        Fr r = x;
        const Fr step = rot >= 0 ? w : w_inv;
        for (int t = 0; t < (rot >= 0 ? rot : -rot); t++) r = fe_mul(r, step);
        return r;
    };
    auto commit = [&](std::vector<Term>& dst, uint32_t key, const Fr& s) {  // s * commitment(key)
        if (key == KEY_H) {
            for (uint32_t i = 0; i < lay.n_h; i++) dst.push_back({fe_mul(s, xn_pow[i]), P.h + i});
        } else {
            dst.push_back({s, key});
        }
    };
    std::vector<Term>& A = out->a;
    std::vector<Term>& B = out->b;
    A.clear();
    B.clear();
    if (!pl.shplonk) {
        ch.v = tr->squeeze();
        const std::vector<int> rots = gwc_rotations(qs);
        for (uint32_t i = 0; i < rots.size(); i++) tr->common_point(pts[np + i]);
        ch.u = tr->squeeze();
        Fr pu = one, eval_multi = Fr::zero();
        for (uint32_t si = 0; si < rots.size(); si++) {
            const Fr z = point_of(rots[si]);
            Fr pv = one, eb = Fr::zero();
            for (const Query& q : qs) {
                if (q.rot != rots[si]) continue;
                commit(B, q.key, fe_mul(pu, pv));
                eb = fe_add(eb, fe_mul(pv, ev[q.eval]));
                pv = fe_mul(pv, ch.v);
            }
            eval_multi = fe_add(eval_multi, fe_mul(pu, eb));
            B.push_back({fe_mul(pu, z), np + si});
            A.push_back({pu, np + si});
            pu = fe_mul(pu, ch.u);
        }
        B.push_back({fe_neg(eval_multi), pl.base_g0()});
    } else {
        std::vector<int> all_rots;
        const std::vector<RSet> rs = shplonk_sets(qs, &all_rots);
        auto eval_of = [&](uint32_t key, int rot) {
            Fr e = Fr::zero();
            for (const Query& q : qs)
                if (q.key == key && q.rot == rot) e = ev[q.eval];
            return e;
        };
        ch.shplonk_y = tr->squeeze();
        ch.v = tr->squeeze();
        tr->common_point(pts[np]);
        ch.u = tr->squeeze();
        tr->common_point(pts[np + 1]);
        const Fr u = ch.u;
        Fr r_outer = Fr::zero(), z0 = one, z0_diff_inv = one, pv = one;
        for (uint32_t i = 0; i < rs.size(); i++) {
            std::vector<Fr> pts_i;
            for (int r : rs[i].rots) pts_i.push_back(point_of(r));
            Fr zd = one;
            for (int r : all_rots)
                if (std::find(rs[i].rots.begin(), rs[i].rots.end(), r) == rs[i].rots.end()) zd = fe_mul(zd, fe_sub(u, point_of(r)));
            if (i == 0) {
                z0 = one;
                for (const Fr& p : pts_i) z0 = fe_mul(z0, fe_sub(u, p));
                if (zd.is_zero()) return false;
                z0_diff_inv = fe_inv_fast(zd);
                zd = one;
            } else {
                zd = fe_mul(zd, z0_diff_inv);
            }
            // Lagrange interpolation through (pts_i, evals) evaluated at u
            const size_t m = pts_i.size();
            std::vector<Fr> basis(m);
            for (size_t j = 0; j < m; j++) {
                Fr num = one, den = one;
                for (size_t t = 0; t < m; t++) {
                    if (t == j) continue;
                    num = fe_mul(num, fe_sub(u, pts_i[t]));
                    den = fe_mul(den, fe_sub(pts_i[j], pts_i[t]));
                }
                if (den.is_zero()) return false;
                basis[j] = fe_mul(num, fe_inv_fast(den));
            }
            Fr py = one, r_inner = Fr::zero();
            for (uint32_t key : rs[i].keys) {
                Fr rx = Fr::zero();
                for (size_t j = 0; j < m; j++) rx = fe_add(rx, fe_mul(eval_of(key, rs[i].rots[j]), basis[j]));
                r_inner = fe_add(r_inner, fe_mul(py, rx));
                commit(B, key, fe_mul(fe_mul(py, pv), zd));
                py = fe_mul(py, ch.shplonk_y);
            }
            r_outer = fe_add(r_outer, fe_mul(fe_mul(pv, r_inner), zd));
            pv = fe_mul(pv, ch.v);
        }
        B.push_back({fe_neg(r_outer), pl.base_g0()});
        B.push_back({fe_neg(z0), np});
        B.push_back({u, np + 1});
        A.push_back({one, np + 1});
    }
    merge_terms(A);
    merge_terms(B);
    return true;
}

// the single-list form: one list for the whole proof (zk_verify_public; no list: the forms without instances)
inline bool prepare(const Layout& lay, const Fr& transcript_repr, const ProofLayout& pl, const uint8_t* proof, const G1Affine* pts,
                    Prepared* out, const Fr* inst = nullptr, size_t n_inst = 0) {
    const InstanceList one{inst, n_inst};
    return prepare_lists(lay, transcript_repr, pl, proof, pts, out, &one, lay.n_inst ? (size_t)1 : (n_inst ? (size_t)1 : (size_t)0));
}

}  // namespace verifier
}  // namespace zk
