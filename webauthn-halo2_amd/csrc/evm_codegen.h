// evm_codegen.h — the EVM verifier of one kind of proof, as the text of a Yul program (zk_evm_verifier).
//
// A further rendering of the verifier's rule (csrc/verifier.h prepare_lists; tests/halo2_ref.py verify and the pinned oracle's
// verifier restate it in Python): the same steps in the same order, but every field operation is EMITTED as text instead of
// performed.  The kind is one key (shape, commitments, transcript_repr), one SRS (g2, s_g2), a circuit count N, an instance count
// m_c per circuit and a multi-open scheme; the transcript is the EVM one.  The proof layout, the query list and the rotation
// sets are verifier.h's.
//
// The program (DESIGN.md "The generated EVM verifier"):
//   calldata   all instances, circuit-major, 32-byte big-endian words; then the proof.  One exact length.
//   memory     [0, TB)   the transcript buffer while the challenges are squeezed (phase 1), the precompiles' input afterwards
//              [TB, top) one 32-byte slot per kept value: challenges, denominators, inverses, intermediate results
//   phase 1    reads every instance, point and evaluation once, checks it (scalar < r; coordinates < q, on the curve, not (0, 0))
//              and absorbs it; a challenge is keccak256 of the buffer mod r, and the hash is the next buffer's first word
//   phase 2    x^n, ONE batched inversion (precompile 5 once), l_0 / l_last / l_blind / l_i, inst_c(x), the y-Horner of every
//              circuit's terms, h(x); the multi-open's scalars per distinct point; one ecMul per point; one pairing
//   verdict    every failed check clears `success`; the program reverts at its end if it is clear
// Values live in memory, not in Yul variables: two variables (f_r, success) are alive outside the helper functions, so the
// text has no "stack too deep".  Host code only: no device memory, no HIP call, no environment.
#pragma once
#include <stdio.h>

#include <string>
#include <vector>

#include "pairing.h"
#include "verifier.h"

namespace zk {
namespace evmgen {

typedef zk_evm_cost evm_verifier_cost;

struct Desc {
    zk_circuit_params params;
    std::vector<G1Affine> fixed, perm;  // the key's commitments (affine Montgomery); the selector description is the shape's (Layout::gate_sel)
    Fr transcript_repr;                 // Montgomery
    G2A g2, s_g2;
    uint32_t n_circuits = 1;
    std::vector<uint32_t> n_instances;  // m_c per circuit (n_circuits of them)
    bool shplonk = false;
};

template <class F>
inline std::string hex_of(const F& mont) {  // canonical value as a 0x literal of 64 digits
    const F c = fe_from_mont(mont);
    char buf[80];
    char* p = buf;
    p += sprintf(p, "0x");
    for (int w = 7; w >= 0; w--) p += sprintf(p, "%08x", c.v[w]);
    return buf;
}
inline std::string hex_words(const uint32_t w[8], uint32_t minus = 0) {  // a modulus (minus a small number: no borrow beyond word 0)
    char buf[80];
    char* p = buf;
    p += sprintf(p, "0x");
    for (int i = 7; i >= 0; i--) p += sprintf(p, "%08x", i ? w[i] : w[0] - minus);
    return buf;
}
inline std::string addr(uint64_t a) {
    char buf[32];
    sprintf(buf, "0x%llx", (unsigned long long)a);
    return buf;
}

// a value of the program: the expression that yields it, how deep the expression nests, and what is known of it at generation
struct Val {
    std::string e;
    int depth = 0;
    int konst = 0;  // 0: unknown, 1: the constant 0, 2: the constant 1
};

class Emit {
   public:
    std::string out;
    uint32_t top = 0;  // the next free memory slot
    evm_verifier_cost cost{};

    void line(const std::string& s) { out += "            " + s + "\n"; }
    Val zero() const { return Val{"0", 0, 1}; }
    Val one() const { return Val{"1", 0, 2}; }
    Val lit(const Fr& mont) const {
        if (mont.is_zero()) return zero();
        if (mont == Fr::one()) return one();
        return Val{hex_of(mont), 0, 0};
    }
    Val at(uint32_t a) const { return Val{"mload(" + addr(a) + ")", 0, 0}; }
    uint32_t alloc() {
        const uint32_t a = top;
        top += 32;
        return a;
    }
    // the value in a slot of its own: what is used more than once, or nests too deep
    Val keep(const Val& v) {
        if (v.depth == 0) return v;
        const uint32_t a = alloc();
        line("mstore(" + addr(a) + ", " + v.e + ")");
        return at(a);
    }
    Val fin(const std::string& e, int depth) {
        Val v{e, depth, 0};
        return depth >= 3 ? keep(v) : v;
    }
    Val mul(const Val& a, const Val& b) {
        if (a.konst == 1 || b.konst == 1) return zero();
        if (a.konst == 2) return b;
        if (b.konst == 2) return a;
        return fin("mulmod(" + a.e + ", " + b.e + ", f_r)", std::max(a.depth, b.depth) + 1);
    }
    Val add(const Val& a, const Val& b) {
        if (a.konst == 1) return b;
        if (b.konst == 1) return a;
        return fin("addmod(" + a.e + ", " + b.e + ", f_r)", std::max(a.depth, b.depth) + 1);
    }
    Val neg(const Val& a) {
        if (a.konst == 1) return a;
        return fin("sub(f_r, " + a.e + ")", a.depth + 1);
    }
    Val sub(const Val& a, const Val& b) {
        if (b.konst == 1) return a;
        return fin("addmod(" + a.e + ", sub(f_r, " + b.e + "), f_r)", std::max(a.depth, b.depth) + 1);
    }
};

// a point of the final sums: where its coordinates come from
struct PointRef {
    std::string x, y;
};

struct SumTerm {
    uint32_t base;
    Val s;
};

// the program text and its static cost; false: the description is not one a key of this engine can have
inline bool generate(const Desc& d, std::string* text, evm_verifier_cost* cost_out) {
    using namespace verifier;
    Layout lay;
    if (!lay.init(d.params)) return false;
    const uint32_t nc = d.n_circuits;
    if (nc == 0 || d.n_instances.size() != nc || d.fixed.size() != lay.n_fix || d.perm.size() != lay.perm_cols.size()) return false;
    uint32_t total_inst = 0, max_inst = 0;
    for (uint32_t m : d.n_instances) {
        if (m > lay.usable || (m && !lay.n_inst)) return false;
        total_inst += m;
        max_inst = std::max(max_inst, m);
    }
    const ProofLayout pl = proof_layout(lay, true, d.shplonk, nc);
    const PointIdx P = point_idx(lay, nc);
    const EvalIdx E = eval_idx(lay, nc);
    const std::vector<Query> qs = build_queries(lay, pl);
    const std::vector<int> gwc_rots = gwc_rotations(qs);
    const uint32_t n_open = pl.n_points - P.opening;
    const uint32_t cd0 = 32 * total_inst;  // the proof's offset in the calldata
    const uint32_t cd_len = cd0 + (uint32_t)pl.len;
    const uint32_t cd_ev = cd0 + P.opening * 64;

    // the transcript buffer: the longest run between two challenges (and room for the pairing's input afterwards)
    uint32_t tb = 0x180;
    for (uint32_t run : {32 * total_inst + 64 * nc * lay.n_adv, 64 * nc * 2 * lay.n_lookups, 64 * (nc * (lay.n_chunks + lay.n_lookups) + 1),
                         64 * lay.n_h, 32 * E.count, 64 * n_open})
        tb = std::max(tb, 32 + run);

    Emit g;
    g.top = tb;
    g.cost.calldata_bytes = cd_len;
    const std::string Q = hex_words(FqParams::P), R = hex_words(FrParams::P);

    g.line("let f_r := " + R);
    g.line("let success := 1");
    // helpers: they see no outer variable, so the moduli are literals
    g.line("function sc(c, m) -> ok {");
    g.line("    let v := calldataload(c)");
    g.line("    mstore(m, v)");
    g.line("    ok := lt(v, " + R + ")");
    g.line("}");
    g.line("function pt(c, m) -> ok {");
    g.line("    let x := calldataload(c)");
    g.line("    let y := calldataload(add(c, 0x20))");
    g.line("    mstore(m, x)");
    g.line("    mstore(add(m, 0x20), y)");
    g.line("    ok := and(lt(x, " + Q + "), lt(y, " + Q + "))");
    g.line("    ok := and(ok, lt(0, add(x, y)))");
    g.line("    let xx := mulmod(x, x, " + Q + ")");
    g.line("    ok := and(ok, eq(mulmod(y, y, " + Q + "), addmod(mulmod(xx, x, " + Q + "), 3, " + Q + ")))");
    g.line("}");
    // the running sum of s * (x, y) lives at 0x00; the term is formed at 0x40
    g.line("function ec_first(x, y, s) -> ok {");
    g.line("    mstore(0x00, x)");
    g.line("    mstore(0x20, y)");
    g.line("    mstore(0x40, s)");
    g.line("    ok := staticcall(gas(), 7, 0x00, 0x60, 0x00, 0x40)");
    g.line("}");
    g.line("function ec_next(x, y, s) -> ok {");
    g.line("    mstore(0x40, x)");
    g.line("    mstore(0x60, y)");
    g.line("    mstore(0x80, s)");
    g.line("    ok := staticcall(gas(), 7, 0x40, 0x60, 0x40, 0x40)");
    g.line("    ok := and(ok, staticcall(gas(), 6, 0x00, 0x80, 0x00, 0x40))");
    g.line("}");
    g.line("function ec_plus(x, y) -> ok {");
    g.line("    mstore(0x40, x)");
    g.line("    mstore(0x60, y)");
    g.line("    ok := staticcall(gas(), 6, 0x00, 0x80, 0x00, 0x40)");
    g.line("}");

    // ---------------------------------------------------------------- phase 1: the transcript
    g.line("success := and(success, eq(calldatasize(), " + addr(cd_len) + "))");
    g.line("mstore(0x0, " + hex_of(d.transcript_repr) + ")");
    uint32_t off = 32, np = 0;
    auto absorb_scalar = [&](uint32_t cd) {
        g.line("success := and(success, sc(" + addr(cd) + ", " + addr(off) + "))");
        off += 32;
    };
    auto absorb_points = [&](uint32_t n) {
        for (uint32_t i = 0; i < n; i++, np++) {
            g.line("success := and(success, pt(" + addr(cd0 + pl.point_off[np]) + ", " + addr(off) + "))");
            off += 64;
        }
    };
    auto squeeze = [&](const char* name) {
        if (off == 32) {  // nothing absorbed since the last challenge: the hash and one byte 0x01
            g.line("mstore8(0x20, 1)");
            off = 33;
        }
        const uint32_t a = g.alloc();
        g.line(std::string("{  // ") + name);
        g.line("    let h := keccak256(0x0, " + addr(off) + ")");
        g.line("    mstore(" + addr(a) + ", mod(h, f_r))");
        g.line("    mstore(0x0, h)");
        g.line("}");
        g.cost.keccak_calls++;
        g.cost.keccak_bytes += off;
        off = 32;
        return g.at(a);
    };
    for (uint32_t i = 0; i < total_inst; i++) absorb_scalar(32 * i);
    absorb_points(nc * lay.n_adv);
    const Val theta = squeeze("theta");
    (void)theta;
    absorb_points(nc * 2 * lay.n_lookups);
    const Val beta = squeeze("beta");
    const Val gamma = squeeze("gamma");
    absorb_points(nc * (lay.n_chunks + lay.n_lookups) + 1);
    const Val y = squeeze("y");
    absorb_points(lay.n_h);
    const Val x = squeeze("x");
    for (uint32_t i = 0; i < E.count; i++) absorb_scalar(cd_ev + 32 * i);
    Val v, u, sy;
    if (!d.shplonk) {
        v = squeeze("v");
        absorb_points(n_open);
        u = squeeze("u");
    } else {
        sy = squeeze("y of the multi-open");
        v = squeeze("v");
        absorb_points(1);
        u = squeeze("u");
        absorb_points(1);  // (checked like every point; no challenge follows it)
    }

    // ---------------------------------------------------------------- phase 2: the identities
    std::vector<Val> ev(E.count + 1);
    for (uint32_t i = 0; i < E.count; i++) ev[i] = Val{"calldataload(" + addr(cd_ev + 32 * i) + ")", 0, 0};
    const Val one = g.one();
    const Fr w = fr_omega(lay.k), w_inv = fe_inv_fast(w);
    auto w_pow = [&](int i) {
        Fr r = Fr::one();
        const Fr step = i >= 0 ? w : w_inv;
        for (int t = 0; t < (i >= 0 ? i : -i); t++) r = fe_mul(r, step);
        return r;
    };
    g.line("// x^n, the denominators and their one batched inversion");
    Val xn = x;
    for (uint32_t i = 0; i < lay.k; i++) xn = g.keep(g.mul(xn, xn));
    const Val xn1 = g.keep(g.sub(xn, one));
    const Val c = g.keep(g.mul(xn1, g.lit(fe_inv_fast(fr_from_u64(lay.n)))));  // (x^n - 1) / n

    // the denominators: x - w^i for i = 0 .. max(m_c, 1) - 1, x - w^-j for j = 1 .. BLINDING_FACTORS + 1, x^n - 1; SHPLONK: x
    // (every Lagrange denominator of a rotation set is a constant times a power of x) and set 0's z_diff
    const uint32_t n_pos = std::max<uint32_t>(max_inst, 1), n_neg = BLINDING_FACTORS + 1;
    std::vector<Val> den;
    for (uint32_t i = 0; i < n_pos; i++) den.push_back(g.keep(g.sub(x, g.lit(w_pow((int)i)))));
    for (uint32_t j = 1; j <= n_neg; j++) den.push_back(g.keep(g.sub(x, g.lit(w_pow(-(int)j)))));
    const uint32_t i_xn1 = (uint32_t)den.size();
    den.push_back(xn1);
    std::vector<int> all_rots;
    std::vector<RSet> rs;
    std::vector<Val> u_minus;  // u - x w^rot, by all_rots
    uint32_t i_x = 0, i_zd0 = 0;
    auto u_minus_of = [&](int rot) { return u_minus[std::find(all_rots.begin(), all_rots.end(), rot) - all_rots.begin()]; };
    auto in_set = [](const RSet& s, int rot) { return std::find(s.rots.begin(), s.rots.end(), rot) != s.rots.end(); };
    if (d.shplonk) {
        rs = shplonk_sets(qs, &all_rots);
        for (int r : all_rots) u_minus.push_back(g.keep(g.sub(u, g.mul(x, g.lit(w_pow(r))))));
        Val zd0 = one;
        for (int r : all_rots)
            if (!in_set(rs[0], r)) zd0 = g.mul(zd0, u_minus_of(r));
        i_x = (uint32_t)den.size();
        den.push_back(x);
        i_zd0 = (uint32_t)den.size();
        den.push_back(g.keep(zd0));
    }
    std::vector<Val> inv(den.size());
    {
        std::vector<Val> pre(den.size());
        pre[0] = den[0];
        for (size_t i = 1; i < den.size(); i++) pre[i] = g.keep(g.mul(pre[i - 1], den[i]));
        g.line("mstore(0x00, 0x20)");
        g.line("mstore(0x20, 0x20)");
        g.line("mstore(0x40, 0x20)");
        g.line("mstore(0x60, " + pre.back().e + ")");
        g.line("mstore(0x80, " + hex_words(FrParams::P, 2) + ")");
        g.line("mstore(0xa0, f_r)");
        g.line("success := and(success, staticcall(gas(), 5, 0x00, 0xc0, 0x00, 0x20))");
        g.cost.modexp++;
        const uint32_t a = g.alloc();
        g.line("mstore(" + addr(a) + ", mload(0x00))");
        Val acc = g.at(a);
        g.line("success := and(success, eq(mulmod(" + pre.back().e + ", " + acc.e + ", f_r), 1))  // no denominator is zero");
        for (size_t i = den.size() - 1; i >= 1; i--) {
            inv[i] = g.keep(g.mul(acc, pre[i - 1]));
            acc = g.keep(g.mul(acc, den[i]));
        }
        inv[0] = acc;
    }
    g.line("// l_0, l_last, l_blind, the l_i of the instance rows");
    std::vector<Val> l_pos(n_pos);  // l_i(x) = w^i (x^n - 1) / (n (x - w^i))
    for (uint32_t i = 0; i < n_pos; i++) l_pos[i] = g.keep(g.mul(g.mul(g.lit(w_pow((int)i)), c), inv[i]));
    std::vector<Val> l_neg(n_neg + 1);
    for (uint32_t j = 1; j <= n_neg; j++) l_neg[j] = g.keep(g.mul(g.mul(g.lit(w_pow(-(int)j)), c), inv[n_pos + j - 1]));
    const Val l0 = l_pos[0], l_last = l_neg[n_neg];
    Val l_blind = g.zero();
    for (uint32_t j = 1; j <= BLINDING_FACTORS; j++) l_blind = g.add(l_blind, l_neg[j]);
    l_blind = g.keep(l_blind);
    const Val active = g.keep(g.sub(g.sub(one, l_last), l_blind));
    std::vector<Val> inst_xs(nc, g.zero());
    for (uint32_t circ = 0, first = 0; circ < nc; first += d.n_instances[circ], circ++) {
        Val acc = g.zero();
        for (uint32_t i = 0; i < d.n_instances[circ]; i++)
            acc = g.add(acc, g.mul(Val{"calldataload(" + addr(32 * (first + i)) + ")", 0, 0}, l_pos[i]));
        inst_xs[circ] = g.keep(acc);
    }

    auto fix = [&](uint32_t f) { return ev[E.fix + f]; };
    const Fr delta = fr_delta_host();
    const Val beta_x = g.keep(g.mul(beta, x));
    Val acc = g.zero();
    auto term = [&](const Val& e) { acc = g.keep(g.add(g.mul(acc, y), e)); };
    for (uint32_t circ = 0; circ < nc; circ++) {
        g.line("// circuit " + std::to_string(circ) + ": gates, permutation, lookups");
        const Val inst_x = inst_xs[circ];
        auto adv = [&](uint32_t col, int rot) {
            for (uint32_t i = 0; i < lay.advice_queries.size(); i++)
                if (lay.advice_queries[i].first == col && lay.advice_queries[i].second == rot) return ev[E.adv_of(circ) + i];
            return g.zero();
        };
        for (uint32_t j = 0; j < lay.n_gate; j++) {
            const uint32_t col = lay.gate_sel[j] & 0xffffffu, form = lay.gate_sel[j] >> 24;
            const Val q = fix(col);
            Val sel = q;
            if (form) sel = g.mul(q, g.sub(g.lit(fr_from_u64(form == 1 ? 2 : 1)), q));  // q (2 - q) / q (1 - q)
            term(g.mul(sel, g.sub(g.add(adv(j, 0), g.mul(adv(j, 1), adv(j, 2))), adv(j, 3))));
        }
        auto col_eval = [&](const Col& col) { return col.type == COL_FIXED ? fix(col.idx) : col.type == COL_INSTANCE ? inst_x : adv(col.idx, 0); };
        auto pe = [&](uint32_t i, uint32_t which) { return ev[E.perm_of(circ) + 3 * i + which]; };
        term(g.mul(l0, g.sub(one, pe(0, 0))));
        const Val zl = pe(lay.n_chunks - 1, 0);
        term(g.mul(l_last, g.sub(g.mul(zl, zl), zl)));
        for (uint32_t i = 1; i < lay.n_chunks; i++) term(g.mul(l0, g.sub(pe(i, 0), pe(i - 1, 2))));
        Fr dpow = Fr::one();  // delta^(columns so far)
        for (uint32_t i = 0; i < lay.n_chunks; i++) {
            const uint32_t lo = i * lay.chunk_len, hi = std::min<uint32_t>(lo + lay.chunk_len, (uint32_t)lay.perm_cols.size());
            Val left = pe(i, 1), right = pe(i, 0);
            for (uint32_t t = lo; t < hi; t++) {
                const Val ce = col_eval(lay.perm_cols[t]);
                left = g.keep(g.mul(left, g.add(g.add(ce, g.mul(beta, ev[E.sigma + t])), gamma)));
                right = g.keep(g.mul(right, g.add(g.add(ce, g.mul(beta_x, g.lit(dpow))), gamma)));
                dpow = fe_mul(dpow, delta);
            }
            term(g.mul(active, g.sub(left, right)));
        }
        for (uint32_t l = 0; l < lay.n_lookups; l++) {
            const Val* le = &ev[E.lookup_of(circ) + 5 * l];
            const Val z = le[0], zn = le[1], ap = le[2], ap_inv = le[3], sp = le[4];
            const Val inp = lay.single ? g.mul(fix(lay.fx_qlookup), adv(0, 0)) : adv(lay.n_gate + l, 0);
            const Val tab = fix(lay.fx_table);
            term(g.mul(l0, g.sub(one, z)));
            term(g.mul(l_last, g.sub(g.mul(z, z), z)));
            const Val left = g.mul(g.mul(zn, g.add(ap, beta)), g.add(sp, gamma));
            const Val right = g.mul(g.mul(z, g.add(inp, beta)), g.add(tab, gamma));
            term(g.mul(active, g.sub(left, right)));
            const Val a_s = g.keep(g.sub(ap, sp));
            term(g.mul(l0, a_s));
            term(g.mul(g.mul(active, a_s), g.sub(ap, ap_inv)));
        }
    }
    g.line("// h(x)");
    ev[E.count] = g.keep(g.mul(acc, inv[i_xn1]));

    // ---------------------------------------------------------------- the multi-open: scalars per distinct point
    g.line("// the multi-open");
    std::vector<Val> xn_pow(lay.n_h);
    xn_pow[0] = one;
    for (uint32_t i = 1; i < lay.n_h; i++) xn_pow[i] = g.keep(g.mul(xn_pow[i - 1], xn));
    std::vector<SumTerm> A, B;
    auto push = [&](std::vector<SumTerm>& dst, uint32_t base, const Val& s) {  // one entry per base: scalars of a repeated base are added
        if (s.konst == 1) return;
        for (SumTerm& t : dst)
            if (t.base == base) {
                t.s = g.keep(g.add(t.s, s));
                return;
            }
        dst.push_back({base, s});
    };
    auto commit = [&](uint32_t key, const Val& s) {
        if (key == KEY_H) {
            const Val sk = g.keep(s);
            for (uint32_t i = 0; i < lay.n_h; i++) push(B, P.h + i, g.mul(sk, xn_pow[i]));
        } else {
            push(B, key, s);
        }
    };
    auto powers = [&](const Val& b, size_t n) {
        std::vector<Val> p(std::max<size_t>(n, 1));
        p[0] = one;
        for (size_t i = 1; i < n; i++) p[i] = g.keep(g.mul(p[i - 1], b));
        return p;
    };
    const uint32_t np0 = P.opening;
    if (!d.shplonk) {
        size_t longest = 0;
        for (int r : gwc_rots) longest = std::max<size_t>(longest, std::count_if(qs.begin(), qs.end(), [&](const Query& q) { return q.rot == r; }));
        const std::vector<Val> vp = powers(v, longest), up = powers(u, gwc_rots.size());
        Val eval_multi = g.zero();
        for (uint32_t si = 0; si < gwc_rots.size(); si++) {
            const Val z = g.mul(x, g.lit(w_pow(gwc_rots[si])));
            Val eb = g.zero();
            uint32_t j = 0;
            for (const Query& q : qs) {
                if (q.rot != gwc_rots[si]) continue;
                commit(q.key, g.mul(up[si], vp[j]));
                eb = g.keep(g.add(eb, g.mul(vp[j], ev[q.eval])));
                j++;
            }
            eval_multi = g.keep(g.add(eval_multi, g.mul(up[si], eb)));
            push(B, np0 + si, g.mul(up[si], z));
            push(A, np0 + si, up[si]);
        }
        push(B, pl.base_g0(), g.neg(eval_multi));
    } else {
        size_t most_keys = 0, most_rots = 0;
        for (const RSet& s : rs) most_keys = std::max(most_keys, s.keys.size()), most_rots = std::max(most_rots, s.rots.size());
        const std::vector<Val> yp = powers(sy, most_keys), vp = powers(v, rs.size()), xip = powers(inv[i_x], most_rots);
        auto eval_of = [&](uint32_t key, int rot) {
            Val e = g.zero();
            for (const Query& q : qs)
                if (q.key == key && q.rot == rot) e = ev[q.eval];
            return e;
        };
        Val r_outer = g.zero(), z0 = one;
        for (uint32_t i = 0; i < rs.size(); i++) {
            const size_t m = rs[i].rots.size();
            Val zd = one;
            if (i == 0) {
                for (int r : rs[i].rots) z0 = g.mul(z0, u_minus_of(r));
                z0 = g.keep(z0);
            } else {
                for (int r : all_rots)
                    if (!in_set(rs[i], r)) zd = g.mul(zd, u_minus_of(r));
                zd = g.keep(g.mul(zd, inv[i_zd0]));
            }
            // the Lagrange basis through the set's points at u: prod_{t != j} (u - p_t) / (x^(m-1) prod_{t != j} (w^r_j - w^r_t))
            std::vector<Val> basis(m);
            for (size_t j = 0; j < m; j++) {
                Val num = one;
                Fr cden = Fr::one();
                for (size_t t = 0; t < m; t++) {
                    if (t == j) continue;
                    num = g.mul(num, u_minus_of(rs[i].rots[t]));
                    cden = fe_mul(cden, fe_sub(w_pow(rs[i].rots[j]), w_pow(rs[i].rots[t])));
                }
                basis[j] = m == 1 ? one : g.keep(g.mul(g.mul(num, xip[m - 1]), g.lit(fe_inv_fast(cden))));
            }
            const Val pv_zd = g.keep(g.mul(vp[i], zd));
            Val r_inner = g.zero();
            uint32_t ki = 0;
            for (uint32_t key : rs[i].keys) {
                Val rx = g.zero();
                for (size_t j = 0; j < m; j++) rx = g.add(rx, g.mul(eval_of(key, rs[i].rots[j]), basis[j]));
                r_inner = g.keep(g.add(r_inner, g.mul(yp[ki], rx)));
                commit(key, g.mul(yp[ki], pv_zd));
                ki++;
            }
            r_outer = g.keep(g.add(r_outer, g.mul(pv_zd, r_inner)));
        }
        push(B, pl.base_g0(), g.neg(r_outer));
        push(B, np0, g.neg(z0));
        push(B, np0 + 1, u);
        push(A, np0 + 1, one);
    }

    // ---------------------------------------------------------------- the two sums and the pairing
    auto point_of = [&](uint32_t base) {
        if (base < pl.n_points) {
            const uint32_t cd = cd0 + pl.point_off[base];
            return PointRef{"calldataload(" + addr(cd) + ")", "calldataload(" + addr(cd + 32) + ")"};
        }
        if (base == pl.base_g0()) return PointRef{"1", "2"};
        const G1Affine& p = base < pl.base_perm() ? d.fixed[base - pl.base_fix()] : d.perm[base - pl.base_perm()];
        return PointRef{hex_of(p.x), hex_of(p.y)};
    };
    auto sum = [&](std::vector<SumTerm>& terms) {  // into 0x00 .. 0x40
        for (SumTerm& t : terms) t.s = g.keep(t.s);
        bool first = true;
        for (const SumTerm& t : terms) {
            const PointRef p = point_of(t.base);
            if (first && t.s.konst == 2) {
                g.line("mstore(0x00, " + p.x + ")");
                g.line("mstore(0x20, " + p.y + ")");
            } else if (first) {
                g.line("success := and(success, ec_first(" + p.x + ", " + p.y + ", " + t.s.e + "))");
                g.cost.ecmul++;
            } else if (t.s.konst == 2) {
                g.line("success := and(success, ec_plus(" + p.x + ", " + p.y + "))");
                g.cost.ecadd++;
            } else {
                g.line("success := and(success, ec_next(" + p.x + ", " + p.y + ", " + t.s.e + "))");
                g.cost.ecmul++;
                g.cost.ecadd++;
            }
            first = false;
        }
    };
    g.line("// lhs: the opening points' sum");
    sum(A);
    g.line("mstore(0xc0, mload(0x00))");
    g.line("mstore(0xe0, mload(0x20))");
    g.line("// rhs: every commitment once");
    sum(B);
    const Fq2 nsy = f2_neg(d.s_g2.y);
    const Fq* words[8] = {&d.g2.x.c1, &d.g2.x.c0, &d.g2.y.c1, &d.g2.y.c0, &d.s_g2.x.c1, &d.s_g2.x.c0, &nsy.c1, &nsy.c0};
    g.line("// e(rhs, g2) e(lhs, -s_g2) = 1: the imaginary part of a G2 coordinate first");
    for (int i = 0; i < 4; i++) g.line("mstore(" + addr(0x40 + 32 * i) + ", " + hex_of(*words[i]) + ")");
    for (int i = 0; i < 4; i++) g.line("mstore(" + addr(0x100 + 32 * i) + ", " + hex_of(*words[4 + i]) + ")");
    g.line("success := and(success, staticcall(gas(), 8, 0x00, 0x180, 0x00, 0x20))");
    g.line("success := and(success, mload(0x00))");
    g.cost.pairing++;
    g.line("if eq(success, 0) { revert(0, 0) }");
    g.line("return(0, 0)");
    g.cost.memory_bytes = g.top;

    char head[1024];
    std::string ms;
    for (uint32_t m : d.n_instances) ms += (ms.empty() ? "" : " ") + std::to_string(m);
    snprintf(head, sizeof(head),
             "// PLONK verifier (halo2, KZG on BN254, Keccak transcript), generated for one kind of proof\n"
             "// shape: k %u, advice %u, lookup advice %u, fixed %u, lookup bits %u, idle gate columns %u, instance columns %u\n"
             "// circuits: %u\n"
             "// instances per circuit: %s\n"
             "// scheme: %s\n"
             "// calldata bytes: %u\n"
             "// memory top: 0x%x\n"
             "// precompile calls: modexp %u, ecAdd %u, ecMul %u, pairing %u\n"
             "// keccak256: %u calls, %u bytes\n",
             lay.k, lay.A, lay.L, lay.F, lay.lookup_bits, lay.idle, lay.n_inst, nc, ms.c_str(), d.shplonk ? "SHPLONK" : "GWC", cd_len, g.top,
             g.cost.modexp, g.cost.ecadd, g.cost.ecmul, g.cost.pairing, g.cost.keccak_calls, g.cost.keccak_bytes);
    if (text) {
        *text = head;
        *text +=
            "object \"plonk_verifier\" {\n"
            "    code {\n"
            "        datacopy(0, dataoffset(\"Runtime\"), datasize(\"Runtime\"))\n"
            "        return(0, datasize(\"Runtime\"))\n"
            "    }\n"
            "    object \"Runtime\" {\n"
            "        code {\n";
        *text += g.out;
        *text +=
            "        }\n"
            "    }\n"
            "}\n";
    }
    if (cost_out) *cost_out = g.cost;
    return true;
}

}  // namespace evmgen
}  // namespace zk
