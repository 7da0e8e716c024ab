// prover_steps.h — the steps of create_proof: ONE definition each, called by the whole-proof driver (prover_lockstep.h
// LockstepRun::run: one lane or several) and the phase-level entry points (prover_phases.hip).  A step enqueues on the stream it is
// given and names its buffers to the stream audit (audit.h) when that is on; WHICH step runs, in which order, on which lane, and
// when the host waits is the callers' business — no step synchronises except where its result is read by the host (the grand
// products' scan totals, the lookup error flag, the evaluations).
#pragma once
#include <algorithm>
#include <deque>
#include <functional>
#include <vector>

#include "pk.h"
#include "transcript.h"

// ------------------------------------------------------------ host helpers ---
// (fr_batch_invert — one Montgomery batch inversion, reached through this header by its callers — is hostutil.h's: the verifier shares it)

// affine forms of `cnt` Jacobian points with ONE field inversion for the whole batch (Montgomery's trick over the z's; the
// identity — z = 0 — is skipped and comes out as (0, 0))
inline void jac_batch_to_affine(const G1Jac* js, uint32_t cnt, G1Affine* af) {
    Fq pre[MSM_MAX_BATCH];
    Fq run = Fq::one();
    for (uint32_t q = 0; q < cnt; q++) {
        pre[q] = run;
        if (!js[q].z.is_zero()) run = fe_mul(run, js[q].z);
    }
    Fq inv = fe_inv_fast(run);
    for (uint32_t q = cnt; q-- > 0;) {
        if (js[q].z.is_zero()) {
            af[q].x = Fq::zero();
            af[q].y = Fq::zero();
            continue;
        }
        const Fq zi = fe_mul(inv, pre[q]);
        inv = fe_mul(inv, js[q].z);
        const Fq zi2 = fe_sqr(zi);
        af[q].x = fe_mul(js[q].x, zi2);
        af[q].y = fe_mul(js[q].y, fe_mul(zi2, zi));
    }
}

inline void aud_note(zk_ctx* c, hipStream_t st, const std::vector<const void*>& rd, const std::vector<const void*>& wr, const char* site) {
    c->audit.op_v(st, rd.data(), rd.size(), wr.data(), wr.size(), site);
}

// ------------------------------------------------------------------ advice ---
// The caller's advice columns into the workspace.  Many columns (advice_staged): ALL of them in one launch over an argument
// block staged in the workspace's h_batch_args / d_batch_args (the caller waits for the stream before that staging is written
// again); otherwise the driver copies column by column (advice_column), each copy right before the column's blinding rows
inline bool advice_staged(const Layout& lay) { return lay.n_adv > BATCH_ARGS_MIN; }
inline int advice_columns_staged(zk_ctx* c, hipStream_t st, zk_pk_rec* pk, const Fr* const* adv) {
    const Layout& lay = pk->lay;
    CopyPair* h = static_cast<CopyPair*>(pk->h_batch_args);
    for (uint32_t j = 0; j < lay.n_adv; j++) h[j] = CopyPair{adv[j], pk->adv_val[j]};
    if (c->audit.on) {
        std::vector<const void*> rd(adv, adv + lay.n_adv), wr(pk->adv_val.begin(), pk->adv_val.end());
        aud_note(c, st, rd, wr, "advice columns into the workspace");
    }
    HIPCHK(c, hipMemcpyAsync(pk->d_batch_args, h, lay.n_adv * sizeof(CopyPair), hipMemcpyHostToDevice, st));
    launch_copy_columns(static_cast<const CopyPair*>(pk->d_batch_args), lay.n_adv, lay.n, st);
    return ZK_OK;
}
inline int advice_column(zk_ctx* c, hipStream_t st, zk_pk_rec* pk, const Fr* const* adv, uint32_t j) {
    if (c->audit.on) c->audit.op(st, {adv[j]}, {pk->adv_val[j]}, "advice column into the workspace");
    HIPCHK(c, hipMemcpyAsync(pk->adv_val[j], adv[j], (size_t)pk->lay.n * sizeof(Fr), hipMemcpyDeviceToDevice, st));
    return ZK_OK;
}

// ----------------------------------------------------------------- lookups ---
// the compressed input expression of lookup l over the advice columns `adv`: the lookup advice column itself, or q_lookup * a
// for the one-column shape (in pk->lk_in[l]; `make`: enqueue that product)
inline const Fr* lookup_input(zk_ctx* c, hipStream_t st, zk_pk_rec* pk, const Fr* const* adv, uint32_t l, bool make) {
    const Layout& lay = pk->lay;
    if (!lay.single) return adv[lay.n_gate + l];
    if (make) {
        if (c->audit.on) c->audit.op(st, {adv[0]}, {pk->lk_in[l]}, "lookup input = q_lookup x advice");
        launch_mul(pk->lk_in[l], pk->fixed_val[lay.fx_qlookup], adv[0], lay.n, st);
    }
    return pk->lk_in[l];
}

// one lookup of a permutation pass: its workspace and advice columns, where a' and s' go
struct LkItem {
    zk_pk_rec* pk;
    const Fr* const* adv;
    uint32_t l;
    Fr *ap, *sp;
};
// permuted input / table of every item, in groups of MAX_LOOKUPS (what LkPtrs holds) over consecutive slices of `lks`: one set
// of launches per group (blockIdx.y = lookup).  The error flag of `lks` is cleared first and accumulates: lookup_permute_failed
inline int lookup_permute(zk_ctx* c, hipStream_t st, const Layout& lay, const std::vector<LkItem>& items, const LookupScratch& lks) {
    HIPCHK(c, hipMemsetAsync(lks.err, 0, 4, st));
    const uint32_t total = (uint32_t)items.size();
    for (uint32_t i0 = 0; i0 < total; i0 += MAX_LOOKUPS) {
        LkPtrs lp;
        memset(&lp, 0, sizeof(lp));
        const uint32_t cnt = std::min<uint32_t>(MAX_LOOKUPS, total - i0);
        std::vector<const void*> rd, wr;
        for (uint32_t i = 0; i < cnt; i++) {
            const LkItem& it = items[i0 + i];
            lp.inp[i] = lookup_input(c, st, it.pk, it.adv, it.l, true);
            lp.ap[i] = it.ap;
            lp.sp[i] = it.sp;
            if (c->audit.on) {
                rd.push_back(lp.inp[i]);
                wr.push_back(it.ap);
                wr.push_back(it.sp);
            }
        }
        if (c->audit.on) aud_note(c, st, rd, wr, "lookup permutation");
        LookupScratch s = lks;  // this group's slice of the scratch: lookup i0's arrays first
        const size_t off = (size_t)i0 * s.stride;
        s.hist += off;
        s.present += off;
        s.absent += off;
        s.off += off;
        s.dex += off;
        s.aex += off;
        s.bsum += off;
        launch_lookup_permute(lp, cnt, lay.usable, 1u << lay.lookup_bits, s, st);
    }
    return ZK_OK;
}
// reads the flag (waits for the stream).  *bad: some input of some lookup is outside the table — halo2's ConstraintSystemFailure
inline int lookup_permute_failed(zk_ctx* c, hipStream_t st, const LookupScratch& lks, bool* bad) {
    uint32_t* err = reinterpret_cast<uint32_t*>(c->host_small);
    HIPCHK(c, hipMemcpyAsync(err, lks.err, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, aud_sync(c, st));
    *bad = *err != 0;
    return ZK_OK;
}

// ------------------------------------------ numerators and denominators ---
// the values of a permutation column: a fixed column of the key, an advice column of `adv`, or the instance column — `inst`, a
// caller's own vector (the phase-level zk_permutation_product_public), or the workspace's when that is null
inline const Fr* perm_col_values(const zk_pk_rec* pk, const Col& col, const Fr* const* adv, const Fr* inst = nullptr) {
    return col.type == COL_FIXED ? pk->fixed_val[col.idx] : col.type == COL_INSTANCE ? (inst ? inst : pk->inst_val) : adv[col.idx];
}
// the arguments of permutation chunk ci: its columns' values (fixed from the key, advice from `adv`), their sigma columns and
// delta^(global column index) — `dcur` runs over the chunks of a proof, starting at one
inline PermArgs perm_chunk_args(const Layout& lay, const zk_pk_rec* pk, uint32_t ci, const Fr* const* adv, const Fr* tw, const Fr& beta,
                                const Fr& gamma, Fr& dcur, const Fr* inst = nullptr) {
    PermArgs a;
    memset(&a, 0, sizeof(a));
    a.n = lay.n;
    const uint32_t lo = ci * lay.chunk_len, hi = std::min<uint32_t>((uint32_t)lay.perm_cols.size(), lo + lay.chunk_len);
    a.ncols = hi - lo;
    const Fr delta = fr_delta();
    for (uint32_t p = lo; p < hi; p++) {
        const Col& col = lay.perm_cols[p];
        a.values[p - lo] = perm_col_values(pk, col, adv, inst);
        a.sigma[p - lo] = pk->sigma_val[p];
        a.delta[p - lo] = dcur;
        dcur = fe_mul(dcur, delta);
    }
    a.tw = tw;
    a.beta = beta;
    a.gamma = gamma;
    a.num = pk->gp_num[ci];
    a.den = pk->gp_den[ci];
    return a;
}
// numerators / denominators of every permutation chunk of one proof into gp_num / gp_den [0, n_chunks): one launch per chunk,
// or — `may_stage` and many chunks — one launch over the argument blocks staged in h_batch_args / d_batch_args.  `inst`: the
// instance column's values where they are not the workspace's own (perm_col_values)
inline int perm_numden_enqueue(zk_ctx* c, hipStream_t st, zk_pk_rec* pk, const Fr* const* adv, const Fr* tw, const Fr& beta, const Fr& gamma,
                               bool may_stage, const Fr* inst = nullptr) {
    const Layout& lay = pk->lay;
    const bool staged = may_stage && lay.n_chunks > BATCH_ARGS_MIN;
    Fr dcur = Fr::one();
    for (uint32_t ci = 0; ci < lay.n_chunks; ci++) {
        const PermArgs a = perm_chunk_args(lay, pk, ci, adv, tw, beta, gamma, dcur, inst);
        if (c->audit.on) {
            std::vector<const void*> rd(a.values, a.values + a.ncols);
            aud_note(c, st, rd, {a.num, a.den}, "permutation numerators / denominators");  // (the staged form launches below, same stream)
        }
        if (staged) static_cast<PermArgs*>(pk->h_batch_args)[ci] = a;
        else launch_perm_numden(a, st);
    }
    if (staged) {
        HIPCHK(c, hipMemcpyAsync(pk->d_batch_args, pk->h_batch_args, lay.n_chunks * sizeof(PermArgs), hipMemcpyHostToDevice, st));
        launch_perm_numden_batch(static_cast<const PermArgs*>(pk->d_batch_args), lay.n_chunks, lay.n, st);
    }
    return ZK_OK;
}
// the same for every lookup of one proof, into gp_num / gp_den [prod0, prod0 + n_lookups); ap / sp: the permuted columns;
// `make_input`: the one-column shape's q_lookup * a is enqueued here (a caller that has not run lookup_permute on this workspace)
inline int lk_numden_enqueue(zk_ctx* c, hipStream_t st, zk_pk_rec* pk, const Fr* const* adv, const Fr* const* ap, const Fr* const* sp,
                             const Fr& beta, const Fr& gamma, uint32_t prod0, bool may_stage, bool make_input) {
    const Layout& lay = pk->lay;
    const bool staged = may_stage && lay.n_lookups > BATCH_ARGS_MIN;
    for (uint32_t l = 0; l < lay.n_lookups; l++) {
        const Fr* inp = lookup_input(c, st, pk, adv, l, make_input);
        Fr *num = pk->gp_num[prod0 + l], *den = pk->gp_den[prod0 + l];
        if (c->audit.on) c->audit.op(st, {ap[l], sp[l], inp}, {num, den}, "lookup numerators / denominators");
        if (staged) static_cast<LkNumDenArgs*>(pk->h_batch_args)[l] = LkNumDenArgs{ap[l], sp[l], inp, pk->fixed_val[lay.fx_table], num, den};
        else launch_lk_numden(ap[l], sp[l], inp, pk->fixed_val[lay.fx_table], beta, gamma, num, den, lay.n, st);
    }
    if (staged) {
        HIPCHK(c, hipMemcpyAsync(pk->d_batch_args, pk->h_batch_args, lay.n_lookups * sizeof(LkNumDenArgs), hipMemcpyHostToDevice, st));
        launch_lk_numden_batch(static_cast<const LkNumDenArgs*>(pk->d_batch_args), lay.n_lookups, beta, gamma, lay.n, st);
    }
    return ZK_OK;
}

// ---------------------------------------------------------- grand products ---
// the products of one workspace: z[p] from pk->gp_num[p] / pk->gp_den[p], p < nprod; products 1 .. chained - 1 start from their
// predecessor's value at row `usable` (the chunks of a permutation argument), every other one from 1
struct GpGroup {
    zk_pk_rec* pk;
    Fr* const* z;
    uint32_t nprod, chained;
};
struct GpScratch {
    GpItem* d_items;  // one per product of all groups
    Fr* scal;         // device: q, q_inv, k, init (one per product each)
    Fr* host;         // pinned: q and q_inv
};
// All products of all groups, halo2's semantics: ONE scan, one host round trip for the block totals, one field inversion, one
// apply.  A zero denominator anywhere (or ZK_OPT_GP_BATCH_INVERT) sends every product down halo2's batch_invert form (0 -> 0),
// product by product.  The numerators / denominators are already enqueued on `st`.
inline int grand_products(zk_ctx* c, hipStream_t st, const Layout& lay, const std::vector<GpGroup>& groups, const GpScratch& s) {
    const uint32_t n = lay.n, usable = lay.usable, nblk = gp_blocks(n);
    uint32_t np = 0;
    for (const GpGroup& g : groups) np += g.nprod;
    std::vector<GpItem> items(np);
    {
        GpItem* it = items.data();
        for (const GpGroup& g : groups)
            for (uint32_t p = 0; p < g.nprod; p++, it++) {
                it->num = g.pk->gp_num[p];
                it->den = g.pk->gp_den[p];
                it->loc_p = g.pk->gp_loc_p[p];
                it->loc_r = g.pk->gp_loc_r[p];
                it->tot_p = g.pk->gp_tot + (size_t)2 * nblk * p;
                it->tot_r = it->tot_p + nblk;
                it->z = g.z[p];
                it->chain = (p > 0 && p < g.chained) ? 1u : 0u;
                it->pad_ = 0;
            }
    }
    if (c->audit.on) {
        std::vector<const void*> rd, wr;
        for (const GpItem& it : items) {
            rd.push_back(it.num);
            rd.push_back(it.den);
            wr.push_back(it.z);
        }
        aud_note(c, st, rd, wr, "grand products");  // (scan + apply, or the batch_invert fallback: same buffers, same stream)
    }
    Fr *q_dev = s.scal, *qinv_dev = s.scal + np, *k_dev = s.scal + 2 * (size_t)np, *init_dev = s.scal + 3 * (size_t)np;
    bool fast = !c->opt_gp_batch_invert;  // zk_ctx_set_option(ZK_OPT_GP_BATCH_INVERT)
    if (fast) {
        HIPCHK(c, hipMemcpyAsync(s.d_items, items.data(), np * sizeof(GpItem), hipMemcpyHostToDevice, st));
        launch_gp_batch_scan(s.d_items, np, n, q_dev, st);
        HIPCHK(c, hipMemcpyAsync(s.host, q_dev, np * sizeof(Fr), hipMemcpyDeviceToHost, st));
        HIPCHK(c, aud_sync(c, st));
        fast = fr_batch_invert(s.host, s.host + np, np);
        if (fast) {
            HIPCHK(c, hipMemcpyAsync(qinv_dev, s.host + np, np * sizeof(Fr), hipMemcpyHostToDevice, st));
            launch_gp_batch_apply(s.d_items, np, n, usable, qinv_dev, k_dev, init_dev, st);
        }
    }
    if (!fast) {
        for (const GpGroup& g : groups)
            for (uint32_t p = 0; p < g.nprod; p++) {
                launch_frac(g.pk->gp_num[p], g.pk->gp_den[p], g.pk->t_frac, n, st);
                const Fr* prev = (p > 0 && p < g.chained) ? g.z[p - 1] + usable : nullptr;
                launch_prefix_product(g.pk->t_frac, g.z[p], n, prev, Fr::one(), g.pk->t_a, g.pk->t_small, st);
            }
    }
    return ZK_OK;
}

// ---------------------------------------------------------------- quotient ---
// h(X) on the extended coset (pk_quotient, divided by X^n - 1) from the coset forms of the workspace's own columns, into h_ext
// `into` / `yscale` / `accumulate`: one pass of a quotient that several circuits share (prover_lockstep.h) — this workspace's terms
// times yscale, stored to `into` or added to it; the plain call below is the pass that stores this workspace's own quotient
inline int quotient_pass_of_workspace(zk_ctx* c, hipStream_t st, zk_pk_rec* pk, bool cosets3, const Fr& beta, const Fr& gamma, const Fr& y,
                                      Fr* into, const Fr& yscale, bool accumulate) {
    const Layout& lay = pk->lay;
    QuotientCosets qc;
    qc.adv.assign(pk->adv_coset.begin(), pk->adv_coset.end());
    qc.z.assign(pk->z_coset.begin(), pk->z_coset.end());
    for (uint32_t l = 0; l < lay.n_lookups; l++) {
        qc.lk_a.push_back(pk->lk_ap_coset[l]);
        qc.lk_s.push_back(pk->lk_sp_coset[l]);
        qc.lk_z.push_back(pk->lk_z_coset[l]);
    }
    qc.inst = pk->inst_coset;
    qc.cosets3 = cosets3;
    if (c->audit.on) {
        std::vector<const void*> rd;
        if (qc.inst) rd.push_back(qc.inst);
        for (auto* v : {&qc.adv, &qc.z, &qc.lk_a, &qc.lk_s, &qc.lk_z})
            for (const Fr* q : *v) rd.push_back(q);
        if (accumulate) rd.push_back(into);
        aud_note(c, st, rd, {into}, accumulate ? "quotient (accumulating pass)" : "quotient");
    }
    return pk_quotient_pass(c, pk, qc, beta, gamma, y, yscale, accumulate, true, into);
}
inline int quotient_of_workspace(zk_ctx* c, hipStream_t st, zk_pk_rec* pk, bool cosets3, const Fr& beta, const Fr& gamma, const Fr& y) {
    return quotient_pass_of_workspace(c, st, pk, cosets3, beta, gamma, y, pk->h_ext, Fr::one(), false);
}

// ------------------------------------------------------------- evaluations ---
struct EvalBufs {
    EvalItem *h_items, *d_items;  // pinned staging (polynomial and point of every item: filled by the caller) and its device twin
    Fr *scratch, *out, *host;     // device scratch and results; pinned: the results, read by the caller on return
};
// every opened value in ONE launch; the host has waited for the results on return
inline int evaluate_enqueue(zk_ctx* c, hipStream_t st, const EvalBufs& b, uint32_t total, uint32_t n) {
    if (c->audit.on) {
        std::vector<const void*> rd;
        for (uint32_t i = 0; i < total; i++) rd.push_back(b.h_items[i].poly);
        aud_note(c, st, rd, {b.out}, "evaluations");
        c->audit.op(st, {b.out}, {b.host}, "evaluations to the host");
    }
    hipEventRecord(c->ev[ZK_T_EVAL][0], st);
    launch_eval_batch(b.h_items, b.d_items, total, n, b.scratch, b.out, st);
    hipEventRecord(c->ev[ZK_T_EVAL][1], st);
    c->ev_valid[ZK_T_EVAL] = true;
    HIPCHK(c, hipMemcpyAsync(b.host, b.out, (size_t)total * sizeof(Fr), hipMemcpyDeviceToHost, st));
    HIPCHK(c, aud_sync(c, st));
    c->audit.host_read(b.host, "evaluations read by the host");
    return ZK_OK;
}

// ----------------------------------------------------- linear combinations ---
struct Term {
    const Fr* poly;
    Fr c;
};
// out = sum_j c_j * in_j over n coefficients, MAX_LC inputs per launch (the later launches accumulate; `accumulate_first`: so does
// the first); the last launch subtracts sub0 from coefficient 0 and low[0 .. n_low) from the first n_low coefficients
inline void lincomb_enqueue(hipStream_t st, Fr* out, uint32_t n, const std::vector<Term>& terms, bool accumulate_first, const Fr* sub0,
                            const Fr* low, uint32_t n_low) {
    size_t done = 0;
    bool first = !accumulate_first;
    do {
        LincombArgs a;
        memset(&a, 0, sizeof(a));
        a.out = out;
        a.n = n;
        const size_t take = std::min<size_t>(MAX_LC, terms.size() - done);
        a.count = (uint32_t)take;
        a.accumulate = first ? 0 : 1;
        for (size_t j = 0; j < take; j++) {
            a.in[j] = terms[done + j].poly;
            a.len[j] = n;
            a.c[j] = terms[done + j].c;
            a.unit[j] = terms[done + j].c == Fr::one();
        }
        done += take;
        if (done == terms.size() && sub0) {
            a.sub0 = 1;
            a.sub0_val = *sub0;
        }
        if (done == terms.size() && n_low) {
            a.sub_low_n = n_low;
            for (uint32_t t = 0; t < n_low; t++) a.sub_low[t] = low[t];
        }
        launch_lincomb(a, st);
        first = false;
    } while (done < terms.size());
}

// ------------------------------------------------------------- commitments ---
// a column to commit, and the transcript that receives its point (the queue of commitments in flight over the MSM lanes is the
// driver's: prover_lockstep.h LockstepRun::Commits — one proof: every column carries the proof's transcript; several: each its owner's)
struct CommitCol {
    const Fr* poly;
    Transcript* to;
};
