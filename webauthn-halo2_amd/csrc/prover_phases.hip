// prover_phases.hip — the phase-level entry points.
//
// For a host that keeps halo2's own prover flow — its transcript, its RNG, its blinding — and off-loads phase by phase
// (examples/prove_host_phases.cpp): the provers of plonk/lookup, plonk/permutation and plonk/vanishing that
// sit between the commitments, over resident columns.  They run the very kernels zk_prove runs; each call is complete on return.
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "prover_steps.h"

using namespace zk;

namespace {
struct PhaseCtx {
    zk_ctx* c;
    zk_pk_rec* pk;
    std::vector<Fr*> adv;
};
// resolves the key and the advice handles (n rows each, Lagrange values, Montgomery)
int phase_open(zk_ctx* c, zk_pk h, const zk_poly* advice, size_t n_advice, PhaseCtx& out) {
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    zk_pk_rec* pk = it->second;
    if (pk->srs_gen != c->srs_gen || pk->verify_only) return ZK_ESTATE;  // a verifying-only key (zk_vk_read / zk_vk_from_parts) has no key polynomials
    if (n_advice != pk->lay.n_adv) return ZK_EINVAL;
    out.c = c;
    out.pk = pk;
    for (size_t j = 0; j < n_advice; j++) {
        const PolyRec* r = ctx_poly(c, advice[j]);
        if (!r || r->n != pk->lay.n) return ZK_EINVAL;
        out.adv.push_back(r->ptr);
    }
    return ctx_bind(c);
}
Fr* phase_vec(zk_ctx* c, zk_poly h, size_t n) {
    const PolyRec* r = ctx_poly(c, h);
    return (!r || r->n != n) ? nullptr : r->ptr;
}
// grand products z[p] of the key's own workspace (num / den already enqueued), complete on return
int phase_grand_products(zk_ctx* c, zk_pk_rec* pk, const std::vector<Fr*>& z, uint32_t chained) {
    if (int rc = grand_products(c, c->stream, pk->lay, {GpGroup{pk, z.data(), (uint32_t)z.size(), chained}},
                                GpScratch{pk->d_gp_items, pk->gp_scal, pk->gp_host}))
        return rc;
    HIPCHK(c, aud_sync(c, c->stream));
    return hipGetLastError() == hipSuccess ? ZK_OK : ZK_EHIP;
}
// every output vector of a phase call is written by its own blocks of a batched launch: the same vector twice among the
// outputs, or an output that another item of the call reads, is a data race that yields garbage — refused before anything is
// launched
bool phase_outputs_ok(const std::vector<const Fr*>& outs, const std::vector<const Fr*>& ins) {
    for (size_t i = 0; i < outs.size(); i++) {
        for (size_t j = i + 1; j < outs.size(); j++)
            if (outs[i] == outs[j]) return false;
        for (const Fr* v : ins)
            if (outs[i] == v) return false;
    }
    return true;
}
}  // namespace

ZK_API(zk_lookup_permute, (zk_ctx* c, zk_pk h, const zk_poly* advice, size_t n_advice, zk_poly* permuted_input, zk_poly* permuted_table, size_t n_lookups), (c, h, advice, n_advice, permuted_input, permuted_table, n_lookups)) {
    if (!c || !advice || !permuted_input || !permuted_table) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    PhaseCtx P;
    int rc = phase_open(c, h, advice, n_advice, P);
    if (rc) return rc;
    const Layout& lay = P.pk->lay;
    if (n_lookups != lay.n_lookups) return ZK_EINVAL;
    std::vector<LkItem> items;
    std::vector<const Fr*> outs, ins(P.adv.begin(), P.adv.end());
    for (uint32_t l = 0; l < lay.n_lookups; l++) {
        Fr *a = phase_vec(c, permuted_input[l], lay.n), *s = phase_vec(c, permuted_table[l], lay.n);
        if (!a || !s) return ZK_EINVAL;
        items.push_back(LkItem{P.pk, P.adv.data(), l, a, s});
        outs.push_back(a);
        outs.push_back(s);
    }
    if (!phase_outputs_ok(outs, ins)) return ZK_EINVAL;  // (a'[l] = s'[m], a repeated handle, an advice column as an output)
    if ((rc = lookup_permute(c, c->stream, lay, items, P.pk->lks))) return rc;
    bool bad = false;
    if ((rc = lookup_permute_failed(c, c->stream, P.pk->lks, &bad))) return rc;
    return bad ? ZK_EWITNESS : ZK_OK;
}

ZK_API(zk_lookup_product, (zk_ctx* c, zk_pk h, const zk_poly* advice, size_t n_advice, const zk_poly* permuted_input, const zk_poly* permuted_table, size_t n_lookups, const uint64_t beta[4], const uint64_t gamma[4], zk_poly* z_out), (c, h, advice, n_advice, permuted_input, permuted_table, n_lookups, beta, gamma, z_out)) {
    if (!c || !advice || !permuted_input || !permuted_table || !beta || !gamma || !z_out) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    PhaseCtx P;
    int rc = phase_open(c, h, advice, n_advice, P);
    if (rc) return rc;
    zk_pk_rec* pk = P.pk;
    const Layout& lay = pk->lay;
    if (n_lookups != lay.n_lookups) return ZK_EINVAL;
    Fr b, g;
    memcpy(&b, beta, 32);
    memcpy(&g, gamma, 32);
    std::vector<Fr*> z;
    std::vector<const Fr*> outs, ins(P.adv.begin(), P.adv.end()), av, sv;
    for (uint32_t l = 0; l < lay.n_lookups; l++) {
        const Fr *a = phase_vec(c, permuted_input[l], lay.n), *s = phase_vec(c, permuted_table[l], lay.n);
        Fr* zl = phase_vec(c, z_out[l], lay.n);
        if (!a || !s || !zl) return ZK_EINVAL;
        av.push_back(a);
        sv.push_back(s);
        ins.push_back(a);
        ins.push_back(s);
        outs.push_back(zl);
        z.push_back(zl);
    }
    if (!phase_outputs_ok(outs, ins)) return ZK_EINVAL;  // (before the first launch: a repeated z, or a z that some lookup reads)
    // (one launch per lookup whatever their number: the call owns no staging)
    if ((rc = lk_numden_enqueue(c, c->stream, pk, P.adv.data(), av.data(), sv.data(), b, g, 0, false, true))) return rc;
    return phase_grand_products(c, pk, z, 0);
}

namespace {
// zk_permutation_product and zk_permutation_product_public: `with_instance` says which rule the key's instance column follows —
// false: the key must have none; true: `instance` is the column of a key that has one and 0 for a key that has none
int permutation_product(zk_ctx* c, zk_pk h, const zk_poly* advice, size_t n_advice, bool with_instance, zk_poly instance, const uint64_t beta[4],
                        const uint64_t gamma[4], zk_poly* z_out, size_t n_chunks) {
    if (!c || !advice || !beta || !gamma || !z_out) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    PhaseCtx P;
    int rc = phase_open(c, h, advice, n_advice, P);
    if (rc) return rc;
    zk_pk_rec* pk = P.pk;
    const Layout& lay = pk->lay;
    if (n_chunks != lay.n_chunks) return ZK_EINVAL;
    if (lay.n_inst && !with_instance) return ZK_EINVAL;  // (zk_permutation_product carries no instance column)
    const Fr* inst = nullptr;
    if (with_instance) {
        // the whole-proof rule (halo2's InvalidInstances): a column for a key with one, none for a key without
        if ((instance != 0) != (lay.n_inst != 0)) return ZK_EINVAL;
        if (lay.n_inst && !(inst = phase_vec(c, instance, lay.n))) return ZK_EINVAL;
    }
    Fr b, g;
    memcpy(&b, beta, 32);
    memcpy(&g, gamma, 32);
    const Fr* tw = nullptr;
    if ((rc = ctx_get_twiddles(c, lay.k, &tw))) return rc;
    std::vector<Fr*> z;
    for (uint32_t ci = 0; ci < lay.n_chunks; ci++) {
        Fr* zc = phase_vec(c, z_out[ci], lay.n);
        if (!zc) return ZK_EINVAL;
        z.push_back(zc);
    }
    {
        std::vector<const Fr*> outs(z.begin(), z.end()), ins(P.adv.begin(), P.adv.end());
        if (inst) ins.push_back(inst);
        if (!phase_outputs_ok(outs, ins)) return ZK_EINVAL;  // (before the first launch: a repeated z, an advice or the instance column as z)
    }
    if ((rc = perm_numden_enqueue(c, c->stream, pk, P.adv.data(), tw, b, g, false, inst))) return rc;  // (one launch per chunk, as above)
    return phase_grand_products(c, pk, z, lay.n_chunks);
}
}  // namespace

ZK_API(zk_permutation_product, (zk_ctx* c, zk_pk h, const zk_poly* advice, size_t n_advice, const uint64_t beta[4], const uint64_t gamma[4], zk_poly* z_out, size_t n_chunks), (c, h, advice, n_advice, beta, gamma, z_out, n_chunks)) {
    return permutation_product(c, h, advice, n_advice, false, 0, beta, gamma, z_out, n_chunks);
}

ZK_API(zk_permutation_product_public, (zk_ctx* c, zk_pk h, const zk_poly* advice, size_t n_advice, zk_poly instance, const uint64_t beta[4], const uint64_t gamma[4], zk_poly* z_out, size_t n_chunks), (c, h, advice, n_advice, instance, beta, gamma, z_out, n_chunks)) {
    return permutation_product(c, h, advice, n_advice, true, instance, beta, gamma, z_out, n_chunks);
}

// `count` (polynomial, point) pairs through the provers' batched evaluation step (evaluate_enqueue: one launch and one host
// round trip for up to EVAL_BATCH_PAIRS pairs), over staging the context keeps: pinned items and results, their device twins
// in the context's scratch.  Nothing is written to `out` before every pair is evaluated.
ZK_API(zk_eval_batch, (zk_ctx* c, const zk_poly* polys, const uint64_t* points, size_t count, uint64_t* out), (c, polys, points, count, out)) {
    if (!c || !polys || !points || !out || count == 0) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    std::vector<const Fr*> ptr(count);
    size_t n = 0;
    for (size_t i = 0; i < count; i++) {
        const PolyRec* r = ctx_poly(c, polys[i]);
        if (!r || r->n == 0 || r->n > 0xffffffffu || (i && r->n != n)) return ZK_EINVAL;  // (the step takes ONE length per launch)
        n = r->n;
        ptr[i] = r->ptr;
    }
    int rc = ctx_bind(c);
    if (rc) return rc;
    constexpr size_t PAIRS = EVAL_BATCH_PAIRS;
    const size_t item_words = (PAIRS * sizeof(EvalItem) + sizeof(Fr) - 1) / sizeof(Fr);  // the device items, in elements of the scratch
    const uint32_t blocks = eval_blocks((uint32_t)n);
    if (!c->eval_batch_host) {
        void* p = nullptr;
        HIPCHK(c, hipHostMalloc(&p, (item_words + PAIRS) * sizeof(Fr)));
        c->eval_batch_host = p;
    }
    if ((rc = ctx_ensure_scratch(c, item_words + PAIRS * blocks + PAIRS))) return rc;
    EvalBufs b;
    b.h_items = static_cast<EvalItem*>(c->eval_batch_host);
    b.host = static_cast<Fr*>(c->eval_batch_host) + item_words;
    b.d_items = reinterpret_cast<EvalItem*>(c->scratch);
    b.scratch = c->scratch + item_words;
    b.out = b.scratch + PAIRS * blocks;
    std::vector<Fr> res(count);
    for (size_t i0 = 0; i0 < count; i0 += PAIRS) {
        const size_t cnt = std::min(PAIRS, count - i0);
        for (size_t i = 0; i < cnt; i++) {
            b.h_items[i].poly = ptr[i0 + i];
            b.h_items[i].pad_ = 0;
            memcpy(&b.h_items[i].x, points + 4 * (i0 + i), 32);
        }
        if ((rc = evaluate_enqueue(c, c->stream, b, (uint32_t)cnt, (uint32_t)n))) return rc;  // (has waited: the staging is free again)
        if (hipGetLastError() != hipSuccess) return ZK_EHIP;
        memcpy(res.data() + i0, b.host, cnt * sizeof(Fr));
    }
    memcpy(out, res.data(), count * sizeof(Fr));
    return ZK_OK;
}

// a copy of one of the key's own polynomials (coefficient form) in a caller's vector: what a phase-driving host evaluates and
// opens beside its own columns (the fixed and permutation polynomials of the ProvingKey)
ZK_API(zk_pk_export_poly, (zk_ctx* c, zk_pk h, int which, size_t index, zk_poly dst), (c, h, which, index, dst)) {
    if (!c) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    zk_pk_rec* pk = it->second;
    if (pk->srs_gen != c->srs_gen || pk->verify_only) return ZK_ESTATE;
    const std::vector<Fr*>* v = which == ZK_PK_FIXED_POLY ? &pk->fixed_poly : which == ZK_PK_SIGMA_POLY ? &pk->sigma_poly : nullptr;
    if (!v || index >= v->size()) return ZK_EINVAL;
    Fr* d = phase_vec(c, dst, pk->lay.n);
    if (!d) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(d, (*v)[index], (size_t)pk->lay.n * sizeof(Fr), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, aud_sync(c, c->stream));
    return ZK_OK;
}

// the vanishing argument's random polynomial: coefficient i = Fr::random of ChaCha20 block first_block + i under `key` — the
// stream `ChaCha20Rng::from_seed(key)` yields when every draw is an Fr::random (one 64-byte block each), i.e. what the host's
// RNG would give for draws first_block .. first_block + n - 1; the host then advances its own RNG by n draws
ZK_API(zk_random_poly, (zk_ctx* c, const uint8_t chacha_key[32], uint64_t first_block, zk_poly out), (c, chacha_key, first_block, out)) {
    if (!c || !chacha_key) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    const PolyRec* r = ctx_poly(c, out);
    if (!r || r->n == 0 || r->n > ((size_t)1 << 28)) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    ChaChaKey key;
    memcpy(key.w, chacha_key, 32);
    launch_chacha_fr(key, first_block, r->ptr, (uint32_t)r->n, c->stream);
    HIPCHK(c, aud_sync(c, c->stream));
    return ZK_OK;
}

// out = sum_j coeffs[j] * in[j] - (sub_low[0] + sub_low[1] X + ..): the multi-open provers' linear combinations (GWC subtracts the
// combined evaluation, SHPLONK the combined remainder polynomial of a rotation set) and h(X) = sum x^(n i) h_i
ZK_API(zk_poly_lincomb, (zk_ctx* c, zk_poly out, const zk_poly* in, const uint64_t* coeffs, size_t count, const uint64_t* sub_low, size_t n_low), (c, out, in, coeffs, count, sub_low, n_low)) {
    if (!c || !in || !coeffs || count == 0 || n_low > 8 || (n_low && !sub_low)) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    const PolyRec* o = ctx_poly(c, out);
    if (!o || o->n > 0xffffffffu) return ZK_EINVAL;
    const size_t n = o->n;
    std::vector<Term> terms(count);
    for (size_t j = 0; j < count; j++) {
        const PolyRec* r = ctx_poly(c, in[j]);
        if (!r || r->n != n || r->ptr == o->ptr) return ZK_EINVAL;
        terms[j].poly = r->ptr;
        memcpy(&terms[j].c, coeffs + 4 * j, 32);
    }
    int rc = ctx_bind(c);
    if (rc) return rc;
    Fr low[8];  // the low-degree polynomial subtracted from the first n_low coefficients
    if (n_low) memcpy(low, sub_low, n_low * 32);
    lincomb_enqueue(c->stream, o->ptr, (uint32_t)n, terms, false, nullptr, low, (uint32_t)n_low);
    HIPCHK(c, aud_sync(c, c->stream));
    return ZK_OK;
}

ZK_API(zk_poly_upload_canonical, (zk_ctx* c, zk_poly h, const uint64_t* host_canonical, size_t n), (c, h, host_canonical, n)) {
    int rc = zk_poly_upload(c, h, host_canonical, n);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    const PolyRec* r = ctx_poly(c, h);
    if (!r) return ZK_EINVAL;
    if ((rc = ctx_bind(c))) return rc;
    launch_to_mont(r->ptr, (uint32_t)n, c->stream);
    if (aud_sync(c, c->stream) != hipSuccess) return ZK_EHIP;
    return ZK_OK;
}
