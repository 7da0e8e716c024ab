// prover_key.hip — the proving key on the device: keygen, its workspace and lock-step members, and the quotient over the key's cosets.
//
// Host orchestration (C++) mirroring halo2_proofs `plonk::keygen_vk` / `keygen_pk` as the reference calls them
// (halo2-circuits/src/ecc/ecdsa_p256.rs:259-260); create_proof is prover.hip, the phase-level entry points prover_phases.hip.
// pk.h declares what crosses files.
#include <stdlib.h>

#include <algorithm>
#include <unordered_map>
#include <vector>

#include "pk.h"
#include "vkrepr.h"

using namespace zk;

namespace {

// ---------------------------------------------------------------- kernels ---
__global__ void sigma_kernel(const uint2* __restrict__ map, const Fr* __restrict__ tw, const Fr* __restrict__ dpow,
                             Fr* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint2 m = map[i];
    fe_store(out + i, fe_mul(fe_load(dpow + m.x), fe_load(tw + m.y)));
}

// ------------------------------------------------------------ small utils ---
bool commit(zk_ctx* c, const Fr* poly, size_t len, int basis, G1Affine* out) {
    G1Jac j;
    if (ctx_msm_device(c, poly, ctx_basis(c, basis), len, &j) != ZK_OK) return false;
    *out = g1_jac_to_affine_host(j);
    return true;
}

}  // namespace

Fr fr_delta() {
    static const Fr delta = [] {
        Fr d = fr_from_u64(7);
        for (int i = 0; i < 28; i++) d = fe_sqr(d);
        return d;
    }();
    return delta;
}

static void bb_destroy(BatchBufs* bb) {
    if (!bb) return;
    if (bb->lk_u32) hipFree(bb->lk_u32);
    if (bb->d_gp_items) hipFree(bb->d_gp_items);
    if (bb->gp_scal) hipFree(bb->gp_scal);
    if (bb->gp_host) hipHostFree(bb->gp_host);
    if (bb->d_evargs) hipFree(bb->d_evargs);
    if (bb->h_evargs) hipHostFree(bb->h_evargs);
    if (bb->ev_scratch) hipFree(bb->ev_scratch);
    if (bb->ev_out) hipFree(bb->ev_out);
    if (bb->tail_host) hipHostFree(bb->tail_host);
    if (bb->inst_host) hipHostFree(bb->inst_host);
    if (bb->inst_dev) hipFree(bb->inst_dev);
    delete bb;
}

void pk_destroy(zk_pk_rec* pk) {
    if (!pk) return;
    for (zk_pk_rec* m : pk->members) pk_destroy(m);  // (a member's key half aliases this record's: only its workspace goes)
    pk->members.clear();
    bb_destroy(pk->bb);
    pk->bb = nullptr;
    wc_destroy(pk->wc);
    pk->wc = nullptr;
    pc_destroy(pk->pc);
    pk->pc = nullptr;
    for (Fr* p : pk->dev) hipFree(p);
    if (pk->tail_host) hipHostFree(pk->tail_host);
    if (pk->rows_host) hipHostFree(pk->rows_host);
    if (pk->rows_dev) hipFree(pk->rows_dev);
    if (pk->lk_u32) hipFree(pk->lk_u32);
    if (pk->gp_host) hipHostFree(pk->gp_host);
    if (pk->d_gp_items) hipFree(pk->d_gp_items);
    if (pk->d_qargs) hipFree(pk->d_qargs);
    if (pk->d_batch_args) hipFree(pk->d_batch_args);
    if (pk->h_batch_args) hipHostFree(pk->h_batch_args);
    if (pk->h_qargs) hipHostFree(pk->h_qargs);
    if (pk->d_lc_terms) hipFree(pk->d_lc_terms);
    if (pk->h_lc_terms) hipHostFree(pk->h_lc_terms);
    if (pk->d_evargs) hipFree(pk->d_evargs);
    if (pk->h_evargs) hipHostFree(pk->h_evargs);
    delete pk;
}

void pk_destroy_all(zk_ctx* c) {
    for (auto& kv : c->pks) pk_destroy(kv.second);
    c->pks.clear();
}

// halo2's transcript_repr of a key made (or read) here: the hash of the pinned verifying key's Debug rendering
// (vkrepr.h) — every shape, never-enabled gate columns included (round 4: their combined selectors are rendered as
// compress_selectors builds them; the stand-in hash of earlier rounds is gone).  A host-supplied value still replaces it.
Fr pk_standin_transcript_repr(const zk_pk_rec* pk) { return vkrepr::transcript_repr(pk->lay, pk->fixed_commit, pk->perm_commit); }

int pk_alloc_workspace(zk_ctx* c, zk_pk_rec* pk) {
    const Layout& lay = pk->lay;
    const uint32_t n = lay.n, N = 4 * n, T = 1u << lay.lookup_bits;
    Dev d{c, pk};
    auto fail = [&](int code) { return code; };  // the caller destroys the key
    // ---- prover workspace
    for (uint32_t j = 0; j < lay.n_adv; j++) {
        pk->adv_val.push_back(d.alloc(n));
        pk->adv_poly.push_back(d.alloc(n));
        pk->adv_coset.push_back(d.alloc(N));
    }
    if (lay.n_inst) {
        pk->inst_val = d.alloc(n);
        pk->inst_poly = d.alloc(n);
        pk->inst_coset = d.alloc(N);
    }
    for (uint32_t ci = 0; ci < lay.n_chunks; ci++) {
        pk->z_val.push_back(d.alloc(n));
        pk->z_poly.push_back(d.alloc(n));
        pk->z_coset.push_back(d.alloc(N));
    }
    for (uint32_t l = 0; l < lay.n_lookups; l++) {
        pk->lk_in.push_back(lay.single ? d.alloc(n) : nullptr);
        pk->lk_ap.push_back(d.alloc(n));
        pk->lk_ap_poly.push_back(d.alloc(n));
        pk->lk_ap_coset.push_back(d.alloc(N));
        pk->lk_sp.push_back(d.alloc(n));
        pk->lk_sp_poly.push_back(d.alloc(n));
        pk->lk_sp_coset.push_back(d.alloc(N));
        pk->lk_z.push_back(d.alloc(n));
        pk->lk_z_poly.push_back(d.alloc(n));
        pk->lk_z_coset.push_back(d.alloc(N));
    }
    pk->random_poly = d.alloc(n);
    pk->h_ext = d.alloc(N);
    pk->h_comb = d.alloc(n);
    pk->t_num = d.alloc(n);
    pk->t_den = d.alloc(n);
    pk->t_frac = d.alloc(n);
    pk->t_a = d.alloc(n);
    pk->t_b = d.alloc(n);
    pk->t_small = d.alloc(n / 16 + 8192);
    pk->kd_scratch = d.alloc((size_t)KD_MAX_BATCH * kate_division_scratch(n));
    {
        const uint32_t nprod = lay.n_chunks + lay.n_lookups;
        for (uint32_t p = 0; p < nprod; p++) {
            pk->gp_num.push_back(d.alloc(n));
            pk->gp_den.push_back(d.alloc(n));
            pk->gp_loc_p.push_back(d.alloc(n));
            pk->gp_loc_r.push_back(d.alloc(n));
        }
        pk->gp_tot = d.alloc((size_t)2 * gp_blocks(n) * nprod);
        pk->gp_scal = d.alloc((size_t)4 * nprod);
        if (hipHostMalloc(&pk->gp_host, (size_t)2 * nprod * sizeof(Fr)) != hipSuccess ||
            hipMalloc(&pk->d_gp_items, nprod * sizeof(GpItem)) != hipSuccess)
            return fail(ZK_ENOMEM);
    }
    if (d.rc) return fail(d.rc);
    if (hipHostMalloc(&pk->tail_host, (pk->max_evals + 16) * sizeof(Fr)) != hipSuccess) return fail(ZK_ENOMEM);
    if (hipHostMalloc(&pk->rows_host, (size_t)ROWS_BLOCKS * ROWS_CAP * sizeof(RowEntry)) != hipSuccess ||
        hipMalloc(&pk->rows_dev, (size_t)ROWS_BLOCKS * ROWS_CAP * sizeof(RowEntry)) != hipSuccess)
        return fail(ZK_ENOMEM);
    if (hipHostMalloc(&pk->h_evargs, pk->max_evals * sizeof(EvalItem)) != hipSuccess ||
        hipMalloc(&pk->d_evargs, pk->max_evals * sizeof(EvalItem)) != hipSuccess)
        return fail(ZK_ENOMEM);
    pk->lc_cap = 2 * (pk->max_evals + 8);
    if (hipHostMalloc(&pk->h_lc_terms, pk->lc_cap * sizeof(LcTerm)) != hipSuccess ||
        hipMalloc(&pk->d_lc_terms, pk->lc_cap * sizeof(LcTerm)) != hipSuccess)
        return fail(ZK_ENOMEM);
    pk->ev_scratch = d.alloc((size_t)pk->max_evals * eval_blocks(n));
    pk->ev_out = d.alloc(pk->max_evals);
    if (d.rc) return fail(d.rc);
    {
        // per lookup: six arrays of T + 2 words and 3 x blocks block sums; one error flag for all
        const uint32_t stride = 6 * (T + 2) + 3 * (T / 1024 + 2);
        if (hipMalloc(&pk->lk_u32, ((size_t)stride * lay.n_lookups + 4) * 4) != hipSuccess) return fail(ZK_ENOMEM);
        uint32_t* b = pk->lk_u32;
        pk->lks.hist = b;
        pk->lks.present = b + (T + 2);
        pk->lks.absent = b + 2 * (T + 2);
        pk->lks.off = b + 3 * (T + 2);
        pk->lks.dex = b + 4 * (T + 2);
        pk->lks.aex = b + 5 * (T + 2);
        pk->lks.bsum = b + 6 * (T + 2);
        pk->lks.stride = stride;
        pk->lks.err = b + (size_t)stride * lay.n_lookups;
    }
    if (hipMalloc(&pk->d_qargs, sizeof(QuotientArgs)) != hipSuccess || hipHostMalloc(&pk->h_qargs, sizeof(QuotientArgs)) != hipSuccess)
        return fail(ZK_ENOMEM);
    {
        size_t bytes = (size_t)lay.n_chunks * sizeof(PermArgs);
        bytes = std::max(bytes, (size_t)lay.n_lookups * sizeof(LkNumDenArgs));
        bytes = std::max(bytes, (size_t)lay.n_adv * sizeof(CopyPair));
        pk->batch_args_bytes = bytes;
        if (hipMalloc(&pk->d_batch_args, bytes) != hipSuccess || hipHostMalloc(&pk->h_batch_args, bytes) != hipSuccess) return fail(ZK_ENOMEM);
    }
    return ZK_OK;
}

// a further workspace for the same key: the record is copied (the key half stays shared — nothing of it is in the copy's
// `dev` list), every workspace member is reset and allocated afresh
static zk_pk_rec* pk_make_member(zk_ctx* c, const zk_pk_rec* pk) {
    zk_pk_rec* m = new (std::nothrow) zk_pk_rec(*pk);
    if (!m) return nullptr;
    m->is_member = true;
    m->dev.clear();
    m->members.clear();
    m->bb = nullptr;
    m->wc = nullptr;
    m->pc = nullptr;
    for (auto* v : {&m->adv_val, &m->adv_poly, &m->adv_coset, &m->z_val, &m->z_poly, &m->z_coset, &m->lk_in, &m->lk_ap, &m->lk_ap_poly,
                    &m->lk_ap_coset, &m->lk_sp, &m->lk_sp_poly, &m->lk_sp_coset, &m->lk_z, &m->lk_z_poly, &m->lk_z_coset, &m->lk_in_coset,
                    &m->gp_num, &m->gp_den, &m->gp_loc_p, &m->gp_loc_r})
        v->clear();
    m->inst_val = m->inst_poly = m->inst_coset = nullptr;
    m->random_poly = m->h_ext = m->h_comb = m->t_num = m->t_den = m->t_frac = m->t_a = m->t_b = m->t_small = m->kd_scratch = nullptr;
    m->tail_host = nullptr;
    m->rows_host = m->rows_dev = nullptr;
    m->lk_u32 = nullptr;
    m->gp_tot = m->gp_scal = m->gp_host = nullptr;
    m->d_gp_items = nullptr;
    m->h_batch_args = m->d_batch_args = nullptr;
    m->d_qargs = m->h_qargs = nullptr;
    m->d_evargs = m->h_evargs = nullptr;
    m->d_lc_terms = m->h_lc_terms = nullptr;
    m->ev_scratch = m->ev_out = nullptr;
    m->lc_used = 0;
    if (pk_alloc_workspace(c, m) != ZK_OK) {
        pk_destroy(m);
        return nullptr;
    }
    return m;
}

int pk_ensure_batch(zk_ctx* c, zk_pk_rec* pk, uint32_t batch) {
    if (batch <= 1) return ZK_OK;
    const Layout& lay = pk->lay;
    const uint32_t n = lay.n, T = 1u << lay.lookup_bits, nprod = lay.n_chunks + lay.n_lookups;
    if ((pk->members.size() + 1 < batch || !pk->bb || pk->bb->cap < batch) && !c->poly_spare.empty()) ctx_release_spares(c);
    while (pk->members.size() + 1 < batch) {
        zk_pk_rec* m = pk_make_member(c, pk);
        if (!m) return ZK_ENOMEM;
        pk->members.push_back(m);
    }
    if (pk->bb && pk->bb->cap >= batch) return ZK_OK;
    aud_sync(c, c->stream);
    bb_destroy(pk->bb);
    pk->bb = nullptr;
    BatchBufs* bb = new (std::nothrow) BatchBufs();
    if (!bb) return ZK_ENOMEM;
    pk->bb = bb;  // (freed with the key whatever happens below)
    const size_t nl = (size_t)batch * lay.n_lookups, np = (size_t)batch * nprod, ne = (size_t)batch * pk->max_evals;
    const uint32_t stride = 6 * (T + 2) + 3 * (T / 1024 + 2);
    if (hipMalloc(&bb->lk_u32, ((size_t)stride * nl + 4) * 4) != hipSuccess || hipMalloc(&bb->d_gp_items, np * sizeof(GpItem)) != hipSuccess ||
        hipMalloc(&bb->gp_scal, 4 * np * sizeof(Fr)) != hipSuccess || hipHostMalloc(&bb->gp_host, 2 * np * sizeof(Fr)) != hipSuccess ||
        hipMalloc(&bb->d_evargs, ne * sizeof(EvalItem)) != hipSuccess || hipHostMalloc(&bb->h_evargs, ne * sizeof(EvalItem)) != hipSuccess ||
        hipMalloc(&bb->ev_scratch, ne * eval_blocks(n) * sizeof(Fr)) != hipSuccess || hipMalloc(&bb->ev_out, ne * sizeof(Fr)) != hipSuccess ||
        hipHostMalloc(&bb->tail_host, ne * sizeof(Fr)) != hipSuccess)
        return ZK_ENOMEM;
    uint32_t* b = bb->lk_u32;
    bb->lks.hist = b;
    bb->lks.present = b + (T + 2);
    bb->lks.absent = b + 2 * (T + 2);
    bb->lks.off = b + 3 * (T + 2);
    bb->lks.dex = b + 4 * (T + 2);
    bb->lks.aex = b + 5 * (T + 2);
    bb->lks.bsum = b + 6 * (T + 2);
    bb->lks.stride = stride;
    bb->lks.err = b + (size_t)stride * nl;
    bb->cap = batch;
    return ZK_OK;
}

int pk_ensure_multi(zk_ctx* c, zk_pk_rec* pk, uint32_t circuits) {
    if (int rc = pk_ensure_batch(c, pk, circuits)) return rc;
    const uint32_t want = 2 * (circuits * pk->max_evals + 8);  // every opened polynomial twice (pk_alloc_workspace), per circuit
    if (pk->lc_cap >= want) return ZK_OK;
    aud_sync(c, c->stream);  // (no proof is in flight between entry points; the lists are idle)
    if (pk->d_lc_terms) hipFree(pk->d_lc_terms);
    if (pk->h_lc_terms) hipHostFree(pk->h_lc_terms);
    pk->d_lc_terms = pk->h_lc_terms = nullptr;
    pk->lc_cap = 0;
    if (hipHostMalloc(&pk->h_lc_terms, want * sizeof(LcTerm)) != hipSuccess || hipMalloc(&pk->d_lc_terms, want * sizeof(LcTerm)) != hipSuccess)
        return ZK_ENOMEM;  // (what was allocated is freed with the key; lc_cap = 0 sends linear combinations down the chunked form)
    pk->lc_cap = want;
    return ZK_OK;
}

// ============================================================ instance column ==

int pk_instance_values(const Layout& lay, const uint64_t* instance_mont, size_t n_instance, std::vector<Fr>* out) {
    if ((n_instance && !instance_mont) || n_instance > (lay.n_inst ? lay.usable : 0u)) return ZK_EINVAL;
    out->resize(n_instance);
    if (n_instance) memcpy(out->data(), instance_mont, n_instance * sizeof(Fr));
    for (const Fr& v : *out)
        if (!v.below_modulus()) return ZK_EINVAL;  // a Montgomery image is < r
    return ZK_OK;
}

int pk_instance_lists(const Layout& lay, size_t count, const uint64_t* const* instances_mont, const size_t* n_instances,
                      std::vector<std::vector<Fr>>* out, std::vector<uint32_t>* same_as) {
    out->assign(count, {});
    if (same_as) {
        same_as->resize(count);
        for (size_t j = 0; j < count; j++) (*same_as)[j] = (uint32_t)j;
    }
    if (!n_instances) return lay.n_inst ? ZK_EINVAL : ZK_OK;
    std::unordered_map<const uint64_t*, uint32_t> first;  // a list's address -> the first list of the call that has it
    for (size_t j = 0; j < count; j++) {
        const uint64_t* src = n_instances[j] && instances_mont ? instances_mont[j] : nullptr;
        if (same_as && src) {
            auto it = first.find(src);
            if (it != first.end() && n_instances[it->second] == n_instances[j]) {
                (*same_as)[j] = it->second;
                continue;
            }
            first.emplace(src, (uint32_t)j);
        }
        if (int r = pk_instance_values(lay, src, n_instances[j], &(*out)[j])) return r;
    }
    return ZK_OK;
}

int pk_instance_upload(zk_ctx* c, hipStream_t st, zk_pk_rec* pk, const std::vector<Fr>& vals) {
    if (!pk->inst_val) return vals.empty() ? ZK_OK : ZK_EINVAL;
    if (vals.size() > pk->lay.usable) return ZK_EINVAL;
    if (c->audit.on) c->audit.op(st, {}, {pk->inst_val}, "instance column into the workspace");
    HIPCHK(c, hipMemsetAsync(pk->inst_val, 0, (size_t)pk->lay.n * sizeof(Fr), st));  // (the Montgomery image of zero is zero)
    if (!vals.empty()) HIPCHK(c, hipMemcpyAsync(pk->inst_val, vals.data(), vals.size() * sizeof(Fr), hipMemcpyHostToDevice, st));
    return ZK_OK;
}

int pk_instance_upload_lanes(zk_ctx* c, hipStream_t st, zk_pk_rec* pk, const std::vector<zk_pk_rec*>& ws, const std::vector<const std::vector<Fr>*>& lists) {
    BatchBufs* bb = pk->bb;
    const uint32_t B = (uint32_t)ws.size(), n = pk->lay.n;
    if (!bb || bb->cap < B || lists.size() != B) return ZK_EINTERNAL;
    size_t total = 0;
    for (uint32_t q = 0; q < B; q++) {
        if (!ws[q]->inst_val || lists[q]->size() > pk->lay.usable) return ZK_EINVAL;
        total += lists[q]->size();
    }
    const size_t head = (size_t)bb->cap * sizeof(InstEntry);  // (a multiple of 16 bytes: the values behind it stay aligned)
    if (!bb->inst_host || bb->inst_vals < total) {
        aud_sync(c, st);  // (an earlier call's upload has long been consumed; the buffers are idle)
        if (bb->inst_host) hipHostFree(bb->inst_host);
        if (bb->inst_dev) hipFree(bb->inst_dev);
        bb->inst_host = bb->inst_dev = nullptr;
        bb->inst_vals = 0;
        const size_t want = std::max<size_t>(total, 64);
        if (hipHostMalloc(&bb->inst_host, head + want * sizeof(Fr)) != hipSuccess || hipMalloc(&bb->inst_dev, head + want * sizeof(Fr)) != hipSuccess)
            return ZK_ENOMEM;  // (what was allocated is freed with the key)
        bb->inst_vals = want;
    }
    if (c->audit.on) c->audit.host_write(bb->inst_host, "instance columns: the host fills the staging");
    InstEntry* e = (InstEntry*)bb->inst_host;
    Fr* hv = (Fr*)((uint8_t*)bb->inst_host + head);
    uint32_t off = 0;
    for (uint32_t q = 0; q < B; q++) {
        const uint32_t len = (uint32_t)lists[q]->size();
        e[q] = InstEntry{ws[q]->inst_val, off, len};
        if (len) memcpy(hv + off, lists[q]->data(), (size_t)len * sizeof(Fr));
        off += len;
    }
    if (c->audit.on) {
        c->audit.op(st, {bb->inst_host}, {bb->inst_dev}, "instance columns: upload of the staging");
        std::vector<const void*> rd{bb->inst_dev}, wr;
        for (zk_pk_rec* m : ws) wr.push_back(m->inst_val);
        c->audit.op_v(st, rd.data(), rd.size(), wr.data(), wr.size(), "instance columns: one launch over the lanes");
    }
    HIPCHK(c, hipMemcpyAsync(bb->inst_dev, bb->inst_host, head + (size_t)total * sizeof(Fr), hipMemcpyHostToDevice, st));
    launch_instance_columns((const InstEntry*)bb->inst_dev, (const Fr*)((const uint8_t*)bb->inst_dev + head), B, n, st);
    HIPCHK(c, hipGetLastError());
    return ZK_OK;
}

ZK_API(zk_pk_num_instance_columns, (zk_ctx* c, zk_pk h, uint32_t* out), (c, h, out)) {
    if (!c || !out) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    *out = it->second->lay.n_inst;
    return ZK_OK;
}

// =================================================================== keygen ==

ZK_API(zk_keygen, (zk_ctx* c, const zk_circuit_params* params, const uint64_t* fixed_canonical, size_t n_fixed_columns, const uint32_t* copies, size_t n_copies, zk_pk* out), (c, params, fixed_canonical, n_fixed_columns, copies, n_copies, out)) {
    if (!c || !params || !fixed_canonical || !out || (n_copies && !copies)) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_bind(c);
    if (rc) return rc;
    ctx_release_spares(c);  // parked vectors are reclaimable: give them back before the key and its workspace are allocated
    Layout lay;
    if (params->num_advice > 1 && 2 * (uint64_t)params->num_idle_gate_columns > params->num_advice) return ZK_ELAYOUT;  // zkmi355.h: more never-enabled selectors than used ones
    if (!lay.init(*params)) return ZK_EINVAL;
    if (n_fixed_columns != lay.n_fix) return ZK_EINVAL;  // fixed_canonical holds n_fixed_columns x n x 4 limbs
    if (c->srs_k != (int)lay.k) return ZK_ESTATE;
    const uint32_t n = lay.n, N = 4 * n, T = 1u << lay.lookup_bits;
    // the lookup path is specialised to halo2-lib's range table: 0..T-1 then zeros
    {
        const uint64_t* tab = fixed_canonical + (size_t)lay.fx_table * n * 4;
        for (uint32_t r = 0; r < n; r++) {
            const uint64_t want = r < T ? r : 0;
            if (tab[4 * r] != want || tab[4 * r + 1] || tab[4 * r + 2] || tab[4 * r + 3]) return ZK_EINVAL;
        }
    }
    // the gate selectors must be what the key's closed-form layout assumes of them (pk.h layout_selectors_fit): 0 / 1 columns
    // that halo2's compress_selectors would leave one fixed column each
    if (!lay.single) {
        std::vector<std::vector<uint8_t>> bits(lay.A, std::vector<uint8_t>(n / 8, 0));
        for (uint32_t j = 0; j < lay.A; j++) {
            if (lay.fx_sel[j] == NO_SELECTOR) continue;
            const uint64_t* col = fixed_canonical + (size_t)lay.fx_sel[j] * n * 4;
            for (uint32_t r = 0; r < n; r++) {
                if (col[4 * r] > 1 || col[4 * r + 1] || col[4 * r + 2] || col[4 * r + 3]) return ZK_EINVAL;  // not a selector column
                if (col[4 * r]) bits[j][r >> 3] |= (uint8_t)(1u << (r & 7));
            }
        }
        if (!layout_selectors_fit(lay, bits)) return ZK_ELAYOUT;
    }
    const uint32_t m = (uint32_t)lay.perm_cols.size();
    for (size_t i = 0; i < n_copies; i++) {
        const uint32_t* e = copies + 4 * i;
        if (e[0] >= m || e[2] >= m || e[1] >= lay.usable || e[3] >= lay.usable) return ZK_EINVAL;
    }
    zk_pk_rec* pk = new (std::nothrow) zk_pk_rec();
    if (!pk) return ZK_ENOMEM;
    pk->lay = lay;
    pk->srs_gen = c->srs_gen;
    pk->max_evals = (uint32_t)(lay.advice_queries.size() + lay.n_fix + lay.perm_cols.size() + 3 * lay.n_chunks +
                               5 * lay.n_lookups + 16);
    Dev d{c, pk};
    hipStream_t st = c->stream;
    const Fr* tw = nullptr;
    const Fr* tw_ext = nullptr;
    if ((rc = ctx_get_twiddles(c, lay.k, &tw)) || (rc = ctx_get_twiddles(c, lay.ext_k, &tw_ext))) {
        pk_destroy(pk);
        return rc;
    }
    auto fail = [&](int code) {
        aud_sync(c, st);
        pk_destroy(pk);
        return code;
    };

    // ---- fixed columns: values -> commitment, coefficients, extended coset
    for (uint32_t f = 0; f < lay.n_fix; f++) {
        Fr *v = d.alloc(n), *p = d.alloc(n), *e = d.alloc(N);
        if (d.rc) return fail(d.rc);
        pk->fixed_val.push_back(v);
        pk->fixed_poly.push_back(p);
        pk->fixed_coset.push_back(e);
        hipMemcpyAsync(v, fixed_canonical + (size_t)f * n * 4, (size_t)n * sizeof(Fr), hipMemcpyHostToDevice, st);
        launch_to_mont(v, n, st);
    }
    // ---- permutation: halo2 permutation::keygen::Assembly (cycle merging), then sigma = delta^c' w^r'
    {
        std::vector<uint2> mapping((size_t)m * n), aux((size_t)m * n);
        std::vector<uint32_t> sizes((size_t)m * n, 1);
        for (uint32_t col = 0; col < m; col++)
            for (uint32_t r = 0; r < n; r++) mapping[(size_t)col * n + r] = aux[(size_t)col * n + r] = make_uint2(col, r);
        auto at = [&](uint2 p) { return (size_t)p.x * n + p.y; };
        auto same = [](uint2 a, uint2 b) { return a.x == b.x && a.y == b.y; };
        for (size_t i = 0; i < n_copies; i++) {
            uint2 l = make_uint2(copies[4 * i], copies[4 * i + 1]), r = make_uint2(copies[4 * i + 2], copies[4 * i + 3]);
            uint2 lc = aux[at(l)], rc2 = aux[at(r)];
            if (same(lc, rc2)) continue;
            if (sizes[at(lc)] < sizes[at(rc2)]) {
                std::swap(lc, rc2);
                std::swap(l, r);
            }
            sizes[at(lc)] += sizes[at(rc2)];
            uint2 it = rc2;
            for (;;) {
                aux[at(it)] = lc;
                it = mapping[at(it)];
                if (same(it, rc2)) break;
            }
            std::swap(mapping[at(l)], mapping[at(r)]);
        }
        std::vector<Fr> dpow(m);
        Fr dl = Fr::one();
        const Fr delta = fr_delta();
        for (uint32_t col = 0; col < m; col++) {
            dpow[col] = dl;
            dl = fe_mul(dl, delta);
        }
        uint2* d_map = nullptr;
        Fr* d_dpow = d.alloc(m);
        if (d.rc || hipMalloc(&d_map, (size_t)n * sizeof(uint2)) != hipSuccess) return fail(ZK_ENOMEM);
        hipMemcpyAsync(d_dpow, dpow.data(), m * sizeof(Fr), hipMemcpyHostToDevice, st);
        for (uint32_t col = 0; col < m; col++) {
            Fr *v = d.alloc(n), *p = d.alloc(n), *e = d.alloc(N);
            if (d.rc) {
                hipFree(d_map);
                return fail(d.rc);
            }
            pk->sigma_val.push_back(v);
            pk->sigma_poly.push_back(p);
            pk->sigma_coset.push_back(e);
            hipMemcpyAsync(d_map, &mapping[(size_t)col * n], (size_t)n * sizeof(uint2), hipMemcpyHostToDevice, st);
            hipLaunchKernelGGL(sigma_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d_map, tw, d_dpow, v, n);
            aud_sync(c, st);  // d_map is reused
        }
        hipFree(d_map);
    }
    // ---- commitments (vk) and polynomial forms (pk)
    auto finish_col = [&](Fr* v, Fr* p, Fr* e, G1Affine* cm) -> int {
        if (!commit(c, v, n, ZK_BASIS_LAGRANGE, cm)) return ZK_EHIP;
        hipMemcpyAsync(p, v, (size_t)n * sizeof(Fr), hipMemcpyDeviceToDevice, st);
        int r2 = ctx_ntt(c, p, n, p, lay.k, true, false, n);
        if (r2) return r2;
        return ctx_ntt(c, p, n, e, lay.ext_k, false, true, N);
    };
    pk->fixed_commit.resize(lay.n_fix);
    pk->perm_commit.resize(m);
    for (uint32_t f = 0; f < lay.n_fix; f++)
        if ((rc = finish_col(pk->fixed_val[f], pk->fixed_poly[f], pk->fixed_coset[f], &pk->fixed_commit[f]))) return fail(rc);
    for (uint32_t col = 0; col < m; col++)
        if ((rc = finish_col(pk->sigma_val[col], pk->sigma_poly[col], pk->sigma_coset[col], &pk->perm_commit[col]))) return fail(rc);
    // ---- l_0, l_last, l_active (= 1 - l_last - l_blind) cosets
    {
        std::vector<Fr> tmp(n, Fr::zero());
        Fr* scratch_n = d.alloc(n);
        pk->l0_coset = d.alloc(N);
        pk->l_last_coset = d.alloc(N);
        pk->l_active_coset = d.alloc(N);
        if (d.rc) return fail(d.rc);
        auto make = [&](Fr* dst) -> int {
            hipMemcpyAsync(scratch_n, tmp.data(), (size_t)n * sizeof(Fr), hipMemcpyHostToDevice, st);
            aud_sync(c, st);
            int r2 = ctx_ntt(c, scratch_n, n, scratch_n, lay.k, true, false, n);
            if (r2) return r2;
            return ctx_ntt(c, scratch_n, n, dst, lay.ext_k, false, true, N);
        };
        tmp[0] = Fr::one();
        if ((rc = make(pk->l0_coset))) return fail(rc);
        tmp[0] = Fr::zero();
        tmp[lay.usable] = Fr::one();  // row n - (bf + 1)
        if ((rc = make(pk->l_last_coset))) return fail(rc);
        for (uint32_t r = 0; r < n; r++) tmp[r] = r < lay.usable ? Fr::one() : Fr::zero();
        if ((rc = make(pk->l_active_coset))) return fail(rc);
    }
    pk->transcript_repr = pk_standin_transcript_repr(pk);
    if ((rc = pk_alloc_workspace(c, pk))) return fail(rc);
    if (aud_sync(c, st) != hipSuccess || hipGetLastError() != hipSuccess) return fail(ZK_EHIP);
    const uint64_t h = c->next_handle++;
    c->pks[h] = pk;
    *out = h;
    return ZK_OK;
}

ZK_API(zk_pk_free, (zk_ctx* c, zk_pk h), (c, h)) {
    if (!c) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    ctx_bind(c);
    aud_sync(c, c->stream);
    pk_destroy(it->second);
    c->pks.erase(it);
    return ZK_OK;
}

ZK_API(zk_vk_export, (zk_ctx* c, zk_pk h, uint64_t* fixed_commitments, uint64_t* perm_commitments, uint64_t transcript_repr[4], uint32_t counts[2]), (c, h, fixed_commitments, perm_commitments, transcript_repr, counts)) {
    if (!c) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    zk_pk_rec* pk = it->second;
    if (pk->srs_gen != c->srs_gen) return ZK_ESTATE;  // the SRS was replaced after this key was made
    if (counts) {
        counts[0] = (uint32_t)pk->fixed_commit.size();
        counts[1] = (uint32_t)pk->perm_commit.size();
    }
    if (fixed_commitments) memcpy(fixed_commitments, pk->fixed_commit.data(), pk->fixed_commit.size() * sizeof(G1Affine));
    if (perm_commitments) memcpy(perm_commitments, pk->perm_commit.data(), pk->perm_commit.size() * sizeof(G1Affine));
    if (transcript_repr) memcpy(transcript_repr, &pk->transcript_repr, 32);
    return ZK_OK;
}

int pk_ensure_cosets3(zk_ctx* c, zk_pk_rec* pk) {
    const Layout& lay = pk->lay;
    if (lay.n_h != 3) return ZK_EINVAL;
    auto to_members = [&]() {  // by-value copies of the record (pk_make_member): the key half is written through
        for (zk_pk_rec* m : pk->members) {
            m->fixed_c3 = pk->fixed_c3;
            m->sigma_c3 = pk->sigma_c3;
            m->l0_c3 = pk->l0_c3;
            m->l_last_c3 = pk->l_last_c3;
            m->l_active_c3 = pk->l_active_c3;
        }
    };
    if (pk->fixed_c3.size() == lay.n_fix && pk->l_active_c3) {
        to_members();
        return ZK_OK;
    }
    const size_t n = lay.n;
    Dev d{c, pk};
    std::vector<const Fr*> src;
    std::vector<Fr*> dst;
    auto add = [&](const Fr* s) {
        Fr* t = d.alloc(3 * n);
        src.push_back(s);
        dst.push_back(t);
        return t;
    };
    std::vector<Fr*> fx, sg;
    for (uint32_t f = 0; f < lay.n_fix; f++) fx.push_back(add(pk->fixed_coset[f]));
    for (size_t p = 0; p < lay.perm_cols.size(); p++) sg.push_back(add(pk->sigma_coset[p]));
    Fr *a0 = add(pk->l0_coset), *a1 = add(pk->l_last_coset), *a2 = add(pk->l_active_coset);
    if (d.rc) return d.rc;  // (what was allocated stays on the key's list and is freed with it)
    launch_coset3_relayout(src.data(), dst.data(), (uint32_t)src.size(), (uint32_t)n, c->stream);
    if (c->audit.on) {
        std::vector<const void*> rd(src.begin(), src.end()), wr(dst.begin(), dst.end());
        c->audit.op_v(c->stream, rd.data(), rd.size(), wr.data(), wr.size(), "key cosets -> coset-major");
    }
    pk->fixed_c3 = fx;
    pk->sigma_c3 = sg;
    pk->l0_c3 = a0;
    pk->l_last_c3 = a1;
    pk->l_active_c3 = a2;
    to_members();
    return ZK_OK;
}

// Evaluator::evaluate_h (+ divide_by_vanishing_poly when `divide`) over resident extended cosets: the key's fixed /
// sigma / l_* cosets and the caller's advice, permutation-product and lookup cosets.  Enqueued on the context stream.
int pk_quotient(zk_ctx* c, zk_pk_rec* pk, const QuotientCosets& qc, const Fr& beta, const Fr& gamma, const Fr& y, bool divide, Fr* out) {
    return pk_quotient_pass(c, pk, qc, beta, gamma, y, Fr::one(), false, divide, out);
}

int pk_quotient_pass(zk_ctx* c, zk_pk_rec* pk, const QuotientCosets& qc, const Fr& beta, const Fr& gamma, const Fr& y, const Fr& yscale,
                     bool accumulate, bool divide, Fr* out) {
    const Layout& lay = pk->lay;
    if (qc.adv.size() != lay.n_adv || qc.z.size() != lay.n_chunks || qc.lk_a.size() != lay.n_lookups ||
        qc.lk_s.size() != lay.n_lookups || qc.lk_z.size() != lay.n_lookups)
        return ZK_EINVAL;
    const Fr* xs = nullptr;
    int rc = ctx_get_coset_points(c, lay.ext_k, &xs);
    if (rc) return rc;
    QuotientArgs& q = *pk->h_qargs;  // pinned: the upload below does not stall the host (the previous use is complete)
    memset(&q, 0, sizeof(q) - sizeof(q.ypow));
    q.log_ext = lay.ext_k;
    q.n_gate = lay.n_gate;
    q.n_adv = lay.n_adv;
    q.n_chunks = lay.n_chunks;
    q.chunk_len = lay.chunk_len;
    q.n_perm = (uint32_t)lay.perm_cols.size();
    q.n_lookups = lay.n_lookups;
    q.single = lay.single ? 1 : 0;
    q.last_rot = lay.last_rot;
    q.fx_table = lay.fx_table;
    q.fx_qlookup = lay.fx_qlookup;
    for (uint32_t j = 0; j < lay.n_adv; j++) q.adv[j] = qc.adv[j];
    const bool c3 = qc.cosets3;
    if (c3 && (lay.n_h != 3 || pk->fixed_c3.size() != lay.n_fix)) return ZK_EINVAL;  // (pk_ensure_cosets3 first)
    for (uint32_t f = 0; f < lay.n_fix; f++) q.fix[f] = c3 ? pk->fixed_c3[f] : pk->fixed_coset[f];
    for (uint32_t j = 0; j < lay.n_gate; j++) q.fx_sel[j] = lay.gate_sel[j];
    for (uint32_t p = 0; p < q.n_perm; p++) {
        q.sigma[p] = c3 ? pk->sigma_c3[p] : pk->sigma_coset[p];
        const Col& col = lay.perm_cols[p];
        if (col.type == COL_INSTANCE && !qc.inst) return ZK_EINVAL;
        q.perm_val[p] = col.type == COL_FIXED ? q.fix[col.idx] : col.type == COL_INSTANCE ? qc.inst : qc.adv[col.idx];
    }
    for (uint32_t ci = 0; ci < lay.n_chunks; ci++) q.z[ci] = qc.z[ci];
    for (uint32_t l = 0; l < lay.n_lookups; l++) {
        q.lk_z[l] = qc.lk_z[l];
        q.lk_a[l] = qc.lk_a[l];
        q.lk_s[l] = qc.lk_s[l];
        q.lk_in[l] = lay.single ? nullptr : qc.adv[lay.n_gate + l];
    }
    q.l0 = c3 ? pk->l0_c3 : pk->l0_coset;
    q.l_last = c3 ? pk->l_last_c3 : pk->l_last_coset;
    q.l_active = c3 ? pk->l_active_c3 : pk->l_active_coset;
    q.xs = xs;
    // the kernel works in the carry-free field's internal form (x * 2^261): its constants are handed over times 32
    const Fr k32 = fr_from_u64(32);
    q.beta = fe_mul(beta, k32);
    q.gamma = fe_mul(gamma, k32);
    q.delta = fe_mul(fr_delta(), k32);
    // 1 / ((zeta w_ext^i)^n - 1): zeta^n * (w_ext^n)^i, w_ext^n is a primitive 4th root
    if (!pk->t_inv_ready) {  // constants of the key's domain: made once, not once per proof
        const Fr zn = fe_pow_u64(c->zeta, lay.n);
        const Fr w4 = fe_pow_u64(fr_omega(lay.ext_k), lay.n);
        Fr cur = zn;
        for (int i = 0; i < 4; i++) {
            pk->t_inv[i] = fe_inv_fast(fe_sub(cur, Fr::one()));
            cur = fe_mul(cur, w4);
        }
        pk->t_inv_ready = true;
    }
    // standard form: the product by it also converts the row back (quotient.hip); 1 = no division
    for (int i = 0; i < 4; i++) q.t_inv[i] = divide ? pk->t_inv[i] : Fr::one();
    q.divide = divide ? 1 : 0;
    q.n_terms = quotient_terms(lay.n_gate, lay.n_chunks, lay.n_lookups);
    if (q.n_terms > MAX_TERMS) return ZK_EINVAL;
    Fr yp = fe_mul(k32, yscale);  // (yscale = 1: the Montgomery product by one is exact, yp = 32)
    for (uint32_t j = q.n_terms; j-- > 0;) {  // ypow[j] = 32 yscale y^(T - 1 - j)
        q.ypow[j] = yp;
        yp = fe_mul(yp, y);
    }
    q.out = out;
    const uint32_t log_slices = quotient_log_slices(lay.ext_k, lay.n_gate);
    if (log_slices) {
        const Fr dstep = fe_pow_u64(fr_delta(), lay.chunk_len);
        Fr dc = k32;
        for (uint32_t ci = 0; ci < lay.n_chunks; ci++) {
            q.delta_chunk[ci] = dc;
            dc = fe_mul(dc, dstep);
        }
    }
    hipStream_t st = c->stream;
    hipEventRecord(c->ev[ZK_T_QUOTIENT][0], st);
    const size_t bytes = sizeof(q) - sizeof(q.ypow) + (size_t)q.n_terms * sizeof(Fr);
    if (hipMemcpyAsync(pk->d_qargs, &q, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return ZK_EHIP;
    if (accumulate) launch_quotient_acc_dev(pk->d_qargs, lay.ext_k, log_slices, st, c3);
    else launch_quotient_dev(pk->d_qargs, lay.ext_k, log_slices, st, c3);
    hipEventRecord(c->ev[ZK_T_QUOTIENT][1], st);
    c->ev_valid[ZK_T_QUOTIENT] = true;
    return ZK_OK;
}

ZK_API(zk_pk_shape, (zk_ctx* c, zk_pk h, uint32_t out[8]), (c, h, out)) {
    if (!c || !out) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    const Layout& lay = it->second->lay;
    const uint32_t v[8] = {lay.k, lay.ext_k, lay.n_adv, lay.n_fix, (uint32_t)lay.perm_cols.size(), lay.n_chunks, lay.n_lookups, lay.n_h};
    memcpy(out, v, sizeof(v));
    return ZK_OK;
}

// zk_quotient and zk_quotient_multi: n_circuits passes into ONE h — circuit 0 the plain kernel, circuits 1 .. N - 1 the
// accumulating one, each with its own powers of y (prover_lockstep.h's chain: pass q carries y^(T (N - 1 - q))).  `with_instance`
// false: the key must have no instance column (zk_quotient); true: instance_ext holds one coset per circuit for a key with the
// column and is null for a key without
static int quotient_passes(zk_ctx* c, zk_pk h, size_t n_circuits, const zk_poly* advice_ext, size_t n_advice, bool with_instance,
                           const zk_poly* instance_ext, const zk_poly* perm_z_ext, size_t n_chunks, const zk_poly* lookup_ext, size_t n_lookups,
                           const uint64_t beta[4], const uint64_t gamma[4], const uint64_t y[4], int divide, zk_poly out_ext) {
    if (!c || !advice_ext || !perm_z_ext || !lookup_ext || !beta || !gamma || !y) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    zk_pk_rec* pk = it->second;
    const Layout& lay = pk->lay;
    if (pk->srs_gen != c->srs_gen || pk->verify_only) return ZK_ESTATE;
    if (n_circuits == 0 || n_circuits > ZK_PROVE_MULTI_MAX) return ZK_EINVAL;
    if (n_advice != lay.n_adv || n_chunks != lay.n_chunks || n_lookups != lay.n_lookups) return ZK_EINVAL;
    if (lay.n_inst && !with_instance) return ZK_EINVAL;  // (zk_quotient carries no instance column)
    if (with_instance && (instance_ext != nullptr) != (lay.n_inst != 0)) return ZK_EINVAL;  // (the whole-proof rule: InvalidInstances)
    const size_t N = (size_t)4 * lay.n;
    auto ext = [&](zk_poly p) -> Fr* {
        const PolyRec* q = ctx_poly(c, p);
        return (!q || q->n != N) ? nullptr : q->ptr;
    };
    Fr* out = ext(out_ext);
    if (!out) return ZK_EINVAL;
    std::vector<QuotientCosets> qcs(n_circuits);
    for (size_t q = 0; q < n_circuits; q++) {
        QuotientCosets& qc = qcs[q];
        for (size_t j = 0; j < n_advice; j++) qc.adv.push_back(ext(advice_ext[q * n_advice + j]));
        for (size_t j = 0; j < n_chunks; j++) qc.z.push_back(ext(perm_z_ext[q * n_chunks + j]));
        for (size_t l = 0; l < n_lookups; l++) {
            const zk_poly* t = lookup_ext + 3 * (q * n_lookups + l);
            qc.lk_a.push_back(ext(t[0]));
            qc.lk_s.push_back(ext(t[1]));
            qc.lk_z.push_back(ext(t[2]));
        }
        if (lay.n_inst) {
            qc.inst = ext(instance_ext[q]);
            if (!qc.inst || qc.inst == out) return ZK_EINVAL;
        }
        for (auto* v : {&qc.adv, &qc.z, &qc.lk_a, &qc.lk_s, &qc.lk_z})
            for (const Fr* p : *v)
                if (!p || p == out) return ZK_EINVAL;
    }
    Fr b, g, yy;
    memcpy(&b, beta, 32);
    memcpy(&g, gamma, 32);
    memcpy(&yy, y, 32);
    int rc = ctx_bind(c);
    if (rc) return rc;
    std::vector<Fr> scale(n_circuits);
    scale[n_circuits - 1] = Fr::one();
    if (n_circuits > 1) {
        const Fr yT = fe_pow_u64(yy, quotient_terms(lay.n_gate, lay.n_chunks, lay.n_lookups));
        for (size_t q = n_circuits - 1; q-- > 0;) scale[q] = fe_mul(scale[q + 1], yT);
    }
    for (size_t q = 0; q < n_circuits; q++) {
        if ((rc = pk_quotient_pass(c, pk, qcs[q], b, g, yy, scale[q], q > 0, divide != 0, out))) return rc;
        HIPCHK(c, aud_sync(c, c->stream));  // the argument block is reused by the next pass and the next call
    }
    return ZK_OK;
}

ZK_API(zk_quotient, (zk_ctx* c, zk_pk h, const zk_poly* advice_ext, size_t n_advice, const zk_poly* perm_z_ext, size_t n_chunks, const zk_poly* lookup_ext, size_t n_lookups, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t y[4], int divide, zk_poly out_ext), (c, h, advice_ext, n_advice, perm_z_ext, n_chunks, lookup_ext, n_lookups, beta, gamma, y, divide, out_ext)) {
    return quotient_passes(c, h, 1, advice_ext, n_advice, false, nullptr, perm_z_ext, n_chunks, lookup_ext, n_lookups, beta, gamma, y, divide, out_ext);
}

ZK_API(zk_quotient_multi, (zk_ctx* c, zk_pk h, size_t n_circuits, const zk_poly* advice_ext, size_t n_advice, const zk_poly* instance_ext, const zk_poly* perm_z_ext, size_t n_chunks, const zk_poly* lookup_ext, size_t n_lookups, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t y[4], int divide, zk_poly out_ext), (c, h, n_circuits, advice_ext, n_advice, instance_ext, perm_z_ext, n_chunks, lookup_ext, n_lookups, beta, gamma, y, divide, out_ext)) {
    return quotient_passes(c, h, n_circuits, advice_ext, n_advice, true, instance_ext, perm_z_ext, n_chunks, lookup_ext, n_lookups, beta, gamma, y, divide, out_ext);
}

ZK_API(zk_pk_set_transcript_repr, (zk_ctx* c, zk_pk h, const uint64_t transcript_repr[4]), (c, h, transcript_repr)) {
    if (!c || !transcript_repr) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    Fr v;
    memcpy(&v, transcript_repr, 32);
    if (!v.below_modulus()) return ZK_EINVAL;  // a Montgomery image is < r
    it->second->transcript_repr = v;
    // the lock-step members are by-value copies of the record (pk_make_member): every key-half field that can change after
    // they were made has to be written through to them, or proofs j > 0 of the next batch would hash the stale value
    for (zk_pk_rec* m : it->second->members) m->transcript_repr = v;
    return ZK_OK;
}
