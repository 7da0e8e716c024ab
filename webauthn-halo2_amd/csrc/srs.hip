// srs.hip — the resident SRS of a context: its block, its window tables, and zk_srs_setup / load / export (reading and
// writing SRS files: serde.hip; downsize, check and update: g1_ntt.hip).
#include <vector>

#include "ctx.h"

// window-multiple tables of both bases for the fixed-base MSM (k >= 10; smaller SRS use the generic path)
int srs_build_tables(zk_ctx* c, uint32_t k) {
    if (k < 10) return ZK_OK;
    const uint32_t n = 1u << k;
    const uint32_t cw = msm_auto_window(n, c->opt_msm_window);
    const size_t cnt = (size_t)nwin_for(cw) * n;
    if (hipMalloc(&c->srs->g_table, cnt * sizeof(G1Affine)) != hipSuccess ||
        hipMalloc(&c->srs->g_lagrange_table, cnt * sizeof(G1Affine)) != hipSuccess)
        return ZK_ENOMEM;
    c->g_table = c->srs->g_table;
    c->g_lagrange_table = c->srs->g_lagrange_table;
    hipError_t e = msm_build_table(c->g, n, cw, c->g_table, c->stream);
    if (e == hipSuccess) e = msm_build_table(c->g_lagrange, n, cw, c->g_lagrange_table, c->stream);
    if (e == hipSuccess) e = msm_bases_have_identity(c->g, n, c->stream, (uint32_t*)c->small, (uint32_t*)c->host_small, &c->g_has_identity);
    if (e == hipSuccess)
        e = msm_bases_have_identity(c->g_lagrange, n, c->stream, (uint32_t*)c->small, (uint32_t*)c->host_small, &c->g_lagrange_has_identity);
    if (e == hipSuccess) e = aud_sync(c, c->stream);
    if (e != hipSuccess) {
        c->last_hip = (int)e;
        return ZK_EHIP;
    }
    c->table_c = cw;
    return ZK_OK;
}

// a fresh, empty block for this context (the previous one is released: freed unless another context still shares it)
static void srs_new_block(zk_ctx* c) {
    c->g2_valid = false;
    c->pair_lines.reset();  // the device pairing's table of the old pair (srs_install puts it back with the old view on failure)
    c->srs_gen++;  // proving keys made under the previous SRS are refused from now on (ZK_ESTATE)
    c->srs = std::make_shared<SrsBlock>();
    c->srs->device = c->device;
    c->g = c->g_lagrange = c->g_table = c->g_lagrange_table = nullptr;
    c->table_c = 0;
    c->srs_k = -1;
}

void srs_adopt(zk_ctx* c, uint32_t k, G1Affine* g, G1Affine* g_lagrange) {
    (void)k;
    srs_new_block(c);
    c->g = c->srs->g = g;
    c->g_lagrange = c->srs->g_lagrange = g_lagrange;
}

// zk_srs_downsize / zk_srs_read_downsize: the two bases become the resident SRS in a NEW block (contexts sharing the old one
// keep it, and their keys), with their window tables; g2 / s_g2 stay as they are.  Until the tables are built the previous SRS
// is kept aside: on failure it is put back, with its tables and its keys, and the two buffers are freed.
int srs_install(zk_ctx* c, uint32_t k, G1Affine* g, G1Affine* g_lagrange) {
    const SrsView old = *c;
    const uint64_t old_gen = c->srs_gen;
    srs_adopt(c, k, g, g_lagrange);
    c->g2_valid = old.g2_valid;
    const int rc = srs_build_tables(c, k);
    if (rc != ZK_OK) {
        static_cast<SrsView&>(*c) = old;  // (the new block goes: it frees both bases and any table built)
        c->srs_gen = old_gen;
        return rc;
    }
    c->srs_k = (int)k;
    return ZK_OK;
}

int srs_alloc(zk_ctx* c, uint32_t k) {
    if (k < 1 || k > 24) return ZK_EINVAL;
    const size_t n = (size_t)1 << k;
    srs_new_block(c);
    if (hipMalloc(&c->srs->g, n * sizeof(G1Affine)) != hipSuccess || hipMalloc(&c->srs->g_lagrange, n * sizeof(G1Affine)) != hipSuccess)
        return ZK_ENOMEM;
    c->g = c->srs->g;
    c->g_lagrange = c->srs->g_lagrange;
    return ZK_OK;
}

ZK_API(zk_srs_setup, (zk_ctx* c, uint32_t k, const uint8_t seed[32]), (c, k, seed)) {
    if (!c || !seed) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_bind(c);
    if (rc) return rc;
    ctx_release_spares(c);  // parked vectors are reclaimable: give them back before the big allocations
    if ((rc = srs_alloc(c, k)) != ZK_OK) return rc;
    const uint32_t n = 1u << k;
    ChaCha20Rng rng(seed);
    const Fr s = rng.next_fr();
    // window-8 table of the generator on the host: table[w*256 + d] = [d * 256^w] G1
    std::vector<G1Affine> table(32 * 256);
    {
        std::vector<G1X> acc(32 * 256);
        G1X base;
        base.x = Fq::one();
        base.y = fe_add(Fq::one(), Fq::one());
        base.zz = Fq::one();
        base.zzz = Fq::one();
        for (int w = 0; w < 32; w++) {
            G1X cur = G1X::identity();
            acc[w * 256] = cur;
            for (int d = 1; d < 256; d++) {
                g1x_add(cur, base);
                acc[w * 256 + d] = cur;
            }
            g1x_add(cur, base);
            base = cur;
        }
        // batch normalisation: invert all ZZZ at once
        std::vector<Fq> pref(acc.size() + 1);
        pref[0] = Fq::one();
        for (size_t i = 0; i < acc.size(); i++) pref[i + 1] = acc[i].is_identity() ? pref[i] : fe_mul(pref[i], acc[i].zzz);
        Fq inv = fe_inv(pref[acc.size()]);
        for (size_t i = acc.size(); i-- > 0;) {
            if (acc[i].is_identity()) {
                table[i].x = Fq::zero();
                table[i].y = Fq::zero();
                continue;
            }
            const Fq t = fe_mul(inv, pref[i]);
            inv = fe_mul(inv, acc[i].zzz);
            const Fq u = fe_mul(acc[i].zz, t);
            table[i].x = fe_mul(acc[i].x, fe_sqr(u));
            table[i].y = fe_mul(acc[i].y, t);
        }
    }
    G1Affine* d_table = nullptr;
    Fr* d_sc = nullptr;
    if (hipMalloc(&d_table, table.size() * sizeof(G1Affine)) != hipSuccess || hipMalloc(&d_sc, (size_t)n * sizeof(Fr)) != hipSuccess) {
        hipFree(d_table);
        return ZK_ENOMEM;
    }
    rc = ZK_OK;
    const Fr* tw = nullptr;
    if (hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(G1Affine), hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = ZK_EHIP;
    if (rc == ZK_OK) rc = ctx_get_twiddles(c, k, &tw);
    if (rc == ZK_OK) {
        // g[i] = [s^i] G
        launch_twiddles(d_sc, s, n, c->stream);
        launch_srs_fixed_base(d_sc, n, d_table, c->g, c->stream);
        // g_lagrange[i] = [L_i(s)] G,  L_i(s) = w^i (s^n - 1) / (n (s - w^i))
        Fr sn = s;
        for (uint32_t i = 0; i < k; i++) sn = fe_sqr(sn);
        const Fr cst = fe_mul(fe_sub(sn, Fr::one()), fe_inv(fr_from_u64(n)));
        launch_srs_lagrange_scalars(tw, n, s, cst, d_sc, c->stream);
        launch_srs_fixed_base(d_sc, n, d_table, c->g_lagrange, c->stream);
        hipError_t e = aud_sync(c, c->stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) {
            c->last_hip = (int)e;
            rc = ZK_EHIP;
        }
    }
    hipFree(d_table);
    hipFree(d_sc);
    if (rc == ZK_OK) rc = srs_build_tables(c, k);
    if (rc == ZK_OK) {
        srs_set_g2_from_secret(c, s);  // g2 = G2 generator, s_g2 = [s]G2 (host side: it only travels through zk_srs_write)
        c->srs_k = (int)k;
    }
    return rc;
}

ZK_API(zk_srs_load, (zk_ctx* c, uint32_t k, const uint64_t* g, const uint64_t* gl), (c, k, g, gl)) {
    if (!c || !g || !gl) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_bind(c);
    if (rc) return rc;
    ctx_release_spares(c);
    if ((rc = srs_alloc(c, k)) != ZK_OK) return rc;
    const size_t bytes = ((size_t)1 << k) * sizeof(G1Affine);
    HIPCHK(c, hipMemcpy(c->g, g, bytes, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->g_lagrange, gl, bytes, hipMemcpyHostToDevice));
    if ((rc = srs_build_tables(c, k)) != ZK_OK) return rc;
    c->srs_k = (int)k;
    return ZK_OK;
}

ZK_API(zk_srs_export, (zk_ctx* c, int basis, uint64_t* out, size_t first, size_t count), (c, basis, out, first, count)) {
    if (!c || !out) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->srs_k < 0) return ZK_ESTATE;
    const size_t n = (size_t)1 << c->srs_k;
    if (first > n || count > n - first) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    const G1Affine* src = ctx_basis(c, basis);
    if (!src) src = c->g;  // (any value but ZK_BASIS_LAGRANGE has always meant the monomial basis here)
    HIPCHK(c, hipMemcpy(out, src + first, count * sizeof(G1Affine), hipMemcpyDeviceToHost));
    return ZK_OK;
}

int zk_srs_k(const zk_ctx* c) { return c ? c->srs_k : -1; }

ZK_API(zk_srs_msm_plan, (const zk_ctx* c, uint32_t* window_bits, uint32_t* windows), (c, window_bits, windows)) {
    if (!c || !window_bits || !windows) return ZK_EINVAL;
    if (c->srs_k < 0) return ZK_ESTATE;
    *window_bits = c->table_c;  // 0: no window-multiple tables (k < 10), zk_commit takes the generic path
    *windows = c->table_c ? nwin_for(c->table_c) : 0;
    return ZK_OK;
}
