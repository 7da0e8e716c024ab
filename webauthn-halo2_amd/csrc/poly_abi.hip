// poly_abi.hip — the resident-polynomial ABI: vectors on the device behind handles, the NTT drivers with the three-coset
// route, and the entry points that transform, evaluate or divide a resident vector.
#include <algorithm>
#include <map>

#include "ctx.h"
#include "prover.h"

// ---- resident polynomials ----------------------------------------------------

// Vectors parked by zk_poly_free (up to POLY_SPARE_BYTES per context) are reclaimable memory: the large allocators
// (zk_keygen, zk_srs_setup / load / read, zk_pk_read, the MSM workspaces) release them up front instead of failing with
// ZK_ENOMEM while they sit idle.  Caller holds c->mu and has bound the device.
void ctx_release_spares(zk_ctx* c) {
    for (auto& r : c->poly_spare) hipFree(r.ptr);
    c->poly_spare.clear();
    c->poly_spare_bytes = 0;
}

ZK_API(zk_poly_alloc, (zk_ctx* c, size_t n, zk_poly* out), (c, n, out)) {
    if (!c || !out || n == 0) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_bind(c);
    if (rc) return rc;
    Fr* p = nullptr;
    for (size_t i = 0; i < c->poly_spare.size(); i++)
        if (c->poly_spare[i].n == n) {  // a vector of this length given back earlier (contents undefined, as hipMalloc's)
            p = c->poly_spare[i].ptr;
            c->poly_spare_bytes -= n * sizeof(Fr);
            c->poly_spare.erase(c->poly_spare.begin() + i);
            break;
        }
    if (!p && hipMalloc(&p, n * sizeof(Fr)) != hipSuccess) {
        // out of memory with vectors parked: let them go and try once more
        ctx_release_spares(c);
        (void)hipGetLastError();
        if (hipMalloc(&p, n * sizeof(Fr)) != hipSuccess) return ZK_ENOMEM;
    }
    const uint64_t h = c->next_handle++;
    c->polys[h] = PolyRec{p, n};
    *out = h;
    return ZK_OK;
}

ZK_API(zk_poly_free, (zk_ctx* c, zk_poly h), (c, h)) {
    if (!c) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    PolyRec* r = ctx_poly(c, h);
    if (!r) return ZK_EINVAL;
    ctx_bind(c);
    aud_sync(c, c->stream);  // nothing of this context still uses it
    const size_t bytes = r->n * sizeof(Fr);
    if (c->poly_spare.size() < zk_ctx::POLY_SPARE_MAX && c->poly_spare_bytes + bytes <= zk_ctx::POLY_SPARE_BYTES) {
        c->poly_spare.push_back(*r);
        c->poly_spare_bytes += bytes;
    } else {
        hipFree(r->ptr);
    }
    c->polys.erase(h);
    return ZK_OK;
}

// Handing a resident vector from one context to another of the same device, without a copy and without either context
// waiting on the other's lock: the owner detaches it (the record leaves the context for a process-wide table), the new owner
// attaches it.  A loader context (its own stream and host thread, e.g. one made with zk_ctx_create_shared) can thus upload
// and convert the next request's advice columns while the proving context is inside zk_prove, and the prover's thread picks
// them up between two proofs.
namespace {
struct Detached {
    PolyRec rec;
    int device;
};
std::mutex g_detached_mu;
std::map<uint64_t, Detached> g_detached;
uint64_t g_detached_next = 1;
}  // namespace

ZK_API(zk_poly_detach, (zk_ctx* c, zk_poly h, uint64_t* token), (c, h, token)) {
    if (!c || !token) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    PolyRec* r = ctx_poly(c, h);
    if (!r) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    HIPCHK(c, aud_sync(c, c->stream));  // whatever this context still does with the vector finishes first
    const Detached d{*r, c->device};
    c->polys.erase(h);
    std::lock_guard<std::mutex> lg(g_detached_mu);
    *token = g_detached_next++;
    g_detached[*token] = d;
    return ZK_OK;
}

ZK_API(zk_poly_attach, (zk_ctx* c, uint64_t token, zk_poly* out), (c, token, out)) {
    if (!c || !out) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    Detached d;
    {
        std::lock_guard<std::mutex> lg(g_detached_mu);
        auto it = g_detached.find(token);
        if (it == g_detached.end() || it->second.device != c->device) return ZK_EINVAL;
        d = it->second;
        g_detached.erase(it);
    }
    const uint64_t nh = c->next_handle++;
    c->polys[nh] = d.rec;
    *out = nh;
    return ZK_OK;
}

// A detached vector that will never be attached (the loader failed between stage and adopt, the target context is gone):
// without this the record — and its device memory — would stay in the process-wide table for the life of the process.
ZK_API(zk_poly_discard, (uint64_t token), (token)) {
    Detached d;
    {
        std::lock_guard<std::mutex> lg(g_detached_mu);
        auto it = g_detached.find(token);
        if (it == g_detached.end()) return ZK_EINVAL;
        d = it->second;
        g_detached.erase(it);
    }
    DeviceScope dev(d.device);
    if (!dev.ok) return ZK_EHIP;
    return hipFree(d.rec.ptr) == hipSuccess ? ZK_OK : ZK_EHIP;  // hipFree waits for the device: nothing still uses the vector
}

ZK_API(zk_poly_len, (zk_ctx* c, zk_poly h, size_t* out), (c, h, out)) {
    if (!c || !out) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    PolyRec* r = ctx_poly(c, h);
    if (!r) return ZK_EINVAL;
    *out = r->n;
    return ZK_OK;
}

ZK_API(zk_poly_upload, (zk_ctx* c, zk_poly h, const uint64_t* host, size_t n), (c, h, host, n)) {
    if (!c || !host) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    PolyRec* r = ctx_poly(c, h);
    if (!r || n > r->n) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(r->ptr, host, n * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
    if (n < r->n) HIPCHK(c, hipMemsetAsync(r->ptr + n, 0, (r->n - n) * sizeof(Fr), c->stream));
    HIPCHK(c, aud_sync(c, c->stream));
    return ZK_OK;
}

ZK_API(zk_poly_download, (zk_ctx* c, zk_poly h, uint64_t* host, size_t n), (c, h, host, n)) {
    if (!c || !host) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    PolyRec* r = ctx_poly(c, h);
    if (!r || n > r->n) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(host, r->ptr, n * sizeof(Fr), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, aud_sync(c, c->stream));
    return ZK_OK;
}

// rows [first, first + count) of a resident vector from the host (Montgomery images): the blinding rows a host appends to a
// column the device made (a', s', z), without shipping the column
ZK_API(zk_poly_upload_range, (zk_ctx* c, zk_poly h, size_t first, const uint64_t* host, size_t count), (c, h, first, host, count)) {
    if (!c || (!host && count)) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    PolyRec* r = ctx_poly(c, h);
    if (!r || first > r->n || count > r->n - first) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    if (count == 0) return ZK_OK;
    HIPCHK(c, hipMemcpyAsync(r->ptr + first, host, count * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, aud_sync(c, c->stream));
    return ZK_OK;
}

// dst[dst_first ..] = src[src_first .. src_first + count): e.g. the h pieces, n-coefficient slices of the quotient
ZK_API(zk_poly_copy_range, (zk_ctx* c, zk_poly dst, size_t dst_first, zk_poly src, size_t src_first, size_t count), (c, dst, dst_first, src, src_first, count)) {
    if (!c) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    PolyRec *d = ctx_poly(c, dst), *s = ctx_poly(c, src);
    if (!d || !s || dst_first > d->n || count > d->n - dst_first || src_first > s->n || count > s->n - src_first) return ZK_EINVAL;
    if (d == s && !(dst_first + count <= src_first || src_first + count <= dst_first)) return ZK_EINVAL;  // overlapping ranges
    int rc = ctx_bind(c);
    if (rc) return rc;
    if (count == 0) return ZK_OK;
    HIPCHK(c, hipMemcpyAsync(d->ptr + dst_first, s->ptr + src_first, count * sizeof(Fr), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, aud_sync(c, c->stream));
    return ZK_OK;
}

ZK_API(zk_poly_copy, (zk_ctx* c, zk_poly dst, zk_poly src), (c, dst, src)) {
    if (!c) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    PolyRec *d = ctx_poly(c, dst), *s = ctx_poly(c, src);
    if (!d || !s || d->n < s->n) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(d->ptr, s->ptr, s->n * sizeof(Fr), hipMemcpyDeviceToDevice, c->stream));
    if (d->n > s->n) HIPCHK(c, hipMemsetAsync(d->ptr + s->n, 0, (d->n - s->n) * sizeof(Fr), c->stream));
    return ZK_OK;
}

// ---- NTT drivers -------------------------------------------------------------
// the fields every job of this file fills alike
static NttJob ntt_job(const zk_ctx* c, Fr* tmp, const Fr* tw, uint32_t log_n, size_t n_in, size_t n_out) {
    NttJob job;
    memset(&job, 0, sizeof(job));
    job.tmp = tmp;
    job.tw = tw;
    job.log_n = log_n;
    job.n_in = (uint32_t)n_in;
    job.n_out = (uint32_t)n_out;
    job.max_log_r = c->opt_ntt_max_r;
    return job;
}
static void ntt_job_coset_pre(NttJob& job, const zk_ctx* c) {  // a_i *= zeta^(i mod 3)
    job.has_pre = 1;
    job.pre[0] = Fr::one();
    job.pre[1] = c->zeta;
    job.pre[2] = c->zeta2;
}
// the ledger's twin of a batched job: reads the sources, writes the destinations, ping-pongs through the context's ONE scratch
static void ntt_audit(zk_ctx* c, hipStream_t st, const Fr* const* srcs, Fr* const* dsts, uint32_t count, const char* what) {
    if (!c->audit.on) return;
    const void *rd[NTT_MAX_BATCH + 1], *wr[NTT_MAX_BATCH + 1];
    for (uint32_t b = 0; b < count; b++) {
        rd[b] = srcs[b];
        wr[b] = dsts[b];
    }
    rd[count] = wr[count] = c->scratch;
    c->audit.op_v(st, rd, count + 1, wr, count + 1, what);
}
// enqueues the job on `st` between the events of the NTT timer
static int ctx_ntt_launch(zk_ctx* c, const NttJob& job, hipStream_t st) {
    aud_record(c, c->ev[ZK_T_NTT][0], st);
    const hipError_t e = ntt_run(job, st);
    aud_record(c, c->ev[ZK_T_NTT][1], st);
    c->ev_valid[ZK_T_NTT] = true;
    if (e != hipSuccess) {
        c->last_hip = (int)e;
        return ZK_EHIP;
    }
    return ZK_OK;
}

int ctx_ntt(zk_ctx* c, const Fr* src, size_t src_n, Fr* dst, uint32_t log_n, bool inverse, bool coset, size_t n_out) {
    return ctx_ntt_batch(c, &src, src_n, &dst, 1, log_n, inverse, coset, n_out);
}

uint32_t ctx_ntt_max_batch(uint32_t log_n) {
    // scratch for the ping-pong is batch x 2^log_n elements: keep it within 2^23 (256 MiB)
    const uint32_t cap = log_n >= 23 ? 1u : 1u << (23 - log_n);
    return cap < NTT_MAX_BATCH ? cap : NTT_MAX_BATCH;
}

int ctx_ntt_batch(zk_ctx* c, const Fr* const* srcs, size_t src_n, Fr* const* dsts, uint32_t batch, uint32_t log_n, bool inverse,
                  bool coset, size_t n_out, hipStream_t on) {
    const hipStream_t st = on ? on : c->stream;
    const size_t N = (size_t)1 << log_n;
    if (batch == 0 || batch > ctx_ntt_max_batch(log_n)) return ZK_EINVAL;
    int rc = ctx_ensure_scratch(c, N * batch);
    if (rc) return rc;
    const Fr* tw;
    if ((rc = ctx_get_twiddles_ntt(c, log_n, &tw)) != ZK_OK) return rc;
    NttJob job = ntt_job(c, c->scratch, tw, log_n, src_n < N ? src_n : N, n_out);
    job.batch = batch;
    for (uint32_t b = 0; b < batch; b++) {
        job.srcs[b] = srcs[b];
        job.dsts[b] = dsts[b];
    }
    job.inverse = inverse ? 1 : 0;
    if (log_n > 7) {
        // two or more passes: the last one folds the conversion to the standard form (and the 1/N of a plain inverse
        // transform) into its inter-pass twiddles, read from a standard-form table (ntt.hip NTT_FOLD)
        if (!inverse) rc = ctx_get_twiddles(c, log_n, &job.tw_last);
        else if (!coset) {
            rc = ctx_get_twiddles_ninv(c, log_n, &job.tw_last);
            job.tw_last_has_post = 1;
        }
        if (rc) return rc;
    }
    if (!inverse && coset) ntt_job_coset_pre(job, c);  // coeff_to_extended
    if (inverse) {  // x 1/N, and for the coset also zeta^-(i mod 3) = {1, zeta^2, zeta}
        // 1 / N: a constant of the transform size, inverted once per context (19 us of Fermat on the launching thread per
        // inverse transform before)
        auto nit = c->ninv.find(log_n);
        if (nit == c->ninv.end()) nit = c->ninv.emplace(log_n, fe_inv_fast(fr_from_u64(N))).first;
        const Fr ninv = nit->second;
        job.has_post = 1;
        job.post[0] = ninv;
        job.post[1] = coset ? fe_mul(ninv, c->zeta2) : ninv;
        job.post[2] = coset ? fe_mul(ninv, c->zeta) : ninv;
    }
    ntt_audit(c, st, srcs, dsts, batch, "NTT batch");
    return ctx_ntt_launch(c, job, st);
}

int ctx_ntt_cosets3(zk_ctx* c, const Fr* const* polys, Fr* const* dsts, uint32_t cols, uint32_t k, hipStream_t on) {
    const hipStream_t st = on ? on : c->stream;
    const size_t n = (size_t)1 << k;
    const uint32_t batch = 3 * cols;
    if (cols == 0 || batch > ctx_ntt_max_batch(k)) return ZK_EINVAL;
    int rc = ctx_ensure_scratch(c, n * batch);
    if (rc) return rc;
    const Fr *tw = nullptr, *pre = nullptr;
    if ((rc = ctx_get_twiddles_ntt(c, k, &tw)) != ZK_OK || (rc = ctx_get_coset3_pre(c, k, &pre)) != ZK_OK) return rc;
    NttJob job = ntt_job(c, c->scratch, tw, k, n, n);
    job.batch = batch;
    for (uint32_t q = 0; q < cols; q++)
        for (uint32_t j = 0; j < 3; j++) {
            job.srcs[3 * q + j] = polys[q];
            job.dsts[3 * q + j] = dsts[q] + (size_t)j * n;
            job.pre_tabs[3 * q + j] = j ? pre + (size_t)(j - 1) * n : nullptr;  // coset 0: zeta^m alone (`pre`)
        }
    if (k > 7 && (rc = ctx_get_twiddles(c, k, &job.tw_last)) != ZK_OK) return rc;
    ntt_job_coset_pre(job, c);
    ntt_audit(c, st, polys, dsts, cols, "NTT batch (three cosets)");
    return ctx_ntt_launch(c, job, st);
}

int ctx_intt_cosets3(zk_ctx* c, Fr* h, uint32_t k) {
    const size_t n = (size_t)1 << k;
    const Fr* srcs[3] = {h, h + n, h + 2 * n};
    Fr* dsts[3] = {h, h + n, h + 2 * n};
    int rc = ctx_ntt_batch(c, srcs, n, dsts, 3, k, true, false, n);  // plain inverse transforms (1/n included), in place
    if (rc) return rc;
    const Fr* tw_ext = nullptr;
    if ((rc = ctx_get_twiddles(c, k + 2, &tw_ext)) != ZK_OK) return rc;
    auto it = c->coset3_consts.find(k);
    if (it == c->coset3_consts.end()) {
        const Fr z = fe_pow_u64(c->zeta, n), i4 = fe_pow_u64(fr_omega(k + 2), n);
        const Fr two = fr_from_u64(2);
        Coset3Consts q;
        q.inv2 = fe_inv_fast(two);
        q.inv_2z = fe_inv_fast(fe_mul(two, z));
        q.zi = fe_mul(z, i4);
        q.inv_2z2 = fe_inv_fast(fe_mul(two, fe_sqr(z)));
        q.zinv[0] = Fr::one();
        q.zinv[1] = c->zeta2;  // zeta^-1 = zeta^2 (a cube root of unity)
        q.zinv[2] = c->zeta;
        it = c->coset3_consts.emplace(k, q).first;
    }
    if (c->audit.on) c->audit.op(c->stream, {h}, {h}, "three cosets -> h pieces");
    launch_coset3_combine(h, tw_ext, (uint32_t)n, it->second, c->stream);
    return ZK_OK;
}

static uint32_t log2_exact(size_t n) {
    uint32_t l = 0;
    while (((size_t)1 << l) < n) l++;
    return ((size_t)1 << l) == n ? l : 0xffffffffu;
}

// the four zk_*_to_* entry points: `src` -> `dst` (the same handle, but for coeff_to_extended, which refuses it) at the size of
// dst; n_out == nullptr: all of it is stored
static int resident_transform(zk_ctx* c, zk_poly src, zk_poly dst, bool inverse, bool coset, const size_t* n_out) {
    if (!c) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    PolyRec *s = ctx_poly(c, src), *d = ctx_poly(c, dst);
    if (!s || !d || (s == d && coset && !inverse) || (n_out && *n_out > d->n)) return ZK_EINVAL;
    const uint32_t lg = log2_exact(d->n);
    if (lg > 26 || s->n > d->n) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    return ctx_ntt(c, s->ptr, s->n, d->ptr, lg, inverse, coset, n_out ? *n_out : d->n);
}

ZK_API(zk_lagrange_to_coeff, (zk_ctx* c, zk_poly h), (c, h)) { return resident_transform(c, h, h, true, false, nullptr); }
ZK_API(zk_coeff_to_lagrange, (zk_ctx* c, zk_poly h), (c, h)) { return resident_transform(c, h, h, false, false, nullptr); }
ZK_API(zk_coeff_to_extended, (zk_ctx* c, zk_poly src, zk_poly dst), (c, src, dst)) { return resident_transform(c, src, dst, false, true, nullptr); }
ZK_API(zk_extended_to_coeff, (zk_ctx* c, zk_poly ext, size_t n_out), (c, ext, n_out)) { return resident_transform(c, ext, ext, true, true, &n_out); }

ZK_API(zk_eval, (zk_ctx* c, zk_poly h, const uint64_t x[4], uint64_t out[4]), (c, h, x, out)) {
    if (!c || !x || !out) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    PolyRec* r = ctx_poly(c, h);
    if (!r || r->n > 0xffffffffu) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    Fr xx;
    memcpy(&xx, x, 32);
    const uint32_t blocks = eval_blocks((uint32_t)r->n);
    aud_record(c, c->ev[ZK_T_EVAL][0], c->stream);
    launch_eval(r->ptr, (uint32_t)r->n, xx, c->small, c->stream);
    aud_record(c, c->ev[ZK_T_EVAL][1], c->stream);
    c->ev_valid[ZK_T_EVAL] = true;
    HIPCHK(c, hipMemcpyAsync(c->host_small, c->small + blocks, sizeof(Fr), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, aud_sync(c, c->stream));
    memcpy(out, c->host_small, 32);
    return ZK_OK;
}

ZK_API(zk_kate_division, (zk_ctx* c, zk_poly hp, const uint64_t z[4], zk_poly hq), (c, hp, z, hq)) {
    if (!c || !z) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    PolyRec* p = ctx_poly(c, hp);
    PolyRec* q = ctx_poly(c, hq);
    if (!p || !q || p->n != q->n || p->n == 0 || p->n > ((size_t)1 << 26)) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    if ((rc = ctx_ensure_scratch(c, kate_division_scratch((uint32_t)p->n)))) return rc;
    Fr zz;
    memcpy(&zz, z, 32);
    launch_kate_division(p->ptr, q->ptr, (uint32_t)p->n, zz, c->scratch, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, aud_sync(c, c->stream));
    return ZK_OK;
}

ZK_API(zk_ntt_bn254_fr, (zk_ctx* c, uint64_t* a, const uint64_t omega[4], uint32_t log_n), (c, a, omega, log_n)) {
    if (!c || !a || !omega || log_n > 26) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_bind(c);
    if (rc) return rc;
    const size_t n = (size_t)1 << log_n;
    Fr w;
    memcpy(&w, omega, 32);
    // the standard root or its inverse use the cached table; anything else gets a one-off table
    const Fr std_w = fr_omega(log_n);
    const Fr* tw = nullptr;
    Fr* own_tw = nullptr;
    uint32_t inverse = 0;
    if (w == std_w) {
        rc = ctx_get_twiddles_ntt(c, log_n, &tw);
    } else if (fe_mul(w, std_w) == Fr::one()) {
        rc = ctx_get_twiddles_ntt(c, log_n, &tw);
        inverse = 1;
    } else {
        if (hipMalloc(&own_tw, n * sizeof(Fr)) != hipSuccess) return ZK_ENOMEM;
        launch_twiddles_internal(own_tw, w, (uint32_t)n, c->stream);
        tw = own_tw;
    }
    if (rc) return rc;
    Fr *d_a = nullptr, *d_t = nullptr;
    if ((rc = seam_buffer(c, 0, n * sizeof(Fr), (void**)&d_a)) || (rc = seam_buffer(c, 1, n * sizeof(Fr), (void**)&d_t))) {
        hipFree(own_tw);
        return rc;
    }
    NttJob job = ntt_job(c, d_t, tw, log_n, n, n);
    job.src = d_a;
    job.dst = d_a;
    job.inverse = inverse;
    if (!own_tw && log_n > 7) rc = ctx_get_twiddles(c, log_n, &job.tw_last);  // best_fft does not scale: c = 1 in both directions
    if (rc == ZK_OK && hipMemcpyAsync(d_a, a, n * sizeof(Fr), hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = ZK_EHIP;
    if (rc == ZK_OK) rc = ctx_ntt_launch(c, job, c->stream);
    // The transform is complete (and known to have succeeded) BEFORE the first byte of the caller's buffer is overwritten: a
    // failed upload or kernel leaves `a` untouched.  (Round 4 staged the result through a zero-filled temporary — 64 MiB of page
    // faults and a second copy per 2^21 call: 19 ms of the call's 19.4; what can still fail below is the copy-out itself.)
    if (rc == ZK_OK && (aud_sync(c, c->stream) != hipSuccess || hipGetLastError() != hipSuccess)) rc = ZK_EHIP;
    if (rc == ZK_OK && (hipMemcpyAsync(a, d_a, n * sizeof(Fr), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                        aud_sync(c, c->stream) != hipSuccess))
        rc = ZK_EHIP;
    aud_sync(c, c->stream);
    hipFree(own_tw);
    return rc;
}
