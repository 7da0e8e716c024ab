// msm_lanes.hip — the MSM lanes of a context (workspaces, passes in flight, where their tails run) and the entry points
// that are one MSM: the fine-grained seam (zk_msm_bn254, zk_msm_srs) and zk_commit / zk_commit_batch.
#include <algorithm>
#include <vector>

#include "ctx.h"

// columns per fixed-base launch asked for (msm_plan.h msm_batch_width; zk_ctx_set_option(ZK_OPT_MSM_BATCH) overrides)
static uint32_t batch_for(const zk_ctx* c, size_t n) { return msm_batch_width(n, c->opt_msm_batch); }

// the widest pass the resident SRS's plan takes when `want` columns are asked for: `want` on the wide path and on the fused
// plan, 1 on the swept sort (every SRS from 2^22), which msm_run runs one column at a time, and without window tables
uint32_t ctx_msm_pass_cap(const zk_ctx* c, uint32_t want) {
    if (c->srs_k < 0 || !c->table_c) return 1;
    return msm_max_pass(c->table_c, (size_t)1 << c->srs_k, want);
}

uint32_t ctx_msm_max_batch(const zk_ctx* c) {
    if (c->srs_k < 0) return 1;
    return ctx_msm_pass_cap(c, batch_for(c, (size_t)1 << c->srs_k));
}

// device staging buffer `which` of at least `bytes` (kept for the next call: a Rust host patched at best_multiexp /
// best_fft calls the seam a dozen times per proof with the same sizes)
int seam_buffer(zk_ctx* c, int which, size_t bytes, void** out) {
    if (c->seam_bytes[which] < bytes) {
        if (c->seam_buf[which]) hipFree(c->seam_buf[which]);
        c->seam_buf[which] = nullptr;
        c->seam_bytes[which] = 0;
        hipError_t e = hipMalloc(&c->seam_buf[which], bytes);
        if (e != hipSuccess) {
            c->last_hip = (int)e;
            return ZK_ENOMEM;
        }
        c->seam_bytes[which] = bytes;
    }
    *out = c->seam_buf[which];
    return ZK_OK;
}

// `table_window` != 0: the workspace serves the fixed-base mode over the resident SRS (window = the tables'); otherwise
// arbitrary bases, whose windows stop at 15 bits
static int get_msm_ws(zk_ctx* c, int lane, size_t n, uint32_t table_window, MsmWorkspace** out) {
    const size_t want = msm_ws_len(n);
    const uint32_t cw = table_window ? table_window : msm_auto_window_generic(want);
    zk_ctx::MsmLane& L = c->lanes[lane];
    MsmWorkspace*& slot = table_window ? L.ws : L.ws_gen;
    // columns per pass the workspace must take: the single prover's batches, or a lock-step batch's wider passes
    // (a plan that runs one column per pass gets a one-column workspace: msm_max_pass, by the resident SRS's length as
    // ctx_msm_pass_cap asks it — not by `n`, which is that length only because the one caller passes it so)
    const uint32_t cols =
        table_window ? msm_max_pass(table_window, (size_t)1 << c->srs_k, std::max(batch_for(c, want), std::min<uint32_t>(c->msm_min_cols, MSM_MAX_BATCH))) : 1u;
    if (slot && (msm_ws_max_n(slot) != want || msm_ws_window(slot) != cw || msm_ws_max_batch(slot) < cols)) {
        aud_sync(c, c->stream);  // (a pass of the lane that has been collected may still have kernels of its tail queued behind others)
        if (c->tail_stream) aud_sync(c, c->tail_stream);
        msm_workspace_destroy(slot);
        slot = nullptr;
    }
    if (!slot) {
        hipError_t e;
        slot = msm_workspace_create(want, cw, table_window != 0, &e, cols);
        if (!slot && e != hipErrorInvalidValue && !c->poly_spare.empty()) {
            ctx_release_spares(c);
            (void)hipGetLastError();
            slot = msm_workspace_create(want, cw, table_window != 0, &e, cols);
        }
        if (!slot) {
            c->last_hip = (int)e;
            return e == hipErrorInvalidValue ? ZK_EINVAL : ZK_ENOMEM;
        }
    }
    L.ws_run = slot;
    *out = slot;
    return ZK_OK;
}

int ctx_msm_begin_batch(zk_ctx* c, int lane, const Fr* const* d_scalars, uint32_t batch, const G1Affine* d_bases, size_t n) {
    if (lane < 0 || lane >= zk_ctx::MSM_LANES || c->lanes[lane].busy || batch == 0) return ZK_EINVAL;
    zk_ctx::MsmLane& L = c->lanes[lane];
    MsmWorkspace* ws;
    // commits against the resident SRS use the precomputed window tables
    const G1Affine* table = nullptr;
    uint32_t stride = 0;
    bool ident = true;  // arbitrary bases: the accumulation tests every operand
    if (c->srs_k >= 0 && c->table_c) {
        if (d_bases == c->g) {
            table = c->g_table;
            ident = c->g_has_identity;
        } else if (d_bases == c->g_lagrange) {
            table = c->g_lagrange_table;
            ident = c->g_lagrange_has_identity;
        }
        stride = 1u << c->srs_k;
    }
    int rc = get_msm_ws(c, lane, table ? (size_t)stride : n, table ? c->table_c : 0u, &ws);
    if (rc) return rc;
    if (batch > 1 && (!table || batch > msm_ws_max_batch(ws))) return ZK_EINVAL;
    // where this pass's reduction tail runs (ctx.h tail_stream): the side stream for up to two proofs in flight on the device
    const int active = ctx_activity_touch(c);
    const uint32_t above = c->opt_tail_main_above ? c->opt_tail_main_above : 2u;  // ZK_OPT_MSM_TAIL_MAIN_ABOVE; measured default (ctx.h)
    const bool tail_on_main = c->opt_tail_stream == 2 || (c->opt_tail_stream == 0 && (uint32_t)active > above);
    if ((!tail_on_main || c->msm_side) && !c->tail_stream && ctx_side_stream(c, &c->tail_stream, 0)) return ZK_EHIP;  // made on first use (see zk_ctx_create)
    L.tail = tail_on_main ? c->stream : c->tail_stream;
    if (L.tail == c->stream) c->acc_n[ZK_T_MSM_TAIL_MAIN]++;
    hipStream_t hs = c->stream;  // where the pass's head and accumulation run
    if (c->msm_side && c->msm_stream) {
        hs = c->msm_stream;
        HIPCHK(c, aud_record(c, c->ev_msm_in, c->stream));  // everything the main stream holds so far: the pass's inputs among it
        HIPCHK(c, aud_wait(c, hs, c->ev_msm_in));
        if (L.tail == c->stream) L.tail = c->tail_stream;    // (never a tail behind the main stream's later kernels)
    }
    c->stream_counts[L.tail == c->stream ? 0 : 1]++;  // zk_ctx_stream_info
    HIPCHK(c, aud_record(c, L.t_head[0], hs));
    msm_ws_set_t1_mode(ws, c->opt_msm_t1);
    const MsmPassArgs pass = {d_scalars, batch, n, d_bases, table, stride, hs, L.tail, L.head_done, L.t_acc, !table || ident, L.host_buf};
    HIPCHK(c, msm_run(ws, pass, &L.pass));
    if (c->audit.on) {
        // the ledger's twin of what msm_run enqueued: head + accumulation on hs (reads the columns, fills the lane's workspace),
        // the head_done hand-off, the tail on L.tail (reads the workspace, writes the lane's pinned result buffer)
        const void* rd[MSM_MAX_BATCH];
        for (uint32_t q = 0; q < batch; q++) rd[q] = d_scalars[q];
        const void* wr[1] = {ws};
        c->audit.op_v(hs, rd, batch, wr, 1, "MSM pass: sort head + accumulation");
        if (L.tail != hs) {
            c->audit.record(L.head_done, hs);
            c->audit.wait(L.tail, L.head_done);
        }
        c->audit.op(L.tail, {ws}, {ws, L.host_buf}, "MSM pass: reduction tail");
    }
    HIPCHK(c, aud_record(c, L.tail_done, L.tail));
    HIPCHK(c, aud_record(c, L.t_head[1], hs));
    c->msm_launches++;
    L.busy = true;
    return ZK_OK;
}

int ctx_msm_begin(zk_ctx* c, int lane, const Fr* d_scalars, const G1Affine* d_bases, size_t n) {
    return ctx_msm_begin_batch(c, lane, &d_scalars, 1, d_bases, n);
}

int ctx_msm_end_batch(zk_ctx* c, int lane, G1Jac* out) {
    if (lane < 0 || lane >= zk_ctx::MSM_LANES || !c->lanes[lane].busy) return ZK_EINVAL;
    zk_ctx::MsmLane& L = c->lanes[lane];
    L.busy = false;
    HIPCHK(c, aud_esync(c, L.tail_done));
    c->audit.host_read(L.host_buf, "MSM pass: the host collects the sums");
    const MsmPass& P = L.pass;
    bool redone;
    HIPCHK(c, msm_collect(L.ws_run, P, L.tail, L.host_buf, out, &redone));
    if (redone) {  // the ledger's twin of what msm_collect did over a degenerate basis
        c->audit.op(L.tail, {L.ws_run}, {L.ws_run, L.host_buf}, "MSM pass: checked redo + tail");
        c->audit.host_stream(L.tail);
    }
    // timers: head (recode .. accumulate, on the context stream) and the accumulate kernel alone
    // (the head ends with the accumulate kernel: t_acc[1] — always complete once the tail is; an event recorded behind the tail's
    // own on the same stream, as round 4 did, is often not: with the tails on the main stream most passes went uncounted)
    float ms = 0.f;
    c->acc_n[ZK_T_MSM]++;
    if (P.n > 0 && hipEventElapsedTime(&ms, L.t_head[0], L.t_acc[1]) == hipSuccess) {
        c->acc_ms[ZK_T_MSM] += ms;
        c->last_plain_ms[ZK_T_MSM] = ms;
    }
    if (P.n > 0 && hipEventElapsedTime(&ms, L.t_acc[0], L.t_acc[1]) == hipSuccess) {
        c->acc_ms[ZK_T_MSM_ACCUM] += ms;
        c->acc_n[ZK_T_MSM_ACCUM]++;
        c->acc_n[ZK_T_MSM_COLUMNS] += P.batch;
        c->last_plain_ms[ZK_T_MSM_ACCUM] = ms;
    }
    if (P.n > 0 && P.plan == MsmPass::WIDE && hipEventElapsedTime(&ms, L.t_acc[2], L.t_acc[3]) == hipSuccess) {
        c->acc_ms[ZK_T_MSM_TAIL] += ms;
        c->acc_n[ZK_T_MSM_TAIL]++;
        c->last_plain_ms[ZK_T_MSM_TAIL] = ms;
    }
    return ZK_OK;
}

void ctx_msm_drain(zk_ctx* c) {
    for (int q = 0; q < zk_ctx::MSM_LANES; q++)
        if (c->lanes[q].busy) {
            aud_esync(c, c->lanes[q].tail_done);
            c->lanes[q].busy = false;
        }
}

int ctx_msm_end(zk_ctx* c, int lane, G1Jac* out) {
    if (lane >= 0 && lane < zk_ctx::MSM_LANES && c->lanes[lane].busy && c->lanes[lane].pass.batch != 1) return ZK_EINVAL;
    return ctx_msm_end_batch(c, lane, out);
}

// synchronous form (also feeds the accumulated timers used by bench.py)
int ctx_msm_device(zk_ctx* c, const Fr* d_scalars, const G1Affine* d_bases, size_t n, G1Jac* out) {
    int rc = ctx_msm_begin(c, 0, d_scalars, d_bases, n);
    if (rc) return rc;
    return ctx_msm_end(c, 0, out);
}

// ---- fine-grained seam -------------------------------------------------------

// what zk_msm_bn254 and zk_msm_srs share: the identity for n = 0, the scalars uploaded through the seam's staging buffer, one MSM,
// the result copied out.  `h_bases` != nullptr: arbitrary bases, uploaded on every call as well; otherwise the resident `d_bases`
static int seam_msm(zk_ctx* c, const uint64_t* scalars, const uint64_t* h_bases, const G1Affine* d_bases, size_t n, uint64_t out[12]) {
    int rc = ctx_bind(c);
    if (rc) return rc;
    G1Jac res;
    if (n == 0) {
        res.x = Fq::one();
        res.y = Fq::one();
        res.z = Fq::zero();
        memcpy(out, &res, 96);
        return ZK_OK;
    }
    Fr* d_s = nullptr;
    if ((rc = seam_buffer(c, 0, n * sizeof(Fr), (void**)&d_s))) return rc;
    if (hipMemcpyAsync(d_s, scalars, n * sizeof(Fr), hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = ZK_EHIP;
    if (rc == ZK_OK && h_bases) {
        G1Affine* d_b = nullptr;
        if ((rc = seam_buffer(c, 1, n * sizeof(G1Affine), (void**)&d_b))) return rc;
        if (hipMemcpyAsync(d_b, h_bases, n * sizeof(G1Affine), hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = ZK_EHIP;
        d_bases = d_b;
    }
    if (rc == ZK_OK) rc = ctx_msm_device(c, d_s, d_bases, n, &res);
    aud_sync(c, c->stream);
    if (rc == ZK_OK) memcpy(out, &res, 96);
    return rc;
}

// arbitrary bases: both operands are uploaded on every call (the resident-SRS form is zk_msm_srs)
ZK_API(zk_msm_bn254, (zk_ctx* c, const uint64_t* scalars, const uint64_t* bases, size_t n, uint64_t out[12]), (c, scalars, bases, n, out)) {
    if (!c || !out || (n && (!scalars || !bases))) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    return seam_msm(c, scalars, bases, nullptr, n, out);
}

ZK_API(zk_msm_srs, (zk_ctx* c, int basis, const uint64_t* scalars, size_t n, uint64_t out[12]), (c, basis, scalars, n, out)) {
    if (!c || !out || (n && !scalars) || !basis_ok(basis)) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->srs_k < 0) return ZK_ESTATE;
    if (n > ((size_t)1 << c->srs_k)) return ZK_EINVAL;
    return seam_msm(c, scalars, nullptr, ctx_basis(c, basis), n, out);
}
ZK_API(zk_commit, (zk_ctx* c, zk_poly h, int basis, uint64_t out[8]), (c, h, basis, out)) {
    if (!c || !out || !basis_ok(basis)) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->srs_k < 0) return ZK_ESTATE;
    PolyRec* r = ctx_poly(c, h);
    const size_t n = (size_t)1 << c->srs_k;
    if (!r || r->n > n) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    G1Jac j;
    rc = ctx_msm_device(c, r->ptr, ctx_basis(c, basis), r->n, &j);
    if (rc) return rc;
    const G1Affine a = g1_jac_to_affine_host(j);
    memcpy(out, &a, 64);
    return ZK_OK;
}

ZK_API(zk_commit_batch, (zk_ctx* c, const zk_poly* hs, size_t count, int basis, uint64_t* out), (c, hs, count, basis, out)) {
    if (!c || !out || !hs || count == 0 || !basis_ok(basis)) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->srs_k < 0) return ZK_ESTATE;
    const size_t n = (size_t)1 << c->srs_k;
    std::vector<const Fr*> ptrs(count);
    size_t len = 0;
    for (size_t i = 0; i < count; i++) {
        PolyRec* r = ctx_poly(c, hs[i]);
        if (!r || r->n > n || (i && r->n != len)) return ZK_EINVAL;  // one length per call
        len = r->n;
        ptrs[i] = r->ptr;
    }
    int rc = ctx_bind(c);
    if (rc) return rc;
    const G1Affine* bases = ctx_basis(c, basis);
    const uint32_t cap = ctx_msm_max_batch(c);
    G1Jac js[MSM_MAX_BATCH];
    for (size_t i0 = 0; i0 < count; i0 += cap) {
        const uint32_t cnt = (uint32_t)(count - i0 < cap ? count - i0 : cap);
        rc = ctx_msm_begin_batch(c, 0, ptrs.data() + i0, cnt, bases, len);
        if (rc) return rc;
        rc = ctx_msm_end_batch(c, 0, js);
        if (rc) return rc;
        for (uint32_t q = 0; q < cnt; q++) {
            const G1Affine a = g1_jac_to_affine_host(js[q]);
            memcpy(out + (i0 + q) * 8, &a, 64);
        }
    }
    return ZK_OK;
}
