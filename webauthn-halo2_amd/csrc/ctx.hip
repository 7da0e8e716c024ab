// ctx.hip — the context of libzkmi355.so: its lifetime, scratch and cached device tables, options, timers and the device
// queries of the C ABI (declarations and the reference routines each entry point replaces: include/zkmi355.h).
#include <stdlib.h>

#include <algorithm>
#include <new>

#include "ctx.h"
#include "prover.h"

namespace zk {
G1Affine g1_jac_to_affine_host(const G1Jac& p) {
    G1Affine r;
    if (p.z.is_zero()) {
        r.x = Fq::zero();
        r.y = Fq::zero();
        return r;
    }
    const Fq zi = fe_inv_fast(p.z);
    const Fq zi2 = fe_sqr(zi);
    r.x = fe_mul(p.x, zi2);
    r.y = fe_mul(p.y, fe_mul(zi2, zi));
    return r;
}
}  // namespace zk

int ctx_bind(zk_ctx* c) {
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) {
        c->last_hip = (int)e;
        return ZK_EHIP;
    }
    return ZK_OK;
}

int ctx_ensure_scratch(zk_ctx* c, size_t n) {
    if (c->scratch_n >= n) return ZK_OK;
    if (c->xform_stream) aud_sync(c, c->xform_stream);  // (transforms in flight use the buffer)
    if (c->scratch) hipFree(c->scratch);
    c->scratch = nullptr;
    c->scratch_n = 0;
    hipError_t e = hipMalloc(&c->scratch, n * sizeof(Fr));
    if (e != hipSuccess) {
        c->last_hip = (int)e;
        return ZK_ENOMEM;
    }
    c->scratch_n = n;
    return ZK_OK;
}

// ---- device tables made once per context and size, read from any of the context's streams afterwards: look up, allocate,
// fill on the main stream through `fill(table)`, wait for the fill, insert
template <class Fill>
static int ctx_cached_table(zk_ctx* c, std::map<uint32_t, Fr*>& cache, uint32_t key, size_t elems, const Fr** out, Fill fill) {
    auto it = cache.find(key);
    if (it != cache.end()) {
        *out = it->second;
        return ZK_OK;
    }
    Fr* tab = nullptr;
    hipError_t e = hipMalloc(&tab, elems * sizeof(Fr));
    if (e != hipSuccess) {
        c->last_hip = (int)e;
        return ZK_ENOMEM;
    }
    if ((e = fill(tab)) != hipSuccess) {
        c->last_hip = (int)e;
        hipFree(tab);
        return ZK_EHIP;
    }
    if ((e = aud_sync(c, c->stream)) != hipSuccess) c->last_hip = (int)e;
    cache[key] = tab;
    *out = tab;
    return ZK_OK;
}

int ctx_get_twiddles(zk_ctx* c, uint32_t log_n, const Fr** out) {
    if (log_n > 28) return ZK_EINVAL;
    const size_t n = (size_t)1 << log_n;
    return ctx_cached_table(c, c->twiddles, log_n, n, out, [&](Fr* tw) {
        launch_twiddles(tw, fr_omega(log_n), (uint32_t)n, c->stream);
        return hipSuccess;
    });
}

int ctx_get_twiddles_ntt(zk_ctx* c, uint32_t log_n, const Fr** out) {
    if (log_n > 28) return ZK_EINVAL;
    const size_t n = (size_t)1 << log_n;
    return ctx_cached_table(c, c->twiddles_ntt, log_n, n, out, [&](Fr* tw) {
        launch_twiddles_internal(tw, fr_omega(log_n), (uint32_t)n, c->stream);
        return hipSuccess;
    });
}

int ctx_get_twiddles_ninv(zk_ctx* c, uint32_t log_n, const Fr** out) {
    if (log_n > 28) return ZK_EINVAL;
    const size_t n = (size_t)1 << log_n;
    return ctx_cached_table(c, c->twiddles_ninv, log_n, n, out, [&](Fr* tw) {
        launch_twiddles_scaled(tw, fr_omega(log_n), fe_inv(fr_from_u64(n)), (uint32_t)n, c->stream);
        return hipSuccess;
    });
}

int ctx_get_coset_points(zk_ctx* c, uint32_t log_n, const Fr** out) {
    const Fr* tw = nullptr;
    int rc = ctx_get_twiddles(c, log_n, &tw);
    if (rc) return rc;
    const size_t n = (size_t)1 << log_n;
    return ctx_cached_table(c, c->coset_points, log_n, n, out, [&](Fr* xs) {
        const hipError_t e = hipMemcpyAsync(xs, tw, n * sizeof(Fr), hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) launch_scale(xs, c->zeta, (uint32_t)n, c->stream);
        return e;
    });
}

// the twists of the three-coset route (poly.hip "three cosets")
int ctx_get_coset3_pre(zk_ctx* c, uint32_t k, const Fr** out) {
    const Fr* tw_ext = nullptr;
    int rc = ctx_get_twiddles(c, k + 2, &tw_ext);
    if (rc) return rc;
    const size_t n = (size_t)1 << k;
    return ctx_cached_table(c, c->coset3_pre, k, 2 * n, out, [&](Fr* tab) {
        const Fr k1024 = fr_from_u64(1024);
        const Fr zp[3] = {k1024, fe_mul(c->zeta, k1024), fe_mul(c->zeta2, k1024)};
        for (uint32_t j = 1; j <= 2; j++) launch_coset3_pre(tw_ext, (uint32_t)n, j, zp, tab + (size_t)(j - 1) * n, c->stream);
        return hipSuccess;
    });
}

// ------------------------------------------------------------------ C ABI --

int device_id_ok(int device_id) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ZK_ENODEV;
    return device_id < 0 || device_id >= ndev ? ZK_EINVAL : ZK_OK;
}

int zk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// PCI address ("0000:c1:00.0") of a device: where its host-side neighbourhood is found (/sys/bus/pci/devices/<id>/numa_node,
// local_cpulist) — a multi-GPU host binds each GPU's worker threads and staging memory to that NUMA node
ZK_API(zk_device_pci_bus_id, (int device_id, char* out, size_t cap), (device_id, out, cap)) {
    if (!out || cap < 16) return ZK_EINVAL;
    if (int rc = device_id_ok(device_id)) return rc;
    if (hipDeviceGetPCIBusId(out, (int)cap, device_id) != hipSuccess) return ZK_EHIP;
    return ZK_OK;
}

// free / total memory of a device: what a host sizes its number of resident pipelines by (ecdsa_p256.py)
ZK_API(zk_device_mem_info, (int device_id, size_t* free_bytes, size_t* total_bytes), (device_id, free_bytes, total_bytes)) {
    if (!free_bytes || !total_bytes) return ZK_EINVAL;
    if (int rc = device_id_ok(device_id)) return rc;
    DeviceScope dev(device_id);
    if (!dev.ok) return ZK_EHIP;
    return hipMemGetInfo(free_bytes, total_bytes) == hipSuccess ? ZK_OK : ZK_EHIP;
}

// page-locked host memory for the buffers a host hands to zk_poly_upload*: the copy is then one DMA at the bus rate instead of
// the runtime's staged copy out of pageable memory (allocate on the thread that is bound to the GPU's NUMA node)
void* zk_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes) != hipSuccess) return nullptr;
    return p;
}
void zk_host_free(void* p) {
    if (p) hipHostFree(p);
}

const char* zk_strerror(int code) {
    switch (code) {
        case ZK_OK: return "ok";
        case ZK_EINVAL: return "invalid argument";
        case ZK_ENOMEM: return "out of memory";
        case ZK_EHIP: return "HIP runtime error";
        case ZK_ENODEV: return "no usable gfx950 device";
        case ZK_ESTATE: return "missing prerequisite (SRS / key not loaded)";
        case ZK_EWITNESS: return "witness does not satisfy the circuit (lookup input outside the table)";
        case ZK_EINTERNAL: return "internal error (C++ exception stopped at the ABI boundary)";
        case ZK_ELAYOUT: return "selector columns outside the layout of compress_selectors the key is built for";
        default: return "unknown error";
    }
}

ZK_API(zk_ctx_create, (int device_id, zk_ctx** out), (device_id, out)) {
    if (!out) return ZK_EINVAL;
    if (int rc = device_id_ok(device_id)) return rc;
    zk_ctx* c = new (std::nothrow) zk_ctx();
    if (!c) return ZK_ENOMEM;
    c->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess ||
        ((c->stream_slot = pool_take_slot(device_id, &c->stream)) < 0 && hipStreamCreate(&c->stream) != hipSuccess) ||
        hipHostMalloc(&c->host_small, 8 * sizeof(Fr)) != hipSuccess ||
        hipMalloc(&c->small, EVAL_SMALL_ELEMS * sizeof(Fr)) != hipSuccess) {  // (2048 + 8: poly_plan.h)
        zk_ctx_destroy(c);
        return ZK_EHIP;
    }
    for (int i = 0; i < ZK_T_COUNT; i++)
        if (hipEventCreate(&c->ev[i][0]) != hipSuccess || hipEventCreate(&c->ev[i][1]) != hipSuccess) {
            zk_ctx_destroy(c);
            return ZK_EHIP;
        }
    // (the transform and MSM streams of a lone proof are made on first use — ctx_lone_streams: the HIP runtime spreads a
    // process's streams over its four hardware queues as they are created, and with four streams per context the MAIN streams of
    // four pipelines all landed on one queue: 100 -> 88 proofs/s, accumulate launches serialised at 0.70 ms, found by bench.py)
    bool ok = true;
    for (hipEvent_t* e : {&c->ev_msm_in, &c->ev_rows, &c->ev_xform}) ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < zk_ctx::MSM_LANES && ok; i++) {
        zk_ctx::MsmLane& L = c->lanes[i];
        L.tail = c->stream;
        for (hipEvent_t& e : L.t_head) ok = ok && hipEventCreate(&e) == hipSuccess;
        for (hipEvent_t& e : L.t_acc) ok = ok && hipEventCreate(&e) == hipSuccess;
        for (hipEvent_t* e : {&L.head_done, &L.tail_done}) ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipHostMalloc(&L.host_buf, (size_t)MSM_MAX_BATCH * 15 * 4 * sizeof(G1X)) == hipSuccess;
    }
    if (!ok) {
        zk_ctx_destroy(c);
        return ZK_EHIP;
    }
    c->zeta = fr_zeta();
    c->zeta2 = fe_sqr(c->zeta);
    ctx_activity_register(c);
    *out = c;
    return ZK_OK;
}

// A second context on the same device that shares `parent`'s resident SRS (bases + window tables, read-only): the way to run
// several proof pipelines per GPU (one zk_ctx per host thread) without a copy of the tables each.  The child sees the SRS as it
// is NOW; either context may later load another SRS for itself (the shared block lives until its last user lets go).
ZK_API(zk_ctx_create_shared, (zk_ctx* parent, zk_ctx** out), (parent, out)) {
    if (!parent || !out) return ZK_EINVAL;
    zk_ctx* c = nullptr;
    int rc = zk_ctx_create(parent->device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(parent->mu);
    if (parent->srs_k >= 0) {
        static_cast<SrsView&>(*c) = *parent;
        // the ten options a child inherits.  NOT inherited: ZK_OPT_STREAM_AUDIT, ZK_OPT_ACTIVITY_HOLD, ZK_OPT_QUOTIENT_DOMAIN,
        // ZK_OPT_STREAM_PRIORITY (the child keeps its defaults)
        c->opt_msm_window = parent->opt_msm_window;  // the tables were built for this window
        c->opt_msm_batch = parent->opt_msm_batch;
        c->opt_ntt_max_r = parent->opt_ntt_max_r;
        c->opt_gp_batch_invert = parent->opt_gp_batch_invert;
        c->opt_tail_stream = parent->opt_tail_stream;
        c->opt_tail_main_above = parent->opt_tail_main_above;
        c->opt_batch_pass_cols = parent->opt_batch_pass_cols;
        c->opt_xform_stream = parent->opt_xform_stream;
        c->opt_msm_stream = parent->opt_msm_stream;
        c->opt_msm_t1 = parent->opt_msm_t1;
        c->srs_gen++;
    }
    *out = c;
    return ZK_OK;
}

void zk_ctx_destroy(zk_ctx* c) {
    if (!c) return;
    ctx_activity_unregister(c);
    hipSetDevice(c->device);
    if (c->stream) aud_sync(c, c->stream);
    if (c->tail_stream) aud_sync(c, c->tail_stream);
    if (c->xform_stream) aud_sync(c, c->xform_stream);
    if (c->msm_stream) aud_sync(c, c->msm_stream);
    for (auto& kv : c->twiddles) hipFree(kv.second);
    for (auto& kv : c->twiddles_ntt) hipFree(kv.second);
    for (auto& kv : c->twiddles_ninv) hipFree(kv.second);
    for (auto& kv : c->coset_points) hipFree(kv.second);
    for (auto& kv : c->coset3_pre) hipFree(kv.second);
    pk_destroy_all(c);
    for (auto& kv : c->polys) hipFree(kv.second.ptr);
    for (auto& r : c->poly_spare) hipFree(r.ptr);
    c->srs.reset();  // frees the bases and tables unless another context shares them
    for (int i = 0; i < zk_ctx::MSM_LANES; i++) {
        zk_ctx::MsmLane& L = c->lanes[i];
        if (L.ws) msm_workspace_destroy(L.ws);
        if (L.ws_gen) msm_workspace_destroy(L.ws_gen);
        if (L.host_buf) hipHostFree(L.host_buf);
        for (int j = 0; j < 2; j++)
            if (L.t_head[j]) hipEventDestroy(L.t_head[j]);
        for (int j = 0; j < 4; j++)
            if (L.t_acc[j]) hipEventDestroy(L.t_acc[j]);
        if (L.head_done) hipEventDestroy(L.head_done);
        if (L.tail_done) hipEventDestroy(L.tail_done);
    }
    if (c->host_small) hipHostFree(c->host_small);
    if (c->eval_batch_host) hipHostFree(c->eval_batch_host);
    if (c->scratch) hipFree(c->scratch);
    for (int i = 0; i < 2; i++)
        if (c->seam_buf[i]) hipFree(c->seam_buf[i]);
    if (c->small) hipFree(c->small);
    verify_ws_destroy(c->vws);
    es256_ws_destroy(c->es256);
    pairing_ws_destroy(c->pairing);
    for (int i = 0; i < ZK_T_COUNT; i++)
        for (int j = 0; j < 2; j++)
            if (c->ev[i][j]) hipEventDestroy(c->ev[i][j]);
    if (c->ev_msm_in) hipEventDestroy(c->ev_msm_in);
    if (c->ev_rows) hipEventDestroy(c->ev_rows);
    if (c->ev_xform) hipEventDestroy(c->ev_xform);
    if (c->stream_slot >= 0) {
        // the slot's streams stay (streams.hip stream pool); a main stream made at its own priority is the context's own
        if (c->stream_own_priority && c->stream) hipStreamDestroy(c->stream);
        pool_release_slot(c->device, c->stream_slot);
    } else {
        if (c->msm_stream) hipStreamDestroy(c->msm_stream);
        if (c->xform_stream) hipStreamDestroy(c->xform_stream);
        if (c->tail_stream) hipStreamDestroy(c->tail_stream);
        if (c->stream) hipStreamDestroy(c->stream);
    }
    delete c;
}

int zk_last_hip_error(const zk_ctx* c) { return c ? c->last_hip : 0; }

ZK_API(zk_sync, (zk_ctx* c), (c)) {
    if (!c) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_bind(c);
    if (rc) return rc;
    HIPCHK(c, aud_sync(c, c->stream));
    return ZK_OK;
}

ZK_API(zk_last_kernel_ms, (zk_ctx* c, int which, float* out_ms), (c, which, out_ms)) {
    if (!c || !out_ms || which < 0 || which >= ZK_T_COUNT) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (which == ZK_T_MSM || which == ZK_T_MSM_ACCUM) {
        *out_ms = c->last_plain_ms[which];
        return ZK_OK;
    }
    if (!c->ev_valid[which]) {
        *out_ms = 0.f;
        return ZK_OK;
    }
    int rc = ctx_bind(c);
    if (rc) return rc;
    HIPCHK(c, aud_esync(c, c->ev[which][1]));
    HIPCHK(c, hipEventElapsedTime(out_ms, c->ev[which][0], c->ev[which][1]));
    return ZK_OK;
}

// ---- shader-clock probe (bench.py's roofline.valu_issue): ONE wave spins for `ticks` of the constant 100 MHz counter
// (s_memrealtime) on a chain of dependent v_mad_u64_u32 and reports what the shader-clock counter (s_memtime) advanced by in
// the same interval.  Run on a context of its own WHILE the workload proves, it reads the clock the chip sustains under that
// load (a lone probe on an idle chip reads the boost clock).  out[0] = shader-clock ticks, out[1] = 100 MHz ticks, out[2] =
// multiply-adds of the chain (one wave, nothing to interleave with: ticks / mads = the multiplier's dependent latency)
__global__ __launch_bounds__(64) void clock_probe_kernel(uint64_t ticks, uint64_t* __restrict__ out) {
    uint64_t acc = threadIdx.x + 1;
    uint32_t a = 0x9e3779b9u + threadIdx.x, b = 0x7f4a7c15u;
    const uint64_t r0 = wall_clock64();
    const uint64_t c0 = clock64();
    uint64_t iters = 0;
    while (wall_clock64() - r0 < ticks) {
#pragma unroll
        for (int i = 0; i < 256; i++) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b) : "vcc");
        iters += 256;
    }
    const uint64_t c1 = clock64();
    const uint64_t r1 = wall_clock64();
    if (threadIdx.x == 0) {
        out[0] = c1 - c0;
        out[1] = r1 - r0;
        out[2] = iters;
        out[3] = acc;  // (keeps the chain alive)
    }
}

ZK_API(zk_clock_probe, (zk_ctx* c, uint32_t millis, uint64_t out[4]), (c, millis, out)) {
    if (!c || !out || millis == 0 || millis > 2000) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_bind(c);
    if (rc) return rc;
    uint64_t* d = reinterpret_cast<uint64_t*>(c->small);         // device scratch of the context (8 field elements)
    uint64_t* h = reinterpret_cast<uint64_t*>(c->host_small);    // its pinned twin
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, c->stream, (uint64_t)millis * 100000ull, d);
    HIPCHK(c, hipMemcpyAsync(h, d, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, aud_sync(c, c->stream));
    memcpy(out, h, 4 * sizeof(uint64_t));
    return ZK_OK;
}

ZK_API(zk_audit_report, (zk_ctx* c, uint64_t counts[2], char* msg, size_t cap), (c, counts, msg, cap)) {
    if (!c || !counts) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    counts[0] = c->audit.checks;
    counts[1] = c->audit.violations;
    if (msg && cap) {
        const size_t len = std::min(cap - 1, c->audit.first.size());
        memcpy(msg, c->audit.first.data(), len);
        msg[len] = 0;
    }
    return ZK_OK;
}

ZK_API(zk_timer_reset, (zk_ctx* c), (c)) {
    if (!c) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    for (int i = 0; i < ZK_T_COUNT; i++) {
        c->acc_ms[i] = 0;
        c->acc_n[i] = 0;
    }
    return ZK_OK;
}

ZK_API(zk_timer_stats, (zk_ctx* c, int which, double* total_ms, uint64_t* count), (c, which, total_ms, count)) {
    if (!c || which < 0 || which >= ZK_T_COUNT || !total_ms || !count) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    *total_ms = c->acc_ms[which];
    *count = c->acc_n[which];
    return ZK_OK;
}

// the options that are a bounded number stored in a member: 0 (the built-in choice) or min .. max
namespace {
struct PlainOption {
    int option;
    int64_t min, max;  // min = 0: any value up to max
    uint32_t zk_ctx::*member;
};
const PlainOption PLAIN_OPTIONS[] = {
    {ZK_OPT_MSM_WINDOW, 9, 17, &zk_ctx::opt_msm_window},
    {ZK_OPT_MSM_TAIL_STREAM, 0, 2, &zk_ctx::opt_tail_stream},
    {ZK_OPT_MSM_TAIL_MAIN_ABOVE, 0, 64, &zk_ctx::opt_tail_main_above},
    {ZK_OPT_MSM_STREAM, 0, 2, &zk_ctx::opt_msm_stream},
    {ZK_OPT_MSM_T1, 0, 2, &zk_ctx::opt_msm_t1},
    {ZK_OPT_XFORM_STREAM, 0, 2, &zk_ctx::opt_xform_stream},
    {ZK_OPT_BATCH_PASS_COLUMNS, 0, MSM_MAX_BATCH, &zk_ctx::opt_batch_pass_cols},
    {ZK_OPT_MSM_BATCH, 0, MSM_MAX_BATCH, &zk_ctx::opt_msm_batch},
    {ZK_OPT_NTT_MAX_RADIX_LOG2, 1, 11, &zk_ctx::opt_ntt_max_r},  // clamped to the tile size in ntt_run
    {ZK_OPT_QUOTIENT_DOMAIN, 0, 2, &zk_ctx::opt_quotient_domain},
};
}  // namespace

ZK_API(zk_ctx_set_option, (zk_ctx* c, int option, int64_t value), (c, option, value)) {
    if (!c || value < 0) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    for (const PlainOption& o : PLAIN_OPTIONS)
        if (o.option == option) {
            if (value && (value < o.min || value > o.max)) return ZK_EINVAL;
            c->*o.member = (uint32_t)value;
            return ZK_OK;
        }
    switch (option) {
        case ZK_OPT_STREAM_AUDIT:
            if (value > 2) return ZK_EINVAL;
            c->audit.reset();
            c->audit.streams[0] = c->stream;
            c->audit.on = value != 0;
            c->audit_fault = value == 2;
            return ZK_OK;
        case ZK_OPT_GP_BATCH_INVERT:
            c->opt_gp_batch_invert = value ? 1 : 0;
            return ZK_OK;
        case ZK_OPT_ACTIVITY_HOLD:
            if (value > 2) return ZK_EINVAL;
            activity::set_option(c->act, c->device, (int)value, activity::now_ns());
            return ZK_OK;
        case ZK_OPT_STREAM_PRIORITY: {
            // experiment (docs/experiments.md "pipelines at different priorities"): the context's MAIN stream is made again at
            // another dispatch priority.  Only meaningful before any work was enqueued (the audit ledger and the lone-proof side
            // streams refer to the main stream by value); the old stream is drained first
            if (value > 2) return ZK_EINVAL;
            for (int i = 0; i < zk_ctx::MSM_LANES; i++)
                if (c->lanes[i].busy) return ZK_EINVAL;  // an MSM pass in flight holds the stream by value
            int rc = ctx_bind(c);
            if (rc) return rc;
            int lo = 0, hi = 0;  // numerically lower = higher priority
            if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) return ZK_EHIP;
            const int pr = value == 1 ? hi : value == 2 ? lo : (lo + hi) / 2;
            hipStream_t ns = nullptr;
            if (hipStreamCreateWithPriority(&ns, hipStreamDefault, pr) != hipSuccess) return ZK_EHIP;
            hipStreamSynchronize(c->stream);
            for (int i = 0; i < zk_ctx::MSM_LANES; i++)
                if (c->lanes[i].tail == c->stream) c->lanes[i].tail = ns;
            if (c->stream_own_priority || c->stream_slot < 0) hipStreamDestroy(c->stream);  // (a slot's main stream stays in its slot)
            c->stream = ns;
            c->stream_own_priority = true;
            c->audit.streams[0] = ns;
            return ZK_OK;
        }
        default: return ZK_EINVAL;
    }
}
