// es256.hip — zk_es256_verify: secp256r1 ECDSA verification of `count` requests in one launch, one signature per lane.
//
// The rule itself is p256_verify_one (p256.hip.h, host and device): the kernel is a loop-less wrapper around it.  Shape:
// workgroups of ONE wave, so a batch spreads over the CUs and up to 16 384 signatures cost about one signature's latency (the
// ~252 doublings under u2 Q are serial, and P-256 has no endomorphism to split them).  Each lane's table Q .. 15 Q is indexed by
// that lane's own digit, so it lives in LDS (15 Jacobian points x 64 lanes = 90 KiB of the CU's 160), never in a register array.
// u1 G comes from a comb of G (64 windows x 15 affine multiples, 60 KiB) that es256_comb_kernel builds on the first call of a
// context — one window per lane, each lane normalising its 15 points with one inversion — and that stays with the context.
// The host side of a call - grow, upload, launch, download, wait - is lane_call.h's round trip.
#include <string.h>

#include <vector>

#include "es256.h"

void es256_ws_destroy(Es256Ws* w) { delete w; }

namespace {

constexpr uint32_t ES256_WG = 64;  // one wave: p256_verify_one's LDS block is laid out for it

// the comb of G: lane w builds window w (4 w doublings of G, its 15 multiples through the LDS block, one inversion)
__global__ __launch_bounds__(ES256_WG) void es256_comb_kernel(P256Affine* table) {
    const uint32_t w = threadIdx.x;
    if (blockIdx.x != 0 || w >= (uint32_t)P256_COMB_WINDOWS) return;
    P256LdsStore st = p256_lds_store();
    p256_comb_window((int)w, st, table + (size_t)w * P256_COMB_ENTRIES);
}

// `settled` (null for zk_es256_verify): reasons an earlier launch already decided, one per record; a lane whose byte is set
// returns at once and leaves its reason as it is (zk_webauthn_verify: `settled` and `reasons` are one array)
__global__ __launch_bounds__(ES256_WG) void es256_verify_kernel(const uint8_t* sigs, uint32_t count, const P256Affine* table, const uint8_t* settled,
                                                                uint8_t* reasons) {
    const uint32_t i = blockIdx.x * ES256_WG + threadIdx.x;
    if (i >= count) return;  // the tail lanes of the last wave touch no memory
    if (settled && settled[i] != ZK_ES256_VALID) return;
    reasons[i] = p256_verify_one(sigs + (size_t)i * 160, table);
}

}  // namespace

// made once per context on its main stream and waited for, like the twiddle tables (ctx.hip ctx_cached_table)
int es256_table(zk_ctx* c) {
    if (!c->es256 && !(c->es256 = new (std::nothrow) Es256Ws())) return ZK_ENOMEM;
    Es256Ws* w = c->es256;
    if (w->table) return ZK_OK;
    P256Affine* t = nullptr;
    if (hipMalloc(&t, (size_t)P256_COMB_POINTS * sizeof(P256Affine)) != hipSuccess) return ZK_ENOMEM;
    if (c->audit.on) c->audit.op(c->stream, {}, {t}, "es256: comb of G (es256_comb_kernel)");
    hipLaunchKernelGGL(es256_comb_kernel, dim3(1), dim3(ES256_WG), 0, c->stream, t);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = aud_sync(c, c->stream);
    if (e != hipSuccess) {
        c->last_hip = (int)e;
        hipFree(t);
        return ZK_EHIP;
    }
    w->table = t;
    return ZK_OK;
}

hipError_t es256_enqueue(zk_ctx* c, const uint8_t* d_sigs, uint32_t count, const uint8_t* d_settled, uint8_t* d_reasons) {
    hipLaunchKernelGGL(es256_verify_kernel, lane_grid(count, ES256_WG), dim3(ES256_WG), 0, c->stream, d_sigs, count,
                       (const P256Affine*)c->es256->table, d_settled, d_reasons);
    return hipGetLastError();
}

ZK_API(zk_es256_verify, (zk_ctx* c, size_t count, const uint8_t* sigs, uint8_t* verdicts, uint8_t* reasons), (c, count, sigs, verdicts, reasons)) {
    if (!c || !sigs || !verdicts || count == 0 || count > ZK_ES256_BATCH_MAX) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    uint64_t aud0;
    int rc = call_enter(c, &aud0);
    if (rc || (rc = es256_table(c))) return rc;
    Es256Ws* w = c->es256;
    std::vector<uint8_t> res(count);
    auto enqueue = [&] { return es256_enqueue(c, (const uint8_t*)w->in.p, (uint32_t)count, nullptr, (uint8_t*)w->out.p); };
    if ((rc = lane_round_trip(c, {{&w->in, sigs, count * 160}}, w->table, &w->out, count, res.data(), count,
                              {"es256: signatures upload", "es256: verification (es256_verify_kernel)", "es256: reasons download"}, enqueue)))
        return rc;
    if ((rc = aud_verdict(c, aud0, ZK_OK))) return rc;
    for (size_t i = 0; i < count; i++) verdicts[i] = res[i] == ZK_ES256_VALID ? 1 : 0;
    if (reasons) memcpy(reasons, res.data(), count);
    return ZK_OK;
}
