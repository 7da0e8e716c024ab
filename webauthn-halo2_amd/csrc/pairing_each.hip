// pairing_each.hip — pairing checks with a G2 point per lane: zk_pairing_check_each and zk_srs_contribution_check_batch.
//
// Where every item brings its own G2 point — a ceremony receipt's s_g2 — there is no walk to prepare, so the lane tests that point
// ([r] q in Jacobian coordinates) and walks it through the Miller loop itself, without an inversion (pairing.h miller_loop_walk);
// the other side of each equation is a fixed point (g2; for a receipt the G2 generator) whose lines still come from a prepared
// table.  A receipt's two equations share s_g2, so its lane walks once into two accumulators.  A lane whose point is improper
// returns before it walks; its neighbours go on alone.  Shape, calls and trip counts are pairing.hip's: workgroups of one wave, the
// tower's products as calls, every loop of constant length.  This is a unit of its own so that pairing_check_kernel's code object
// stays what it was.  The host side of a call is lane_call.h's round trip, over pairing.hip's staging buffers.
#include <string.h>

#include <vector>

#include "pairing_ws.h"
#include "srs_update.h"

namespace {

constexpr uint32_t PAIRING_WG = 64;  // one wave

// a lane's G2 point from its 128-byte image (x.c0 || x.c1 || y.c0 || y.c1; all zero: the identity)
__device__ __forceinline__ G2A g2_load(const Fq* p) {
    G2A q;
    q.x.c0 = fe_load(p);
    q.x.c1 = fe_load(p + 1);
    q.y.c0 = fe_load(p + 2);
    q.y.c1 = fe_load(p + 3);
    q.inf = f2_is_zero(q.x) && f2_is_zero(q.y);
    return q;
}

// lane i decides e(a_i, q_i) = e(b_i, g2); table->line[1] is g2's walk
__global__ __launch_bounds__(PAIRING_WG) void pairing_check_each_kernel(const G1Affine* __restrict__ a, const G1Affine* __restrict__ b, const Fq* __restrict__ q,
                                                                        uint32_t count, const PairingTable* __restrict__ table, uint8_t* __restrict__ reasons) {
    const uint32_t i = blockIdx.x * PAIRING_WG + threadIdx.x;
    if (i >= count) return;
    reasons[i] = pairing_check_walk(affine_load(a + i), affine_load(b + i), g2_load(q + 4 * (size_t)i), *table);
}

// lane i writes the flag byte of receipt i (a zk_srs_contribution: 40 words); table->line[1] is the G2 generator's walk
constexpr uint32_t RECEIPT_FQ = sizeof(zk_srs_contribution) / sizeof(Fq);
static_assert(sizeof(zk_srs_contribution) == 320 && sizeof(G1Affine) == 64 && sizeof(Fq) == 32, "a receipt is three G1 images and a G2 image");
__global__ __launch_bounds__(PAIRING_WG) void contribution_check_kernel(const Fq* __restrict__ receipts, uint32_t count, const PairingTable* __restrict__ table,
                                                                        uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * PAIRING_WG + threadIdx.x;
    if (i >= count) return;
    const Fq* r = receipts + RECEIPT_FQ * (size_t)i;
    const G1Affine* g = reinterpret_cast<const G1Affine*>(r);
    flags[i] = (uint8_t)contribution_check_lanes(affine_load(g), affine_load(g + 1), affine_load(g + 2), g2_load(r + 6), *table);
}

// `count` host triples (a_i, b_i, q_i) against the table at d_table (its line[1]: g2's walk), one launch
int pairing_each_launch(zk_ctx* c, PairingWs* w, size_t count, const G1Affine* a, const G1Affine* b, const uint64_t* q, const void* d_table, uint8_t* reasons) {
    const size_t pts = count * sizeof(G1Affine);
    auto enqueue = [&] {
        hipLaunchKernelGGL(pairing_check_each_kernel, lane_grid(count, PAIRING_WG), dim3(PAIRING_WG), 0, c->stream, (const G1Affine*)w->a.p,
                           (const G1Affine*)w->b.p, (const Fq*)w->q.p, (uint32_t)count, (const PairingTable*)d_table, (uint8_t*)w->out.p);
        return hipGetLastError();
    };
    return lane_round_trip(c, {{&w->a, a, pts}, {&w->b, b, pts}, {&w->q, q, count * 128}}, d_table, &w->out, count, reasons, count,
                           {"pairing: triples upload", "pairing: checks (pairing_check_each_kernel)", "pairing: reasons download"}, enqueue);
}

// the table whose line[1] is the G2 generator's walk: what every receipt's fixed side reads.  Made once per context
int generator_table(zk_ctx* c, PairingWs* w, const void** out) {
    if (!w->gen) {
        void* d = nullptr;
        if (hipMalloc(&d, sizeof(PairingTable)) != hipSuccess) return ZK_ENOMEM;
        const G2A none{f2_zero(), f2_zero(), true};
        if (int rc = pairing_table_upload(c, g2_generator(), none, d)) {
            hipFree(d);
            return rc;
        }
        w->gen = d;
    }
    *out = w->gen;
    return ZK_OK;
}

// the flag bytes of `count` receipts, one launch; flags: a host array of `count`
int contribution_launch(zk_ctx* c, PairingWs* w, size_t count, const zk_srs_contribution* r, const void* d_table, uint8_t* flags) {
    auto enqueue = [&] {
        hipLaunchKernelGGL(contribution_check_kernel, lane_grid(count, PAIRING_WG), dim3(PAIRING_WG), 0, c->stream, (const Fq*)w->q.p, (uint32_t)count,
                           (const PairingTable*)d_table, (uint8_t*)w->out.p);
        return hipGetLastError();
    };
    return lane_round_trip(c, {{&w->q, r, count * sizeof(zk_srs_contribution)}}, d_table, &w->out, count, flags, count,
                           {"pairing: receipts upload", "pairing: receipts (contribution_check_kernel)", "pairing: flags download"}, enqueue);
}

}  // namespace

ZK_API(zk_pairing_check_each, (zk_ctx* c, size_t count, const uint64_t* a, const uint64_t* b, const uint64_t* q, const uint64_t g2[16], uint8_t* verdicts, uint8_t* reasons), (c, count, a, b, q, g2, verdicts, reasons)) {
    if (!c || !a || !b || !q || !verdicts || count == 0 || count > ZK_PAIRING_BATCH_MAX) return ZK_EINVAL;
    G2A own;
    if (g2) {
        own = g2_from_raw((const uint8_t*)g2);
        if (!g2_is_proper(own)) return ZK_EINVAL;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    if (!g2 && (c->srs_k < 0 || !c->g2_valid)) return ZK_ESTATE;
    uint64_t aud0;
    int rc = call_enter(c, &aud0);
    PairingWs* w;
    if (rc || (rc = pairing_ws(c, &w))) return rc;
    const void* table;
    if (g2) {  // the lanes read g2's walk alone: the table's other half stays empty
        const G2A none{f2_zero(), f2_zero(), true};
        if ((rc = w->own.grow(c, sizeof(PairingTable))) || (rc = pairing_table_upload(c, own, none, w->own.p))) return rc;
        table = w->own.p;
    } else if ((rc = pairing_resident_table(c, &table))) {
        return rc;
    }
    std::vector<uint8_t> res(count);
    if ((rc = pairing_each_launch(c, w, count, reinterpret_cast<const G1Affine*>(a), reinterpret_cast<const G1Affine*>(b), q, table, res.data()))) return rc;
    if ((rc = aud_verdict(c, aud0, ZK_OK))) return rc;
    for (size_t i = 0; i < count; i++) verdicts[i] = res[i] == ZK_PAIRING_VALID ? 1 : 0;
    if (reasons) memcpy(reasons, res.data(), count);
    return ZK_OK;
}

ZK_API(zk_srs_contribution_check_batch, (zk_ctx* c, size_t count, const zk_srs_contribution* r, uint32_t* flags), (c, count, r, flags)) {
    if (!c || !r || !flags || count == 0 || count > ZK_SRS_CONTRIB_BATCH_MAX) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    uint64_t aud0;
    int rc = call_enter(c, &aud0);
    PairingWs* w;
    const void* table;
    if (rc || (rc = pairing_ws(c, &w)) || (rc = generator_table(c, w, &table))) return rc;
    std::vector<uint8_t> res(count);
    if ((rc = contribution_launch(c, w, count, r, table, res.data()))) return rc;
    G1Affine g1;
    const bool resident = c->srs_k >= 1;
    if (resident) HIPCHK(c, hipMemcpy(&g1, c->g + 1, sizeof(G1Affine), hipMemcpyDeviceToHost));
    if ((rc = aud_verdict(c, aud0, ZK_OK))) return rc;
    for (size_t i = 0; i < count; i++) {
        uint32_t f = res[i];
        if (resident && memcmp(&g1, r[i].after_g1, sizeof(G1Affine)) == 0) f |= ZK_SRS_CONTRIB_RESIDENT;
        if (i == 0 || memcmp(r[i].before_g1, r[i - 1].after_g1, sizeof(r[i].before_g1)) == 0) f |= ZK_SRS_CONTRIB_CHAINED;
        flags[i] = f;
    }
    return ZK_OK;
}
