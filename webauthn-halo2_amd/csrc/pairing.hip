// pairing.hip — the KZG pairing check on the device: zk_pairing_check_batch, and the route zk_verify_batch takes for a failing
// fold under ZK_VERIFY_PAIRING_DEVICE (verify.hip settle).
//
// One check per lane: lane i decides e(a_i, s_g2) e(-b_i, g2) = 1 against ONE (g2, s_g2) pair per call, so `count` independent
// checks cost about one check's latency (zk_es256_verify's shape).  The rule itself is pairing_check_lines (pairing.h, host and
// device): the kernel is a loop-less wrapper around it.  Both G2 points being fixed, the walk of T through the Miller loop is
// done once on the host (pairing_table_make: 102 steps per point, slope and constant of each, 26 KiB with the Frobenius
// constants) and uploaded; every lane reads the same line at the same time, and inverts nothing until the one Fq inversion of
// the final exponentiation's easy part.  The hard part is the table-free chain of pairing.h (three powers by u).
// Shape: workgroups of ONE wave, so a batch spreads over the CUs and a lane may use the whole register file of its SIMD slot;
// the Fq2 / Fq6 / Fq12 products are calls (pairing.h ZK_PAIR_MULFN), so the Fq12 values live in scratch and the code stays a
// small multiple of the instruction cache instead of one straight line of 33 000 field products.  Every loop has a constant
// trip count, no lane waits for another, and lanes beyond `count` return before touching memory.
// The resident SRS's table is kept with the SRS view (ctx.h PairLinesDev) and dropped with the block or the pair; a caller's own
// pair gets a table per call.
// The checks with a G2 point per lane (zk_pairing_check_each, zk_srs_contribution_check_batch) are pairing_each.hip's; they share
// the staging buffers and the two table helpers below (pairing_ws.h).  The host side of a call - grow, upload, launch, download,
// wait - is lane_call.h's round trip.
#include <string.h>

#include <vector>

#include "pairing_ws.h"
#include "srs_update.h"

void pairing_ws_destroy(PairingWs* w) { delete w; }

namespace {

constexpr uint32_t PAIRING_WG = 64;  // one wave

__global__ __launch_bounds__(PAIRING_WG) void pairing_check_kernel(const G1Affine* __restrict__ a, const G1Affine* __restrict__ b, uint32_t count,
                                                                   const PairingTable* __restrict__ table, uint8_t* __restrict__ reasons) {
    const uint32_t i = blockIdx.x * PAIRING_WG + threadIdx.x;
    if (i >= count) return;  // the tail lanes of the last wave touch no memory
    reasons[i] = pairing_check_lines(affine_load(a + i), affine_load(b + i), *table);
}

}  // namespace

int pairing_ws(zk_ctx* c, PairingWs** out) {
    if (!c->pairing && !(c->pairing = new (std::nothrow) PairingWs())) return ZK_ENOMEM;
    *out = c->pairing;
    return ZK_OK;
}

// the table of (g2, s_g2) into the device buffer d (sizeof(PairingTable) bytes), waited for: the host copy goes out of scope
int pairing_table_upload(zk_ctx* c, const G2A& g2, const G2A& s_g2, void* d) {
    std::vector<PairingTable> t(1);
    pairing_table_make(g2, s_g2, t.data());
    if (c->audit.on) c->audit.op(c->stream, {}, {d}, "pairing: prepared lines upload");
    HIPCHK(c, hipMemcpyAsync(d, t.data(), sizeof(PairingTable), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, aud_sync(c, c->stream));
    return ZK_OK;
}

namespace {

// `count` host pairs against the table at d_table, one launch; reasons: a host array of `count`
int pairing_launch(zk_ctx* c, PairingWs* w, size_t count, const G1Affine* a, const G1Affine* b, const void* d_table, uint8_t* reasons) {
    const size_t pts = count * sizeof(G1Affine);
    auto enqueue = [&] {
        hipLaunchKernelGGL(pairing_check_kernel, lane_grid(count, PAIRING_WG), dim3(PAIRING_WG), 0, c->stream, (const G1Affine*)w->a.p,
                           (const G1Affine*)w->b.p, (uint32_t)count, (const PairingTable*)d_table, (uint8_t*)w->out.p);
        return hipGetLastError();
    };
    return lane_round_trip(c, {{&w->a, a, pts}, {&w->b, b, pts}}, d_table, &w->out, count, reasons, count,
                           {"pairing: pairs upload", "pairing: checks (pairing_check_kernel)", "pairing: reasons download"}, enqueue);
}

}  // namespace

// the resident pair's table, made on first use
int pairing_resident_table(zk_ctx* c, const void** out) {
    uint8_t key[256];
    memcpy(key, c->g2_raw, 128);
    memcpy(key + 128, c->s_g2_raw, 128);
    if (c->pair_lines && memcmp(c->pair_lines->key, key, 256) == 0) {
        *out = c->pair_lines->d;
        return ZK_OK;
    }
    std::shared_ptr<PairLinesDev> t = std::make_shared<PairLinesDev>();
    t->device = c->device;
    if (hipMalloc(&t->d, sizeof(PairingTable)) != hipSuccess) return ZK_ENOMEM;
    if (int rc = pairing_table_upload(c, g2_from_raw(c->g2_raw), g2_from_raw(c->s_g2_raw), t->d)) return rc;
    memcpy(t->key, key, 256);
    c->pair_lines = t;
    *out = t->d;
    return ZK_OK;
}

int pairing_check_resident(zk_ctx* c, size_t count, const G1Affine* a, const G1Affine* b, uint8_t* reasons) {
    PairingWs* w;
    const void* table;
    int rc;
    if ((rc = pairing_ws(c, &w)) || (rc = pairing_resident_table(c, &table))) return rc;
    return pairing_launch(c, w, count, a, b, table, reasons);
}

ZK_API(zk_pairing_check_batch, (zk_ctx* c, size_t count, const uint64_t* a, const uint64_t* b, const uint64_t g2[16], const uint64_t s_g2[16], uint8_t* verdicts, uint8_t* reasons), (c, count, a, b, g2, s_g2, verdicts, reasons)) {
    if (!c || !a || !b || !verdicts || count == 0 || count > ZK_PAIRING_BATCH_MAX || (g2 == nullptr) != (s_g2 == nullptr)) return ZK_EINVAL;
    G2A own[2];
    if (g2) {  // the tests a receipt's s_g2 gets: reduced, on the twist, of order r, not the identity
        own[0] = g2_from_raw((const uint8_t*)g2);
        own[1] = g2_from_raw((const uint8_t*)s_g2);
        if (!g2_is_proper(own[0]) || !g2_is_proper(own[1])) return ZK_EINVAL;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    if (!g2 && (c->srs_k < 0 || !c->g2_valid)) return ZK_ESTATE;
    uint64_t aud0;
    int rc = call_enter(c, &aud0);
    PairingWs* w;
    if (rc || (rc = pairing_ws(c, &w))) return rc;
    std::vector<uint8_t> res(count);
    const G1Affine *pa = reinterpret_cast<const G1Affine*>(a), *pb = reinterpret_cast<const G1Affine*>(b);
    if (g2) {
        if ((rc = w->own.grow(c, sizeof(PairingTable))) || (rc = pairing_table_upload(c, own[0], own[1], w->own.p)) ||
            (rc = pairing_launch(c, w, count, pa, pb, w->own.p, res.data())))
            return rc;
    } else if ((rc = pairing_check_resident(c, count, pa, pb, res.data()))) {
        return rc;
    }
    if ((rc = aud_verdict(c, aud0, ZK_OK))) return rc;
    for (size_t i = 0; i < count; i++) verdicts[i] = res[i] == ZK_PAIRING_VALID ? 1 : 0;
    if (reasons) memcpy(reasons, res.data(), count);
    return ZK_OK;
}
