// webauthn.hip — zk_webauthn_verify: the relying party's check of `count` WebAuthn assertions, one per lane, in two launches.
//
// The rule is webauthn.hip.h's (host and device in one form).  What stays on the host: the argument checks, the SIZE verdict (a
// request outside the caps is never uploaded and gets no lane), and the expected clientDataJSON prefix E of every request
// (base64url of the challenge and two concatenations: a few hundred bytes of string work, and the lane then compares bytes).
// Everything of variable length goes into ONE blob behind one fixed-size descriptor per request: one upload (webauthn.hip.h
// webauthn_pack: host only, so that the tests run it under the sanitizers).  The round trip is lane_call.h's.
//   launch 1  webauthn_digest_kernel, workgroups of 256, one request per lane: the byte rules (rpIdHash, flags, E, DER), both
//             SHA-256 passes, the 160-byte record and a provisional reason.  Lanes of a wave hash different lengths; that
//             divergence is accepted (no sorting: a hash is a few microseconds against the curve's milliseconds).
//   launch 2  es256.hip's verification kernel over those records, in its one-wave workgroups with its LDS layout; a lane whose
//             provisional reason is set returns at once, so the final reason is the provisional one where set, else the curve's.
// Reasons, counters and records come back in one download.  The comb of G and the staging buffers are zk_es256_verify's.
#include <string.h>

#include <vector>

#include "es256.h"
#include "webauthn.hip.h"

namespace {

constexpr uint32_t WEBAUTHN_WG = 256;

__global__ __launch_bounds__(WEBAUTHN_WG) void webauthn_digest_kernel(const WebauthnDesc* descs, const uint8_t* blob, uint32_t count, uint8_t* reasons,
                                                                      uint32_t* counts, uint8_t* records) {
    const uint32_t i = blockIdx.x * WEBAUTHN_WG + threadIdx.x;
    if (i >= count) return;  // the tail lanes of the last workgroup touch no memory
    const WebauthnDesc* d = descs + i;
    uint32_t sign_count;
    reasons[i] = webauthn_digest_one(blob + d->ad_off, d->ad_len, blob + d->cd_off, d->cd_len, blob + d->sig_off, d->sig_len, blob + d->e_off, d->e_len,
                                     d->x, d->y, d->rp_id_hash, d->flags_required, d->allow_cross_origin != 0, records + (size_t)i * 160, &sign_count);
    counts[i] = sign_count;
}

}  // namespace

ZK_API(zk_webauthn_verify,
       (zk_ctx* c, size_t count, const zk_webauthn_assertion* a, uint8_t* verdicts, uint8_t* reasons, uint8_t* records, uint32_t* sign_counts),
       (c, count, a, verdicts, reasons, records, sign_counts)) {
    if (!c || !a || !verdicts || count == 0 || count > ZK_WEBAUTHN_BATCH_MAX) return ZK_EINVAL;
    for (size_t i = 0; i < count; i++)
        if ((!a[i].authenticator_data && a[i].authenticator_data_len) || (!a[i].client_data_json && a[i].client_data_json_len) ||
            (!a[i].signature && a[i].signature_len) || (!a[i].challenge && a[i].challenge_len) || (!a[i].origin && a[i].origin_len))
            return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    uint64_t aud0;
    int rc = call_enter(c, &aud0);
    if (rc || (rc = es256_table(c))) return rc;
    Es256Ws* w = c->es256;

    const WebauthnImage im = webauthn_pack(a, count);
    // the output buffer: reasons (padded to words), counters and records, which all come back
    const size_t n = im.live.size(), desc_bytes = n * sizeof(WebauthnDesc);
    const size_t reasons_bytes = webauthn_padded(n), out_bytes = reasons_bytes + n * 4 + n * 160;
    std::vector<uint8_t> out(out_bytes);
    if (n) {
        auto enqueue = [&] {
            const uint8_t* d_in = (const uint8_t*)w->in.p;
            uint8_t* d_out = (uint8_t*)w->out.p;
            uint8_t* d_records = d_out + reasons_bytes + n * 4;
            hipLaunchKernelGGL(webauthn_digest_kernel, lane_grid(n, WEBAUTHN_WG), dim3(WEBAUTHN_WG), 0, c->stream, (const WebauthnDesc*)d_in, d_in + desc_bytes,
                               (uint32_t)n, d_out, (uint32_t*)(d_out + reasons_bytes), d_records);
            if (hipError_t e = hipGetLastError()) return e;
            if (c->audit.on) c->audit.op(c->stream, {w->out.p, w->table}, {w->out.p}, "webauthn: verification of the records (es256_verify_kernel)");
            return es256_enqueue(c, d_records, (uint32_t)n, d_out, d_out);
        };
        if ((rc = lane_round_trip(c, {{&w->in, im.bytes.data(), im.bytes.size()}}, nullptr, &w->out, out_bytes, out.data(), out_bytes,
                                  {"webauthn: descriptors and blob upload", "webauthn: rules, hashes, records (webauthn_digest_kernel)",
                                   "webauthn: reasons, counters, records download"},
                                  enqueue)))
            return rc;
        if ((rc = aud_verdict(c, aud0, ZK_OK))) return rc;
    }

    for (size_t i = 0; i < count; i++) verdicts[i] = 0;
    if (reasons) memset(reasons, ZK_WEBAUTHN_SIZE, count);
    if (records) memset(records, 0, count * 160);
    if (sign_counts) memset(sign_counts, 0, count * sizeof(uint32_t));
    for (size_t j = 0; j < n; j++) {
        const size_t i = im.live[j];
        verdicts[i] = out[j] == ZK_WEBAUTHN_VALID ? 1 : 0;
        if (reasons) reasons[i] = out[j];
        if (records) memcpy(records + i * 160, out.data() + reasons_bytes + n * 4 + j * 160, 160);
        if (sign_counts) memcpy(sign_counts + i, out.data() + reasons_bytes + j * 4, 4);
    }
    return ZK_OK;
}
