// webauthn.hip — zk_webauthn_verify: the relying party's check of `count` WebAuthn assertions, one per lane, in two launches.
//
// The rule is webauthn.hip.h's (host and device in one form).  What stays on the host: the argument checks, the SIZE verdict (a
// request outside the caps is never uploaded and gets no lane), and the expected clientDataJSON prefix E of every request
// (base64url of the challenge and two concatenations: a few hundred bytes of string work, and the lane then compares bytes).
// Everything of variable length goes into ONE blob behind one fixed-size descriptor per request: one upload.
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

// one request as the lane sees it; the offsets count from the start of the blob
struct WebauthnDesc {
    uint32_t ad_off, ad_len, cd_off, cd_len, sig_off, sig_len, e_off, e_len;
    uint8_t x[32], y[32], rp_id_hash[32];
    uint8_t flags_required, allow_cross_origin, pad[2];
};
static_assert(sizeof(WebauthnDesc) == 132, "the descriptor is packed words and bytes");

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
    int rc = ctx_bind(c);
    if (rc) return rc;
    const uint64_t aud0 = c->audit.violations;
    c->audit.base_of.clear();
    if ((rc = es256_table(c))) return rc;
    Es256Ws* w = c->es256;

    // the live requests (those inside the caps), their descriptors and the blob
    std::vector<uint32_t> live;
    live.reserve(count);
    size_t blob_bytes = 0;
    for (size_t i = 0; i < count; i++)
        if (webauthn_size_ok(a[i].authenticator_data_len, a[i].client_data_json_len, a[i].signature_len, a[i].challenge_len, a[i].origin_len)) {
            live.push_back((uint32_t)i);
            blob_bytes += a[i].authenticator_data_len + a[i].client_data_json_len + a[i].signature_len + WEBAUTHN_PREFIX_MAX;
        }
    const size_t n = live.size(), desc_bytes = n * sizeof(WebauthnDesc);
    const size_t reasons_bytes = (n + 3) & ~(size_t)3, out_bytes = reasons_bytes + n * 4 + n * 160;
    std::vector<uint8_t> out(out_bytes);
    if (n) {
        std::vector<uint8_t> in(desc_bytes + blob_bytes);
        uint8_t* blob = in.data() + desc_bytes;
        uint32_t pos = 0;
        auto put = [&](const uint8_t* p, size_t len) {
            const uint32_t at = pos;
            if (len) memcpy(blob + pos, p, len);
            pos += (uint32_t)len;
            return at;
        };
        for (size_t j = 0; j < n; j++) {
            const zk_webauthn_assertion& q = a[live[j]];
            WebauthnDesc d;
            memset(&d, 0, sizeof d);
            d.ad_len = (uint32_t)q.authenticator_data_len, d.ad_off = put(q.authenticator_data, q.authenticator_data_len);
            d.cd_len = (uint32_t)q.client_data_json_len, d.cd_off = put(q.client_data_json, q.client_data_json_len);
            d.sig_len = (uint32_t)q.signature_len, d.sig_off = put(q.signature, q.signature_len);
            d.e_off = pos;
            d.e_len = webauthn_expected_prefix(q.challenge, q.challenge_len, q.origin, q.origin_len, blob + pos);
            pos += d.e_len;
            memcpy(d.x, q.pubkey_x, 32);
            memcpy(d.y, q.pubkey_y, 32);
            memcpy(d.rp_id_hash, q.rp_id_hash, 32);
            d.flags_required = q.flags_required;
            d.allow_cross_origin = q.allow_cross_origin;
            memcpy(in.data() + j * sizeof(WebauthnDesc), &d, sizeof d);
        }
        const size_t in_bytes = desc_bytes + pos;
        if ((rc = es256_grow(c, &w->in, &w->c_in, in_bytes)) || (rc = es256_grow(c, &w->out, &w->c_out, out_bytes))) return rc;
        uint8_t* d_in = (uint8_t*)w->in;
        uint8_t* d_out = (uint8_t*)w->out;
        uint8_t* d_records = d_out + reasons_bytes + n * 4;
        if (c->audit.on) c->audit.op(c->stream, {}, {w->in}, "webauthn: descriptors and blob upload");
        HIPCHK(c, hipMemcpyAsync(d_in, in.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
        if (c->audit.on) c->audit.op(c->stream, {w->in}, {w->out}, "webauthn: rules, hashes, records (webauthn_digest_kernel)");
        hipLaunchKernelGGL(webauthn_digest_kernel, dim3((uint32_t)((n + WEBAUTHN_WG - 1) / WEBAUTHN_WG)), dim3(WEBAUTHN_WG), 0, c->stream,
                           (const WebauthnDesc*)d_in, (const uint8_t*)(d_in + desc_bytes), (uint32_t)n, d_out, (uint32_t*)(d_out + reasons_bytes), d_records);
        HIPCHK(c, hipGetLastError());
        if (c->audit.on) c->audit.op(c->stream, {w->out, w->table}, {w->out}, "webauthn: verification of the records (es256_verify_kernel)");
        HIPCHK(c, es256_enqueue(c, d_records, (uint32_t)n, d_out, d_out));
        if (c->audit.on) c->audit.op(c->stream, {w->out}, {}, "webauthn: reasons, counters, records download");
        HIPCHK(c, hipMemcpyAsync(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, aud_sync(c, c->stream));  // (the staging vectors are pageable)
        if ((rc = aud_verdict(c, aud0, ZK_OK))) return rc;
    }

    for (size_t i = 0; i < count; i++) verdicts[i] = 0;
    if (reasons) memset(reasons, ZK_WEBAUTHN_SIZE, count);
    if (records) memset(records, 0, count * 160);
    if (sign_counts) memset(sign_counts, 0, count * sizeof(uint32_t));
    for (size_t j = 0; j < n; j++) {
        const size_t i = live[j];
        verdicts[i] = out[j] == ZK_WEBAUTHN_VALID ? 1 : 0;
        if (reasons) reasons[i] = out[j];
        if (records) memcpy(records + i * 160, out.data() + reasons_bytes + n * 4 + j * 160, 160);
        if (sign_counts) memcpy(sign_counts + i, out.data() + reasons_bytes + j * 4, 4);
    }
    return ZK_OK;
}
