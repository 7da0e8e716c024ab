// webauthn_register.hip — zk_webauthn_register: the relying party's check of `count` WebAuthn registrations, one per lane, in two
// launches.  The stage in front of zk_webauthn_verify: it says where the key of a credential came from.
//
// The rule is webauthn_register.hip.h's (host and device in one form).  What stays on the host, as in webauthn.hip: the argument
// checks, the SIZE verdict (a request outside the caps is never uploaded and gets no lane) and the expected clientDataJSON prefix E
// of every request.  Everything of variable length goes into ONE blob behind one fixed-size descriptor per request: one upload
// (webauthn_register.hip.h webauthn_register_pack: host only, so that the tests run it under the sanitizers).  The round trip is
// lane_call.h's.
//   launch 1  webauthn_register_kernel, workgroups of 256, one registration per lane: the CBOR walk, the authData and credential
//             rules, the COSE template, E, the key's curve test, the statement under the policy; for a packed self statement the
//             DER parse, both SHA-256 passes and the 160-byte record.  It writes a provisional reason, the credential, and one
//             `settled` byte per lane that is non-zero unless the lane's record still has to be verified.
//   launch 2  es256.hip's verification kernel over those records; a settled lane returns at once, so the final reason is the
//             provisional one where the lane was settled, else the curve's.
// Reasons and credentials come back in one download; the host blanks the credential of every refused lane.
// The comb of G and the staging buffers are zk_es256_verify's.
#include <string.h>

#include <vector>

#include "es256.h"
#include "webauthn_register.hip.h"

static_assert(sizeof(zk::WebauthnCredential) == sizeof(zk_webauthn_credential) && offsetof(zk::WebauthnCredential, aaguid) == offsetof(zk_webauthn_credential, aaguid) &&
                  offsetof(zk::WebauthnCredential, auth_data_off) == offsetof(zk_webauthn_credential, auth_data_off) &&
                  offsetof(zk::WebauthnCredential, sign_count) == offsetof(zk_webauthn_credential, sign_count) &&
                  offsetof(zk::WebauthnCredential, attestation) == offsetof(zk_webauthn_credential, attestation),
              "the header's copy of the credential is the public one");

namespace {

constexpr uint32_t WEBAUTHN_REGISTER_WG = 256;

__global__ __launch_bounds__(WEBAUTHN_REGISTER_WG) void webauthn_register_kernel(const WebauthnRegisterDesc* descs, const uint8_t* blob, uint32_t count,
                                                                                 uint8_t* reasons, uint8_t* settled, WebauthnCredential* creds,
                                                                                 uint8_t* records) {
    const uint32_t i = blockIdx.x * WEBAUTHN_REGISTER_WG + threadIdx.x;
    if (i >= count) return;  // the tail lanes of the last workgroup touch no memory
    const WebauthnRegisterDesc* d = descs + i;
    bool to_verify;
    const uint8_t reason = webauthn_register_one(blob + d->obj_off, d->obj_len, blob + d->cd_off, d->cd_len, blob + d->e_off, d->e_len, d->rp_id_hash,
                                                 d->flags_required, d->allow_cross_origin != 0, d->policy, records + (size_t)i * 160, creds + i, &to_verify);
    reasons[i] = reason;
    settled[i] = to_verify ? ZK_ES256_VALID : 0xFF;  // refused, or accepted without a signature: no curve work for this lane
}

}  // namespace

ZK_API(zk_webauthn_register,
       (zk_ctx* c, size_t count, const zk_webauthn_registration* r, uint8_t* verdicts, uint8_t* reasons, zk_webauthn_credential* creds),
       (c, count, r, verdicts, reasons, creds)) {
    if (!c || !r || !verdicts || count == 0 || count > ZK_WEBAUTHN_BATCH_MAX) return ZK_EINVAL;
    for (size_t i = 0; i < count; i++)
        if ((!r[i].attestation_object && r[i].attestation_object_len) || (!r[i].client_data_json && r[i].client_data_json_len) ||
            (!r[i].challenge && r[i].challenge_len) || (!r[i].origin && r[i].origin_len) || r[i].attestation_policy > ZK_WEBAUTHN_ATT_NONE_OR_SELF)
            return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    uint64_t aud0;
    int rc = call_enter(c, &aud0);
    if (rc || (rc = es256_table(c))) return rc;
    Es256Ws* w = c->es256;

    const WebauthnImage im = webauthn_register_pack(r, count);
    // the output buffer: reasons (padded to words) and credentials, which come back; settled bytes and records, which stay there
    const size_t n = im.live.size(), desc_bytes = n * sizeof(WebauthnRegisterDesc);
    const size_t bytes_n = webauthn_padded(n), down_bytes = bytes_n + n * sizeof(WebauthnCredential), out_bytes = down_bytes + bytes_n + n * 160;
    std::vector<uint8_t> out(down_bytes);
    if (n) {
        auto enqueue = [&] {
            const uint8_t* d_in = (const uint8_t*)w->in.p;
            uint8_t* d_out = (uint8_t*)w->out.p;
            uint8_t* d_settled = d_out + down_bytes;
            uint8_t* d_records = d_settled + bytes_n;
            hipLaunchKernelGGL(webauthn_register_kernel, lane_grid(n, WEBAUTHN_REGISTER_WG), dim3(WEBAUTHN_REGISTER_WG), 0, c->stream,
                               (const WebauthnRegisterDesc*)d_in, d_in + desc_bytes, (uint32_t)n, d_out, d_settled, (WebauthnCredential*)(d_out + bytes_n),
                               d_records);
            if (hipError_t e = hipGetLastError()) return e;
            if (c->audit.on)
                c->audit.op(c->stream, {w->out.p, w->table}, {w->out.p}, "webauthn register: verification of the records (es256_verify_kernel)");
            return es256_enqueue(c, d_records, (uint32_t)n, d_settled, d_out);
        };
        if ((rc = lane_round_trip(c, {{&w->in, im.bytes.data(), im.bytes.size()}}, nullptr, &w->out, out_bytes, out.data(), down_bytes,
                                  {"webauthn register: descriptors and blob upload", "webauthn register: walk, rules, records (webauthn_register_kernel)",
                                   "webauthn register: reasons and credentials download"},
                                  enqueue)))
            return rc;
        if ((rc = aud_verdict(c, aud0, ZK_OK))) return rc;
    }

    for (size_t i = 0; i < count; i++) verdicts[i] = 0;
    if (reasons) memset(reasons, ZK_WEBAUTHN_SIZE, count);
    if (creds) memset(creds, 0, count * sizeof(zk_webauthn_credential));
    for (size_t j = 0; j < n; j++) {
        const size_t i = im.live[j];
        verdicts[i] = out[j] == ZK_WEBAUTHN_VALID ? 1 : 0;
        if (reasons) reasons[i] = out[j];
        if (creds && verdicts[i]) memcpy(creds + i, out.data() + bytes_n + j * sizeof(WebauthnCredential), sizeof(WebauthnCredential));
    }
    return ZK_OK;
}
