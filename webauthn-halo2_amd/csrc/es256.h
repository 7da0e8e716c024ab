// es256.h — what es256.hip shares with webauthn.hip and webauthn_register.hip: the context's ES256 state and the launch of the
// verification kernel.  The round trip of a call is lane_call.h's.
#pragma once
#include "lane_call.h"
#include "p256.hip.h"

// the context's ES256 state: the comb of G and the staging buffers (zk_es256_verify, zk_webauthn_verify and zk_webauthn_register
// all stage through them: the context's lock lets one call at a time use them)
struct Es256Ws {
    P256Affine* table = nullptr;
    DevBuf in, out;
    ~Es256Ws() { if (table) hipFree(table); }
};

// c->es256 and its comb of G exist afterwards (built on the first call of a context).  Caller holds the context lock, device bound
int es256_table(zk_ctx* c);
// es256_verify_kernel over `count` 160-byte device records on the main stream.  d_settled: null, or one byte per record - a lane
// whose byte is not ZK_ES256_VALID returns at once and leaves d_reasons[i] alone (the two may be one array)
hipError_t es256_enqueue(zk_ctx* c, const uint8_t* d_sigs, uint32_t count, const uint8_t* d_settled, uint8_t* d_reasons);
