// es256.h — what es256.hip shares with webauthn.hip: the context's ES256 state and the launch of the verification kernel.
#pragma once
#include "ctx.h"
#include "p256.hip.h"

// the context's ES256 state: the comb of G and the grow-only staging buffers (zk_es256_verify and zk_webauthn_verify both stage
// through them: the context's lock lets one call at a time use them)
struct Es256Ws {
    P256Affine* table = nullptr;
    void *in = nullptr, *out = nullptr;
    size_t c_in = 0, c_out = 0;
};

// grow-only: *p holds at least `bytes` afterwards (the stream is drained before a smaller buffer is freed)
int es256_grow(zk_ctx* c, void** p, size_t* cap, size_t bytes);
// c->es256 and its comb of G exist afterwards (built on the first call of a context).  Caller holds the context lock, device bound
int es256_table(zk_ctx* c);
// es256_verify_kernel over `count` 160-byte device records on the main stream.  d_settled: null, or one byte per record - a lane
// whose byte is not ZK_ES256_VALID returns at once and leaves d_reasons[i] alone (the two may be one array)
hipError_t es256_enqueue(zk_ctx* c, const uint8_t* d_sigs, uint32_t count, const uint8_t* d_settled, uint8_t* d_reasons);
