// lane_call.h — the host side of the calls with one item per lane (zk_pairing_check_batch, zk_pairing_check_each,
// zk_srs_contribution_check_batch, zk_es256_verify, zk_webauthn_verify, zk_webauthn_register): `count` independent items are
// uploaded, decided in one or two launches, and one reason byte per item (with whatever else a lane wrote) comes back.  No kernels
// here: the grow-only device buffer the calls stage through, the prelude of an entry point, the grid of `count` lanes, and the
// round trip itself.  What differs between the calls comes in as data or as the callable that enqueues the launches.
#pragma once
#include <algorithm>
#include <initializer_list>

#include "ctx.h"

// a device buffer that only grows: the contexts' staging buffers (PairingWs, Es256Ws)
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    ~DevBuf() { release(); }  // (with the device of its context current: the *_ws_destroy functions)
    void release() {
        if (p) hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // at least `bytes` afterwards, 4096 at the least; the stream is drained before a smaller buffer is let go
    int grow(zk_ctx* c, size_t bytes) {
        if (cap >= bytes) return ZK_OK;
        if (p) hipStreamSynchronize(c->stream);
        release();
        const size_t want = std::max<size_t>(bytes, 4096);
        if (hipMalloc(&p, want) != hipSuccess) return ZK_ENOMEM;
        cap = want;
        return ZK_OK;
    }
};

// The prelude of an entry point, under the context's lock: the device bound, the audit's violation count remembered for
// aud_verdict, and the ledger's cache of allocation bases dropped (allocations may have changed hands since the last call)
static inline int call_enter(zk_ctx* c, uint64_t* aud0) {
    if (int rc = ctx_bind(c)) return rc;
    *aud0 = c->audit.violations;
    c->audit.base_of.clear();
    return ZK_OK;
}

// the grid of `count` lanes in workgroups of `wg`
static inline dim3 lane_grid(size_t count, uint32_t wg) { return dim3((uint32_t)((count + wg - 1) / wg)); }

struct LaneUpload { DevBuf* to; const void* from; size_t bytes; };  // from: host memory

// One round trip on the context's main stream; label: the ledger's names of upload, launch and download.  The buffers of `up` (at
// most three) and `out` are grown (out to out_bytes: a call may keep more there than it fetches); the uploads go out under one
// ledger entry; the launch is entered as reading the uploaded buffers and `table` (a resident input of the kernel, or null) and
// writing `out`; enqueue() launches and returns hipGetLastError() - a call of two launches checks the first, enters the second in
// the ledger itself and returns the second's; out[0 .. host_bytes) comes back into `host` under one entry, and the stream is
// waited for (the host arrays are pageable)
template <class Enqueue>
int lane_round_trip(zk_ctx* c, std::initializer_list<LaneUpload> up, const void* table, DevBuf* out, size_t out_bytes, void* host, size_t host_bytes,
                    const char* const (&label)[3], Enqueue&& enqueue) {
    for (const LaneUpload& u : up)
        if (int rc = u.to->grow(c, u.bytes)) return rc;
    if (int rc = out->grow(c, out_bytes)) return rc;
    const void *bufs[4], *const written = out->p;
    size_t n = 0;
    for (const LaneUpload& u : up) bufs[n++] = u.to->p;
    c->audit.op_v(c->stream, nullptr, 0, bufs, n, label[0]);  // (returns at once with the audit off)
    for (const LaneUpload& u : up) HIPCHK(c, hipMemcpyAsync(u.to->p, u.from, u.bytes, hipMemcpyHostToDevice, c->stream));
    bufs[n] = table;  // (the ledger skips a null)
    c->audit.op_v(c->stream, bufs, n + 1, &written, 1, label[1]);
    HIPCHK(c, enqueue());
    c->audit.op_v(c->stream, &written, 1, nullptr, 0, label[2]);
    HIPCHK(c, hipMemcpyAsync(host, out->p, host_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, aud_sync(c, c->stream));
    return ZK_OK;
}
