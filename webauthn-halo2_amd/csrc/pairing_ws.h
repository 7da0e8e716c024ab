// pairing_ws.h — what the two units of the device pairing share on the host (pairing.hip: one (g2, s_g2) pair per call;
// pairing_each.hip: a G2 point per lane): the context's staging buffers and the upload of prepared lines.
#pragma once
#include "ctx.h"
#include "pairing.h"

// the context's staging buffers (grow-only) and the table of a caller's own pair
struct PairingWs {
    void *a = nullptr, *b = nullptr, *out = nullptr, *own = nullptr;
    size_t c_a = 0, c_b = 0, c_out = 0, c_own = 0;
    void *q = nullptr, *gen = nullptr;  // the G2 point of every lane (or the receipts); the table of the G2 generator, made once
    size_t c_q = 0;
};

// *p to at least `bytes` (grow-only; the stream is drained before a buffer is let go)
int pw_grow(zk_ctx* c, void** p, size_t* cap, size_t bytes);
// the context's buffers, made on first use
int pairing_ws(zk_ctx* c, PairingWs** out);
// the table of (g2, s_g2) into the device buffer d (sizeof(PairingTable) bytes), waited for
int pairing_table_upload(zk_ctx* c, const G2A& g2, const G2A& s_g2, void* d);
// the resident pair's table, made on first use and kept with the SRS view
int pairing_resident_table(zk_ctx* c, const void** out);
