// pairing_ws.h — what the two units of the device pairing share on the host (pairing.hip: one (g2, s_g2) pair per call;
// pairing_each.hip: a G2 point per lane): the context's staging buffers and the upload of prepared lines.  The round trip of a
// call is lane_call.h's.
#pragma once
#include "lane_call.h"
#include "pairing.h"

// the context's staging buffers and the table of a caller's own pair
struct PairingWs {
    DevBuf a, b, out, own;
    DevBuf q;             // the G2 point of every lane (or the receipts)
    void* gen = nullptr;  // the table of the G2 generator, made once
    ~PairingWs() { if (gen) hipFree(gen); }
};

// the context's buffers, made on first use
int pairing_ws(zk_ctx* c, PairingWs** out);
// the table of (g2, s_g2) into the device buffer d (sizeof(PairingTable) bytes), waited for
int pairing_table_upload(zk_ctx* c, const G2A& g2, const G2A& s_g2, void* d);
// the resident pair's table, made on first use and kept with the SRS view
int pairing_resident_table(zk_ctx* c, const void** out);
