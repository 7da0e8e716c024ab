// streams.hip — the per-device stream pool, the measured placement of its streams (zk_stream_placement) and the context's side
// of the activity table (activity.h).
#include <algorithm>
#include <chrono>

#include "ctx.h"
#include "placement.h"

// ---- streams are kept, not destroyed, and made in a deliberate order (round 6).  The HIP runtime ties a stream to one of its
// (four) hardware queues when the stream is made: the first four streams of a process get a queue each, every later one the queue
// with the fewest streams on it (ties: the highest queue) — read off rocprofv3's Queue_Id with tools/queue_map.py.  Streams that
// share a queue run in order, so WHICH streams share matters: a process that had destroyed a set of contexts got 190 instead of 228
// proofs/s from its next four pipelines (k = 17, tools/inflight_k17.py 4 4: main streams sharing queues), and a context whose lone
// proof finds its tail and its transform stream on one queue takes 12.0 instead of 11.1 ms (k = 19).  So the first context of a
// device makes, in this order, the MAIN streams of the device's first four contexts (queues 0 .. 3) and then four blocks of four
// side streams (each block: queues 3, 2, 1, 0) - and the same again for four more contexts (main streams on queues 3 .. 0).  Context slot i owns main stream i and, from block i, the side streams that do
// not sit on its main's queue: its tail stream on queue 3 - i (so that the tails of the first two pipelines do not meet either),
// its transform and MSM streams on the other two.  zk_ctx_destroy drains the slot's streams and frees the slot for the next
// context; contexts beyond the eight slots (and a main stream made at its own priority, ZK_OPT_STREAM_PRIORITY) make their streams as
// before and destroy them.  The pool is never freed (40 idle streams per device for the life of the process).  If another runtime
// assigns queues differently nothing breaks: this is placement, not correctness.  zk_stream_placement (below) measures which
// streams really share a queue and, asked to, deals the slots again from what it measured.
namespace {
constexpr int POOL_SLOTS = placement::POOL_SLOTS;  // two layers of four: slots 4 .. 7 repeat the pattern (their main streams land on queues 3 .. 0)
struct StreamSlots {
    bool primed = false;
    hipStream_t main[POOL_SLOTS] = {};
    hipStream_t side[POOL_SLOTS][4] = {};  // [slot][j]: block `slot`, j-th made: queue 3 - j
    bool used[POOL_SLOTS] = {};
    // zk_stream_placement: streams a calibration left over or made beyond its need (never destroyed), the pinned stamps of the
    // probe, and the class of every stream as last measured
    bool made = false;  // all forty streams exist
    hipStream_t parked[placement::MAX_STREAMS] = {};
    int n_parked = 0;
    placement::Stamp* stamps = nullptr;
    std::map<hipStream_t, uint8_t> cls;
};
struct StreamPool {
    std::mutex mu;
    std::map<int, StreamSlots> dev;
};
StreamPool& stream_pool() {
    static StreamPool* p = new StreamPool();  // (leaked on purpose: the HIP runtime may be gone before static destructors run)
    return *p;
}
// the hardware queue of slot s's main stream under the runtime's rule (first four streams: a queue each; then the least loaded
// queue, ties to the highest): layer 0 = queues 0 .. 3, layer 1 (made after layer 0's side blocks) = queues 3 .. 0
using placement::slot_main_queue;
// makes the device's streams on first use (current device = the pool's; the pool's mutex is held)
void pool_prime(StreamSlots& d) {
    if (d.primed) return;
    d.primed = true;
    bool ok = true;
    for (int layer = 0; layer < POOL_SLOTS / 4 && ok; layer++) {
        for (int i = 4 * layer; i < 4 * layer + 4 && ok; i++) ok = hipStreamCreate(&d.main[i]) == hipSuccess;
        for (int i = 4 * layer; i < 4 * layer + 4 && ok; i++)
            for (int j = 0; j < 4 && ok; j++) ok = hipStreamCreate(&d.side[i][j]) == hipSuccess;
    }
    d.made = ok;
    if (!ok) {  // (out of resources: no slots on this device, contexts make their own streams)
        for (int i = 0; i < POOL_SLOTS; i++) d.used[i] = true;
    }
}
}  // namespace
// a free slot of the device (current device = `device`), or -1: the caller makes its own streams
int pool_take_slot(int device, hipStream_t* main_out) {
    StreamPool& p = stream_pool();
    std::lock_guard<std::mutex> lk(p.mu);
    StreamSlots& d = p.dev[device];
    pool_prime(d);
    // layer 1 is handed out from the top: slot 7's main stream shares queue 0 with slot 0's, so the fifth context doubles up with the
    // FIRST one (the oldest, most likely idle: a set-up or probe context) rather than with the fourth
    static const int order[POOL_SLOTS] = {0, 1, 2, 3, 7, 6, 5, 4};
    for (int k = 0; k < POOL_SLOTS; k++) {
        const int i = order[k];
        if (!d.used[i]) {
            d.used[i] = true;
            *main_out = d.main[i];
            return i;
        }
    }
    return -1;
}
void pool_release_slot(int device, int slot) {
    StreamPool& p = stream_pool();
    std::lock_guard<std::mutex> lk(p.mu);
    StreamSlots& d = p.dev[device];
    hipStreamSynchronize(d.main[slot]);
    for (int j = 0; j < 4; j++) hipStreamSynchronize(d.side[slot][j]);
    d.used[slot] = false;
}
// role: 0 the tail stream, 1 the transform stream, 2 the MSM stream
int ctx_side_stream(zk_ctx* c, hipStream_t* out, int role) {
    if (*out) return ZK_OK;
    if (c->stream_slot >= 0) {
        // side j sits on queue 3 - j: the tail takes the queue opposite the main's, never the main's own, whose side stream is
        // the block's spare (placement.h role_side)
        const int i = c->stream_slot;
        StreamPool& p = stream_pool();
        std::lock_guard<std::mutex> lk(p.mu);
        *out = p.dev[c->device].side[i][placement::role_side(i, role)];
        return ZK_OK;
    }
    return hipStreamCreate(out) == hipSuccess ? ZK_OK : ZK_EHIP;
}

// the two further streams a LONE proof spreads over (ctx.h xform_stream, msm_stream), made when the first such proof asks
int ctx_lone_streams(zk_ctx* c) {
    if (ctx_side_stream(c, &c->xform_stream, 1) || ctx_side_stream(c, &c->msm_stream, 2)) return ZK_EHIP;
    return ZK_OK;
}

// ---- the context's side of the activity table (activity.h): how busy the device is, as far as this process can see
void ctx_activity_register(zk_ctx* c) { activity::register_slot(c->act, c->device); }
void ctx_activity_unregister(zk_ctx* c) { activity::unregister_slot(c->act, c->device); }
// stamps this context and returns the number of contexts (this one included) active on its device
int ctx_activity_touch(zk_ctx* c) { return activity::touch(c->act, c->device, activity::now_ns()); }
// a whole-proof call begins / ends on this context (prover.hip ProveQuiesce)
void ctx_activity_hold(zk_ctx* c, bool on) { activity::hold(c->act, c->device, on, activity::now_ns()); }
// ---- zk_stream_placement: which hardware queue each pool stream sits on, measured (placement.h / placement.hip), and on
// request the pool dealt again from the measurement.  The whole call holds the pool's mutex: no context is made, destroyed or
// given a side stream meanwhile.  PROCESS-LOCAL like the activity table: work of other processes on the GPU is not seen.
namespace {
// every stream of the device in the probe's index order: main[0 .. 8), side[0 .. 8)[0 .. 4), parked
int pool_list(const StreamSlots& d, hipStream_t* list) {
    int n = 0;
    for (int i = 0; i < POOL_SLOTS; i++) list[n++] = d.main[i];
    for (int i = 0; i < POOL_SLOTS; i++)
        for (int j = 0; j < 4; j++) list[n++] = d.side[i][j];
    for (int i = 0; i < d.n_parked; i++) list[n++] = d.parked[i];
    return n;
}
placement::Classes pool_measure(StreamSlots& d, zk_placement* rep) {
    hipStream_t list[placement::MAX_STREAMS];
    const int n = pool_list(d, list);
    const placement::Classes c = placement_probe(list, n, d.stamps);
    d.cls.clear();
    if (!c.unresolved)
        for (int i = 0; i < n; i++) d.cls[list[i]] = c.cls[i];
    const uint32_t rounds = rep->rounds + c.rounds;
    placement::report(c, rep);
    rep->rounds = rounds;
    rep->streams = (uint32_t)n;
    return c;
}
int placement_run(int device, int mode, zk_placement* rep) {
    const auto h0 = std::chrono::steady_clock::now();
    StreamPool& p = stream_pool();
    std::lock_guard<std::mutex> lk(p.mu);
    if (activity::count(device, activity::now_ns()) > 0) return ZK_ESTATE;
    StreamSlots& d = p.dev[device];
    if (mode == 1 && d.made)
        for (int i = 0; i < POOL_SLOTS; i++)
            if (d.used[i]) return ZK_ESTATE;
    pool_prime(d);
    if (!d.made) return ZK_EHIP;  // (the device gave no forty streams: there is no pool to place)
    if (!d.stamps && hipHostMalloc(&d.stamps, placement::MAX_STREAMS * sizeof(placement::Stamp)) != hipSuccess) return ZK_EHIP;
    memset(rep, 0, sizeof(*rep));
    placement::Classes c = pool_measure(d, rep);
    if (c.error) return ZK_EHIP;
    bool calibrated = false;
    while (mode == 1 && !calibrated && !c.unresolved && c.n_classes == 4 && (rep->flags & ZK_PLACEMENT_OK) != ZK_PLACEMENT_OK) {
        const placement::Deal dl = placement::deal(c);
        if (dl.dealt) {
            hipStream_t list[placement::MAX_STREAMS];
            pool_list(d, list);
            for (int i = 0; i < POOL_SLOTS; i++) {
                d.main[i] = list[dl.main[i]];
                for (int j = 0; j < 4; j++) d.side[i][j] = list[dl.side[i][j]];
            }
            for (int i = 0; i < dl.n_parked; i++) d.parked[i] = list[dl.parked[i]];
            d.n_parked = dl.n_parked;
            calibrated = true;
        } else {
            // a class is short: further streams, wherever the runtime puts them, measured with the rest — at least four at a
            // time: a runtime that balances its queues fills the short ones within one turn
            const int make = std::min(std::max(dl.need_more, 4), placement::MAX_STREAMS - c.n);
            if (make <= 0) break;
            for (int i = 0; i < make; i++)
                if (hipStreamCreate(&d.parked[d.n_parked]) == hipSuccess) d.n_parked++;
                else return ZK_EHIP;
        }
        c = pool_measure(d, rep);  // the streams in their new places (or with the new ones)
        if (c.error) return ZK_EHIP;
    }
    if (calibrated) rep->flags |= ZK_PLACEMENT_CALIBRATED;
    rep->probe_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - h0).count();
    return ZK_OK;
}
}  // namespace

ZK_API(zk_stream_placement, (int device_id, int mode, zk_placement* out), (device_id, mode, out)) {
    if (!out || (mode != 0 && mode != 1)) return ZK_EINVAL;
    if (int rc = device_id_ok(device_id)) return rc;
    DeviceScope dev(device_id);
    if (!dev.ok) return ZK_EHIP;
    zk_placement rep;
    const int rc = placement_run(device_id, mode, &rep);
    if (rc == ZK_OK) *out = rep;
    return rc;
}

ZK_API(zk_ctx_stream_info, (zk_ctx* c, zk_ctx_streams* out), (c, out)) {
    if (!c || !out) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s[4] = {c->stream, c->tail_stream, c->xform_stream, c->msm_stream};
    StreamPool& p = stream_pool();
    std::lock_guard<std::mutex> lp(p.mu);
    const StreamSlots& d = p.dev[c->device];
    out->slot = c->stream_slot;
    for (int q = 0; q < 4; q++) {
        // a side stream the context has not asked for yet: the one its slot holds for that role
        if (!s[q] && q > 0 && c->stream_slot >= 0) s[q] = d.side[c->stream_slot][placement::role_side(c->stream_slot, q - 1)];
        const auto it = d.cls.find(s[q]);
        out->queue[q] = it == d.cls.end() ? placement::UNKNOWN : it->second;
        out->counts[q] = c->stream_counts[q];
    }
    return ZK_OK;
}
