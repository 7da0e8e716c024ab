// placement.h — which hardware queue each stream of the pool sits on: the host logic of zk_stream_placement (include/zkmi355.h).
// Pure C++, no HIP: time stamps -> classes, classes -> the report's flags, classes -> a deal of the pool
// (tests/placement_logic_check.cpp runs it on made-up stamps).  The device half — the kernel that takes the stamps — is placement.hip.
//
// THE MEASUREMENT.  Kernels of streams that share a hardware queue run in order; kernels of streams on different queues run side
// by side (streams.hip "streams are kept").  A one-workgroup kernel stamps the constant 100 MHz counter when it starts, spins for a
// given number of ticks and stamps it again.  One ROUND picks a pivot stream, enqueues a LONG spin (T_p) on it and then a SHORT
// one (T_s) on every other stream that has no class yet:
//   * a short kernel that started at or after the pivot's end waited behind it: same queue, same class;
//   * one that started more than a GUARD interval before the pivot's end ran beside it: another queue;
//   * anything in between (or a round the host took too long to enqueue) is ambiguous: the round is repeated once, and if it
//     is ambiguous again the whole result is UNRESOLVED (n_queues = 0) rather than a guess.
// Rounds go on (pivot = the first stream without a class) until every stream has one: one round per class.  More than
// MAX_CLASSES classes is unresolved too (a runtime that runs streams of one queue side by side would show a class per stream).
//
// THE CONSTANTS, in ticks of 10 ns, for n streams in a round (the pool has 40, a calibrated device at most 64):
//   T_s   = 50 us.  Long against what separates two kernels that follow each other on one queue (a few us of dispatch) and
//           against any skew of the counter between compute units (it is one chip-wide counter), short enough that n of them
//           in a row stay in the low milliseconds.
//   GUARD = 1 ms = 20 T_s.  A short kernel on ANOTHER queue starts as soon as its own queue lets it; nothing ties that moment
//           to the pivot's end, so the band "less than GUARD before the end" is hit only by accident and costs a repeat.
//   E(n)  = 50 us x n: the host's budget for enqueueing the round (a launch is 5 - 10 us; the host times itself, and a round
//           that took longer — a descheduled thread — is discarded as ambiguous, because a late launch looks like a wait).
//   T_p   = (n - 1) T_s + E(n) + 2 GUARD.  The latest start of a short kernel on another queue: every other short kernel
//           serialised before it on its queue, (n - 2) T_s, and the last launch leaving the host E(n) after the pivot's — that
//           must lie more than GUARD before the pivot's end; the second GUARD covers the dispatch gaps between n serialised
//           kernels.  n = 40: 1.95 + 2.0 + 2.0 = 5.95 ms; n = 64: 8.35 ms.
// A probe is a warm-up launch per stream plus one round per class, each T_p plus the short kernels queued behind the pivot:
// four classes of ten -> 4 x (5.95 + 0.5) ms + synchronisation.  Measured on an MI355X: 27 - 29 ms for 40 or 44 streams on four
// queues, 15 ms on two, 95 ms for a calibration that makes streams (three probes); a process's first call adds the runtime's
// start-up and the forty hipStreamCreate, 140 - 400 ms (docs/experiments.md "stream placement probe").
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/zkmi355.h"

namespace zk {
namespace placement {

constexpr int POOL_SLOTS = 8, POOL_SIDES = 4;
constexpr int POOL_STREAMS = POOL_SLOTS + POOL_SLOTS * POOL_SIDES;  // 40: index i < 8 = main[i], 8 + 4 i + j = side[i][j]
constexpr int MAX_STREAMS = 64;                                     // per device, parked surplus of a calibration included
constexpr int MAX_CLASSES = 9;
constexpr uint8_t UNKNOWN = 255;

constexpr uint64_t TICKS_PER_US = 100;
constexpr uint64_t T_SHORT = 50 * TICKS_PER_US;
constexpr uint64_t GUARD = 1000 * TICKS_PER_US;
constexpr uint64_t enqueue_budget(int n) { return 50 * TICKS_PER_US * (uint64_t)n; }
constexpr uint64_t t_pivot(int n) { return (uint64_t)(n > 1 ? n - 1 : 0) * T_SHORT + enqueue_budget(n) + 2 * GUARD; }

struct Stamp {
    uint64_t t0, t1;  // the counter when the kernel started / after its spin; 0 = never written
};

enum Verdict { OTHER = 0, SAME = 1, AMBIGUOUS = 2 };
inline Verdict judge(const Stamp& pivot, const Stamp& s) {
    if (pivot.t0 == 0 || pivot.t1 <= pivot.t0 || s.t0 == 0 || s.t1 < s.t0) return AMBIGUOUS;  // a kernel that did not run
    if (s.t0 >= pivot.t1) return SAME;
    if (s.t0 + GUARD < pivot.t1) return OTHER;
    return AMBIGUOUS;
}

struct Classes {
    int n = 0;                 // streams
    int n_classes = 0;         // 0: unresolved
    bool unresolved = false;
    int error = 0;             // what a round returned below zero (a HIP failure), classification abandoned
    uint32_t rounds = 0;
    uint8_t cls[MAX_STREAMS];  // class of stream i, numbered in order of first appearance; UNKNOWN when unresolved
};

// run(pivot, active, stamps): enqueue one round — the long spin on `pivot`, short ones on every other i with active[i] —, wait
// for it and fill stamps[i] for those streams.  Returns 0, 1 (the host overran its budget: discard the round) or < 0 (error).
template <class Run>
inline Classes classify(int n, Run&& run) {
    Classes r;
    r.n = n;
    memset(r.cls, UNKNOWN, sizeof(r.cls));
    auto give_up = [&r]() {
        r.unresolved = true;
        r.n_classes = 0;
        memset(r.cls, UNKNOWN, sizeof(r.cls));
        return r;
    };
    if (n < 1 || n > MAX_STREAMS) return give_up();
    int k = 0;
    for (;;) {
        int pivot = -1, others = 0;
        uint8_t active[MAX_STREAMS] = {0};
        for (int i = 0; i < n; i++)
            if (r.cls[i] == UNKNOWN) {
                active[i] = 1;
                if (pivot < 0) pivot = i;
                else others++;
            }
        if (pivot < 0) break;
        if (k == MAX_CLASSES) return give_up();
        if (others == 0) {  // the last stream without a class has nothing left to share a queue with
            r.cls[pivot] = (uint8_t)k++;
            break;
        }
        Stamp st[MAX_STREAMS];
        bool ambiguous = true;
        for (int attempt = 0; attempt < 2 && ambiguous; attempt++) {
            memset(st, 0, sizeof(st));
            const int rc = run(pivot, (const uint8_t*)active, st);
            r.rounds++;
            if (rc < 0) {
                r.error = rc;
                return give_up();
            }
            ambiguous = rc != 0;
            for (int i = 0; i < n && !ambiguous; i++)
                if (active[i] && i != pivot && judge(st[pivot], st[i]) == AMBIGUOUS) ambiguous = true;
        }
        if (ambiguous) return give_up();
        r.cls[pivot] = (uint8_t)k;
        for (int i = 0; i < n; i++)
            if (active[i] && i != pivot && judge(st[pivot], st[i]) == SAME) r.cls[i] = (uint8_t)k;
        k++;
    }
    r.n_classes = k;
    return r;
}

// which side stream of its block a pooled context takes for a role (0 tail, 1 transform, 2 MSM; 3: the block's spare).  Side j is
// meant to sit on queue 3 - j and the slot's main stream on queue mq = slot_main_queue(slot): the tail takes the queue opposite
// the main's (j = mq, queue 3 - mq), transform and MSM the two others, and j = 3 - mq — the main's own queue — stays spare.
constexpr int slot_main_queue(int s) { return s < 4 ? s : 7 - s; }
inline int role_side(int slot, int role) {
    const int mq = slot_main_queue(slot);
    int js[4], m = 0;
    js[m++] = mq;
    for (int j = 0; j < 4; j++)
        if (j != mq && j != 3 - mq) js[m++] = j;
    js[m++] = 3 - mq;
    return js[role];
}
constexpr int main_index(int slot) { return slot; }
constexpr int side_index(int slot, int j) { return POOL_SLOTS + POOL_SIDES * slot + j; }

// the report of the pool's first POOL_STREAMS classes (cls in the index order above).  Fills everything but rounds / streams /
// probe_ms; CALIBRATED is the caller's.
inline void report(const Classes& c, zk_placement* out) {
    memset(out, 0, sizeof(*out));
    memset(out->main_queue, UNKNOWN, sizeof(out->main_queue));
    memset(out->role_queue, UNKNOWN, sizeof(out->role_queue));
    memset(out->spare_queue, UNKNOWN, sizeof(out->spare_queue));
    if (c.unresolved || c.n_classes == 0 || c.n < POOL_STREAMS) {
        out->flags = ZK_PLACEMENT_UNRESOLVED;
        return;
    }
    uint32_t seen = 0;
    for (int i = 0; i < POOL_STREAMS; i++) seen |= 1u << c.cls[i];
    out->n_queues = (uint32_t)__builtin_popcount(seen);
    for (int s = 0; s < POOL_SLOTS; s++) {
        out->main_queue[s] = c.cls[main_index(s)];
        for (int role = 0; role < 3; role++) out->role_queue[s][role] = c.cls[side_index(s, role_side(s, role))];
        out->spare_queue[s] = c.cls[side_index(s, role_side(s, 3))];
    }
    auto distinct4 = [](uint8_t a, uint8_t b, uint8_t d, uint8_t e) { return a != b && a != d && a != e && b != d && b != e && d != e; };
    uint32_t f = 0;
    if (distinct4(out->main_queue[0], out->main_queue[1], out->main_queue[2], out->main_queue[3])) f |= ZK_PLACEMENT_MAINS_OK;
    bool lone = true, layer1 = true;
    for (int s = 0; s < POOL_SLOTS; s++)
        lone = lone && distinct4(out->main_queue[s], out->role_queue[s][0], out->role_queue[s][1], out->role_queue[s][2]);
    for (int s = 0; s < 4; s++) layer1 = layer1 && out->main_queue[7 - s] == out->main_queue[s];
    if (lone) f |= ZK_PLACEMENT_LONE_OK;
    if (distinct4(out->main_queue[0], out->main_queue[1], out->role_queue[0][0], out->role_queue[1][0])) f |= ZK_PLACEMENT_PAIR_OK;
    if (layer1) f |= ZK_PLACEMENT_LAYER1_OK;
    out->flags = f;
}

// THE DEAL.  The pool's code relies on: main[i] on class i (i < 4), main[7 - i] on main[i]'s class, side[i][j] on the class of
// main[3 - j] — ten streams of each of four classes.  From measured classes of n streams (the pool's and any parked ones) the
// deal picks, per class, its first ten streams in index order: two mains, then one side stream per slot.  A pool that already
// follows the rule is dealt to itself.  With another number of classes than four nothing is dealt (dealt = false, need_more = 0:
// the invariants cannot hold); a class short of ten streams asks for `need_more` further streams to be made and measured.
struct Deal {
    bool dealt = false;
    int need_more = 0;
    int main[POOL_SLOTS];
    int side[POOL_SLOTS][POOL_SIDES];
    int parked[MAX_STREAMS];  // the streams the deal leaves over, in index order
    int n_parked = 0;
};
inline Deal deal(const Classes& c) {
    Deal d;
    if (c.unresolved || c.n_classes != 4) return d;
    int list[4][MAX_STREAMS], cnt[4] = {0, 0, 0, 0};
    for (int i = 0; i < c.n; i++) {
        if (c.cls[i] > 3) return d;
        list[c.cls[i]][cnt[c.cls[i]]++] = i;
    }
    const int per = 2 + POOL_SLOTS;
    for (int q = 0; q < 4; q++)
        if (cnt[q] < per) d.need_more += per - cnt[q];
    if (d.need_more) return d;
    for (int q = 0; q < 4; q++) {
        d.main[q] = list[q][0];
        d.main[7 - q] = list[q][1];
        for (int s = 0; s < POOL_SLOTS; s++) d.side[s][3 - q] = list[q][2 + s];
        for (int m = per; m < cnt[q]; m++) d.parked[d.n_parked++] = list[q][m];
    }
    // (parked streams in index order: a later probe numbers the same streams the same way)
    for (int a = 1; a < d.n_parked; a++)
        for (int b = a; b > 0 && d.parked[b - 1] > d.parked[b]; b--) {
            const int t = d.parked[b];
            d.parked[b] = d.parked[b - 1];
            d.parked[b - 1] = t;
        }
    d.dealt = true;
    return d;
}

}  // namespace placement

#ifdef __HIPCC__
// the device half (placement.hip): classes of streams[0 .. n) of the current device; `stamps`: pinned host memory for MAX_STREAMS stamps
placement::Classes placement_probe(const hipStream_t* streams, int n, placement::Stamp* stamps);
#endif

}  // namespace zk
