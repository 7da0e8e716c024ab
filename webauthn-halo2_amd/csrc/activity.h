// activity.h — how busy a device is, as far as this process can see: contexts that enqueued an MSM pass within the last few
// milliseconds.  Pure C++, no HIP (tests/activity_logic_check.cpp runs it with made-up clocks); the context's side of it is
// streams.hip ctx_activity_*.  Every context owns a slot of its device's table and stamps it in ctx_msm_begin_batch — the one
// place every MSM pass goes through, whoever asked for it (zk_prove, zk_commit / zk_commit_batch, zk_msm_srs, zk_msm_bn254,
// zk_keygen, zk_pk_read): a host that drives the phase-level ABI from four threads is seen exactly like four zk_prove calls
// (round 4 counted zk_prove calls only).  PROCESS-LOCAL: contexts of other processes on the same GPU are invisible.
#pragma once
#include <stdint.h>

#include <atomic>
#include <chrono>

namespace zk {
namespace activity {

constexpr int DEVICES = 64, SLOTS = 64;
constexpr int64_t WINDOW_NS = 4 * 1000 * 1000;  // a proving context enqueues a pass every 0.3 .. 1.5 ms
// ... but not during its quotient / evaluation / multi-open phases, which under four pipelines last longer than the window: a
// context inside a whole-proof call (zk_prove, zk_prove_batch) holds its slot "active" for the length of the call (hold), or
// the count would dip to two or three several times per proof and passes of the OTHER contexts would take the side-stream
// regime under full load
constexpr int64_t HELD = INT64_MAX;

struct Table {
    std::atomic<int64_t> ts[DEVICES][SLOTS];  // 0: never stamped; HELD; or the time of the last stamp
    std::atomic<uint64_t> used[DEVICES];
};
inline Table g_table;  // (one per process: static storage, zero-initialised)

// one context's part: its slot and the ZK_OPT_ACTIVITY_HOLD rules
struct State {
    int slot = -1;         // this context's slot in its device's table; -1: none (65th context of a device, device outside the table)
    bool held = false;     // inside a whole-proof call: the slot counts as active whatever its last stamp
    bool no_hold = false;  // ZK_OPT_ACTIVITY_HOLD = 1: round 5's rule (stamps only)
    bool pinned = false;   // ZK_OPT_ACTIVITY_HOLD = 2: active until the option is changed
};

inline int64_t now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline bool device_ok(int device) { return device >= 0 && device < DEVICES; }

inline void register_slot(State& s, int device) {
    s.slot = -1;
    if (!device_ok(device)) return;
    std::atomic<uint64_t>& used = g_table.used[device];
    uint64_t cur = used.load();
    for (;;) {
        if (~cur == 0) return;  // more than 64 contexts on one device: the surplus ones are not counted
        const int slot = __builtin_ctzll(~cur);
        if (used.compare_exchange_weak(cur, cur | (1ull << slot))) {
            g_table.ts[device][slot].store(0);
            s.slot = slot;
            return;
        }
    }
}
inline void unregister_slot(State& s, int device) {
    if (s.slot < 0 || !device_ok(device)) return;
    g_table.ts[device][s.slot].store(0);
    g_table.used[device].fetch_and(~(1ull << s.slot));
    s.slot = -1;
}
// registered contexts active on a device at `now`: held, or stamped within the window
inline int count(int device, int64_t now) {
    if (!device_ok(device)) return 0;
    int active = 0;
    uint64_t used = g_table.used[device].load();
    while (used) {
        const int slot = __builtin_ctzll(used);
        used &= used - 1;
        const int64_t ts = g_table.ts[device][slot].load();
        if (ts && (ts == HELD || now - ts < WINDOW_NS)) active++;
    }
    return active;
}
// stamps this context and returns the number of contexts (this one included) active on its device
inline int touch(State& s, int device, int64_t now) {
    if (!device_ok(device)) return 1;
    if (s.slot >= 0 && !s.held) g_table.ts[device][s.slot].store(now);
    return (s.slot >= 0 ? 0 : 1) + count(device, now);
}
// a whole-proof call begins / ends on this context (prover.hip ProveQuiesce)
inline void hold(State& s, int device, bool on, int64_t now) {
    if (on && s.no_hold) return;  // ZK_OPT_ACTIVITY_HOLD = 1
    if (!on && s.pinned) return;  // ZK_OPT_ACTIVITY_HOLD = 2: the host holds this context active itself
    s.held = on;
    if (s.slot < 0 || !device_ok(device)) return;
    g_table.ts[device][s.slot].store(on ? HELD : now);
}
// ZK_OPT_ACTIVITY_HOLD = value.  2: held from now on, whatever the entry points used (a phase-level host's worker context);
// 0 / 1 let go of such a hold
inline void set_option(State& s, int device, int value, int64_t now) {
    s.no_hold = value == 1;
    s.pinned = value == 2;
    if (!s.held || value != 2) hold(s, device, false, now);
    if (value == 2) hold(s, device, true, now);
}

}  // namespace activity
}  // namespace zk
