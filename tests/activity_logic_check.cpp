// Host-only check of the activity table (csrc/activity.h) with made-up clocks: slots, the window's edge, holds and the
// ZK_OPT_ACTIVITY_HOLD rules.  The table is the process's one: every block leaves it as it found it.
#include <cstdio>
#include "activity.h"
using namespace zk::activity;

static int fails = 0;
#define EXPECT(cond)                                           \
    do {                                                       \
        if (!(cond)) {                                         \
            printf("FAILED line %d: %s\n", __LINE__, #cond);   \
            fails++;                                           \
        }                                                      \
    } while (0)

int main() {
    const int D = 3;               // the device of most blocks
    const int64_t T = 1000000000;  // a stamp, ns
    {   // register gives distinct slots; the 65th context of a device gets none, yet counts itself in touch
        State s[SLOTS + 1];
        uint64_t seen = 0;
        for (int i = 0; i < SLOTS; i++) {
            register_slot(s[i], D);
            EXPECT(s[i].slot >= 0 && s[i].slot < SLOTS && !(seen >> s[i].slot & 1));
            if (s[i].slot >= 0) seen |= 1ull << s[i].slot;
        }
        EXPECT(~seen == 0);
        register_slot(s[SLOTS], D);
        EXPECT(s[SLOTS].slot == -1);
        EXPECT(count(D, T) == 0);              // registered, never stamped: not active
        EXPECT(touch(s[SLOTS], D, T) == 1);    // nobody else active: itself
        EXPECT(touch(s[0], D, T) == 1);
        EXPECT(touch(s[SLOTS], D, T) == 2);    // s[0] and itself
        EXPECT(count(D, T) == 1);              // ... but the table holds no stamp of the surplus context
        EXPECT(count(D + 1, T) == 0);          // another device sees nothing of it
        // unregister frees the slot for reuse (and forgets its stamp)
        const int freed = s[5].slot;
        touch(s[5], D, T);
        EXPECT(count(D, T) == 2);
        unregister_slot(s[5], D);
        EXPECT(s[5].slot == -1 && count(D, T) == 1);
        register_slot(s[SLOTS], D);
        EXPECT(s[SLOTS].slot == freed && count(D, T) == 1);
        unregister_slot(s[5], D);              // twice: nothing
        EXPECT(count(D, T) == 1);
        for (int i = 0; i <= SLOTS; i++) unregister_slot(s[i], D);
        EXPECT(count(D, T) == 0 && g_table.used[D].load() == 0);
    }
    {   // the window: active at stamp + window - 1 ns, not at stamp + window
        State a, b;
        register_slot(a, D);
        register_slot(b, D);
        EXPECT(a.slot != b.slot);
        EXPECT(touch(a, D, T) == 1);
        EXPECT(count(D, T + WINDOW_NS - 1) == 1);
        EXPECT(count(D, T + WINDOW_NS) == 0);
        EXPECT(touch(b, D, T + WINDOW_NS - 1) == 2);
        EXPECT(touch(b, D, T + WINDOW_NS) == 1);
        // a held slot counts at any `now`; touch does not overwrite the hold; releasing it stamps `now`
        hold(a, D, true, T);
        EXPECT(a.held);
        EXPECT(count(D, T + 3 * WINDOW_NS) == 1 && count(D, T + 1000 * WINDOW_NS) == 1 && count(D, INT64_MAX - 1) == 1);
        EXPECT(touch(a, D, T + 5 * WINDOW_NS) == 1);
        EXPECT(g_table.ts[D][a.slot].load() == HELD);
        const int64_t T2 = T + 10 * WINDOW_NS;
        hold(a, D, false, T2);
        EXPECT(!a.held && g_table.ts[D][a.slot].load() == T2);
        EXPECT(count(D, T2 + WINDOW_NS - 1) == 1 && count(D, T2 + WINDOW_NS) == 0);
        unregister_slot(a, D);
        unregister_slot(b, D);
    }
    {   // a device index outside the table is ignored: no slot, no count, touch = the caller alone, hold keeps the flag only
        for (int dev : {-1, DEVICES, DEVICES + 7}) {
            State s;
            register_slot(s, dev);
            EXPECT(s.slot == -1);
            EXPECT(count(dev, T) == 0);
            EXPECT(touch(s, dev, T) == 1);
            hold(s, dev, true, T);
            EXPECT(s.held && count(dev, T) == 0);
            hold(s, dev, false, T);
            unregister_slot(s, dev);
            s.slot = 2;  // (a slot number with a device outside the table: still nothing is written)
            unregister_slot(s, dev);
            EXPECT(s.slot == 2);
        }
        // the last device of the table is inside it
        State s;
        register_slot(s, DEVICES - 1);
        EXPECT(s.slot == 0 && touch(s, DEVICES - 1, T) == 1 && count(DEVICES - 1, T) == 1);
        unregister_slot(s, DEVICES - 1);
    }
    {   // ZK_OPT_ACTIVITY_HOLD = 1, no hold: a whole-proof call does not hold, stamps still count
        State s;
        register_slot(s, D);
        set_option(s, D, 1, T);
        EXPECT(s.no_hold && !s.pinned);
        hold(s, D, true, T);
        EXPECT(!s.held && count(D, T + 1) == 1 && count(D, T + WINDOW_NS) == 0);  // (the option's own release stamped T)
        hold(s, D, false, T + 1);
        EXPECT(touch(s, D, T + 2) == 1 && count(D, T + 2 + WINDOW_NS) == 0);
        // = 2, pinned: held from now on; the end of a whole-proof call does not release it, nor does its begin change anything
        set_option(s, D, 2, T + 3);
        EXPECT(s.pinned && !s.no_hold && s.held && count(D, T + 1000 * WINDOW_NS) == 1);
        hold(s, D, true, T + 4);
        hold(s, D, false, T + 5);
        EXPECT(s.held && g_table.ts[D][s.slot].load() == HELD);
        set_option(s, D, 2, T + 6);  // again: stays held
        EXPECT(s.held && g_table.ts[D][s.slot].load() == HELD);
        // = 0 lets go of the pin and stamps `now`; the default rule holds and releases
        set_option(s, D, 0, T + 7);
        EXPECT(!s.pinned && !s.no_hold && !s.held && g_table.ts[D][s.slot].load() == T + 7);
        hold(s, D, true, T + 8);
        EXPECT(s.held && count(D, T + 1000 * WINDOW_NS) == 1);
        // = 2 set inside a whole-proof call keeps the hold; = 1 set inside one releases it
        set_option(s, D, 2, T + 9);
        EXPECT(s.held && g_table.ts[D][s.slot].load() == HELD);
        set_option(s, D, 1, T + 10);
        EXPECT(!s.held && g_table.ts[D][s.slot].load() == T + 10);
        unregister_slot(s, D);
        EXPECT(g_table.used[D].load() == 0);
    }
    printf("activity logic: %d failures\n", fails);
    return fails ? 1 : 0;
}
