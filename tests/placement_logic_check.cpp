// Host-only check of the stream-placement logic (csrc/placement.h): made-up time stamps -> classes -> report flags -> deal.
// No device: a round is simulated from a table "stream i sits on queue q" — every queue runs its kernels in order, queues run
// side by side, launches leave the host 5 us apart.  The queue tables are those the documented runtime rule gives (the first
// four streams of a process get a queue each, later ones the least loaded queue, ties to the highest) after 0 .. 5 foreign streams.
#include <cstdio>
#include <vector>

#include "placement.h"
using namespace zk::placement;

static int fails = 0;
#define EXPECT(cond)                                         \
    do {                                                     \
        if (!(cond)) {                                       \
            printf("FAILED line %d: %s\n", __LINE__, #cond); \
            fails++;                                         \
        }                                                    \
    } while (0)

// one simulated round over streams on queues `q`: what placement.hip's round hands to classify()
struct Sim {
    std::vector<int> q;
    int calls = 0;
    int overrun_calls = 0;            // the first so many rounds report a host that overran its budget
    int bend = -1, bend_calls = 0;    // stream `bend` starts GUARD / 2 before the pivot's end in the first `bend_calls` rounds
    int operator()(int pivot, const uint8_t* active, Stamp* st) {
        const int n = (int)q.size();
        const uint64_t T0 = 123456789, step = 5 * TICKS_PER_US;
        std::vector<uint64_t> free_at(64, 0);
        st[pivot] = {T0, T0 + t_pivot(n)};
        free_at[q[pivot]] = st[pivot].t1;
        int m = 1;
        for (int i = 0; i < n; i++) {
            if (!active[i] || i == pivot) continue;
            uint64_t start = T0 + step * m++;
            if (free_at[q[i]] > start) start = free_at[q[i]] + 2 * TICKS_PER_US;  // (dispatch gap behind the previous kernel)
            if (i == bend && calls < bend_calls) start = st[pivot].t1 - GUARD / 2;
            st[i] = {start, start + T_SHORT};
            free_at[q[i]] = st[i].t1;
        }
        return calls++ < overrun_calls ? 1 : 0;
    }
};

// the runtime's rule, stream by stream
struct Rule {
    std::vector<int> load;
    int made = 0;
    explicit Rule(int queues = 4) : load(queues, 0) {}
    int make() {
        int best = 0;
        if (made < (int)load.size()) best = made;
        else
            for (int k = 0; k < (int)load.size(); k++)
                if (load[k] <= load[best]) best = k;  // least loaded, ties to the highest
        made++;
        load[best]++;
        return best;
    }
    // queue of every pool stream, in the probe's index order, after `foreign` streams made first
    std::vector<int> pool(int foreign) {
        for (int i = 0; i < foreign; i++) make();
        std::vector<int> q(POOL_STREAMS);
        for (int layer = 0; layer < 2; layer++) {  // the pool's creation order (streams.hip pool_prime)
            for (int i = 4 * layer; i < 4 * layer + 4; i++) q[main_index(i)] = make();
            for (int i = 4 * layer; i < 4 * layer + 4; i++)
                for (int j = 0; j < 4; j++) q[side_index(i, j)] = make();
        }
        return q;
    }
};
static std::vector<int> rule_layout(int foreign, int queues = 4) { return Rule(queues).pool(foreign); }

static bool same_partition(const Classes& c, const std::vector<int>& q) {
    for (size_t a = 0; a < q.size(); a++)
        for (size_t b = 0; b < q.size(); b++)
            if ((c.cls[a] == c.cls[b]) != (q[a] == q[b])) return false;
    return true;
}

// the queue table after a deal: stream list[i] moves to its dealt place
static std::vector<int> apply(const Deal& d, const std::vector<int>& q) {
    std::vector<int> r;
    for (int i = 0; i < POOL_SLOTS; i++) r.push_back(q[d.main[i]]);
    for (int i = 0; i < POOL_SLOTS; i++)
        for (int j = 0; j < POOL_SIDES; j++) r.push_back(q[d.side[i][j]]);
    for (int i = 0; i < d.n_parked; i++) r.push_back(q[d.parked[i]]);
    return r;
}

int main() {
    {   // the verdict's edges, and the pivot's length against the worst case it must outlast
        const Stamp p = {1000, 1000 + t_pivot(40)};
        EXPECT(judge(p, {p.t1, p.t1 + T_SHORT}) == SAME);
        EXPECT(judge(p, {p.t1 - 1, p.t1 + T_SHORT}) == AMBIGUOUS);
        EXPECT(judge(p, {p.t1 - GUARD, p.t1}) == AMBIGUOUS);
        EXPECT(judge(p, {p.t1 - GUARD - 1, p.t1}) == OTHER);
        EXPECT(judge(p, {0, 0}) == AMBIGUOUS);  // a kernel that never ran
        EXPECT(judge({0, 0}, {5, 6}) == AMBIGUOUS);
        for (int n = 2; n <= MAX_STREAMS; n++) EXPECT(t_pivot(n) > (uint64_t)(n - 2) * T_SHORT + enqueue_budget(n) + GUARD);
        EXPECT(t_pivot(40) == 595000);  // 5.95 ms
    }
    {   // four classes of ten: the pool as the rule makes it in a process without earlier streams
        Sim s;
        s.q = rule_layout(0);
        const Classes c = classify(POOL_STREAMS, s);
        EXPECT(!c.unresolved && c.n_classes == 4 && c.rounds == 4 && same_partition(c, s.q));
        int cnt[4] = {0, 0, 0, 0};
        for (int i = 0; i < POOL_STREAMS; i++) cnt[c.cls[i]]++;
        EXPECT(cnt[0] == 10 && cnt[1] == 10 && cnt[2] == 10 && cnt[3] == 10);
        zk_placement r;
        report(c, &r);
        EXPECT(r.n_queues == 4 && r.flags == ZK_PLACEMENT_OK);
        for (int i = 0; i < 4; i++) EXPECT(r.main_queue[i] == i && r.main_queue[7 - i] == i);
        for (int i = 0; i < POOL_SLOTS; i++) EXPECT(r.spare_queue[i] == r.main_queue[i] && r.role_queue[i][0] == 3 - r.main_queue[i]);
        const Deal d = deal(c);  // a pool that follows the rule is dealt to itself
        EXPECT(d.dealt && d.need_more == 0 && d.n_parked == 0 && apply(d, s.q) == s.q);
    }
    {   // two classes: no four distinct queues anywhere, nothing to deal
        Sim s;
        s.q = rule_layout(0, 2);
        const Classes c = classify(POOL_STREAMS, s);
        EXPECT(!c.unresolved && c.n_classes == 2 && c.rounds == 2 && same_partition(c, s.q));
        zk_placement r;
        report(c, &r);
        EXPECT(r.n_queues == 2 && !(r.flags & (ZK_PLACEMENT_MAINS_OK | ZK_PLACEMENT_LONE_OK | ZK_PLACEMENT_PAIR_OK | ZK_PLACEMENT_UNRESOLVED)));
        const Deal d = deal(c);
        EXPECT(!d.dealt && d.need_more == 0);
    }
    {   // one class, and a single stream
        Sim s;
        s.q.assign(POOL_STREAMS, 0);
        Classes c = classify(POOL_STREAMS, s);
        EXPECT(c.n_classes == 1 && c.rounds == 1);
        zk_placement r;
        report(c, &r);
        EXPECT(r.n_queues == 1 && r.flags == ZK_PLACEMENT_LAYER1_OK);
        EXPECT(!deal(c).dealt && deal(c).need_more == 0);
        s.q.assign(1, 0);
        c = classify(1, s);
        EXPECT(c.n_classes == 1 && c.rounds == 0 && s.calls == 1);  // (no round needed: Sim was not called again)
    }
    {   // every stream on a queue of its own: given up after nine classes, not forty rounds
        Sim s;
        for (int i = 0; i < POOL_STREAMS; i++) s.q.push_back(i);
        const Classes c = classify(POOL_STREAMS, s);
        EXPECT(c.unresolved && c.n_classes == 0 && c.rounds == 9 && c.cls[0] == UNKNOWN);
        zk_placement r;
        report(c, &r);
        EXPECT(r.n_queues == 0 && r.flags == ZK_PLACEMENT_UNRESOLVED && r.main_queue[0] == UNKNOWN);
        EXPECT(!deal(c).dealt && deal(c).need_more == 0);
        // nine queues are still told apart
        Sim s9;
        for (int i = 0; i < POOL_STREAMS; i++) s9.q.push_back(i % 9);
        const Classes c9 = classify(POOL_STREAMS, s9);
        EXPECT(!c9.unresolved && c9.n_classes == 9 && same_partition(c9, s9.q));
    }
    {   // one ambiguous stamp: the round is repeated once; ambiguous again = unresolved
        Sim s;
        s.q = rule_layout(0);
        s.bend = 17;
        s.bend_calls = 1;
        Classes c = classify(POOL_STREAMS, s);
        EXPECT(!c.unresolved && c.n_classes == 4 && c.rounds == 5 && same_partition(c, s.q));
        Sim t;
        t.q = rule_layout(0);
        t.bend = 17;
        t.bend_calls = 2;
        c = classify(POOL_STREAMS, t);
        EXPECT(c.unresolved && c.n_classes == 0 && c.rounds == 2);
        // a host that overran its enqueue budget: the same
        Sim u;
        u.q = rule_layout(0);
        u.overrun_calls = 1;
        c = classify(POOL_STREAMS, u);
        EXPECT(!c.unresolved && c.n_classes == 4 && c.rounds == 5);
        Sim v;
        v.q = rule_layout(0);
        v.overrun_calls = 2;
        c = classify(POOL_STREAMS, v);
        EXPECT(c.unresolved && c.rounds == 2);
        // a failing round ends it
        c = classify(POOL_STREAMS, [](int, const uint8_t*, Stamp*) { return -7; });
        EXPECT(c.unresolved && c.error == -7 && c.rounds == 1);
    }
    for (int f = 0; f <= 5; f++) {  // the deal, on what the rule gives after f foreign streams
        Sim s;
        Rule rule;
        s.q = rule.pool(f);
        Classes c = classify(POOL_STREAMS, s);
        EXPECT(!c.unresolved && c.n_classes == 4 && same_partition(c, s.q));
        zk_placement r;
        report(c, &r);
        // only the untouched process gets the pattern: one to three foreign streams put two of the first four mains on one
        // queue, four or five turn the order of the mains' queues against the side blocks'
        EXPECT((r.flags == ZK_PLACEMENT_OK) == (f == 0));
        if (f >= 1 && f <= 3) EXPECT(!(r.flags & ZK_PLACEMENT_MAINS_OK));
        // one to three foreign streams leave the pool an uneven share of the queues (f = 1: 9 / 10 / 10 / 11): the deal asks
        // for more streams first, as the engine then makes them — at least four at a time, a full turn of the rule
        Deal d = deal(c);
        EXPECT(d.dealt == (f == 0 || f >= 4));
        while (!d.dealt && d.need_more > 0 && (int)s.q.size() < MAX_STREAMS) {
            for (int i = 0, m = d.need_more < 4 ? 4 : d.need_more; i < m && (int)s.q.size() < MAX_STREAMS; i++) s.q.push_back(rule.make());
            c = classify((int)s.q.size(), s);
            EXPECT(c.n_classes == 4 && same_partition(c, s.q));
            d = deal(c);
        }
        EXPECT(d.dealt && d.need_more == 0 && d.n_parked == (int)s.q.size() - POOL_STREAMS && s.q.size() <= 44);
        Sim s2;
        s2.q = apply(d, s.q);
        EXPECT(s2.q.size() == s.q.size());
        const Classes c2 = classify((int)s2.q.size(), s2);
        report(c2, &r);
        EXPECT(r.n_queues == 4 && r.flags == ZK_PLACEMENT_OK);
        for (int i = 0; i < 4; i++) {
            EXPECT(r.main_queue[i] == i && r.main_queue[7 - i] == i);                               // mains, both layers
            for (int j = 0; j < 4; j++) EXPECT(c2.cls[side_index(i, j)] == 3 - j && c2.cls[side_index(7 - i, j)] == 3 - j);  // side[i][j] on class 3 - j
        }
        std::vector<int> seen(MAX_STREAMS, 0);  // every stream dealt or parked, once
        for (int i = 0; i < POOL_SLOTS; i++) {
            seen[d.main[i]]++;
            for (int j = 0; j < POOL_SIDES; j++) seen[d.side[i][j]]++;
        }
        for (int i = 0; i < d.n_parked; i++) seen[d.parked[i]]++;
        for (int i = 0; i < (int)s.q.size(); i++) EXPECT(seen[i] == 1);
    }
    {   // a class short of streams asks for more; once they are there the surplus of the others is parked
        Sim s;
        s.q = rule_layout(0);
        int moved = 0;
        for (int i = POOL_STREAMS - 1; i >= 0 && moved < 3; i--)
            if (s.q[i] == 3) {
                s.q[i] = 0;  // 13 / 10 / 10 / 7
                moved++;
            }
        Classes c = classify(POOL_STREAMS, s);
        EXPECT(c.n_classes == 4);
        Deal d = deal(c);
        EXPECT(!d.dealt && d.need_more == 3);
        for (int i = 0; i < 3; i++) s.q.push_back(3);  // the rule puts new streams on the least loaded queue
        c = classify((int)s.q.size(), s);
        EXPECT(c.n == 43 && c.n_classes == 4 && same_partition(c, s.q));
        d = deal(c);
        EXPECT(d.dealt && d.need_more == 0 && d.n_parked == 3);
        Sim s2;
        s2.q = apply(d, s.q);
        const Classes c2 = classify((int)s2.q.size(), s2);
        zk_placement r;
        report(c2, &r);
        EXPECT(r.n_queues == 4 && r.flags == ZK_PLACEMENT_OK);
        for (int i = 0; i < d.n_parked; i++) EXPECT(s.q[d.parked[i]] == 0);
        // ... and new streams that land on the wrong queue are no help: asked again
        Sim w;
        w.q = s.q;
        for (int i = 40; i < 43; i++) w.q[i] = 1;
        d = deal(classify(43, w));
        EXPECT(!d.dealt && d.need_more == 3);
    }
    {   // the side stream of every role: distinct per slot, the spare on the main's own queue (streams.hip ctx_side_stream)
        for (int sl = 0; sl < POOL_SLOTS; sl++) {
            int seen = 0;
            for (int role = 0; role < 4; role++) seen |= 1 << role_side(sl, role);
            EXPECT(seen == 15 && role_side(sl, 0) == slot_main_queue(sl) && role_side(sl, 3) == 3 - slot_main_queue(sl));
        }
    }
    printf("placement logic: %d failures\n", fails);
    return fails ? 1 : 0;
}
