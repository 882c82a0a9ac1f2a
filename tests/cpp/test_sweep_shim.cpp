// C++ test of include/kadgpu.hpp's RoutingTableMirror::nodesStats / expireBuckets and the DhtMirror forwarders
// (Dht::getNodesStats dht.cpp:2470-2495, Dht::expireBuckets dht.cpp:942-956) over test doubles shaped like OpenDHT's
// types, as tests/cpp/test_triage_shim.cpp: the counts against a host loop over the doubles, the removed nodes and
// changed buckets against the doubles' own isExpired(), and queries on the shrunk table against the oracle, without
// a full liveness upload (syncTimes) having run in between. Needs a GPU. Exit 0 = pass.
#include <array>
#include <chrono>
#include <cstdio>
#include <list>
#include <memory>
#include <random>
#include <vector>

#include "kadgpu.hpp"

extern "C" int orc_flat_rt_closest(uint32_t, const uint8_t*, const uint8_t*, uint32_t, const uint8_t*, const uint32_t*,
                                   uint32_t, const uint8_t*, uint32_t, uint32_t*, uint8_t*, int);

namespace mock {
using clock = std::chrono::steady_clock;
using time_point = clock::time_point;
using InfoHash = std::array<uint8_t, 20>;
struct Node {
    InfoHash id;
    time_point time{time_point::min()}, reply_time{time_point::min()};
    bool expired_ = false;
    bool isExpired() const { return expired_; }
    bool isGood(time_point now) const {
        return !expired_ && reply_time >= now - std::chrono::minutes(120) && time >= now - std::chrono::minutes(10);
    }
};
struct Bucket {
    InfoHash first;
    std::list<std::shared_ptr<Node>> nodes;
};
using RoutingTable = std::list<Bucket>;
}  // namespace mock

static int fails = 0;
#define EXPECT(c, ...) do { if (!(c)) { fails++; if (fails < 30) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } } while (0)

using namespace mock;
using Mirror = kadgpu::RoutingTableMirror<RoutingTable>;
using NodePtr = std::shared_ptr<Node>;

static RoutingTable make_table(uint32_t n, uint64_t seed, time_point t0) {
    std::vector<uint8_t> ids(20ull * n);
    kadgpu::check(kad_synth_ids(seed, n, ids.data()), "synth");
    std::vector<uint32_t> perm(n), off(n + 2);
    std::vector<uint8_t> first(20ull * (n + 1));
    uint32_t B = 0;
    kadgpu::check(kad_split_table(n, ids.data(), 8, perm.data(), first.data(), off.data(), &B), "split");
    std::mt19937_64 g(seed ^ 7);
    RoutingTable rt;
    for (uint32_t b = 0; b < B; b++) {
        Bucket bk;
        std::memcpy(bk.first.data(), &first[20ull * b], 20);
        for (uint32_t j = off[b]; j < off[b + 1]; j++) {
            auto nd = std::make_shared<Node>();
            std::memcpy(nd->id.data(), &ids[20ull * perm[j]], 20);
            const unsigned u = g() % 100;
            nd->time = t0 - std::chrono::milliseconds(g() % 400000);
            nd->reply_time = t0 - std::chrono::seconds(g() % 7000);
            if (u < 8) nd->reply_time = time_point::min();           // never replied
            else if (u < 30) nd->reply_time = nd->time;              // time == reply_time
            else if (u < 50) nd->time = nd->reply_time - std::chrono::seconds(1 + g() % 100);  // time < reply_time
            else if (u >= 92) nd->expired_ = true;
            bk.nodes.push_back(nd);
        }
        rt.push_back(bk);
    }
    return rt;
}

struct Counts {
    unsigned good = 0, dubious = 0, incoming = 0, expired = 0;
};

// Dht::getNodesStats' loop (dht.cpp:2470-2495), plus the nodes expireBuckets would remove.
static Counts host_stats(const RoutingTable& rt, time_point now) {
    Counts c;
    for (const auto& b : rt)
        for (const auto& n : b.nodes) {
            if (n->isGood(now)) {
                c.good++;
                if (n->time > n->reply_time) c.incoming++;
            } else if (!n->isExpired()) {
                c.dubious++;
            }
            if (n->isExpired()) c.expired++;
        }
    return c;
}

static void check_stats(const Mirror& m, const RoutingTable& rt, time_point now, const char* what) {
    const kadgpu::NodesStats got = m.nodesStats(now);
    const Counts w = host_stats(rt, now);
    EXPECT(got.good == w.good && got.dubious == w.dubious && got.incoming == w.incoming && got.expired == w.expired,
           "%s: stats %u %u %u %u vs %u %u %u %u", what, got.good, got.dubious, got.incoming, got.expired, w.good, w.dubious,
           w.incoming, w.expired);
}

// The oracle's answer on the host table as it is now, compared with the mirror's result vectors.
static void check_rt(const RoutingTable& rt, const std::vector<std::vector<NodePtr>>& got,
                     const std::vector<InfoHash>& targets, uint32_t count, time_point now, const char* what) {
    std::vector<uint8_t> ids, st, first;
    std::vector<uint32_t> off;
    std::vector<const Node*> flat;
    for (auto& b : rt) {
        off.push_back((uint32_t)flat.size());
        first.insert(first.end(), b.first.begin(), b.first.end());
        for (auto& nd : b.nodes) {
            ids.insert(ids.end(), nd->id.begin(), nd->id.end());
            st.push_back((uint8_t)((nd->isGood(now) ? 1 : 0) | (nd->isExpired() ? 2 : 0)));
            flat.push_back(nd.get());
        }
    }
    off.push_back((uint32_t)flat.size());
    const uint32_t q = (uint32_t)targets.size();
    std::vector<uint32_t> want(q * count);
    std::vector<uint8_t> wcnt(q);
    orc_flat_rt_closest((uint32_t)flat.size(), ids.data(), st.data(), (uint32_t)rt.size(), first.data(), off.data(), q,
                        reinterpret_cast<const uint8_t*>(targets.data()), count, want.data(), wcnt.data(), 4);
    EXPECT(got.size() == q, "%s: rows", what);
    for (uint32_t i = 0; i < q && i < got.size(); i++) {
        const uint32_t m = wcnt[i];
        EXPECT(got[i].size() == m, "%s: rt count q=%u (%zu vs %u)", what, i, got[i].size(), m);
        for (uint32_t j = 0; j < got[i].size() && j < m; j++)
            EXPECT(got[i][j].get() == flat[want[(size_t)i * count + j]], "%s: rt node q=%u j=%u", what, i, j);
    }
}

// Dht::expireBuckets on the host lists: the removed nodes in table order and the indices of the buckets that lost one.
static void host_expire(RoutingTable& rt, std::vector<const Node*>& removed, std::vector<uint32_t>& buckets) {
    uint32_t bi = 0;
    for (auto& b : rt) {
        bool changed = false;
        for (auto it = b.nodes.begin(); it != b.nodes.end();) {
            if ((*it)->isExpired()) {
                removed.push_back(it->get());
                it = b.nodes.erase(it);
                changed = true;
            } else {
                ++it;
            }
        }
        if (changed) buckets.push_back(bi);
        bi++;
    }
}

int main() {
    const time_point t0 = clock::now();
    const time_point now = t0 + std::chrono::minutes(3);
    std::mt19937_64 g(91);
    RoutingTable rt = make_table(600, 0x5EEB, t0);
    Mirror m(rt, t0, 0);
    std::vector<InfoHash> targets(200);  // above the host-path limit: device batches
    for (auto& t : targets)
        for (auto& x : t) x = (uint8_t)g();
    EXPECT(m.hostBatchLimit() < targets.size(), "the query batch must take the device path");

    check_stats(m, rt, t0, "snapshot");
    check_stats(m, rt, now, "later");
    {
        const Counts c = host_stats(rt, now);
        EXPECT(c.good >= 32 && c.dubious >= 32 && c.incoming >= 32 && c.expired >= 32 && c.good - c.incoming >= 32,
               "ground: %u %u %u %u", c.good, c.dubious, c.incoming, c.expired);
    }
    // liveness changes reported node by node: more nodes expire, some are heard of again
    size_t k = 0;
    for (auto& b : rt)
        for (auto& n : b.nodes) {
            if (k % 11 == 3) { n->expired_ = true; m.nodeUpdated(n); }
            else if (k % 13 == 5) { n->time = now; n->reply_time = now - std::chrono::seconds(2); n->expired_ = false; m.nodeUpdated(n); }
            k++;
        }
    check_stats(m, rt, now, "after updates");
    EXPECT(m.syncTimesCalls() == 1, "only the snapshot uploads every node's liveness (%zu)", m.syncTimesCalls());

    // expireBuckets: the doubles whose isExpired() holds, and the buckets that held them
    const size_t n_before = m.nodeCount();
    const kadgpu::Expired<NodePtr> ex = m.expireBuckets(now);
    std::vector<const Node*> w_removed;
    std::vector<uint32_t> w_buckets;
    host_expire(rt, w_removed, w_buckets);
    EXPECT(w_removed.size() >= 80 && w_buckets.size() >= 40, "ground: %zu removed, %zu buckets", w_removed.size(), w_buckets.size());
    EXPECT(ex.removed.size() == w_removed.size(), "removed %zu vs %zu", ex.removed.size(), w_removed.size());
    for (size_t i = 0; i < ex.removed.size() && i < w_removed.size(); i++)
        EXPECT(ex.removed[i].get() == w_removed[i] && ex.removed[i]->isExpired(), "removed node %zu", i);
    EXPECT(ex.buckets == w_buckets, "changed buckets (%zu vs %zu)", ex.buckets.size(), w_buckets.size());
    EXPECT(m.nodeCount() == n_before - w_removed.size() && m.bucketCount() == rt.size(), "mirror size");
    EXPECT(m.expireCalls() == 1, "one kad_table_expire that removed nodes");

    // the shrunk table answers at once, and at a later time, with no full liveness upload in between
    check_rt(rt, m.findClosestNodesBatch(targets, now, 8), targets, 8, now, "after expire");
    check_stats(m, rt, now, "after expire");
    const time_point later = now + std::chrono::minutes(8);  // most nodes' `time` has passed the 10 minutes by then
    check_rt(rt, m.findClosestNodesBatch(targets, later, 14), targets, 14, later, "later");
    check_stats(m, rt, later, "later, after expire");
    EXPECT(host_stats(rt, later).good < host_stats(rt, now).good, "ground: nodes went dubious");
    EXPECT(m.syncTimesCalls() == 1, "expireBuckets must not upload every node's liveness (%zu)", m.syncTimesCalls());
    // node-by-node reports still land on the right nodes after the remap
    for (auto& b : rt)
        if (!b.nodes.empty()) { b.nodes.front()->time = later; b.nodes.front()->reply_time = later; m.nodeUpdated(b.nodes.front()); }
    check_stats(m, rt, later, "updates after expire");
    check_rt(rt, m.findClosestNodesBatch(targets, later, 8), targets, 8, later, "updates after expire");
    // nothing left to expire
    const kadgpu::Expired<NodePtr> none = m.expireBuckets(later);
    EXPECT(none.removed.empty() && none.buckets.empty() && m.expireCalls() == 1, "second expireBuckets");
    // pending ops are flushed first (flush re-uploads the liveness: that is the path expireBuckets spares)
    {
        NodePtr victim;
        for (auto& b : rt)
            if (b.nodes.size() >= 2) { victim = b.nodes.back(); b.nodes.pop_back(); break; }
        m.nodeRemoved(victim);
        NodePtr dead;
        for (auto& b : rt)
            if (b.nodes.size() >= 3) { dead = b.nodes.front(); break; }
        dead->expired_ = true;
        m.nodeUpdated(dead);
        const kadgpu::Expired<NodePtr> one = m.expireBuckets(later);
        std::vector<const Node*> wr;
        std::vector<uint32_t> wb;
        host_expire(rt, wr, wb);
        EXPECT(one.removed.size() == 1 && wr.size() == 1 && one.removed[0].get() == wr[0] && one.buckets == wb, "expire after flush");
        check_rt(rt, m.findClosestNodesBatch(targets, later, 8), targets, 8, later, "expire after flush");
    }

    // the per-family forwarders
    {
        RoutingTable rt4 = make_table(300, 0x7A1A6E, t0), rt6;
        kadgpu::DhtMirror<RoutingTable> dht;
        dht.snapshot(rt4, rt6, t0, 0);
        dht.setClock([&] { return now; });
        unsigned good = 0, dubious = 0, incoming = 0;
        const unsigned tot = dht.getNodesStats(AF_INET, &good, &dubious, &incoming);
        const Counts w = host_stats(rt4, now);
        EXPECT(tot == w.good + w.dubious && good == w.good && dubious == w.dubious && incoming == w.incoming, "forwarder stats");
        EXPECT(dht.getNodesStats(AF_INET6, &good, &dubious, &incoming) == 0 && good == 0 && dubious == 0 && incoming == 0,
               "forwarder stats, empty family");
        const auto e4 = dht.expireBuckets(AF_INET);
        const auto e6 = dht.expireBuckets(AF_INET6);
        std::vector<const Node*> wr;
        std::vector<uint32_t> wb;
        host_expire(rt4, wr, wb);
        EXPECT(e4.removed.size() == wr.size() && e4.buckets == wb && e6.removed.empty() && e6.buckets.empty(), "forwarder expire");
        check_rt(rt4, dht.buckets(AF_INET).findClosestNodesBatch(targets, now, 8), targets, 8, now, "forwarder expire");
    }
    if (fails) {
        std::fprintf(stderr, "FAIL: %d\n", fails);
        return 1;
    }
    std::printf("PASS removed %zu buckets %zu\n", w_removed.size(), w_buckets.size());
    return 0;
}
