// C++ test of include/kadgpu.hpp's RoutingTableMirror::onNewNodeBatch / DhtMirror::onNewNodeBatch (Dht::onNewNode(node, 0),
// dht.cpp:867-936) over test doubles shaped like OpenDHT's types, as tests/cpp/test_resp_shim.cpp: the batch against
// the doubles' own onNewNode decision for each candidate taken alone (a walk of the std::list table, as the reference
// does it). Reference-shaped tables of 300 nodes (split policy, 8 per bucket), one with mixed liveness and one all
// good. Needs a GPU. Exit 0 = pass.
#include <array>
#include <chrono>
#include <cstdio>
#include <list>
#include <memory>
#include <random>
#include <vector>

#include "kadgpu.hpp"

namespace mock {
using clock = std::chrono::steady_clock;
using time_point = clock::time_point;
struct InfoHash : std::array<uint8_t, 20> {
    int lowbit() const {  // infohash.h: the lowest set bit, counted from the most significant one; -1 for zero
        int i, j;
        for (i = 19; i >= 0; i--)
            if ((*this)[i] != 0) break;
        if (i < 0) return -1;
        for (j = 7; j >= 0; j--)
            if (((*this)[i] & (0x80 >> j)) != 0) break;
        return 8 * i + j;
    }
};
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

static RoutingTable make_table(uint32_t n, uint64_t seed, time_point t0, bool all_good) {
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
            const unsigned u = all_good ? 50 : g() % 100;
            nd->time = t0 - std::chrono::milliseconds(g() % 400000);
            nd->reply_time = t0 - std::chrono::seconds(g() % 7000);
            if (u < 8) nd->reply_time = time_point::min();  // never replied
            else if (u >= 92) nd->expired_ = true;
            bk.nodes.push_back(nd);
        }
        rt.push_back(bk);
    }
    return rt;
}

static RoutingTable::const_iterator find_bucket(const RoutingTable& rt, const InfoHash& id) {  // routing_table.cpp:113-127
    if (rt.empty()) return rt.end();
    auto b = rt.begin();
    while (true) {
        auto next = std::next(b);
        if (next == rt.end()) return b;
        if (id < next->first) return b;  // std::array compares lexicographically = InfoHash::cmp
        b = next;
    }
}

struct Want {
    uint8_t verdict;
    const Node* node;
    uint32_t bucket;
};

// Dht::onNewNode(node, 0)'s decision for a node with this ID (dht.cpp:867-936), nothing mutated.
static Want decide(const RoutingTable& rt, const InfoHash& id, const InfoHash* myid, time_point now, bool bootstrap) {
    const auto b = find_bucket(rt, id);
    if (b == rt.end()) return Want{KAD_NN_NONE, nullptr, KAD_NO_NODE};
    const uint32_t bi = (uint32_t)std::distance(rt.begin(), b);
    const bool mybucket = myid && find_bucket(rt, *myid) == b;
    const uint8_t mb = mybucket ? KAD_NN_MYBUCKET : 0;
    for (const auto& n : b->nodes)
        if (n->id == id) return Want{(uint8_t)(KAD_NN_KNOWN | mb), n.get(), bi};
    for (const auto& n : b->nodes)
        if (n->isExpired()) return Want{(uint8_t)(KAD_NN_REPLACE | mb), n.get(), bi};
    if (b->nodes.size() >= KAD_TARGET_NODES) {
        const Node* ping = nullptr;
        for (const auto& n : b->nodes)
            if (!n->isGood(now)) { ping = n.get(); break; }
        const int bit2 = std::next(b) != rt.end() ? std::next(b)->first.lowbit() : -1;
        const unsigned depth = (unsigned)(std::max(b->first.lowbit(), bit2) + 1);
        if ((mybucket || (bootstrap && depth < 6)) && (!ping || rt.size() == 1))
            return Want{(uint8_t)(KAD_NN_SPLIT | mb), ping, bi};
        return Want{(uint8_t)(KAD_NN_FULL | mb), ping, bi};
    }
    return Want{(uint8_t)(KAD_NN_INSERT | mb), nullptr, bi};
}

static std::vector<InfoHash> make_candidates(const RoutingTable& rt, const InfoHash& myid, std::mt19937_64& g) {
    std::vector<InfoHash> c;
    for (int i = 0; i < 1024; i++) {
        InfoHash h;
        for (auto& x : h) x = (uint8_t)g();
        c.push_back(h);
    }
    for (const auto& b : rt)
        for (const auto& n : b.nodes) {
            c.push_back(n->id);
            InfoHash h = n->id;
            h[19] ^= 1;
            c.push_back(h);
        }
    for (unsigned k = 0; k < 160 * 4; k++) {  // sharing k / 4 leading bits with myid
        const unsigned s = k / 4;
        InfoHash h;
        for (auto& x : h) x = (uint8_t)g();
        for (unsigned j = 0; j < s / 8; j++) h[j] = myid[j];
        const uint8_t keep = (uint8_t)(0xFF00u >> (s % 8)), flip = (uint8_t)(0x80u >> (s % 8));
        h[s / 8] = (uint8_t)((myid[s / 8] & keep) | ((myid[s / 8] ^ flip) & flip) | (h[s / 8] & ~keep & ~flip));
        c.push_back(h);
    }
    return c;
}

int main() {
    const time_point t0 = clock::now();
    const time_point now = t0 + std::chrono::minutes(3);
    std::mt19937_64 g(77);
    size_t kinds[6] = {0, 0, 0, 0, 0, 0}, mine = 0;
    for (int all_good = 0; all_good < 2; all_good++) {
        const RoutingTable rt = make_table(300, 0x7A1A6E + all_good, t0, all_good != 0);
        Mirror m(rt, t0, 0);
        InfoHash random_id;
        for (auto& x : random_id) x = (uint8_t)g();
        InfoHash full_id = rt.begin()->nodes.front()->id;  // a node of a full bucket, if there is one
        for (const auto& b : rt)
            if (b.nodes.size() >= KAD_TARGET_NODES) { full_id = b.nodes.front()->id; break; }
        const InfoHash* selves[3] = {&random_id, &full_id, nullptr};
        for (const InfoHash* myid : selves) {
            const std::vector<InfoHash> cand = make_candidates(rt, myid ? *myid : random_id, g);
            for (int boot = 0; boot < 2; boot++) {
                const std::vector<kadgpu::NewNodeVerdict> got = m.onNewNodeBatch(cand.data(), cand.size(), myid, now, boot != 0);
                EXPECT(got.size() == cand.size(), "size");
                for (size_t i = 0; i < cand.size() && i < got.size(); i++) {
                    const Want w = decide(rt, cand[i], myid, now, boot != 0);
                    const Node* gn = got[i].node == KAD_NO_NODE ? nullptr : m.node(got[i].node).get();
                    EXPECT(got[i].verdict == w.verdict && gn == w.node && got[i].bucket == w.bucket,
                           "table %d boot %d i=%zu: verdict %u vs %u, node %p vs %p, bucket %u vs %u", all_good, boot, i,
                           got[i].verdict, w.verdict, (const void*)gn, (const void*)w.node, got[i].bucket, w.bucket);
                    kinds[w.verdict & KAD_NN_KIND_MASK]++;
                    mine += (w.verdict & KAD_NN_MYBUCKET) != 0;
                }
            }
        }
    }
    for (int k = KAD_NN_KNOWN; k <= (int)KAD_NN_FULL; k++) EXPECT(kinds[k] >= 32, "kind %d occurred %zu times", k, kinds[k]);
    EXPECT(mine >= 32, "MYBUCKET occurred %zu times", mine);
    // the per-family forwarder, and a table without buckets
    {
        const RoutingTable rt4 = make_table(300, 0x7A1A6E, t0, false), rt6;
        kadgpu::DhtMirror<RoutingTable> dht;
        dht.snapshot(rt4, rt6, t0, 0);
        dht.setClock([&] { return now; });
        InfoHash myid;
        for (auto& x : myid) x = (uint8_t)g();
        const std::vector<InfoHash> cand = make_candidates(rt4, myid, g);
        const auto g4 = dht.onNewNodeBatch(cand.data(), cand.size(), AF_INET, &myid, true);
        const auto g6 = dht.onNewNodeBatch(cand.data(), cand.size(), AF_INET6, &myid, true);
        for (size_t i = 0; i < cand.size(); i++) {
            const Want w = decide(rt4, cand[i], &myid, now, true);
            EXPECT(g4[i].verdict == w.verdict && g4[i].bucket == w.bucket, "forwarder v4 i=%zu", i);
            EXPECT(g6[i].verdict == KAD_NN_NONE && g6[i].node == KAD_NO_NODE && g6[i].bucket == KAD_NO_NODE,
                   "forwarder v6 (no bucket) i=%zu", i);
        }
    }
    if (fails) {
        std::fprintf(stderr, "FAIL: %d\n", fails);
        return 1;
    }
    std::printf("PASS kinds %zu %zu %zu %zu %zu mine %zu\n", kinds[1], kinds[2], kinds[3], kinds[4], kinds[5], mine);
    return 0;
}
