// C++ test of the storage-responsibility calls of include/kadgpu.hpp (RoutingTableMirror::isTooFarBatch,
// DhtMirror::maintainStorageBatch; Dht::maintainStorage dht.cpp:2909-2937, Dht::onAnnounce dht.cpp:3352-3358) over
// test doubles shaped like OpenDHT's types, as tests/cpp/test_shim.cpp: the device path (batches) against the host
// path (findClosestNodesHost and a host xor compare), for q = 1 and q = 4096. Needs a GPU. Exit 0 = pass.
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
struct InfoHash : std::array<uint8_t, 20> {};
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
            nd->time = t0 - std::chrono::milliseconds(g() % 594000);
            nd->reply_time = t0 - std::chrono::seconds(g() % 7140);
            if (u < 8) nd->reply_time = time_point::min();  // never replied
            else if (u >= 85 && u < 95) nd->expired_ = true;
            bk.nodes.push_back(nd);
        }
        rt.push_back(bk);
    }
    return rt;
}

// Random targets, and targets sharing c = 0..159 leading bits with myid (these put myid inside the answers' windows).
static std::vector<InfoHash> make_targets(size_t q, const InfoHash& myid, std::mt19937_64& g) {
    std::vector<InfoHash> t(q);
    for (size_t i = 0; i < q; i++) {
        for (auto& x : t[i]) x = (uint8_t)g();
        if (i & 1) {
            const unsigned c = (unsigned)(i / 2) % 160;
            for (unsigned k = 0; k < c / 8; k++) t[i][k] = myid[k];
            const uint8_t keep = (uint8_t)(0xFF00u >> (c % 8)), flip = (uint8_t)(0x80u >> (c % 8));
            t[i][c / 8] = (uint8_t)((myid[c / 8] & keep) | ((myid[c / 8] ^ flip) & flip) | (t[i][c / 8] & ~keep & ~flip));
        }
    }
    t[0] = myid;
    return t;
}

// The reference's own steps on the host: findClosestNodesHost, then InfoHash::xorCmp(nodes.back()->id, myid) < 0.
static uint8_t host_far(const Mirror& m, const InfoHash& h, const InfoHash& myid, time_point now, size_t count,
                        size_t min_nodes) {
    const auto r = m.findClosestNodesHost(h, now, count);
    if (r.size() < std::max<size_t>(min_nodes, 1)) return 0;
    for (unsigned k = 0; k < 20; k++) {
        const uint8_t a = r.back()->id[k] ^ h[k], s = myid[k] ^ h[k];
        if (a != s) return a < s ? 1 : 0;
    }
    return 0;
}

int main() {
    const time_point t0 = clock::now();
    const RoutingTable rt4 = make_table(20000, 0xC0FFEE, t0), rt6 = make_table(3000, 0xBEEF6, t0);
    std::mt19937_64 g(99);
    InfoHash myid;
    for (auto& x : myid) x = (uint8_t)g();
    Mirror m4(rt4, t0, 0);
    const time_point now = t0 + std::chrono::minutes(3);
    for (size_t q : {(size_t)1, (size_t)4096}) {
        const std::vector<InfoHash> targets = make_targets(q, myid, g);
        for (auto cm : {std::make_pair((size_t)KAD_TARGET_NODES, (size_t)1),
                        std::make_pair((size_t)KAD_SEARCH_NODES, (size_t)KAD_TARGET_NODES), std::make_pair((size_t)40, (size_t)1)}) {
            m4.setHostPath(0);  // every batch to the device
            const std::vector<uint8_t> dev = m4.isTooFarBatch(targets, myid, now, cm.first, cm.second);
            m4.setHostPath(1u << 20, 64);  // and to the host path
            const std::vector<uint8_t> host = m4.isTooFarBatch(targets, myid, now, cm.first, cm.second);
            m4.setHostPath(Mirror::kHostPathAuto);
            EXPECT(dev.size() == q && host.size() == q, "sizes q=%zu", q);
            size_t ones = 0;
            for (size_t i = 0; i < q; i++) {
                const uint8_t want = host_far(m4, targets[i], myid, now, cm.first, cm.second);
                EXPECT(dev[i] == want, "isTooFarBatch device q=%zu i=%zu count=%zu: %u vs %u", q, i, cm.first, dev[i], want);
                EXPECT(host[i] == want, "isTooFarBatch host q=%zu i=%zu count=%zu", q, i, cm.first);
                ones += want;
            }
            if (q > 1) EXPECT(ones >= 32 && q - ones >= 32, "both verdicts must occur: %zu far of %zu", ones, q);
        }
    }
    // Dht::maintainStorage over both families
    kadgpu::DhtMirror<RoutingTable> dht;
    dht.snapshot(rt4, rt6, t0, 0);
    for (size_t q : {(size_t)1, (size_t)4096}) {
        const std::vector<InfoHash> keys = make_targets(q, myid, g);
        for (int dev = 0; dev < 2; dev++) {
            dht.buckets(AF_INET).setHostPath(dev ? 0 : 1u << 20);
            dht.buckets(AF_INET6).setHostPath(dev ? 0 : 1u << 20);
            const std::vector<uint8_t> got = dht.maintainStorageBatch(keys, myid, now);
            EXPECT(got.size() == q, "maintainStorageBatch size");
            size_t discard = 0;
            for (size_t i = 0; i < q && i < got.size(); i++) {
                const uint8_t want = (uint8_t)(host_far(dht.buckets(AF_INET), keys[i], myid, now, 8, 1) |
                                               (host_far(dht.buckets(AF_INET6), keys[i], myid, now, 8, 1) << 1));
                EXPECT(got[i] == want, "maintainStorageBatch %s q=%zu i=%zu: %u vs %u", dev ? "device" : "host", q, i,
                       got[i], want);
                discard += want == 3;
            }
            if (q > 1) EXPECT(discard >= 32 && q - discard >= 32, "discards: %zu of %zu", discard, q);
        }
    }
    if (fails) {
        std::fprintf(stderr, "FAIL: %d\n", fails);
        return 1;
    }
    std::printf("PASS\n");
    return 0;
}
