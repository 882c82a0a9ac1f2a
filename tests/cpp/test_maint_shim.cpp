// C++ test of include/kadgpu.hpp's bucket-time calls (RoutingTableMirror::bucketMaintenance, onReportedAddrBatch,
// onReportedAddr, resetBucketTimes, snapshot's upload of Bucket::time, flush after a split, and the DhtMirror forwarders)
// over test doubles shaped like OpenDHT's types, with std::mt19937 at fixed seeds. The yardstick is the reference's own
// code restated on the doubles: Dht::bucketMaintenance's loop (dht.cpp:2832-2850) over every bucket,
// RoutingTable::randomId (routing_table.cpp:27-45), Bucket::randomNode (:15-25), Dht::onReportedAddr (dht.cpp:3174-3178)
// with the linear findBucket (routing_table.cpp:113-127), and RoutingTable::split (:137-163). The shim must return the
// loop's {bucket, q, id, node} and leave the generator in the same state (the next eight draws). Needs a GPU.
// Exit 0 = pass.
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <list>
#include <memory>
#include <random>
#include <vector>

#include "kadgpu.hpp"

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
    time_point time{time_point::min()};
    std::list<std::shared_ptr<Node>> nodes;
};
using RoutingTable = std::list<Bucket>;
}  // namespace mock

static int fails = 0;
#define EXPECT(c, ...) do { if (!(c)) { fails++; if (fails < 30) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } } while (0)

using namespace mock;
using Mirror = kadgpu::RoutingTableMirror<RoutingTable>;
using NodePtr = std::shared_ptr<Node>;
using Pick = kadgpu::MaintenancePick<NodePtr>;

// ---- the reference, restated on the doubles ---------------------------------------------------------------------------
static int lowbit(const InfoHash& h) {
    int i, j;
    for (i = 19; i >= 0; i--)
        if (h[i] != 0) break;
    if (i < 0) return -1;
    for (j = 7; j >= 0; j--)
        if ((h[i] & (0x80 >> j)) != 0) break;
    return 8 * i + j;
}

static int depth_of(const RoutingTable& rt, RoutingTable::const_iterator it) {
    const int bit1 = lowbit(it->first);
    const int bit2 = std::next(it) != rt.end() ? lowbit(std::next(it)->first) : -1;
    return std::max(bit1, bit2) + 1;
}

template <class Rng>
static InfoHash random_id(const RoutingTable& rt, RoutingTable::const_iterator it, Rng& rd) {
    std::uniform_int_distribution<uint8_t> rand_byte;
    const int bit = depth_of(rt, it);
    if (bit >= 160) return it->first;
    const int b = bit / 8;
    InfoHash id_return{};
    std::copy_n(it->first.begin(), b, id_return.begin());
    id_return[b] = (uint8_t)(it->first[b] & (0xFF00 >> (bit % 8)));
    id_return[b] |= rand_byte(rd) >> (bit % 8);
    for (unsigned i = b + 1; i < 20; i++) id_return[i] = rand_byte(rd);
    return id_return;
}

template <class Rng>
static NodePtr random_node(Bucket& b, Rng& rd) {
    if (b.nodes.empty()) return nullptr;
    std::uniform_int_distribution<unsigned> rand_node(0, (unsigned)b.nodes.size() - 1);
    unsigned nn = rand_node(rd);
    for (auto& n : b.nodes)
        if (!nn--) return n;
    return b.nodes.back();
}

struct RefPick {
    bool found = false;
    uint32_t bucket = KAD_NO_NODE, q = KAD_NO_NODE;
    InfoHash id{};
    NodePtr node;
    unsigned candidates = 0;  // buckets that passed :2833 before the loop ended
};

template <class Rng>
static RefPick ref_maintenance(RoutingTable& list, time_point now, Rng& rd) {
    std::bernoulli_distribution rand_trial(1. / 8.);
    RefPick out;
    uint32_t bi = 0;
    for (auto b = list.begin(); b != list.end(); ++b, ++bi) {
        if (b->time < now - std::chrono::minutes(10) || b->nodes.empty()) {
            out.candidates++;
            InfoHash id = random_id(list, b, rd);
            auto q = b;
            uint32_t qi = bi;
            if (std::next(b) != list.end() && (q->nodes.empty() || rand_trial(rd))) { q = std::next(b); qi = bi + 1; }
            if (b != list.begin() && (q->nodes.empty() || rand_trial(rd))) {
                auto r = std::prev(b);
                if (!r->nodes.empty()) { q = r; qi = bi - 1; }
            }
            auto n = random_node(*q, rd);
            if (n) {
                out.found = true; out.bucket = bi; out.q = qi; out.id = id; out.node = n;
                return out;
            }
        }
    }
    return out;
}

static RoutingTable::iterator find_bucket(RoutingTable& rt, const InfoHash& id) {
    auto b = rt.begin();
    while (true) {
        auto next = std::next(b);
        if (next == rt.end()) return b;
        if (std::memcmp(id.data(), next->first.data(), 20) < 0) return b;
        b = next;
    }
}

static void ref_reported(RoutingTable& rt, const InfoHash& id, time_point now) { find_bucket(rt, id)->time = now; }

static void ref_split(RoutingTable& rt, RoutingTable::iterator b) {
    const int bit = depth_of(rt, b);
    InfoHash new_id = b->first;
    new_id[bit / 8] |= (uint8_t)(0x80 >> (bit % 8));
    Bucket nb;
    nb.first = new_id;
    nb.time = b->time;
    rt.insert(std::next(b), nb);
    std::list<NodePtr> nodes;
    nodes.splice(nodes.begin(), b->nodes);
    while (!nodes.empty()) {
        auto n = nodes.begin();
        auto d = find_bucket(rt, (*n)->id);
        d->nodes.splice(d->nodes.begin(), nodes, n);
    }
}

// ---- tables ---------------------------------------------------------------------------------------------------------
// 2^depth buckets of equal range (depth <= 8), widths[b] nodes each, Bucket::time from times[b].
static RoutingTable uniform_table(unsigned depth, const std::vector<unsigned>& widths, const std::vector<time_point>& times,
                                  uint64_t seed) {
    std::mt19937_64 g(seed);
    RoutingTable rt;
    for (unsigned b = 0; b < (1u << depth); b++) {
        Bucket bk;
        bk.first.fill(0);
        bk.first[0] = (uint8_t)(b << (8 - depth));
        bk.time = times[b];
        for (unsigned j = 0; j < widths[b]; j++) {
            auto nd = std::make_shared<Node>();
            for (auto& x : nd->id) x = (uint8_t)g();
            nd->id[0] = (uint8_t)((b << (8 - depth)) | (nd->id[0] & ((1u << (8 - depth)) - 1)));
            bk.nodes.push_back(nd);
        }
        rt.push_back(bk);
    }
    return rt;
}

static RoutingTable split_table(uint32_t n, uint64_t seed) {
    std::vector<uint8_t> ids(20ull * n);
    kadgpu::check(kad_synth_ids(seed, n, ids.data()), "synth");
    std::vector<uint32_t> perm(n), off(n + 2);
    std::vector<uint8_t> first(20ull * (n + 1));
    uint32_t B = 0;
    kadgpu::check(kad_split_table(n, ids.data(), 8, perm.data(), first.data(), off.data(), &B), "split");
    RoutingTable rt;
    for (uint32_t b = 0; b < B; b++) {
        Bucket bk;
        std::memcpy(bk.first.data(), &first[20ull * b], 20);
        for (uint32_t j = off[b]; j < off[b + 1]; j++) {
            auto nd = std::make_shared<Node>();
            std::memcpy(nd->id.data(), &ids[20ull * perm[j]], 20);
            bk.nodes.push_back(nd);
        }
        rt.push_back(bk);
    }
    return rt;
}

// ---- comparisons ----------------------------------------------------------------------------------------------------
struct Tally {
    unsigned found = 0, none = 0, max_candidates = 0, moved_next = 0, moved_prev = 0, first_hit = 0;
};

// The shim against the loop for seeds 1..n_seeds: the pick, and the generator's state through its next eight draws.
static Tally compare(Mirror& m, RoutingTable& rt, time_point now, unsigned n_seeds, const char* what,
                     uint32_t cap = Mirror::kMaintenanceCap) {
    Tally t;
    for (unsigned seed = 1; seed <= n_seeds; seed++) {
        std::mt19937 ra(seed), rb(seed);
        const RefPick want = ref_maintenance(rt, now, ra);
        const Pick got = m.bucketMaintenance(rt, now, rb, cap);
        EXPECT(got.found == want.found, "%s seed %u: found %d vs %d", what, seed, (int)got.found, (int)want.found);
        if (want.found && got.found) {
            EXPECT(got.bucket == want.bucket && got.q == want.q, "%s seed %u: bucket %u q %u vs %u %u", what, seed, got.bucket,
                   got.q, want.bucket, want.q);
            EXPECT(got.id == want.id, "%s seed %u: id", what, seed);
            EXPECT(got.node.get() == want.node.get(), "%s seed %u: node", what, seed);
            t.found++;
            t.first_hit += want.candidates == 1;
            t.moved_next += want.q == want.bucket + 1;
            t.moved_prev += want.q + 1 == want.bucket;
        } else {
            t.none++;
        }
        bool same = true;
        for (int k = 0; k < 8; k++) same &= ra() == rb();
        EXPECT(same, "%s seed %u: the generator is left in another state", what, seed);
        t.max_candidates = std::max(t.max_candidates, want.candidates);
    }
    return t;
}

static void check_times(const Mirror& m, const RoutingTable& rt, const char* what) {
    const std::vector<int64_t> got = m.bucketTimes();
    EXPECT(got.size() == rt.size(), "%s: %zu bucket times for %zu buckets", what, got.size(), rt.size());
    size_t k = 0;
    for (const auto& b : rt) {
        if (k < got.size()) EXPECT(got[k] == kadgpu::to_ns(b.time), "%s: time of bucket %zu", what, k);
        k++;
    }
}

int main() {
    const time_point now = clock::now() + std::chrono::hours(1000);
    const time_point stale = now - std::chrono::minutes(10) - std::chrono::nanoseconds(1), fresh = now - std::chrono::minutes(3);
    const time_point tmin = time_point::min();

    // a node in the first candidate: a snapshot whose times were never written (all time_point::min())
    {
        RoutingTable rt = split_table(600, 0xB0C4);
        Mirror m(rt, now, 0);
        check_times(m, rt, "fresh snapshot");
        const Tally t = compare(m, rt, now, 64, "first candidate");
        EXPECT(t.found == 64 && t.first_hit >= 48 && t.moved_next >= 1, "ground: %u found, %u at once, %u moved", t.found,
               t.first_hit, t.moved_next);
    }
    // NEVER buckets first: four empty buckets whose neighbours are empty, then the empty bucket before a full one
    {
        std::vector<unsigned> w(32, 3);
        std::vector<time_point> tm(32, fresh);
        for (unsigned b = 0; b < 5; b++) w[b] = 0;
        tm[2] = stale; tm[9] = stale; tm[10] = tmin;
        RoutingTable rt = uniform_table(5, w, tm, 11);
        Mirror m(rt, now, 0);
        check_times(m, rt, "uploaded times");
        const Tally t = compare(m, rt, now, 64, "after NEVER buckets");
        EXPECT(t.found == 64 && t.max_candidates == 5, "ground: %u found after %u candidates", t.found, t.max_candidates);
    }
    // a MAYBE bucket first: bucket 0 is stale with nodes, its neighbour empty; one seed in eight moves on to bucket 1
    {
        std::vector<unsigned> w(32, 3);
        std::vector<time_point> tm(32, fresh);
        w[1] = w[2] = 0;
        tm[0] = stale;
        RoutingTable rt = uniform_table(5, w, tm, 12);
        Mirror m(rt, now, 0);
        const Tally t = compare(m, rt, now, 128, "MAYBE first");
        EXPECT(t.found == 128 && t.max_candidates == 2 && t.moved_prev >= 4, "ground: %u found, %u candidates, %u from prev",
               t.found, t.max_candidates, t.moved_prev);
    }
    // no node at all: every bucket empty (every one a NEVER candidate, randomId still draws); and no candidate at all
    {
        std::vector<unsigned> w(8, 0);
        std::vector<time_point> tm(8, fresh);
        RoutingTable rt = uniform_table(3, w, tm, 13);
        Mirror m(rt, now, 0);
        Tally t = compare(m, rt, now, 16, "all empty");
        EXPECT(t.none == 16 && t.max_candidates == 8, "ground: %u none, %u candidates", t.none, t.max_candidates);
        w.assign(8, 2);
        RoutingTable full = uniform_table(3, w, tm, 14);
        Mirror mf(full, now, 0);
        t = compare(mf, full, now, 4, "no candidate");
        EXPECT(t.none == 4 && t.max_candidates == 0, "ground: %u none, %u candidates", t.none, t.max_candidates);
        RoutingTable none;
        Mirror me(none, now, 0);
        t = compare(me, none, now, 2, "no bucket");
        EXPECT(t.none == 2, "no bucket");
    }
    // more candidates than one chunk: 11 NEVER buckets at cap 4 are three calls, the node comes in the third
    {
        std::vector<unsigned> w(32, 3);
        std::vector<time_point> tm(32, fresh);
        for (unsigned b = 0; b < 12; b++) w[b] = 0;
        RoutingTable rt = uniform_table(5, w, tm, 15);
        Mirror m(rt, now, 0);
        const size_t before = m.maintenanceCalls();
        const Tally t = compare(m, rt, now, 8, "chunks", 4);
        EXPECT(t.found == 8 && t.max_candidates == 12, "ground: %u found after %u candidates", t.found, t.max_candidates);
        EXPECT(m.maintenanceCalls() - before == 8 * 3, "chunked calls: %zu", m.maintenanceCalls() - before);
    }
    // onReportedAddr in a batch and one by one, the reset, and a flush after splits
    {
        RoutingTable rt = split_table(600, 0x7E57);
        size_t k = 0;
        for (auto& b : rt) {
            b.time = k % 3 == 0 ? fresh : k % 3 == 1 ? stale : tmin;
            k++;
        }
        Mirror m(rt, now, 0);
        check_times(m, rt, "snapshot");
        compare(m, rt, now, 16, "snapshot");
        std::mt19937_64 g(5);
        std::vector<InfoHash> ids;
        for (const auto& b : rt) {
            ids.push_back(b.first);
            InfoHash below = b.first;  // the ID just below a first belongs to the bucket before
            for (int x = 19; x >= 0; x--)
                if (below[x]-- != 0) break;
            ids.push_back(below);
        }
        InfoHash ones;
        ones.fill(0xFF);
        ids.push_back(ones);
        while (ids.size() % 64 != 1) {
            InfoHash r;
            for (auto& x : r) x = (uint8_t)g();
            ids.push_back(r);
        }
        const time_point t1 = now + std::chrono::seconds(1);
        std::vector<InfoHash> some(ids.begin() + 40, ids.begin() + 120);
        for (const auto& id : some) ref_reported(rt, id, t1);
        m.onReportedAddrBatch(some, t1);
        check_times(m, rt, "batch of 80");
        compare(m, rt, t1, 16, "batch of 80");
        const time_point t2 = now + std::chrono::seconds(2);
        for (size_t i = 0; i < 6; i++) {
            ref_reported(rt, ids[i * 7], t2);
            m.onReportedAddr(ids[i * 7], t2);
        }
        check_times(m, rt, "single reports");
        // splits on the host table, reported, then flushed: the new buckets carry their source's time
        const time_point t3 = now + std::chrono::seconds(3);
        const size_t B0 = rt.size();
        for (size_t idx : {size_t(0), B0, B0 / 2, B0 / 2 + 1}) {  // the first, the last, one in the middle and its new half
            ref_split(rt, std::next(rt.begin(), (long)idx));
            m.bucketSplit(idx);
        }
        m.flush(t3);
        EXPECT(m.bucketCount() == B0 + 4 && rt.size() == B0 + 4, "splits: %zu buckets", m.bucketCount());
        check_times(m, rt, "after splits");
        const time_point late = now + std::chrono::minutes(10);  // the buckets reported at t1, t2 are fresh, the rest stale
        const Tally t = compare(m, rt, late, 32, "after splits");
        EXPECT(t.found == 32, "after splits: found %u", t.found);
        for (const auto& id : ids) ref_reported(rt, id, t3);
        m.onReportedAddrBatch(ids, t3);
        check_times(m, rt, "every bucket reported");
        compare(m, rt, t3, 4, "every bucket fresh");
        for (auto& b : rt) b.time = tmin;
        m.resetBucketTimes();
        check_times(m, rt, "reset");
        compare(m, rt, t3, 8, "reset");
    }
    // the per-family forwarders
    {
        RoutingTable rt4 = split_table(300, 0xF4), rt6 = split_table(200, 0xF6);
        for (auto& b : rt6) b.time = fresh;
        kadgpu::DhtMirror<RoutingTable> dht;
        dht.snapshot(rt4, rt6, now, 0);
        dht.setClock([&] { return now; });
        std::vector<InfoHash> ids;
        for (const auto& b : rt4) ids.push_back(b.first);
        ids.resize(ids.size() / 2);
        for (const auto& id : ids) ref_reported(rt4, id, now);
        dht.onReportedAddrBatch(AF_INET, ids);
        ref_reported(rt6, ids[3], now);
        dht.onReportedAddr(AF_INET6, ids[3]);
        check_times(dht.buckets(AF_INET), rt4, "forwarder v4");
        check_times(dht.buckets(AF_INET6), rt6, "forwarder v6");
        for (unsigned seed = 1; seed <= 8; seed++) {
            for (int fam = 0; fam < 2; fam++) {
                RoutingTable& rt = fam ? rt6 : rt4;
                std::mt19937 ra(seed), rb(seed);
                const RefPick want = ref_maintenance(rt, now, ra);
                const Pick got = dht.bucketMaintenance(fam ? AF_INET6 : AF_INET, rt, rb);
                EXPECT(got.found == want.found && got.bucket == want.bucket && got.q == want.q && got.node.get() == want.node.get() &&
                           (!want.found || got.id == want.id) && ra() == rb(),
                       "forwarder maintenance family %d seed %u", fam, seed);
            }
        }
        for (auto& b : rt4) b.time = tmin;
        for (auto& b : rt6) b.time = tmin;
        dht.resetBucketTimes();
        check_times(dht.buckets(AF_INET), rt4, "forwarder reset v4");
        check_times(dht.buckets(AF_INET6), rt6, "forwarder reset v6");
    }
    if (fails) {
        std::fprintf(stderr, "FAIL: %d\n", fails);
        return 1;
    }
    std::printf("PASS\n");
    return 0;
}
