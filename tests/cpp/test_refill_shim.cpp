// C++ test of include/kadgpu.hpp's SearchesMirror::refillBatch, the snapshot / sync overloads that set
// KAD_SN_REMOVABLE, and DhtMirror::refillBatch (Dht::refill, dht.cpp:1647-1668) over test doubles shaped like OpenDHT's
// types, as tests/cpp/test_searches_shim.cpp: the batch against the doubles' own refill (getCachedNodes,
// node_cache.cpp:36-66, then insertNode with removeExpiredNode, dht.cpp:961-1047) search by search. After every round
// the host replays the rows on its own searches, reports the overflowed ones to sync, and the device set is exported
// and compared with the host's lists. A second round runs eleven minutes later (other entries are removable, some
// cached nodes have expired behind the mirror's back). Needs a GPU. Exit 0 = pass.
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <list>
#include <map>
#include <memory>
#include <random>
#include <vector>

#include "kadgpu.hpp"

namespace mock {
using Clock = std::chrono::steady_clock;
using time_point = Clock::time_point;
constexpr size_t SEARCH_NODES = 14;
struct InfoHash : std::array<uint8_t, 20> {
    int xorCmp(const InfoHash& a, const InfoHash& b) const {  // infohash.h: <0 if a is closer to *this than b
        for (size_t i = 0; i < 20; i++) {
            const uint8_t x = a[i] ^ (*this)[i], y = b[i] ^ (*this)[i];
            if (x != y) return x < y ? -1 : 1;
        }
        return 0;
    }
};
struct Node {
    InfoHash id;
    bool expired_ = false;
    time_point time;
    bool isExpired() const { return expired_; }
};
static const std::chrono::minutes NODE_EXPIRE_TIME(10);
struct SearchNode {
    std::shared_ptr<Node> node;
    bool candidate = false;
    bool isBad() const { return !node || node->isExpired() || candidate; }  // dht.cpp:458-460
};
struct Search {
    InfoHash id;
    bool expired = false;
    std::vector<SearchNode> nodes;

    bool removeExpiredNode(time_point now) {  // dht.h:628-640
        for (size_t e = nodes.size(); e != 0;) {
            const Node& n = *nodes[--e].node;
            if (n.isExpired() && n.time + NODE_EXPIRE_TIME < now) {
                nodes.erase(nodes.begin() + (std::ptrdiff_t)e);
                return true;
            }
        }
        return false;
    }
    // Dht::Search::insertNode (dht.cpp:961-1047) with an empty token, one family, one Node per ID.
    bool insertNode(const std::shared_ptr<Node>& snode, time_point now) {
        const InfoHash& nid = snode->id;
        size_t n = nodes.size();
        while (n != 0) {
            --n;
            if (nodes[n].node->id == nid) return false;
            if (id.xorCmp(nid, nodes[n].node->id) > 0) {
                ++n;
                break;
            }
        }
        size_t t = nodes.size(), bad = 0;
        bool full = false;
        if (expired) {
            if (nodes.size() >= SEARCH_NODES) {
                full = true;
                t = SEARCH_NODES;
            }
        } else {
            bad = (size_t)std::count_if(nodes.begin(), nodes.end(), [](const SearchNode& sn) { return sn.isBad(); });
            full = nodes.size() - bad >= SEARCH_NODES;
            while (t - bad > SEARCH_NODES) {
                --t;
                if (nodes[t].isBad()) bad--;
            }
        }
        if (full) {
            if (t != nodes.size()) nodes.resize(t);
            if (n >= t) return false;
        }
        SearchNode sn;
        sn.node = snode;
        nodes.insert(nodes.begin() + (std::ptrdiff_t)n, sn);
        snode->time = now;
        if (snode->isExpired()) {
            if (!expired) bad++;
        } else if (expired) {
            bad = nodes.size() - 1;
            expired = false;
        }
        while (nodes.size() - bad > SEARCH_NODES) {
            if (!expired && nodes.back().isBad()) bad--;
            nodes.pop_back();
        }
        removeExpiredNode(now);
        return true;
    }
};
using SearchMap = std::map<InfoHash, std::shared_ptr<Search>>;
using NodeMap = std::map<InfoHash, std::weak_ptr<Node>>;
struct Bucket {
    InfoHash first;
    std::list<std::shared_ptr<Node>> nodes;
};
using RoutingTable = std::list<Bucket>;

// NodeCache::getCachedNodes for one family (node_cache.cpp:36-66)
static std::vector<std::shared_ptr<Node>> getCachedNodes(const NodeMap& c, const InfoHash& id, size_t count) {
    auto it_p = c.lower_bound(id), it_n = it_p;
    std::vector<std::shared_ptr<Node>> nodes;
    NodeMap::const_iterator it;
    if (it_p != c.begin()) --it_p;
    while (nodes.size() < count && (it_n != c.end() || it_p != c.end())) {
        if (it_p == c.end()) it = it_n++;
        else if (it_n == c.end()) it = it_p--;
        else it = id.xorCmp(it_p->first, it_n->first) < 0 ? it_p-- : it_n++;
        if (it == c.begin()) it_p = c.end();
        if (auto n = it->second.lock())
            if (!n->isExpired()) nodes.emplace_back(std::move(n));
    }
    return nodes;
}
}  // namespace mock

static int fails = 0;
#define EXPECT(c, ...) do { if (!(c)) { fails++; if (fails < 30) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } } while (0)

using namespace mock;

static InfoHash rand_id(std::mt19937_64& g) {
    InfoHash h;
    for (auto& b : h) b = (uint8_t)g();
    return h;
}

static InfoHash near_id(std::mt19937_64& g, const InfoHash& of, size_t bytes) {
    InfoHash h = rand_id(g);
    std::copy(of.begin(), of.begin() + (std::ptrdiff_t)bytes, h.begin());
    return h;
}

static time_point some_time(std::mt19937_64& g, time_point now) {
    static const int back[4] = {0, 100, 700, 1300};
    return now - std::chrono::seconds(back[g() % 4]);
}

struct Cache {
    std::vector<std::shared_ptr<Node>> owners;
    NodeMap map;
};

static Cache make_cache(uint32_t n, uint64_t seed, time_point now) {
    std::mt19937_64 g(seed);
    Cache c;
    while (c.map.size() < n) {
        auto nd = std::make_shared<Node>();
        nd->id = rand_id(g);
        nd->expired_ = g() % 5 == 0;
        nd->time = some_time(g, now);
        if (c.map.emplace(nd->id, nd).second) c.owners.push_back(nd);
    }
    return c;
}

// Searches whose lists hold cached nodes around the search ID and strangers sharing a prefix with it.
static SearchMap make_searches(uint32_t S, uint64_t seed, const Cache& c, time_point now) {
    std::mt19937_64 g(seed);
    SearchMap m;
    while (m.size() < S) {
        auto s = std::make_shared<Search>();
        s->id = g() % 4 == 0 ? near_id(g, c.owners[g() % c.owners.size()]->id, 6) : rand_id(g);
        const unsigned kind = g() % 6;  // empty, short, full, expired, long with bad nodes, short and expired
        const size_t n = kind == 0 ? 0 : kind == 1 || kind == 5 ? 1 + g() % 13 : kind == 2 ? 14 : kind == 3 ? 14 + g() % 5
                                                                                                 : 15 + g() % 16;
        std::vector<std::shared_ptr<Node>> picked;
        auto around = c.map.lower_bound(s->id);
        for (int k = 0; k < 12 && around != c.map.begin(); k++) --around;
        for (int k = 0; k < 24 && around != c.map.end() && picked.size() < n; k++, ++around)
            if (g() % 3 == 0) picked.push_back(around->second.lock());
        const size_t share = 1 + g() % 4;
        while (picked.size() < n) {
            auto nd = std::make_shared<Node>();
            nd->id = near_id(g, s->id, share);
            nd->time = some_time(g, now);
            const bool fresh = nd->id != s->id && !c.map.count(nd->id) &&
                               std::none_of(picked.begin(), picked.end(),
                                            [&](const std::shared_ptr<Node>& p) { return p->id == nd->id; });
            if (fresh) picked.push_back(nd);
        }
        std::sort(picked.begin(), picked.end(), [&](const std::shared_ptr<Node>& a, const std::shared_ptr<Node>& b) {
            return s->id.xorCmp(a->id, b->id) < 0;
        });
        for (const auto& nd : picked) {
            SearchNode sn;
            sn.node = nd;
            const bool cached = c.map.count(nd->id) != 0;
            if ((kind == 3 || kind == 5) && !nd->expired_) (cached ? sn.candidate : nd->expired_) = true;
            if (kind == 4 && g() % 3 == 0) (cached || (g() & 1) ? sn.candidate : nd->expired_) = true;
            if (kind == 2 && nd->expired_ && !cached) nd->expired_ = false;
            s->nodes.push_back(sn);
        }
        s->expired = kind == 3 || kind == 5;
        m[s->id] = s;
    }
    return m;
}

static bool removable(const Node& n, time_point now) { return n.isExpired() && n.time + NODE_EXPIRE_TIME < now; }

// The device set against the host's searches: n, IDs and flag bytes (KAD_SN_REMOVABLE at `now`) of every list.
static void compare_export(const char* what, const kad_searches* ss, const SearchMap& m, time_point now) {
    uint32_t S = 0, cap = 0;
    EXPECT(kad_searches_info(ss, &S, &cap, nullptr) == KAD_OK && S == m.size(), "%s: info", what);
    std::vector<uint8_t> flags(S), nid((size_t)S * cap * 20), nfl((size_t)S * cap);
    std::vector<uint32_t> n(S);
    EXPECT(kad_searches_export(ss, nullptr, flags.data(), n.data(), nid.data(), nfl.data(), nullptr, nullptr) == KAD_OK,
           "%s: export", what);
    uint32_t s = 0;
    for (const auto& kv : m) {
        const Search& sr = *kv.second;
        bool same = n[s] == sr.nodes.size() && flags[s] == (sr.expired ? KAD_SR_EXPIRED : 0u);
        for (size_t j = 0; same && j < sr.nodes.size(); j++) {
            const size_t e = (size_t)s * cap + j;
            const uint8_t fl = (uint8_t)((sr.nodes[j].isBad() ? KAD_SN_BAD : 0u) |
                                         (removable(*sr.nodes[j].node, now) ? KAD_SN_REMOVABLE : 0u));
            same = std::equal(sr.nodes[j].node->id.begin(), sr.nodes[j].node->id.end(), &nid[e * 20]) && nfl[e] == fl;
        }
        EXPECT(same, "%s: search %u differs from the host's (n %u, host %zu)", what, s, n[s], sr.nodes.size());
        s++;
    }
}

struct Round {
    size_t inserted = 0, overflow = 0, shrunk = 0;
};

// One refill round: the batch against the doubles' refill on `m`, which is left refilled; returns the overflowed IDs.
template <class Batch>
static std::vector<InfoHash> refill_round(const char* what, SearchMap& m, const NodeMap& cache,
                                          const std::vector<InfoHash>& ids, time_point now, Batch batch, Round& st) {
    const auto got = batch(ids);
    std::vector<InfoHash> over;
    EXPECT(got.size() == ids.size(), "%s: size", what);
    for (size_t i = 0; i < ids.size() && i < got.size(); i++) {
        Search& sr = *m[ids[i]];
        const std::vector<std::shared_ptr<Node>> row = getCachedNodes(cache, sr.id, SEARCH_NODES);
        EXPECT(row == got[i].nodes, "%s: search %zu: row of %zu nodes, want %zu", what, i, got[i].nodes.size(), row.size());
        const size_t before = sr.nodes.size();
        unsigned mask = 0;
        for (size_t j = 0; j < row.size(); j++)  // dht.cpp:1659-1663
            if (sr.insertNode(row[j], now)) mask |= 1u << j;
        if (got[i].overflow) {
            over.push_back(ids[i]);
            EXPECT(got[i].inserted == 0, "%s: search %zu: overflowed with a mask", what, i);
            st.overflow++;
        } else {
            EXPECT(got[i].inserted == mask, "%s: search %zu: inserted %04x, want %04x", what, i, got[i].inserted, mask);
        }
        st.inserted += (size_t)__builtin_popcount(mask);
        st.shrunk += mask && sr.nodes.size() < before + (size_t)__builtin_popcount(mask);
    }
    return over;
}

int main() {
    const time_point now = Clock::now();
    Cache c4 = make_cache(2000, 1, now), c6 = make_cache(300, 2, now);
    SearchMap m4 = make_searches(150, 3, c4, now), m6 = make_searches(40, 4, c6, now), none;
    std::vector<InfoHash> all4, all6;
    for (const auto& kv : m4) all4.push_back(kv.first);
    for (const auto& kv : m6) all6.push_back(kv.first);
    try {
        kadgpu::NodeCacheMirror<NodeMap> NC;
        NC.snapshot(c4.map, c6.map);
        {  // the untimed snapshot keeps taking plain integers for device and cap: they must not select the timed form
            kadgpu::SearchesMirror<SearchMap> P;
            P.snapshot(m6, 0, 14);
            P.snapshot(m6, 0);
            EXPECT(P.size() == m6.size() && P.cap() >= 14, "snapshot(map, 0, 14)");
            P.sync(std::vector<InfoHash>(1, all6[0]));
            compare_export("untimed snapshot", P.handle(), m6, now - std::chrono::hours(1));  // no removable bits
        }
        kadgpu::SearchesMirror<SearchMap> M;
        M.snapshot(m4, now, 0, 14);  // slabs as small as the lists allow: some refills overflow
        compare_export("snapshot", M.handle(), m4, now);
        EXPECT(M.refillBatch(NC.family(AF_INET), std::vector<InfoHash>(), now).empty(), "empty batch");

        // round 1: two thirds of the searches, in shuffled order
        std::vector<InfoHash> ids;
        for (size_t i = 0; i < all4.size(); i++)
            if (i % 3) ids.push_back(all4[i]);
        std::shuffle(ids.begin(), ids.end(), std::mt19937_64(7));
        Round r1;
        std::vector<InfoHash> over = refill_round("round 1", m4, c4.map, ids, now, [&](const std::vector<InfoHash>& v) {
            return M.refillBatch(NC.family(AF_INET), v, now); }, r1);
        EXPECT(r1.inserted > 100 && r1.shrunk > 5, "round 1: %zu inserts, %zu shrinking refills", r1.inserted, r1.shrunk);
        M.sync(over, now);
        compare_export("round 1", M.handle(), m4, now);

        // round 2, eleven minutes later: entries turned removable, and cached nodes expired without a notification
        const time_point later = now + std::chrono::minutes(11);
        for (size_t i = 0; i < c4.owners.size(); i += 7)
            if (!c4.owners[i]->expired_) {
                c4.owners[i]->expired_ = true;
                c4.owners[i]->time = later - std::chrono::seconds(30);
            }
        std::vector<InfoHash> touched;  // the searches that hold one of those nodes changed their flags
        for (const auto& kv : m4) touched.push_back(kv.first);
        M.sync(touched, later);
        compare_export("resync", M.handle(), m4, later);
        Round r2;
        over = refill_round("round 2", m4, c4.map, all4, later, [&](const std::vector<InfoHash>& v) {
            return M.refillBatch(NC.family(AF_INET), v, later); }, r2);
        EXPECT(r2.inserted > 20 && r2.overflow > 0, "round 2: %zu inserts, %zu handed back", r2.inserted, r2.overflow);
        M.sync(over, later);
        compare_export("round 2", M.handle(), m4, later);

        bool threw = false;
        try {
            M.refillBatch(NC.family(AF_INET), std::vector<InfoHash>(2, all4[0]), later);
        } catch (const kadgpu::Error& e) {
            threw = e.code() == KAD_ERR_INVALID;
        }
        EXPECT(threw, "a search listed twice did not throw");

        // DhtMirror forwards by family at its clock; a snapshot without a time has no removable bits, so the searches
        // that need them are patched first
        kadgpu::DhtMirror<RoutingTable, Clock, SearchMap> D;
        D.setClock([&] { return now; });
        D.snapshotSearches(none, m6);
        Round r3;
        over = refill_round("dht v6", m6, c6.map, all6, now, [&](const std::vector<InfoHash>& v) {
            return D.refillBatch(NC, AF_INET6, v); }, r3);
        EXPECT(r3.inserted > 10, "dht v6: %zu inserts", r3.inserted);
        D.syncSearches(AF_INET6, over, now);
        compare_export("dht v6", D.searches(AF_INET6).handle(), m6, now);
        EXPECT(D.refillBatch(NC, AF_INET, std::vector<InfoHash>()).empty(), "empty family");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    if (fails) {
        std::fprintf(stderr, "%d failures\n", fails);
        return 1;
    }
    std::printf("PASS\n");
    return 0;
}
