// C++ test of include/kadgpu.hpp's SearchesMirror::update and DhtMirror::updateSearches (kad_searches_apply) over test
// doubles shaped like OpenDHT's types, as tests/cpp/test_searches_shim.cpp and tests/cpp/test_refill_shim.cpp: searches
// are erased from the map (Dht::expireSearches, dht.cpp:1060-1074), new ones emplaced (Dht::search, :1691-1693; one of
// them already holds nodes, one re-uses the ID of an erased search), then update() is told. Afterwards
// trySearchInsertBatch must equal the doubles' insertNode on copies, refillBatch on the new searches the doubles' refill
// (:1647-1668), and the exported device set the host's lists. An unmirrored ID in `erased` must throw. Needs a GPU.
// Exit 0 = pass.
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
    unsigned refusal = 0;  // why the last insertNode returned false: KAD_SR_STOP_*

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
            if (nodes[n].node->id == nid) {
                refusal = KAD_SR_STOP_KNOWN;
                return false;
            }
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
            if (n >= t) {
                refusal = expired ? KAD_SR_STOP_FAR_EXPIRED : KAD_SR_STOP_FAR;
                return false;
            }
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

// accept(s, x) by the double's insertNode on a copy: 0xFF if it accepts, else the stop code.
static unsigned probe(const Search& s, const InfoHash& x, time_point now) {
    Search c = s;
    auto nd = std::make_shared<Node>();
    nd->id = x;
    return c.insertNode(nd, now) ? 0xFFu : c.refusal;
}

static kadgpu::SearchInsertVerdict want(const SearchMap& m, const InfoHash& x, time_point now) {
    std::vector<const Search*> v;
    for (const auto& kv : m) v.push_back(kv.second.get());
    const uint32_t lb = (uint32_t)std::distance(m.begin(), m.lower_bound(x));
    uint32_t fwd = 0, back = 0;
    unsigned fs = KAD_SR_STOP_END, bs = KAD_SR_STOP_END;
    for (size_t s = lb; s < v.size(); s++) {
        const unsigned r = probe(*v[s], x, now);
        if (r != 0xFFu) { fs = r; break; }
        fwd++;
    }
    for (size_t s = lb; s > 0;) {
        const unsigned r = probe(*v[--s], x, now);
        if (r != 0xFFu) { bs = r; break; }
        back++;
    }
    return kadgpu::SearchInsertVerdict{lb, fwd, back, (uint8_t)(fs | bs << 4)};
}

// candidates: random, every search ID and its neighbours in the last byte, members of the lists
static std::vector<InfoHash> make_cands(const SearchMap& m, uint64_t seed) {
    std::mt19937_64 g(seed);
    std::vector<InfoHash> out;
    for (const auto& kv : m) {
        InfoHash up = kv.first, down = kv.first;
        up[19]++;
        down[19]--;
        out.insert(out.end(), {kv.first, up, down, rand_id(g), near_id(g, kv.first, 1 + g() % 12)});
        if (!kv.second->nodes.empty()) out.push_back(kv.second->nodes[g() % kv.second->nodes.size()].node->id);
    }
    return out;
}

template <class Batch>
static void compare_verdicts(const char* what, const SearchMap& m, time_point now, Batch batch) {
    const std::vector<InfoHash> cands = make_cands(m, 11);
    const std::vector<kadgpu::SearchInsertVerdict> got = batch(cands.data(), cands.size());
    EXPECT(got.size() == cands.size(), "%s: size", what);
    for (size_t i = 0; i < cands.size() && i < got.size(); i++) {
        const kadgpu::SearchInsertVerdict w = want(m, cands[i], now);
        EXPECT(got[i].lb == w.lb && got[i].fwd == w.fwd && got[i].back == w.back && got[i].stop == w.stop,
               "%s: candidate %zu: got lb %u fwd %u back %u stop %02x, want lb %u fwd %u back %u stop %02x", what, i,
               got[i].lb, got[i].fwd, got[i].back, got[i].stop, w.lb, w.fwd, w.back, w.stop);
    }
}

// The batch refill of `ids` against the doubles' refill on `m`, which is left refilled; returns the overflowed IDs.
template <class Batch>
static std::vector<InfoHash> refill_round(const char* what, SearchMap& m, const NodeMap& cache,
                                          const std::vector<InfoHash>& ids, time_point now, Batch batch, size_t& inserted) {
    const auto got = batch(ids);
    std::vector<InfoHash> over;
    EXPECT(got.size() == ids.size(), "%s: size", what);
    for (size_t i = 0; i < ids.size() && i < got.size(); i++) {
        Search& sr = *m[ids[i]];
        const std::vector<std::shared_ptr<Node>> row = getCachedNodes(cache, sr.id, SEARCH_NODES);
        EXPECT(row == got[i].nodes, "%s: search %zu: row of %zu nodes, want %zu", what, i, got[i].nodes.size(), row.size());
        unsigned mask = 0;
        for (size_t j = 0; j < row.size(); j++)  // dht.cpp:1659-1663
            if (sr.insertNode(row[j], now)) mask |= 1u << j;
        if (got[i].overflow)
            over.push_back(ids[i]);
        else
            EXPECT(got[i].inserted == mask, "%s: search %zu: inserted %04x, want %04x", what, i, got[i].inserted, mask);
        inserted += (size_t)__builtin_popcount(mask);
    }
    return over;
}

// Dht::expireSearches and Dht::search on the map: every `stride`-th search goes, `fresh` new empty ones come, the
// first erased ID is used again by an empty search, and one new search already holds five nodes.
static void change_map(SearchMap& m, const Cache& c, uint64_t seed, size_t stride, size_t fresh, time_point now,
                       std::vector<InfoHash>& erased, std::vector<InfoHash>& added) {
    std::mt19937_64 g(seed);
    size_t i = 0;
    for (auto it = m.begin(); it != m.end(); i++) {
        if (i % stride == 1) {
            erased.push_back(it->first);
            it = m.erase(it);
        } else {
            ++it;
        }
    }
    auto emplace = [&](const InfoHash& id) {
        auto s = std::make_shared<Search>();
        s->id = id;
        if (m.emplace(id, s).second) added.push_back(id);
        return s;
    };
    emplace(erased[0]);
    InfoHash lo, hi;
    lo.fill(0x00);
    hi.fill(0xFF);
    emplace(lo);
    emplace(hi);
    while (added.size() < fresh) emplace(g() % 3 == 0 ? near_id(g, c.owners[g() % c.owners.size()]->id, 6) : rand_id(g));
    auto s = emplace(rand_id(g));
    for (const auto& nd : getCachedNodes(c.map, s->id, 5)) s->insertNode(nd, now);
    std::shuffle(added.begin(), added.end(), g);
}

int main() {
    const time_point now = Clock::now();
    Cache c4 = make_cache(2000, 1, now), c6 = make_cache(300, 2, now);
    SearchMap m4 = make_searches(150, 3, c4, now), m6 = make_searches(40, 4, c6, now), none;
    try {
        kadgpu::NodeCacheMirror<NodeMap> NC;
        NC.snapshot(c4.map, c6.map);
        kadgpu::SearchesMirror<SearchMap> M;
        M.snapshot(m4, now, 0, 32);
        compare_export("snapshot", M.handle(), m4, now);

        std::vector<InfoHash> erased, added;
        change_map(m4, c4, 21, 4, 30, now, erased, added);
        EXPECT(erased.size() > 30 && added.size() == 31, "%zu erased, %zu added", erased.size(), added.size());
        M.update(erased, added, now);
        EXPECT(M.size() == m4.size(), "update: %zu mirrored, the map holds %zu", M.size(), m4.size());
        compare_export("update", M.handle(), m4, now);
        compare_verdicts("update", m4, now, [&](const InfoHash* p, size_t q) { return M.trySearchInsertBatch(p, q); });
        size_t inserted = 0;
        std::vector<InfoHash> over = refill_round("refill of the new", m4, c4.map, added, now,
            [&](const std::vector<InfoHash>& v) { return M.refillBatch(NC.family(AF_INET), v, now); }, inserted);
        EXPECT(inserted > 200, "refill of the new searches: %zu inserts", inserted);
        M.sync(over, now);
        compare_export("refilled", M.handle(), m4, now);
        compare_verdicts("refilled", m4, now, [&](const InfoHash* p, size_t q) { return M.trySearchInsertBatch(p, q); });

        // rejected updates leave the mirror as it was
        std::mt19937_64 g(99);
        const InfoHash stranger = rand_id(g);
        int threw = 0;
        try {
            M.update(std::vector<InfoHash>(1, stranger), std::vector<InfoHash>());
        } catch (const kadgpu::Error& e) {
            threw += e.code() == KAD_ERR_INVALID;
        }
        try {  // already mirrored and not erased
            M.update(std::vector<InfoHash>(), std::vector<InfoHash>(1, added[0]));
        } catch (const kadgpu::Error& e) {
            threw += e.code() == KAD_ERR_INVALID;
        }
        try {  // not in the map
            M.update(std::vector<InfoHash>(), std::vector<InfoHash>(1, stranger));
        } catch (const kadgpu::Error& e) {
            threw += e.code() == KAD_ERR_INVALID;
        }
        EXPECT(threw == 3, "%d of 3 bad updates threw KAD_ERR_INVALID", threw);
        compare_export("after rejected updates", M.handle(), m4, now);
        M.update(std::vector<InfoHash>(), std::vector<InfoHash>());  // nothing to do
        M.update(added, std::vector<InfoHash>());                    // only erased, without a time
        for (const auto& id : added) m4.erase(id);
        compare_export("erased again", M.handle(), m4, now);

        // DhtMirror forwards by family at its clock
        kadgpu::DhtMirror<RoutingTable, Clock, SearchMap> D;
        D.setClock([&] { return now; });
        D.snapshotSearches(none, m6);
        erased.clear();
        added.clear();
        change_map(m6, c6, 22, 3, 8, now, erased, added);
        D.updateSearches(AF_INET6, erased, added);
        // snapshotSearches takes no time: the kept searches carry no removable bits, and the new ones hold live nodes
        const time_point never = now - std::chrono::hours(1);
        compare_export("dht v6", D.searches(AF_INET6).handle(), m6, never);
        compare_verdicts("dht v6", m6, now, [&](const InfoHash* p, size_t q) { return D.trySearchInsertBatch(p, q, AF_INET6); });
        inserted = 0;
        over = refill_round("dht v6", m6, c6.map, added, now,
            [&](const std::vector<InfoHash>& v) { return D.refillBatch(NC, AF_INET6, v); }, inserted);
        EXPECT(inserted > 50, "dht v6: %zu inserts", inserted);
        D.syncSearches(AF_INET6, over, now);
        compare_export("dht v6 refilled", D.searches(AF_INET6).handle(), m6, never);
        D.updateSearches(AF_INET, std::vector<InfoHash>(), std::vector<InfoHash>());  // an empty family
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
