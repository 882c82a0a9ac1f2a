// C++ test of include/kadgpu.hpp's SearchesMirror::insertBatch and DhtMirror::insertBatch (Search::insertNode on
// candidates of the caller, dht.cpp:961-1047) over test doubles shaped like OpenDHT's types, as
// tests/cpp/test_refill_shim.cpp: the batch against the doubles' own insertNode (with removeExpiredNode), candidate by
// candidate. After every round the host replays the inserts on its own searches, reports the searches handed back to
// sync, and the device set is exported and compared with the host's lists. A second round runs eleven minutes later
// without any sync in between: the expired nodes the first round inserted are removable by then, so the mirror has to
// patch those searches by itself before it inserts. Needs a GPU. Exit 0 = pass.
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
struct Bucket {
    InfoHash first;
    std::list<std::shared_ptr<Node>> nodes;
};
using RoutingTable = std::list<Bucket>;
}  // namespace mock

static int fails = 0;
#define EXPECT(c, ...) do { if (!(c)) { fails++; if (fails < 30) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } } while (0)

using namespace mock;
typedef std::shared_ptr<Node> NodeP;

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

static bool removable(const Node& n, time_point now) { return n.isExpired() && n.time + NODE_EXPIRE_TIME < now; }

// Searches of strangers sharing a prefix with the search ID: empty, short, full, expired, long with bad nodes (expired
// ones at any time, so some are removable), short and expired.
static SearchMap make_searches(uint32_t S, uint64_t seed, time_point now) {
    std::mt19937_64 g(seed);
    SearchMap m;
    while (m.size() < S) {
        auto s = std::make_shared<Search>();
        s->id = rand_id(g);
        const unsigned kind = g() % 6;
        const size_t n = kind == 0 ? 0 : kind == 1 || kind == 5 ? 1 + g() % 13 : kind == 2 ? 14 : kind == 3 ? 14 + g() % 5
                                                                                                 : 15 + g() % 16;
        std::vector<NodeP> picked;
        const size_t share = 1 + g() % 4;
        while (picked.size() < n) {
            auto nd = std::make_shared<Node>();
            nd->id = near_id(g, s->id, share);
            nd->time = some_time(g, now);
            if (nd->id != s->id && std::none_of(picked.begin(), picked.end(), [&](const NodeP& p) { return p->id == nd->id; }))
                picked.push_back(nd);
        }
        std::sort(picked.begin(), picked.end(), [&](const NodeP& a, const NodeP& b) { return s->id.xorCmp(a->id, b->id) < 0; });
        for (const auto& nd : picked) {
            SearchNode sn;
            sn.node = nd;
            if (kind == 3 || kind == 5) nd->expired_ = true;
            if (kind == 4 && g() % 3 == 0) ((g() & 1) ? sn.candidate : nd->expired_) = true;
            s->nodes.push_back(sn);
        }
        s->expired = kind == 3 || kind == 5;
        m[s->id] = s;
    }
    return m;
}

// 0 to 20 candidates for one search: strangers near it (a third expired; `old` lets some of those be removable),
// members of the search, repeats of earlier candidates.
static std::vector<NodeP> make_cands(std::mt19937_64& g, const Search& s, time_point now, bool old) {
    std::vector<NodeP> out;
    const size_t n = g() % 21;
    while (out.size() < n) {
        const unsigned kind = g() % 8;
        if (kind == 0 && !out.empty()) {
            out.push_back(out[g() % out.size()]);
        } else if (kind == 1 && !s.nodes.empty()) {
            const NodeP& mnode = s.nodes[g() % s.nodes.size()].node;
            if (old || !removable(*mnode, now)) out.push_back(mnode);
        } else {
            auto nd = std::make_shared<Node>();
            nd->id = near_id(g, s.id, kind < 4 ? 1 + g() % 4 : 0);
            nd->expired_ = g() % 3 == 0;
            nd->time = old ? some_time(g, now) : now - std::chrono::seconds(g() % 500);
            if (nd->id != s.id) out.push_back(nd);
        }
    }
    return out;
}

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
    size_t inserted = 0, refused = 0, overflow = 0, held = 0, sent = 0;
};

// One round: the batch against the doubles' insertNode on `m`, which is left with the inserts applied; returns the IDs
// handed back.
template <class Batch>
static std::vector<InfoHash> insert_round(const char* what, SearchMap& m, const std::vector<InfoHash>& ids,
                                          const std::vector<std::vector<NodeP>>& nodes, time_point now, Batch batch,
                                          Round& st) {
    std::vector<bool> held(ids.size(), false);  // before the host's inserts write node->time
    for (size_t i = 0; i < ids.size(); i++)
        for (const auto& n : nodes[i]) held[i] = held[i] || removable(*n, now);
    const std::vector<kadgpu::InsertResult> got = batch(ids, nodes);
    std::vector<InfoHash> over;
    EXPECT(got.size() == ids.size(), "%s: size", what);
    for (size_t i = 0; i < ids.size() && i < got.size(); i++) {
        Search& sr = *m[ids[i]];
        EXPECT(got[i].inserted.size() == nodes[i].size(), "%s: search %zu: %zu result bytes", what, i, got[i].inserted.size());
        EXPECT(!held[i] || got[i].overflow, "%s: search %zu: a removable candidate was sent", what, i);
        st.held += held[i];
        st.sent += !held[i];
        for (size_t j = 0; j < nodes[i].size(); j++) {
            const bool ok = sr.insertNode(nodes[i][j], now);
            st.inserted += ok;
            st.refused += !ok;
            if (got[i].overflow)
                EXPECT(j >= got[i].inserted.size() || got[i].inserted[j] == 0, "%s: search %zu: handed back with a result", what, i);
            else
                EXPECT(j < got[i].inserted.size() && got[i].inserted[j] == (ok ? 1 : 0),
                       "%s: search %zu, candidate %zu: want %d", what, i, j, (int)ok);
        }
        if (got[i].overflow) {
            over.push_back(ids[i]);
            st.overflow++;
        }
    }
    return over;
}

int main() {
    const time_point now = Clock::now();
    SearchMap m4 = make_searches(150, 3, now), m6 = make_searches(40, 4, now), none;
    std::vector<InfoHash> all4, all6;
    for (const auto& kv : m4) all4.push_back(kv.first);
    for (const auto& kv : m6) all6.push_back(kv.first);
    std::mt19937_64 g(11);
    try {
        kadgpu::SearchesMirror<SearchMap> M;
        M.snapshot(m4, now, 0, 14);  // slabs as small as the lists allow: some inserts overflow
        compare_export("snapshot", M.handle(), m4, now);
        EXPECT(M.insertBatch(std::vector<InfoHash>(), std::vector<std::vector<NodeP>>(), now).empty(), "empty batch");

        // round 1: two thirds of the searches, in shuffled order; one search in eight gets candidates of any age
        std::vector<InfoHash> ids;
        for (size_t i = 0; i < all4.size(); i++)
            if (i % 3) ids.push_back(all4[i]);
        std::shuffle(ids.begin(), ids.end(), std::mt19937_64(7));
        std::vector<std::vector<NodeP>> nodes;
        for (size_t i = 0; i < ids.size(); i++) nodes.push_back(make_cands(g, *m4[ids[i]], now, i % 8 == 0));
        Round r1;
        std::vector<InfoHash> over = insert_round("round 1", m4, ids, nodes, now,
            [&](const std::vector<InfoHash>& v, const std::vector<std::vector<NodeP>>& n) { return M.insertBatch(v, n, now); }, r1);
        EXPECT(r1.inserted > 200 && r1.refused > 50 && r1.held > 2 && r1.sent > 50 && r1.overflow >= r1.held,
               "round 1: %zu inserts, %zu refusals, %zu held, %zu sent, %zu handed back", r1.inserted, r1.refused, r1.held,
               r1.sent, r1.overflow);
        M.sync(over, now);
        compare_export("round 1", M.handle(), m4, now);

        // round 2, eleven minutes later, nothing reported in between: every expired node of round 1 is removable now
        const time_point later = now + std::chrono::minutes(11);
        nodes.clear();
        for (size_t i = 0; i < all4.size(); i++) nodes.push_back(make_cands(g, *m4[all4[i]], later, false));
        Round r2;
        over = insert_round("round 2", m4, all4, nodes, later,
            [&](const std::vector<InfoHash>& v, const std::vector<std::vector<NodeP>>& n) { return M.insertBatch(v, n, later); }, r2);
        EXPECT(r2.inserted > 200 && r2.sent > 100, "round 2: %zu inserts, %zu sent", r2.inserted, r2.sent);
        M.sync(over, later);
        // every search was listed: sent ones were patched where their bits had moved, the others went through sync
        compare_export("round 2", M.handle(), m4, later);

        bool threw = false;
        try {
            M.insertBatch(std::vector<InfoHash>(2, all4[0]), std::vector<std::vector<NodeP>>(2), later);
        } catch (const kadgpu::Error& e) {
            threw = e.code() == KAD_ERR_INVALID;
        }
        EXPECT(threw, "a search listed twice did not throw");

        // DhtMirror forwards by family at its clock; a snapshot without a time has no removable bits, so the searches
        // that need them are patched first
        kadgpu::DhtMirror<RoutingTable, Clock, SearchMap> D;
        D.setClock([&] { return now; });
        D.snapshotSearches(none, m6);
        nodes.clear();
        for (size_t i = 0; i < all6.size(); i++) nodes.push_back(make_cands(g, *m6[all6[i]], now, false));
        Round r3;
        over = insert_round("dht v6", m6, all6, nodes, now,
            [&](const std::vector<InfoHash>& v, const std::vector<std::vector<NodeP>>& n) { return D.insertBatch(AF_INET6, v, n); }, r3);
        EXPECT(r3.inserted > 30, "dht v6: %zu inserts", r3.inserted);
        D.syncSearches(AF_INET6, over, now);
        compare_export("dht v6", D.searches(AF_INET6).handle(), m6, now);
        EXPECT(D.insertBatch(AF_INET, std::vector<InfoHash>(), std::vector<std::vector<NodeP>>()).empty(), "empty family");
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
