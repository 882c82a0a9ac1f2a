// C++ test of include/kadgpu.hpp's SearchesMirror::markNodes and DhtMirror::markNodes (node status changes carried to
// the device set) over test doubles shaped like OpenDHT's types, with Node objects shared between the
// searches through the NodeCache as in tests/cpp/test_refill_shim.cpp. After a snapshot, nodes expire and reply and
// `candidate` bits flip on the host; one markNodes reports them, and the device set is exported and compared with the
// host's lists, its verdicts with those of a fresh snapshot, the returned counts with the host's own loops. Eleven
// minutes later a second markNodes sets KAD_SN_REMOVABLE on the entries whose ten minutes ran out; then insertBatch and
// refillBatch run with nothing synced in between and must equal the host's own walk. Needs a GPU. Exit 0 = pass.
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <list>
#include <map>
#include <memory>
#include <random>
#include <set>
#include <utility>
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

struct InsertRound {
    size_t inserted = 0, refused = 0, overflow = 0, held = 0, sent = 0;
};

// One round: the batch against the doubles' insertNode on `m`, which is left with the inserts applied; returns the IDs
// handed back.
template <class Batch>
static std::vector<InfoHash> insert_round(const char* what, SearchMap& m, const std::vector<InfoHash>& ids,
                                          const std::vector<std::vector<NodeP>>& nodes, time_point now, Batch batch,
                                          InsertRound& st) {
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


// ---- markNodes -------------------------------------------------------------------------------------------------------
// every Node some search of m holds, once
static std::vector<NodeP> nodes_of(const SearchMap& m) {
    std::set<const Node*> seen;
    std::vector<NodeP> out;
    for (const auto& kv : m)
        for (const auto& sn : kv.second->nodes)
            if (seen.insert(sn.node.get()).second) out.push_back(sn.node);
    return out;
}

static std::vector<std::vector<uint8_t>> flags_of(const SearchMap& m, time_point now) {
    std::vector<std::vector<uint8_t>> out;
    for (const auto& kv : m) {
        out.emplace_back();
        for (const auto& sn : kv.second->nodes)
            out.back().push_back((uint8_t)((sn.isBad() ? KAD_SN_BAD : 0u) | (removable(*sn.node, now) ? KAD_SN_REMOVABLE : 0u)));
    }
    return out;
}

typedef std::vector<std::pair<InfoHash, NodeP>> Pairs;

// The pairs a host owes for the changed nodes: every entry with `candidate` set whose node is one of them.
static void candidate_pairs(const SearchMap& m, const std::vector<NodeP>& changed, Pairs& pairs) {
    std::set<const Node*> in;
    for (const auto& n : changed) in.insert(n.get());
    for (const auto& kv : m)
        for (const auto& sn : kv.second->nodes)
            if (sn.candidate && in.count(sn.node.get())) pairs.push_back(std::make_pair(kv.first, sn.node));
}

// What markNodes returned against the host's own lists: exactly the searches whose flag bytes differ from `before`, in
// map order, each with n, getNumberOfBadNodes(), getNumberOfConsecutiveBadNodes() (dht.cpp:583-597), full and expired.
static size_t check_marked(const char* what, const std::vector<kadgpu::MarkedSearch<InfoHash>>& got, const SearchMap& m,
                           const std::vector<std::vector<uint8_t>>& before, time_point now) {
    const std::vector<std::vector<uint8_t>> after = flags_of(m, now);
    size_t k = 0, s = 0;
    for (const auto& kv : m) {
        const Search& sr = *kv.second;
        if (before[s] != after[s]) {
            EXPECT(k < got.size() && got[k].id == kv.first, "%s: search %zu changed and is not reported in its place", what, s);
            if (k < got.size() && got[k].id == kv.first) {
                size_t bad = 0, lead = 0;
                for (const auto& sn : sr.nodes) bad += sn.isBad();
                while (lead < sr.nodes.size() && sr.nodes[lead].isBad()) lead++;
                const bool full = sr.expired ? sr.nodes.size() >= SEARCH_NODES : sr.nodes.size() - bad >= SEARCH_NODES;
                EXPECT(got[k].n == sr.nodes.size() && got[k].bad == bad && got[k].lead_bad == lead && got[k].full == full &&
                           got[k].expired == sr.expired,
                       "%s: search %zu: counts %u %u %u %d %d, host %zu %zu %zu %d %d", what, s, got[k].n, got[k].bad,
                       got[k].lead_bad, (int)got[k].full, (int)got[k].expired, sr.nodes.size(), bad, lead, (int)full,
                       (int)sr.expired);
            }
            k++;
        }
        s++;
    }
    EXPECT(k == got.size(), "%s: %zu searches reported, %zu changed", what, got.size(), k);
    return k;
}

// The records the fix kernel wrote are those of a fresh snapshot: the same verdicts for candidates on and beside the
// members and for strangers.
static void compare_verdicts(const char* what, const kadgpu::SearchesMirror<SearchMap>& M, const SearchMap& m,
                             time_point now, std::mt19937_64& g) {
    kadgpu::SearchesMirror<SearchMap> F;
    F.snapshot(m, now, 0, M.cap());
    std::vector<InfoHash> cand;
    for (const auto& kv : m) {
        cand.push_back(near_id(g, kv.first, 1 + g() % 4));
        if (!kv.second->nodes.empty()) {
            const InfoHash& member = kv.second->nodes[g() % kv.second->nodes.size()].node->id;
            cand.push_back(member);
            cand.push_back(near_id(g, member, 19));
        }
        cand.push_back(rand_id(g));
    }
    const auto a = M.trySearchInsertBatch(cand.data(), cand.size()), b = F.trySearchInsertBatch(cand.data(), cand.size());
    size_t differ = 0;
    for (size_t i = 0; i < cand.size(); i++)
        differ += a[i].lb != b[i].lb || a[i].fwd != b[i].fwd || a[i].back != b[i].back || a[i].stop != b[i].stop;
    EXPECT(differ == 0, "%s: %zu of %zu verdicts differ from a fresh snapshot's", what, differ, cand.size());
}

// One tick of status changes on the shared nodes: timeouts, replies, candidate flips. Returns what the host reports.
static void tick(SearchMap& m, time_point now, std::mt19937_64& g, std::vector<NodeP>& changed, Pairs& pairs) {
    const std::vector<NodeP> all = nodes_of(m);
    for (size_t i = 0; i < all.size(); i++) {
        const unsigned r = g() % 10;
        if (r == 0 && !all[i]->expired_) {  // a request timed out: setExpired(), time stays
            all[i]->expired_ = true;
            changed.push_back(all[i]);
        } else if (r == 1) {  // a reply: expired_ = false, time = now
            all[i]->expired_ = false;
            all[i]->time = now;
            changed.push_back(all[i]);
        } else if (r == 2) {  // reported twice, although nothing moved
            changed.push_back(all[i]);
            changed.push_back(all[i]);
        }
    }
    for (auto& kv : m)
        for (auto& sn : kv.second->nodes)
            if (g() % 12 == 0) {  // a candidate confirmed (dht.cpp:1038) or a new one (:1109)
                sn.candidate = !sn.candidate;
                pairs.push_back(std::make_pair(kv.first, sn.node));
            }
    candidate_pairs(m, changed, pairs);
}

int main() {
    const time_point now = Clock::now();
    Cache c4 = make_cache(2000, 1, now), c6 = make_cache(300, 2, now);
    SearchMap m4 = make_searches(150, 3, c4, now), m6 = make_searches(40, 4, c6, now), none;
    std::vector<InfoHash> all4, all6;
    for (const auto& kv : m4) all4.push_back(kv.first);
    for (const auto& kv : m6) all6.push_back(kv.first);
    std::mt19937_64 g(17);
    try {
        kadgpu::SearchesMirror<SearchMap> M;
        M.snapshot(m4, now, 0, 32);
        compare_export("snapshot", M.handle(), m4, now);
        EXPECT(M.markNodes(std::vector<NodeP>(), Pairs(), now).empty(), "nothing to mark");

        // tick 1: nodes expire and reply, candidates flip; one markNodes, nothing uploaded
        std::vector<std::vector<uint8_t>> before = flags_of(m4, now);
        std::vector<NodeP> changed;
        Pairs pairs;
        tick(m4, now, g, changed, pairs);
        pairs.push_back(std::make_pair(all4[0], std::make_shared<Node>()));  // not a member: changes nothing
        auto got = M.markNodes(changed, pairs, now);
        const size_t k1 = check_marked("tick 1", got, m4, before, now);
        EXPECT(k1 > 30 && changed.size() > 100 && pairs.size() > 50, "tick 1: %zu searches changed by %zu nodes, %zu pairs",
               k1, changed.size(), pairs.size());
        compare_export("tick 1", M.handle(), m4, now);
        compare_verdicts("tick 1", M, m4, now, g);
        // the same report again changes nothing
        before = flags_of(m4, now);
        got = M.markNodes(changed, pairs, now);
        EXPECT(got.empty() && check_marked("tick 1 again", got, m4, before, now) == 0, "a repeated report changed %zu searches",
               got.size());

        // eleven minutes later: the expired nodes whose ten minutes ran out are reported, and become removable
        const time_point later = now + std::chrono::minutes(11);
        before = flags_of(m4, now);
        changed.clear();
        for (const auto& n : nodes_of(m4))
            if (removable(*n, now) != removable(*n, later)) changed.push_back(n);
        got = M.markNodes(changed, Pairs(), later);
        const size_t k2 = check_marked("tick 2", got, m4, before, later);
        EXPECT(k2 > 20 && !changed.empty(), "tick 2: %zu searches changed by %zu nodes", k2, changed.size());
        compare_export("tick 2", M.handle(), m4, later);
        compare_verdicts("tick 2", M, m4, later, g);

        // insertBatch, then refillBatch, with nothing synced in between: the recorded upload times are still those of the
        // snapshot, and the bits markNodes wrote are what the inserts' removeExpiredNode needs
        std::vector<std::vector<NodeP>> nodes;
        for (size_t i = 0; i < all4.size(); i++) nodes.push_back(make_cands(g, *m4[all4[i]], later, false));
        InsertRound r1;
        std::vector<InfoHash> over = insert_round("insert", m4, all4, nodes, later,
            [&](const std::vector<InfoHash>& v, const std::vector<std::vector<NodeP>>& n) { return M.insertBatch(v, n, later); }, r1);
        EXPECT(r1.inserted > 200 && r1.sent > 100, "insert: %zu inserts, %zu sent", r1.inserted, r1.sent);
        M.sync(over, later);
        compare_export("insert", M.handle(), m4, later);
        kadgpu::NodeCacheMirror<NodeMap> NC;
        NC.snapshot(c4.map, c6.map);
        Round r2;
        over = refill_round("refill", m4, c4.map, all4, later, [&](const std::vector<InfoHash>& v) {
            return M.refillBatch(NC.family(AF_INET), v, later); }, r2);
        EXPECT(r2.inserted > 20, "refill: %zu inserts", r2.inserted);
        M.sync(over, later);
        compare_export("refill", M.handle(), m4, later);

        // a mirror without times takes the bits of the first markNodes; a pair on a search that is not mirrored throws
        bool threw = false;
        try {
            Pairs bad(1, std::make_pair(rand_id(g), nodes_of(m4)[0]));
            M.markNodes(std::vector<NodeP>(), bad, later);
        } catch (const kadgpu::Error& e) {
            threw = e.code() == KAD_ERR_INVALID;
        }
        EXPECT(threw, "a pair on an unknown search did not throw");

        // DhtMirror forwards by family at its clock
        kadgpu::DhtMirror<RoutingTable, Clock, SearchMap> D;
        D.setClock([&] { return now; });
        D.snapshotSearches(none, m6);
        D.syncSearches(AF_INET6, all6, now);
        before = flags_of(m6, now);
        changed.clear();
        pairs.clear();
        tick(m6, now, g, changed, pairs);
        const auto got6 = D.markNodes(AF_INET6, changed, pairs);
        EXPECT(check_marked("dht v6", got6, m6, before, now) > 5, "dht v6: %zu searches changed", got6.size());
        compare_export("dht v6", D.searches(AF_INET6).handle(), m6, now);
        EXPECT(D.markNodes(AF_INET, std::vector<NodeP>(), Pairs()).empty(), "empty family");
        // a family without live searches still hears of every node that timed out or replied
        EXPECT(!changed.empty() && D.markNodes(AF_INET, changed, Pairs()).empty(), "empty family, %zu nodes", changed.size());
        {
            kadgpu::SearchesMirror<SearchMap> E;
            E.snapshot(none, now);
            EXPECT(E.markNodes(changed, Pairs(), now).empty(), "mirror of no searches, %zu nodes", changed.size());
            bool refused = false;
            try {
                E.markNodes(std::vector<NodeP>(), Pairs(1, std::make_pair(all6[0], changed[0])), now);
            } catch (const kadgpu::Error& e) {
                refused = e.code() == KAD_ERR_INVALID;
            }
            EXPECT(refused, "a pair on a mirror of no searches did not throw");
        }
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
