// C++ test of include/kadgpu.hpp's SearchesMirror::trySearchInsertTick and DhtMirror::trySearchInsertTick (a whole tick
// of Dht::trySearchInsert applied on the device, dht.cpp:816-849) over test doubles shaped like OpenDHT's types, as
// tests/cpp/test_sr_insert_shim.cpp. A snapshot; a tick of 500 candidates with repeats and one removable candidate in the
// middle, which must come back LEFT together with everything after it; the caller's replay of the APPLIED candidates in
// (round, position) order, every insertNode checked against the verdict, then the host walk of the LEFT ones; the result
// against a twin map that took Dht::trySearchInsert candidate by candidate, and the device set against the host's lists;
// then trySearchInsertBatch verdicts against the host's own walk. Needs a GPU. Exit 0 = pass.
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

// A tick's candidates over `m`: strangers near a search (a quarter of them expired, none removable), members that are
// not removable, repeats of earlier candidates; at old_at a stranger that expired long ago. The same seed over an equal
// map gives the same tick.
static std::vector<NodeP> make_tick(const SearchMap& m, size_t q, uint64_t seed, time_point now, size_t old_at) {
    std::mt19937_64 g(seed);
    std::vector<const Search*> ss;
    for (const auto& kv : m) ss.push_back(kv.second.get());
    std::vector<NodeP> out;
    while (out.size() < q) {
        const Search& s = *ss[g() % ss.size()];
        const unsigned kind = g() % 8;
        if (out.size() == old_at) {
            auto nd = std::make_shared<Node>();
            nd->id = near_id(g, s.id, 2);
            nd->expired_ = true;
            nd->time = now - std::chrono::seconds(1300);
            out.push_back(nd);
        } else if (kind == 0 && !out.empty()) {
            out.push_back(out[g() % out.size()]);
        } else if (kind == 1 && !s.nodes.empty()) {
            const NodeP& mnode = s.nodes[g() % s.nodes.size()].node;
            if (!removable(*mnode, now)) out.push_back(mnode);
        } else {
            auto nd = std::make_shared<Node>();
            nd->id = near_id(g, s.id, kind < 5 ? 1 + g() % 3 : 0);
            nd->expired_ = g() % 4 == 0;
            nd->time = now - std::chrono::seconds(g() % 500);
            if (nd->id != s.id) out.push_back(nd);
        }
    }
    return out;
}

// Dht::trySearchInsert (dht.cpp:816-849); the probed searches are appended to touched.
static bool try_search_insert(SearchMap& m, const NodeP& n, time_point now, std::vector<InfoHash>* touched) {
    bool inserted = false;
    const auto closest = m.lower_bound(n->id);
    for (auto it = closest; it != m.end(); ++it) {
        if (touched) touched->push_back(it->first);
        if (!it->second->insertNode(n, now)) break;
        inserted = true;
    }
    for (auto it = closest; it != m.begin();) {
        --it;
        if (touched) touched->push_back(it->first);
        if (!it->second->insertNode(n, now)) break;
        inserted = true;
    }
    return inserted;
}

struct Tick {
    size_t applied = 0, skipped = 0, left = 0, inserts = 0, left_before_applied = 0;
};

// The caller's half of a tick: the APPLIED candidates replayed in (round, position) order, every insertNode against the
// verdict; then the LEFT ones walked in order. Returns the searches to report to sync.
static std::vector<InfoHash> replay(const char* what, SearchMap& m, const std::vector<NodeP>& nodes,
                                    const kadgpu::TickResult<InfoHash>& res, time_point now, Tick& st) {
    std::vector<InfoHash> changed(res.overflowed);
    EXPECT(res.verdicts.size() == nodes.size(), "%s: %zu verdicts", what, res.verdicts.size());
    std::vector<size_t> order;
    bool seen_left = false;
    for (size_t j = 0; j < res.verdicts.size(); j++) {
        const uint8_t kind = res.verdicts[j].kind;
        if (kind == KAD_SR_TICK_APPLIED) {
            order.push_back(j);
            st.left_before_applied += seen_left;
        }
        seen_left = seen_left || kind == KAD_SR_TICK_LEFT;
        st.skipped += kind == KAD_SR_TICK_SKIPPED;
        st.left += kind == KAD_SR_TICK_LEFT;
    }
    std::stable_sort(order.begin(), order.end(),
                     [&](size_t a, size_t b) { return res.verdicts[a].round < res.verdicts[b].round; });
    st.applied += order.size();
    for (size_t j : order) {
        const kadgpu::TickVerdict<InfoHash>& v = res.verdicts[j];
        const auto closest = m.lower_bound(nodes[j]->id);
        EXPECT((closest == m.end()) == v.at_end && (v.at_end || closest->first == v.lb_id) &&
               v.lb == (uint32_t)std::distance(m.begin(), closest), "%s: candidate %zu: lower bound", what, j);
        uint32_t f = 0, b = 0;
        auto it = closest;
        for (; it != m.end(); ++it) {
            if (!it->second->insertNode(nodes[j], now)) break;
            f++;
        }
        EXPECT(f == v.fwd && (it == m.end()) == ((v.stop & 15) == KAD_SR_STOP_END),
               "%s: candidate %zu (round %u): %u searches forwards, verdict %u", what, j, v.round, f, v.fwd);
        bool ran_out = true;
        for (it = closest; it != m.begin();) {
            --it;
            if (!it->second->insertNode(nodes[j], now)) {
                ran_out = false;
                break;
            }
            b++;
        }
        EXPECT(b == v.back && ran_out == ((v.stop >> 4) == KAD_SR_STOP_END),
               "%s: candidate %zu (round %u): %u searches backwards, verdict %u", what, j, v.round, b, v.back);
        st.inserts += f + b;
    }
    for (size_t j = 0; j < res.verdicts.size(); j++) {
        if (res.verdicts[j].kind != KAD_SR_TICK_LEFT) continue;
        const bool old = removable(*nodes[j], now);
        if (try_search_insert(m, nodes[j], now, &changed) && old)  // its REMOVABLE bit is gone wherever it is a member
            for (const auto& kv : m)
                for (const auto& sn : kv.second->nodes)
                    if (sn.node == nodes[j]) changed.push_back(kv.first);
    }
    return changed;
}

static void compare_maps(const char* what, const SearchMap& a, const SearchMap& b) {
    EXPECT(a.size() == b.size(), "%s: sizes", what);
    auto ia = a.begin();
    auto ib = b.begin();
    for (size_t s = 0; ia != a.end() && ib != b.end(); ++ia, ++ib, s++) {
        const Search &x = *ia->second, &y = *ib->second;
        bool same = ia->first == ib->first && x.expired == y.expired && x.nodes.size() == y.nodes.size();
        for (size_t j = 0; same && j < x.nodes.size(); j++)
            same = x.nodes[j].node->id == y.nodes[j].node->id && x.nodes[j].isBad() == y.nodes[j].isBad() &&
                   x.nodes[j].node->time == y.nodes[j].node->time;
        EXPECT(same, "%s: search %zu differs from the sequential one (%zu nodes, sequential %zu)", what, s, x.nodes.size(),
               y.nodes.size());
    }
}

// trySearchInsertBatch against the host's own walk: insertNode on a copy of every search the walk reaches
template <class Mirror>
static void compare_verdicts(const char* what, const Mirror& M, const SearchMap& m, const std::vector<InfoHash>& probes,
                             time_point now) {
    const std::vector<kadgpu::SearchInsertVerdict> got = M.trySearchInsertBatch(probes.data(), probes.size());
    for (size_t i = 0; i < probes.size(); i++) {
        auto takes = [&](const Search& s) {
            Search c = s;
            auto nd = std::make_shared<Node>();
            nd->id = probes[i];
            nd->time = now;
            return c.insertNode(nd, now);
        };
        auto refusal = [&](const Search& s) -> uint32_t {
            for (const auto& sn : s.nodes)
                if (sn.node->id == probes[i]) return KAD_SR_STOP_KNOWN;
            return s.expired ? KAD_SR_STOP_FAR_EXPIRED : KAD_SR_STOP_FAR;
        };
        const auto closest = m.lower_bound(probes[i]);
        uint32_t f = 0, b = 0, fs = KAD_SR_STOP_END, bs = KAD_SR_STOP_END;
        for (auto it = closest; it != m.end(); ++it) {
            if (!takes(*it->second)) {
                fs = refusal(*it->second);
                break;
            }
            f++;
        }
        for (auto it = closest; it != m.begin();) {
            --it;
            if (!takes(*it->second)) {
                bs = refusal(*it->second);
                break;
            }
            b++;
        }
        EXPECT(got[i].lb == (uint32_t)std::distance(m.begin(), closest) && got[i].fwd == f && got[i].back == b &&
               got[i].stop == (fs | bs << 4), "%s: probe %zu: got %u +%u -%u %02x, host +%u -%u %02x", what, i, got[i].lb,
               got[i].fwd, got[i].back, got[i].stop, f, b, fs | bs << 4);
    }
}

int main() {
    const time_point now = Clock::now();
    SearchMap m4 = make_searches(150, 3, now), twin4 = make_searches(150, 3, now), m6 = make_searches(40, 4, now),
              twin6 = make_searches(40, 4, now), none;
    const size_t Q = 500, OLD = 250;
    const std::vector<NodeP> c4 = make_tick(m4, Q, 5, now, OLD), t4 = make_tick(twin4, Q, 5, now, OLD);
    const std::vector<NodeP> c6 = make_tick(m6, 200, 6, now, (size_t)-1), t6 = make_tick(twin6, 200, 6, now, (size_t)-1);
    std::vector<InfoHash> probes;
    for (size_t j = 0; j < 200; j++) probes.push_back(c4[j]->id);
    std::mt19937_64 g(13);
    for (size_t j = 0; j < 50; j++) probes.push_back(rand_id(g));
    for (const auto& n : t4) try_search_insert(twin4, n, now, nullptr);
    for (const auto& n : t6) try_search_insert(twin6, n, now, nullptr);
    try {
        kadgpu::SearchesMirror<SearchMap> M;
        M.snapshot(m4, now, 0, 32);
        compare_export("snapshot", M.handle(), m4, now);
        EXPECT(M.trySearchInsertTick(std::vector<NodeP>(), now).verdicts.empty(), "empty tick");
        {  // a tick that starts with a removable candidate: nothing is sent
            const std::vector<NodeP> first(2, c4[OLD]);
            const kadgpu::TickResult<InfoHash> r = M.trySearchInsertTick(first, now);
            EXPECT(r.verdicts.size() == 2 && r.verdicts[0].kind == KAD_SR_TICK_LEFT && r.verdicts[1].kind == KAD_SR_TICK_LEFT &&
                   r.overflowed.empty(), "a removable first candidate");
            compare_export("nothing sent", M.handle(), m4, now);
        }
        // twelve rounds only (half of the searches are short and accept anything, so the candidates' walks meet and a
        // round decides about nine of them): what still waits comes back LEFT among APPLIED ones, and the host walks it
        const kadgpu::TickResult<InfoHash> res = M.trySearchInsertTick(c4, now, 12);
        for (size_t j = OLD; j < res.verdicts.size(); j++)
            EXPECT(res.verdicts[j].kind == KAD_SR_TICK_LEFT, "candidate %zu behind the removable one is not LEFT", j);
        Tick st;
        const std::vector<InfoHash> changed = replay("tick", m4, c4, res, now, st);
        EXPECT(st.applied >= 30 && st.skipped >= 5 && st.left >= Q - OLD && st.inserts >= 30,
               "tick: %zu applied, %zu skipped, %zu left, %zu inserts, %zu applied behind a left one", st.applied, st.skipped,
               st.left, st.inserts, st.left_before_applied);
        std::printf("tick: %zu applied, %zu skipped, %zu left, %zu inserts, %zu applied behind a left one, %zu overflowed\n",
                    st.applied, st.skipped, st.left, st.inserts, st.left_before_applied, res.overflowed.size());
        compare_maps("tick", m4, twin4);
        M.sync(changed, now);
        compare_export("tick", M.handle(), m4, now);
        compare_verdicts("tick", M, m4, probes, now);

        // DhtMirror forwards by family at its clock; a snapshot without a time has no removable bits, so the searches
        // that need them are patched first. No round limit and no removable candidate: nothing is LEFT but for an overflow
        kadgpu::DhtMirror<RoutingTable, Clock, SearchMap> D;
        D.setClock([&] { return now; });
        D.snapshotSearches(none, m6);
        const kadgpu::TickResult<InfoHash> r6 = D.trySearchInsertTick(AF_INET6, c6);
        Tick s6;
        const std::vector<InfoHash> changed6 = replay("dht v6", m6, c6, r6, now, s6);
        EXPECT(s6.applied > 20 && (s6.left == 0 || !r6.overflowed.empty()), "dht v6: %zu applied, %zu left, %zu overflowed",
               s6.applied, s6.left, r6.overflowed.size());
        compare_maps("dht v6", m6, twin6);
        D.syncSearches(AF_INET6, changed6, now);
        compare_export("dht v6", D.searches(AF_INET6).handle(), m6, now);
        const kadgpu::TickResult<InfoHash> r0 = D.trySearchInsertTick(AF_INET, c6);  // a family without searches
        EXPECT(r0.verdicts.size() == c6.size() && r0.verdicts[0].kind == KAD_SR_TICK_SKIPPED && r0.verdicts[0].at_end,
               "empty family");
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
