// C++ test of include/kadgpu.hpp's SearchesMirror::trySearchInsertBatch / sync and DhtMirror's forwarders
// (Dht::trySearchInsert, dht.cpp:816-849) over test doubles shaped like OpenDHT's types, as
// tests/cpp/test_triage_shim.cpp: the batch against the doubles' own insertNode (dht.cpp:961-1047) run on a copy of each
// probed search. 120 searches per family in mixed states (empty, short, full, expired, lists with bad nodes past the
// trim position); after a round of real inserts the changed searches are synced and the batch is checked again.
// Needs a GPU. Exit 0 = pass.
#include <algorithm>
#include <array>
#include <cstdio>
#include <list>
#include <map>
#include <memory>
#include <random>
#include <vector>

#include "kadgpu.hpp"

namespace mock {
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
    bool isExpired() const { return expired_; }
};
struct SearchNode {
    std::shared_ptr<Node> node;
    bool candidate = false;
    bool isBad() const { return !node || node->isExpired() || candidate; }  // dht.cpp:458-460
};
struct Search {
    InfoHash id;
    bool expired = false;
    std::vector<SearchNode> nodes;
    int refusal = 0;  // why the last insertNode refused: KAD_SR_STOP_*

    // Dht::Search::insertNode (dht.cpp:961-1047) with an empty token, one family, one Node per ID; removeExpiredNode is
    // left out (the doubles carry no node times).
    bool insertNode(const std::shared_ptr<Node>& snode) {
        const InfoHash& nid = snode->id;
        bool found = false;
        size_t n = nodes.size();
        while (n != 0) {
            --n;
            if (nodes[n].node->id == nid) {
                found = true;
                break;
            }
            if (id.xorCmp(nid, nodes[n].node->id) > 0) {
                ++n;
                break;
            }
        }
        if (found) {
            refusal = KAD_SR_STOP_KNOWN;
            return false;
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

static InfoHash rand_id(std::mt19937_64& g) {
    InfoHash h;
    for (auto& b : h) b = (uint8_t)g();
    return h;
}

// An ID sharing its first `bytes` bytes with `of`.
static InfoHash near_id(std::mt19937_64& g, const InfoHash& of, size_t bytes) {
    InfoHash h = rand_id(g);
    std::copy(of.begin(), of.begin() + (std::ptrdiff_t)bytes, h.begin());
    return h;
}

static SearchMap make_searches(uint32_t S, uint64_t seed) {
    std::mt19937_64 g(seed);
    SearchMap m;
    while (m.size() < S) {
        auto s = std::make_shared<Search>();
        s->id = rand_id(g);
        const unsigned kind = g() % 5;  // empty, short, full, expired, long with bad nodes
        const size_t n = kind == 0 ? 0 : kind == 1 ? 1 + g() % 13 : kind == 2 ? 14 : kind == 3 ? 14 + g() % 5 : 15 + g() % 16;
        const size_t share = 1 + g() % 12;
        std::vector<InfoHash> ids;
        while (ids.size() < n) {
            const InfoHash h = near_id(g, s->id, share);
            if (h != s->id && std::find(ids.begin(), ids.end(), h) == ids.end()) ids.push_back(h);
        }
        std::sort(ids.begin(), ids.end(), [&](const InfoHash& a, const InfoHash& b) { return s->id.xorCmp(a, b) < 0; });
        for (const auto& h : ids) {
            SearchNode sn;
            sn.node = std::make_shared<Node>();
            sn.node->id = h;
            if (kind == 3) sn.node->expired_ = true;
            if (kind == 4 && g() % 3 == 0) (g() & 1 ? sn.candidate : sn.node->expired_) = true;
            s->nodes.push_back(sn);
        }
        s->expired = kind == 3;
        m[s->id] = s;
    }
    return m;
}

static std::vector<InfoHash> make_cands(const SearchMap& m, uint32_t q, uint64_t seed) {
    std::mt19937_64 g(seed);
    std::vector<std::shared_ptr<Search>> v;
    for (const auto& kv : m) v.push_back(kv.second);
    std::vector<InfoHash> out;
    while (out.size() < q) {
        const auto& s = *v[g() % v.size()];
        switch (g() % 5) {
        case 0: out.push_back(rand_id(g)); break;
        case 1: out.push_back(s.id); break;
        case 2: out.push_back(near_id(g, s.id, 1 + g() % 16)); break;
        case 3: if (!s.nodes.empty()) out.push_back(s.nodes[g() % s.nodes.size()].node->id); break;
        default:
            if (!s.nodes.empty()) {
                InfoHash h = s.nodes[std::min<size_t>(s.nodes.size(), SEARCH_NODES) - 1].node->id;
                h[19] ^= 1;
                out.push_back(h);
            }
        }
    }
    return out;
}

// accept(s, x) by the double's insertNode on a copy: 0xFF if it accepts, else the stop code.
static unsigned probe(const Search& s, const InfoHash& x) {
    Search c = s;
    auto nd = std::make_shared<Node>();
    nd->id = x;
    return c.insertNode(nd) ? 0xFFu : (unsigned)c.refusal;
}

static kadgpu::SearchInsertVerdict want(const SearchMap& m, const InfoHash& x) {
    std::vector<const Search*> v;
    for (const auto& kv : m) v.push_back(kv.second.get());
    const uint32_t lb = (uint32_t)std::distance(m.begin(), m.lower_bound(x));
    uint32_t fwd = 0, back = 0;
    unsigned fs = KAD_SR_STOP_END, bs = KAD_SR_STOP_END;
    for (size_t s = lb; s < v.size(); s++) {
        const unsigned r = probe(*v[s], x);
        if (r != 0xFFu) { fs = r; break; }
        fwd++;
    }
    for (size_t s = lb; s > 0;) {
        const unsigned r = probe(*v[--s], x);
        if (r != 0xFFu) { bs = r; break; }
        back++;
    }
    return kadgpu::SearchInsertVerdict{lb, fwd, back, (uint8_t)(fs | bs << 4)};
}

template <class Batch>
static void compare(const char* what, const SearchMap& m, const std::vector<InfoHash>& cands, Batch batch,
                    unsigned* stops) {
    const std::vector<kadgpu::SearchInsertVerdict> got = batch(cands.data(), cands.size());
    EXPECT(got.size() == cands.size(), "%s: size", what);
    for (size_t i = 0; i < cands.size() && i < got.size(); i++) {
        const kadgpu::SearchInsertVerdict w = want(m, cands[i]);
        EXPECT(got[i].lb == w.lb && got[i].fwd == w.fwd && got[i].back == w.back && got[i].stop == w.stop,
               "%s: candidate %zu: got lb %u fwd %u back %u stop %02x, want lb %u fwd %u back %u stop %02x", what, i,
               got[i].lb, got[i].fwd, got[i].back, got[i].stop, w.lb, w.fwd, w.back, w.stop);
        stops[w.stop & 15]++;
        stops[w.stop >> 4]++;
    }
}

int main() {
    SearchMap m4 = make_searches(120, 1), m6 = make_searches(120, 2), none;
    const std::vector<InfoHash> c4 = make_cands(m4, 1500, 3), c6 = make_cands(m6, 1500, 4);
    unsigned stops[16] = {0};
    try {
        kadgpu::SearchesMirror<SearchMap> M;
        M.snapshot(m4);
        EXPECT(M.size() == 120 && M.cap() >= 32, "snapshot size");
        compare("mirror", m4, c4, [&](const InfoHash* p, size_t q) { return M.trySearchInsertBatch(p, q); }, stops);
        EXPECT(M.trySearchInsertBatch(c4.data(), 0).empty(), "empty batch");
        for (int k = 0; k < 4; k++) EXPECT(stops[k] > 0, "stop code %d never expected", k);

        // the host's inserts: every candidate into the searches its verdict names; each must accept
        const auto got = M.trySearchInsertBatch(c4.data(), 200);
        std::vector<Search*> v;
        for (auto& kv : m4) v.push_back(kv.second.get());
        std::vector<InfoHash> changed;
        std::vector<char> touched(v.size(), 0);
        size_t inserts = 0;
        for (size_t i = 0; i < got.size(); i++) {
            bool clean = true;
            for (uint32_t s = got[i].lb - got[i].back; s < got[i].lb + got[i].fwd; s++) clean = clean && !touched[s];
            if (!clean) continue;  // an earlier candidate of the batch changed one of its searches
            for (uint32_t s = got[i].lb - got[i].back; s < got[i].lb + got[i].fwd; s++) {
                auto nd = std::make_shared<Node>();
                nd->id = c4[i];
                EXPECT(v[s]->insertNode(nd), "search %u refused candidate %zu against its verdict", s, i);
                touched[s] = 1;
                changed.push_back(v[s]->id);
                inserts++;
            }
        }
        EXPECT(inserts > 20, "only %zu inserts", inserts);
        M.sync(changed);
        compare("after sync", m4, c4, [&](const InfoHash* p, size_t q) { return M.trySearchInsertBatch(p, q); }, stops);
        bool threw = false;
        try {
            std::mt19937_64 g(99);
            M.sync(std::vector<InfoHash>(1, rand_id(g)));
        } catch (const kadgpu::Error& e) {
            threw = e.code() == KAD_ERR_INVALID;
        }
        EXPECT(threw, "sync of an unknown search did not throw");

        // a list that outgrows the slabs: the mirror takes a new snapshot by itself
        {
            Search& s = *v[0];
            std::mt19937_64 g(5);
            s.nodes.clear();
            s.expired = false;
            std::vector<InfoHash> ids;
            while (ids.size() < 40) ids.push_back(near_id(g, s.id, 2));
            std::sort(ids.begin(), ids.end(), [&](const InfoHash& a, const InfoHash& b) { return s.id.xorCmp(a, b) < 0; });
            for (const auto& h : ids) {
                SearchNode sn;
                sn.node = std::make_shared<Node>();
                sn.node->id = h;
                sn.candidate = true;
                s.nodes.push_back(sn);
            }
            M.sync(std::vector<InfoHash>(1, s.id));
            EXPECT(M.cap() >= 40, "cap %u after a list of 40", M.cap());
            compare("after growth", m4, c4, [&](const InfoHash* p, size_t q) { return M.trySearchInsertBatch(p, q); },
                    stops);
        }

        // DhtMirror forwards by family; an empty family answers zeros
        kadgpu::DhtMirror<RoutingTable, std::chrono::steady_clock, SearchMap> D;
        D.snapshotSearches(m4, m6);
        compare("dht v4", m4, c4, [&](const InfoHash* p, size_t q) { return D.trySearchInsertBatch(p, q, AF_INET); }, stops);
        compare("dht v6", m6, c6, [&](const InfoHash* p, size_t q) { return D.trySearchInsertBatch(p, q, AF_INET6); }, stops);
        D.snapshotSearches(none, m6);
        for (const auto& r : D.trySearchInsertBatch(c4.data(), 50, AF_INET))
            EXPECT(r.lb == 0 && r.fwd == 0 && r.back == 0 && r.stop == 0, "empty family");
        D.syncSearches(AF_INET6, std::vector<InfoHash>(1, m6.begin()->first));
        compare("dht v6 synced", m6, c6, [&](const InfoHash* p, size_t q) { return D.trySearchInsertBatch(p, q, AF_INET6); },
                stops);
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
