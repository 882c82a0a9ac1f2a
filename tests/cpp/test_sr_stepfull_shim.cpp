// C++ test of include/kadgpu.hpp's SearchesMirror::markDue / stepBatchFull and DhtMirror::markSearchDue /
// stepSearchesFull (the whole Dht::searchStep on the device set) over test doubles shaped like OpenDHT's
// types. The doubles keep what the reference keeps in getStatus, listenStatus, acked and probe_query as fields per search
// node and per search (listeners, announces, whether the probe query satisfies the get query) and run their own three
// send loops entry by entry. After a snapshot the step bits go up with markEntries and the due bits with markDue; a step
// in verdict mode and two with KAD_STEP_APPLY are compared search by search with the doubles' searchStep, which is then
// replayed on the host; the device set is exported and compared with the host's lists byte for byte; replies, acks and
// expired listens go up with markEntries and markDue in between. Needs a GPU. Exit 0 = pass.
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <list>
#include <map>
#include <memory>
#include <random>
#include <utility>
#include <vector>

#include "kadgpu.hpp"

namespace mock {
using Clock = std::chrono::steady_clock;
using time_point = Clock::time_point;
constexpr size_t SEARCH_NODES = 14, TARGET_NODES = 8, LISTEN_NODES = 4, MAX_REQUESTED_SEARCH_NODES = 4, SEARCH_MAX_BAD_NODES = 25;
struct InfoHash : std::array<uint8_t, 20> {
    int xorCmp(const InfoHash& a, const InfoHash& b) const {
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
struct SearchNode {
    std::shared_ptr<Node> node;
    bool candidate = false;
    bool in_flight = false;      // a get request of the search's own query is pending in getStatus, dht.cpp:392-397
    bool replied = false;        // last_get_reply within NODE_EXPIRE_TIME, :279-282
    bool refused = false;        // canGet's getStatus and pagination clauses say no, :306-323
    bool listenStatus = false;   // a listen request is pending or was answered less than LISTEN_EXPIRE_TIME ago, :447-453
    bool acked = false;          // acked[vid] holds a request that is pending or still fresh, :431-441
    bool probe_query = false;    // getStatus[probe_query] is pending: getAnnounceTime is max
    bool isBad() const { return !node || node->isExpired() || candidate; }  // :458-460
    bool isSynced() const { return !node->isExpired() && replied; }         // :279-282
    bool pending() const { return in_flight || probe_query; }               // :392-397 over every query
    // :302-324; blocks: the probe query satisfies the search's get query (pending_sq_status)
    bool canGet(bool blocks) const { return !node->isExpired() && !refused && !(blocks && probe_query); }
};
struct Step {
    std::vector<std::shared_ptr<Node>> sent, listened, probed;
    size_t n = 0, bad = 0, lead_bad = 0, solicited = 0;
    bool skipped = false, is_short = false, synced = false, done = false, exhausted = false, expire = false;
};
struct Search {
    InfoHash id;
    bool expired = false;
    bool listeners = false, announce = false, probe_blocks = false;  // the two containers' emptiness; the queries' relation
    std::vector<SearchNode> nodes;
    bool listenDue(const SearchNode& n) const { return listeners && !n.listenStatus; }               // getListenTime <= now
    bool announceDue(const SearchNode& n) const { return announce && !n.acked && !n.probe_query; }   // getAnnounceTime <= now
    uint8_t mode() const {
        return (uint8_t)((listeners ? KAD_STEP_LISTEN : 0u) | (announce ? KAD_STEP_ANNOUNCE : 0u) |
                         (announce && probe_blocks ? KAD_STEP_PROBE_BLOCKS : 0u));
    }

    size_t solicited() const {  // currentlySolicitedNodeCount, :514-520
        size_t c = 0;
        for (const auto& n : nodes) c += !n.isBad() && n.pending();
        return c;
    }
    bool isSynced() const {  // :1467-1478
        unsigned i = 0;
        for (const auto& n : nodes) {
            if (n.isBad()) continue;
            if (!n.isSynced()) return false;
            if (++i == TARGET_NODES) break;
        }
        return i > 0;
    }
    void expire() {  // :649-653
        expired = true;
        nodes.clear();
    }
    // Dht::searchStep (:1344-1464) without the network: the nodes a get request goes to, in order, and what it found.
    // `apply` makes the sends and the expiry take effect on this search.
    Step searchStep(bool done_if_synced, bool no_send, bool apply) {
        Step st;
        Search work = *this;
        st.n = nodes.size();
        for (const auto& n : nodes) st.bad += n.isBad();
        while (st.lead_bad < nodes.size() && nodes[st.lead_bad].isBad()) st.lead_bad++;
        st.solicited = solicited();
        if (expired) {
            st.skipped = true;
            return st;
        }
        st.is_short = nodes.size() - st.bad < SEARCH_NODES;
        st.synced = isSynced();
        if (st.synced) {
            if (listeners) {  // :1384-1428
                unsigned i = 0;
                for (auto& sn : work.nodes) {
                    if (!sn.isSynced()) continue;
                    if (listenDue(sn)) {
                        st.listened.push_back(sn.node);
                        sn.listenStatus = true;
                    }
                    if (!sn.candidate && ++i == LISTEN_NODES) break;
                }
            }
            if (announce) {  // searchSendAnnounceValue, :1237-1339
                unsigned i = 0;
                for (auto& sn : work.nodes) {
                    if (!(sn.isSynced() && announceDue(sn))) continue;
                    st.probed.push_back(sn.node);
                    sn.probe_query = true;
                    if (!sn.candidate && ++i == TARGET_NODES) break;
                }
            }
        }
        st.done = st.synced && done_if_synced;
        if (work.solicited() < MAX_REQUESTED_SEARCH_NODES && !no_send) {
            SearchNode* sent;
            do {
                sent = nullptr;
                if (!st.done && work.solicited() < MAX_REQUESTED_SEARCH_NODES) {  // searchSendGetValues, :1173
                    for (auto& sn : work.nodes)
                        if (sn.canGet(announce && probe_blocks)) {
                            sent = &sn;
                            break;
                        }
                    if (!sent) st.exhausted = true;
                }
                if (sent) {
                    sent->in_flight = sent->refused = true;  // getStatus[query] = the request
                    st.sent.push_back(sent->node);
                }
            } while (sent && work.solicited() < MAX_REQUESTED_SEARCH_NODES);
        }
        st.solicited = work.solicited();
        st.expire = st.lead_bad >= std::min(nodes.size(), SEARCH_MAX_BAD_NODES);
        if (apply) {
            *this = work;
            if (st.expire) expire();
        }
        return st;
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

static uint8_t step_bits(const Search& sr, const SearchNode& sn) {
    // an expired candidate cannot be asked: NOGET says what BAD no longer does (kadgpu.h)
    const bool noget = sn.refused || (sn.candidate && sn.node->isExpired()) || (sr.announce && sr.probe_blocks && sn.probe_query);
    return (uint8_t)((sn.candidate ? KAD_SN_CANDIDATE : 0u) | (sn.pending() ? KAD_SN_PENDING : 0u) |
                     (sn.isSynced() ? KAD_SN_SYNCED : 0u) | (noget ? KAD_SN_NOGET : 0u));
}

static uint8_t due_bits(const Search& sr, const SearchNode& sn) {
    return (uint8_t)((sr.listenDue(sn) ? KAD_SN_LISTEN_DUE : 0u) | (sr.announceDue(sn) ? KAD_SN_ANNOUNCE_DUE : 0u));
}

// kind: 0 empty, 1 fresh nodes, 2 synced, 3 mostly bad from the front, 4 requests in flight, 5 long and mixed, 6 expired
static SearchMap make_searches(uint32_t S, uint64_t seed, time_point now) {
    std::mt19937_64 g(seed);
    SearchMap m;
    while (m.size() < S) {
        auto s = std::make_shared<Search>();
        s->id = rand_id(g);
        const unsigned kind = (unsigned)(m.size() % 7);
        const size_t n = kind == 0 ? 0 : kind == 5 ? 20 + g() % 30 : kind == 3 ? 1 + g() % 30 : 1 + g() % 20;
        std::vector<NodeP> picked;
        while (picked.size() < n) {
            auto nd = std::make_shared<Node>();
            nd->id = rand_id(g);
            nd->id[0] = s->id[0];
            nd->time = now;
            if (nd->id != s->id && std::none_of(picked.begin(), picked.end(), [&](const NodeP& p) { return p->id == nd->id; }))
                picked.push_back(nd);
        }
        std::sort(picked.begin(), picked.end(), [&](const NodeP& a, const NodeP& b) { return s->id.xorCmp(a->id, b->id) < 0; });
        const size_t bad_front = kind == 3 ? g() % (n + 1) : 0;
        for (size_t e = 0; e < picked.size(); e++) {
            SearchNode sn;
            sn.node = picked[e];
            const unsigned r = (unsigned)(g() % 10);
            if (e < bad_front || (kind == 5 && r == 0)) (g() & 1 ? sn.candidate : sn.node->expired_) = true;
            if (kind == 5 && r == 1) sn.candidate = sn.node->expired_ = true;
            if (kind == 2 || (kind == 5 && r < 5)) sn.replied = sn.refused = true;
            if (kind == 2 && r == 9 && (m.size() / 7) % 2) sn.replied = false;
            if (kind == 2 && r == 8) sn.refused = false;  // synced and still something to get from it
            if (kind == 2 && r < 2) sn.candidate = true;  // a synced candidate: picked by both loops, counted by neither
            sn.listenStatus = g() % 3 == 0;
            sn.acked = g() % 4 == 0;
            if (kind == 4 && r < 6) sn.in_flight = sn.refused = true;
            if (kind == 5 && r == 6) sn.in_flight = true;  // a request for another query
            s->nodes.push_back(sn);
        }
        s->expired = kind == 6;
        const unsigned role = (unsigned)((m.size() / 7) % 5);  // kind 2 (synced) meets every role
        s->listeners = role <= 2;
        s->announce = role >= 2 && role <= 3;
        s->probe_blocks = (m.size() / 35) % 2 == 1;
        m[s->id] = s;
    }
    return m;
}

// The device set against the host's searches: n, IDs and every flag byte, step bits included.
static void compare_export(const char* what, const kad_searches* ss, const SearchMap& m) {
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
            const uint8_t fl = (uint8_t)((sr.nodes[j].isBad() ? KAD_SN_BAD : 0u) | step_bits(sr, sr.nodes[j]) | due_bits(sr, sr.nodes[j]));
            same = std::equal(sr.nodes[j].node->id.begin(), sr.nodes[j].node->id.end(), &nid[e * 20]) && nfl[e] == fl;
        }
        for (size_t j = sr.nodes.size(); same && j < cap; j++) same = nfl[(size_t)s * cap + j] == 0;
        EXPECT(same, "%s: search %u differs from the host's (n %u, host %zu)", what, s, n[s], sr.nodes.size());
        s++;
    }
}

struct Seen {
    size_t sent = 0, synced = 0, done = 0, exhausted = 0, expire = 0, skipped = 0, is_short = 0, more_than_four = 0;
    size_t listened = 0, probed = 0, closed = 0, nine = 0;
};

template <class Stepped>
static void compare_step(const char* what, const Stepped& got, const Step& want, uint8_t mode, Seen& seen) {
    const uint32_t bits = (want.skipped ? KAD_STEP_SKIPPED : 0u) | (want.is_short ? KAD_STEP_SHORT : 0u) |
                          (want.synced ? KAD_STEP_SYNCED : 0u) | (want.done ? KAD_STEP_DONE : 0u) |
                          (want.exhausted ? KAD_STEP_EXHAUSTED : 0u) | (want.expire ? KAD_STEP_EXPIRE : 0u);
    EXPECT(got.bits == bits, "%s: bits %02x, host %02x (mode %02x)", what, got.bits, bits, mode);
    EXPECT(got.picks == want.sent, "%s: %zu picks, host %zu", what, got.picks.size(), want.sent.size());
    EXPECT(got.listen == want.listened, "%s: %zu listens, host %zu", what, got.listen.size(), want.listened.size());
    EXPECT(got.announce == want.probed, "%s: %zu probes, host %zu", what, got.announce.size(), want.probed.size());
    seen.listened += want.listened.size();
    seen.probed += want.probed.size();
    seen.closed += !want.probed.empty() && want.sent.empty() && want.solicited >= 4;
    seen.nine += want.probed.size() > 8 || want.listened.size() > 4;
    EXPECT(got.n == want.n && got.bad == want.bad && got.lead_bad == want.lead_bad && got.solicited == want.solicited,
           "%s: counts %u %u %u %u, host %zu %zu %zu %zu", what, got.n, got.bad, got.lead_bad, got.solicited, want.n, want.bad,
           want.lead_bad, want.solicited);
    seen.sent += want.sent.size();
    seen.synced += want.synced;
    seen.done += want.done;
    seen.exhausted += want.exhausted;
    seen.expire += want.expire;
    seen.skipped += want.skipped;
    seen.is_short += want.is_short;
    seen.more_than_four += want.sent.size() > 4;
}

int main() {
    const time_point now = Clock::now();
    std::mt19937_64 g(99);
    SearchMap m4 = make_searches(140, 1, now), m6 = make_searches(9, 2, now);
    Seen seen;
    try {
        kadgpu::DhtMirror<RoutingTable, Clock, SearchMap> dht;
        dht.setClock([now] { return now; });
        dht.snapshotSearches(m4, m6, 0);
        for (SearchMap* m : {&m4, &m6}) {
            const sa_family_t af = m == &m4 ? AF_INET : AF_INET6;
            const kad_searches* ss = dht.searches(af).handle();
            // the step bits of every entry that carries any; one pair twice, one node its search does not hold
            std::vector<std::pair<InfoHash, NodeP>> pairs;
            for (const auto& kv : *m)
                for (const auto& sn : kv.second->nodes)
                    if (step_bits(*kv.second, sn)) pairs.push_back(std::make_pair(kv.first, sn.node));
            const size_t real = pairs.size();
            pairs.push_back(pairs.front());
            auto stranger = std::make_shared<Node>();
            stranger->id = rand_id(g);
            pairs.push_back(std::make_pair(m->begin()->first, stranger));
            const std::vector<uint8_t> found = dht.markSearchEntries(af, pairs, step_bits);
            EXPECT(found.size() == pairs.size() && found.back() == 0 && found[real] == 1, "markEntries: found bytes");
            EXPECT(std::count(found.begin(), found.end(), (uint8_t)1) == (std::ptrdiff_t)real + 1, "markEntries: found count");
            // the due bits likewise, with the same repeat and the same stranger
            std::vector<std::pair<InfoHash, NodeP>> dues;
            for (const auto& kv : *m)
                for (const auto& sn : kv.second->nodes)
                    if (due_bits(*kv.second, sn)) dues.push_back(std::make_pair(kv.first, sn.node));
            const size_t real_due = dues.size();
            EXPECT(real_due > 0, "some entry is due");
            dues.push_back(dues.front());
            dues.push_back(pairs.back());
            const std::vector<uint8_t> dfound = dht.markSearchDue(af, dues, due_bits);
            EXPECT(dfound.size() == dues.size() && dfound.back() == 0 && dfound[real_due] == 1, "markDue: found bytes");
            EXPECT(std::count(dfound.begin(), dfound.end(), (uint8_t)1) == (std::ptrdiff_t)real_due + 1, "markDue: found count");
            compare_export("after markEntries and markDue", ss, *m);

            std::vector<InfoHash> ids;
            for (const auto& kv : *m) ids.push_back(kv.first);
            std::shuffle(ids.begin(), ids.end(), g);
            std::vector<uint8_t> modes(ids.size());
            for (size_t k = 0; k < ids.size(); k++) {
                const Search& sr = *(*m)[ids[k]];
                modes[k] = (uint8_t)(sr.mode() | (g() % 9 == 0 ? KAD_STEP_NO_SEND : 0u));
                // a search without listeners and announces, every other one of them without callbacks either
                if (!sr.mode() && (k % 2 == 0 || g() % 4 == 0)) modes[k] |= KAD_STEP_DONE_IF_SYNCED;
            }
            // verdict mode: the host's own step, nothing applied anywhere
            auto got = dht.stepSearchesFull(af, ids, modes);
            EXPECT(got.size() == ids.size(), "verdict: size");
            for (size_t k = 0; k < ids.size() && k < got.size(); k++) {
                EXPECT(got[k].id == ids[k], "verdict: order");
                compare_step("verdict", got[k], (*m)[ids[k]]->searchStep(modes[k] & KAD_STEP_DONE_IF_SYNCED, modes[k] & KAD_STEP_NO_SEND, false),
                             modes[k], seen);
            }
            compare_export("after the verdicts", ss, *m);
            // applied, twice; replies, acks, timeouts and expired listens in between
            for (int round = 0; round < 2; round++) {
                std::vector<uint8_t> am(modes);
                for (auto& md : am) md |= KAD_STEP_APPLY;
                got = dht.searches(af).stepBatchFull(ids, am);
                std::vector<std::pair<InfoHash, NodeP>> ends, due_ends;
                for (size_t k = 0; k < ids.size() && k < got.size(); k++) {
                    Search& sr = *(*m)[ids[k]];
                    const Step want = sr.searchStep(modes[k] & KAD_STEP_DONE_IF_SYNCED, modes[k] & KAD_STEP_NO_SEND, true);
                    compare_step(round ? "applied again" : "applied", got[k], want, am[k], seen);
                    for (auto& sn : sr.nodes) {
                        bool step_change = false, due_change = false;
                        if (sn.in_flight && g() % 3) {  // a get ends: a reply, or a timeout that allows a retry
                            sn.in_flight = false;
                            if (g() & 1) sn.replied = true; else sn.refused = false;
                            step_change = true;
                        }
                        if (sn.probe_query && g() % 3) {  // a probe ends: the put it triggers is acked, or it timed out
                            sn.probe_query = false;
                            sn.acked = g() % 3 != 0;
                            step_change = due_change = true;
                        }
                        if (sn.listenStatus && g() % 5 == 0) {  // a listen expired: due again
                            sn.listenStatus = false;
                            due_change = true;
                        }
                        if (step_change) ends.push_back(std::make_pair(ids[k], sn.node));
                        if (due_change) due_ends.push_back(std::make_pair(ids[k], sn.node));
                    }
                }
                // the ends are on the host only: the device still holds the requests as in flight
                const std::vector<uint8_t> f = dht.searches(af).markEntries(ends, step_bits);
                EXPECT(std::count(f.begin(), f.end(), (uint8_t)1) == (std::ptrdiff_t)ends.size(), "ends: all found");
                const std::vector<uint8_t> fd = dht.searches(af).markDue(due_ends, due_bits);
                EXPECT(std::count(fd.begin(), fd.end(), (uint8_t)1) == (std::ptrdiff_t)due_ends.size(), "due ends: all found");
                compare_export(round ? "after the second round" : "after the first round", ss, *m);
            }
            bool threw = false;
            try {
                std::vector<InfoHash> twice(2, ids[0]);
                dht.searches(af).stepBatchFull(twice);
            } catch (const kadgpu::Error&) {
                threw = true;
            }
            EXPECT(threw, "a search listed twice is refused");
            threw = false;
            try {  // DONE_IF_SYNCED says "no listeners": the engine refuses the pair
                dht.searches(af).stepBatchFull(std::vector<InfoHash>(1, ids[0]),
                                               std::vector<uint8_t>(1, (uint8_t)(KAD_STEP_DONE_IF_SYNCED | KAD_STEP_LISTEN)));
            } catch (const kadgpu::Error&) {
                threw = true;
            }
            EXPECT(threw, "an invalid mode is refused");
            EXPECT(dht.searches(af).stepBatchFull(std::vector<InfoHash>()).empty(), "no searches, no answer");
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    EXPECT(seen.sent && seen.synced && seen.done && seen.exhausted && seen.expire && seen.skipped && seen.is_short &&
               seen.listened && seen.probed && seen.closed && seen.nine,
           "mechanisms: sent %zu synced %zu done %zu exhausted %zu expire %zu skipped %zu short %zu listened %zu probed %zu "
           "closed %zu past the count %zu", seen.sent, seen.synced, seen.done, seen.exhausted, seen.expire, seen.skipped,
           seen.is_short, seen.listened, seen.probed, seen.closed, seen.nine);
    if (fails) {
        std::fprintf(stderr, "%d failures\n", fails);
        return 1;
    }
    std::printf("PASS sent %zu, listened %zu, probed %zu, synced %zu, done %zu, exhausted %zu, expired %zu\n", seen.sent,
                seen.listened, seen.probed, seen.synced, seen.done, seen.exhausted, seen.expire);
    return 0;
}
