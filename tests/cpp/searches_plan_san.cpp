// The host plan of a device search set (opendht_amd/csrc/kad_searches_plan.cpp) under AddressSanitizer and
// UndefinedBehaviorSanitizer: a stand-alone program, compiled together with the plan file by
// tests/test_searches_san.py. CSR-to-slab planning and the trim over empty lists, n == cap, S == 0 and rejected inputs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/kadgpu.h"
#include "../../opendht_amd/csrc/kad_searches_plan.h"

namespace {

int failures = 0;
#define EXPECT(c)                                                    \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                              \
        }                                                            \
    } while (0)

typedef std::vector<uint8_t> Id;

Id rand_id(std::mt19937_64& g) {
    Id v(20);
    for (auto& b : v) b = (uint8_t)g();
    return v;
}

bool closer(const Id& self, const Id& a, const Id& b) {
    for (int i = 0; i < 20; i++) {
        const uint8_t x = a[i] ^ self[i], y = b[i] ^ self[i];
        if (x != y) return x < y;
    }
    return false;
}

struct Set {
    std::vector<uint8_t> ids, flags, nid, nfl;
    std::vector<uint32_t> off{0};
};

// S searches with the given list lengths, valid.
Set make(std::mt19937_64& g, const std::vector<uint32_t>& n) {
    Set s;
    std::vector<Id> sid(n.size());
    for (auto& v : sid) v = rand_id(g);
    std::sort(sid.begin(), sid.end());
    for (size_t i = 0; i < n.size(); i++) {
        s.ids.insert(s.ids.end(), sid[i].begin(), sid[i].end());
        s.flags.push_back((g() & 3) == 0 ? KAD_SR_EXPIRED : 0);
        std::vector<Id> l(n[i]);
        for (auto& v : l) v = rand_id(g);
        std::sort(l.begin(), l.end(), [&](const Id& a, const Id& b) { return closer(sid[i], a, b); });
        for (auto& v : l) {
            s.nid.insert(s.nid.end(), v.begin(), v.end());
            s.nfl.push_back((g() & 1) ? KAD_SN_BAD : 0);
        }
        s.off.push_back(s.off.back() + n[i]);
    }
    return s;
}

int plan(const Set& s, uint32_t cap, kadplan::SearchesPlan& p) {
    std::string err;
    const uint32_t S = (uint32_t)s.flags.size();
    int rc = kadplan::searches_check_ids(S, s.ids.data(), err);
    if (rc) return rc;
    return kadplan::searches_plan(S, cap, s.ids.data(), s.flags.data(), s.off.data(), s.nid.data(), s.nfl.data(), p, err);
}

}  // namespace

int main() {
    std::mt19937_64 g(7);
    // the trim: empty list, NULL flags, short and long lists of every kind
    {
        uint32_t full = 9, t = 9;
        EXPECT(kad_search_trim(0, nullptr, 0, &full, &t) == KAD_OK && full == 0 && t == 0);
        EXPECT(kad_search_trim(0, nullptr, KAD_SR_EXPIRED, &full, &t) == KAD_OK && full == 0 && t == 0);
        EXPECT(kad_search_trim(1, nullptr, 0, &full, &t) == KAD_ERR_INVALID);
        EXPECT(kad_search_trim(0, nullptr, 0, nullptr, &t) == KAD_ERR_INVALID);
        for (uint32_t n = 0; n <= 64; n++)
            for (int rep = 0; rep < 20; rep++) {
                std::vector<uint8_t> fl(n);  // exactly n bytes: a read past the list is caught
                for (auto& f : fl) f = (g() % 3 == 0) ? KAD_SN_BAD : 0;
                for (uint32_t sf : {0u, (uint32_t)KAD_SR_EXPIRED}) {
                    EXPECT(kad_search_trim(n, n ? fl.data() : nullptr, sf, &full, &t) == KAD_OK);
                    EXPECT(t <= n && full <= 1);
                    uint32_t good = 0;
                    for (uint32_t i = 0; i < t; i++) good += !(fl[i] & KAD_SN_BAD);
                    if (sf) {
                        EXPECT(full == (n >= 14) && t == (n >= 14 ? 14 : n));
                    } else {
                        EXPECT(good <= 14 && (t == n || good == 14));
                    }
                }
            }
    }
    // S == 0
    {
        Set s;
        kadplan::SearchesPlan p;
        std::string err;
        EXPECT(kadplan::searches_check_ids(0, nullptr, err) == KAD_OK);
        EXPECT(kadplan::searches_plan(0, 14, nullptr, nullptr, s.off.data(), nullptr, nullptr, p, err) == KAD_OK);
        EXPECT(p.rec.empty() && p.mkey.empty() && p.mtail.empty() && p.mflag.empty());
    }
    // every list empty (node arrays of size 0), lists of exactly cap entries, mixed lengths
    for (uint32_t cap : {14u, 15u, 40u}) {
        for (int kind = 0; kind < 3; kind++) {
            std::vector<uint32_t> n(37);
            for (auto& v : n) v = kind == 0 ? 0 : kind == 1 ? cap : (uint32_t)(g() % (cap + 1));
            const Set s = make(g, n);
            kadplan::SearchesPlan p;
            EXPECT(plan(s, cap, p) == KAD_OK);
            EXPECT(p.rec.size() == n.size() * kadplan::SREC_WORDS && p.mkey.size() == n.size() * cap &&
                   p.mtail.size() == 3 * n.size() * cap && p.mflag.size() == n.size() * cap);
            for (size_t i = 0; i < n.size(); i++) {
                const uint32_t* r = p.rec.data() + i * kadplan::SREC_WORDS;
                uint32_t full, t;
                kad_search_trim(n[i], n[i] ? s.nfl.data() + s.off[i] : nullptr, s.flags[i], &full, &t);
                EXPECT(r[kadplan::SREC_N] == n[i] && r[kadplan::SREC_T] == t);
                EXPECT((r[kadplan::SREC_BITS] & kadplan::SREC_FULL) == full);
                EXPECT(((r[kadplan::SREC_BITS] & kadplan::SREC_EXPIRED) != 0) == (s.flags[i] != 0));
                for (uint32_t j = 0; j < n[i]; j++) EXPECT(p.mflag[i * cap + j] == s.nfl[s.off[i] + j]);
                for (uint32_t j = n[i]; j < cap; j++) EXPECT(p.mkey[i * cap + j] == 0 && p.mflag[i * cap + j] == 0);
            }
        }
    }
    // rejected inputs: equal and descending search IDs, an unsorted list, a duplicate node, offsets going back, a
    // list over cap (after the order checks)
    {
        const Set ok = make(g, {3, 0, 16, 5});
        kadplan::SearchesPlan p;
        EXPECT(plan(ok, 16, p) == KAD_OK);
        EXPECT(plan(ok, 15, p) == KAD_ERR_UNSUPPORTED);
        Set s = ok;
        std::memcpy(&s.ids[20], &s.ids[0], 20);
        EXPECT(plan(s, 16, p) == KAD_ERR_INVALID);
        s = ok;
        std::swap_ranges(s.ids.begin(), s.ids.begin() + 20, s.ids.begin() + 40);
        EXPECT(plan(s, 16, p) == KAD_ERR_INVALID);
        s = ok;
        std::swap_ranges(s.nid.begin(), s.nid.begin() + 20, s.nid.begin() + 20);
        EXPECT(plan(s, 15, p) == KAD_ERR_INVALID);  // before the length check
        s = ok;
        std::memcpy(&s.nid[20 * 4], &s.nid[20 * 3], 20);
        EXPECT(plan(s, 16, p) == KAD_ERR_INVALID);
        s = ok;
        s.off[2] = 1;
        EXPECT(plan(s, 16, p) == KAD_ERR_INVALID);
    }
    if (failures) return 1;
    std::printf("PASS\n");
    return 0;
}
