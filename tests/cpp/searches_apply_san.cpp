// The host plan of kad_searches_apply (kadplan::searches_apply_plan, opendht_amd/csrc/kad_searches_plan.cpp) under
// AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, compiled together with the plan file by
// tests/test_searches_apply_san.py. Every plan is compared with a brute-force merge written here: sets of 0 to a few
// hundred searches; erase none, all, the first, the last, runs; inserts before, after and between; erased and
// re-inserted IDs; IDs that share their top 64 bits (and all but the last byte) with a neighbour; rejected inputs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
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

std::vector<uint8_t> flat(const std::vector<Id>& v) {
    std::vector<uint8_t> out;
    for (const auto& id : v) out.insert(out.end(), id.begin(), id.end());
    return out;
}

// S distinct ascending IDs: random ones and runs that differ from their neighbour in the last byte only
std::vector<Id> make_ids(std::mt19937_64& g, size_t S) {
    std::vector<Id> out;
    while (out.size() < S) {
        Id v = rand_id(g);
        v[19] &= 0xF0;
        const size_t run = (g() & 3) ? 1 : 1 + g() % 5;
        for (size_t k = 0; k < run && out.size() < S; k++) {
            v[19] = (uint8_t)((v[19] & 0xF0) | (2 * k));  // even last nibble: the odd ones stay free for inserts
            out.push_back(v);
        }
    }
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
    return out;
}

int run_plan(const std::vector<Id>& ids, const std::vector<uint32_t>& erase, const std::vector<Id>& ins,
             kadplan::SearchesApplyPlan& p, std::string* msg = nullptr) {
    // exact-size copies: a read past any input is an AddressSanitizer report
    const std::vector<uint8_t> a = flat(ids), b = flat(ins);
    const std::vector<uint32_t> e(erase);
    std::string err;
    const int rc = kadplan::searches_apply_plan((uint32_t)ids.size(), a.data(), e.data(), (uint32_t)e.size(), b.data(),
                                                (uint32_t)ins.size(), p, err);
    if (msg) *msg = err;
    EXPECT((rc == KAD_OK) == err.empty());
    return rc;
}

// the merge by brute force: a std::map of ID -> source word
void check(const std::vector<Id>& ids, const std::vector<uint32_t>& erase, const std::vector<Id>& ins) {
    kadplan::SearchesApplyPlan p;
    EXPECT(run_plan(ids, erase, ins, p) == KAD_OK);
    std::map<Id, uint32_t> m;
    for (uint32_t s = 0; s < ids.size(); s++)
        if (!std::binary_search(erase.begin(), erase.end(), s)) m[ids[s]] = s;
    for (uint32_t j = 0; j < ins.size(); j++) {
        EXPECT(!m.count(ins[j]));
        m[ins[j]] = kadplan::SRC_NEW | j;
    }
    EXPECT(p.src.size() == m.size() && p.ids.size() == 20 * m.size());
    EXPECT(p.remap.size() == ids.size() && p.new_index.size() == ins.size());
    if (failures) return;
    std::vector<uint32_t> remap(ids.size(), KAD_NO_NODE), new_index(ins.size(), KAD_NO_NODE);
    uint32_t at = 0;
    for (const auto& kv : m) {
        EXPECT(p.src[at] == kv.second);
        EXPECT(std::memcmp(&p.ids[20 * (size_t)at], kv.first.data(), 20) == 0);
        if (kv.second & kadplan::SRC_NEW)
            new_index[kv.second & ~kadplan::SRC_NEW] = at;
        else
            remap[kv.second] = at;
        at++;
    }
    EXPECT(remap == p.remap);
    EXPECT(new_index == p.new_index);
}

Id bump(Id v, int by) {  // the neighbour in the last byte
    v[19] = (uint8_t)(v[19] + by);
    return v;
}

}  // namespace

int main() {
    std::mt19937_64 g(12345);
    // the empty set and tiny ones
    check({}, {}, {});
    check({}, {}, {rand_id(g)});
    check({}, {}, {rand_id(g), rand_id(g), rand_id(g)});
    for (size_t S : {1u, 2u, 3u, 14u, 63u, 64u, 65u, 300u}) {
        const std::vector<Id> ids = make_ids(g, S);
        const uint32_t n = (uint32_t)ids.size();
        std::vector<uint32_t> all(n);
        for (uint32_t s = 0; s < n; s++) all[s] = s;
        const Id lo(20, 0x00), hi(20, 0xFF);
        check(ids, {}, {});
        check(ids, all, {});                         // erase all
        check(ids, {0}, {});                         // the first
        check(ids, {n - 1}, {});                     // the last
        check(ids, {}, {lo});                        // an insert before
        check(ids, {}, {hi});                        // after
        check(ids, {}, {hi, lo});                    // both, in descending order
        check(ids, all, {hi, lo, ids[n / 2]});       // everything replaced, one ID re-used
        check(ids, {n / 2}, {ids[n / 2]});           // erased and inserted again
        if (n >= 2) check(ids, {0, n - 1}, {ids[n - 1], ids[0]});
        // between: beside every kept search, differing in the last byte only (the top 64 bits are shared)
        std::vector<Id> between;
        for (uint32_t s = 0; s < n; s += 3) between.push_back(bump(ids[s], 1));
        std::shuffle(between.begin(), between.end(), g);
        check(ids, {}, between);
        for (int round = 0; round < 20; round++) {   // runs of erased searches, scattered inserts
            std::vector<uint32_t> erase;
            for (uint32_t s = 0; s < n;) {
                const uint32_t run = 1 + (uint32_t)(g() % 9), gap = (uint32_t)(g() % 12);
                for (uint32_t k = 0; k < run && s < n; k++) erase.push_back(s++);
                s += gap;
            }
            std::vector<Id> ins;
            for (uint32_t s = 0; s < n; s++) {
                const bool erased = std::binary_search(erase.begin(), erase.end(), s);
                if (erased && (g() & 1)) ins.push_back(ids[s]);        // re-used
                if ((g() & 3) == 0) ins.push_back(bump(ids[s], 1));    // beside it
            }
            for (int k = 0; k < 5; k++) ins.push_back(rand_id(g));
            std::shuffle(ins.begin(), ins.end(), g);
            check(ids, erase, ins);
        }
        // rejected inputs, each leaving no trace the caller would read
        kadplan::SearchesApplyPlan p;
        std::string msg;
        EXPECT(run_plan(ids, {n}, {}, p, &msg) == KAD_ERR_INVALID && msg.find("below S") != std::string::npos);
        EXPECT(run_plan(ids, {0, 0}, {}, p) == KAD_ERR_INVALID);
        if (n >= 2) EXPECT(run_plan(ids, {1, 0}, {}, p) == KAD_ERR_INVALID);
        EXPECT(run_plan(ids, {0xFFFFFFFFu}, {}, p) == KAD_ERR_INVALID);
        EXPECT(run_plan(ids, {}, {lo, hi, lo}, p, &msg) == KAD_ERR_INVALID && msg.find("equal") != std::string::npos);
        EXPECT(run_plan(ids, {}, {ids[0]}, p, &msg) == KAD_ERR_INVALID && msg.find("kept") != std::string::npos);
        EXPECT(run_plan(ids, {}, {lo, ids[n - 1]}, p) == KAD_ERR_INVALID);
        EXPECT(run_plan(ids, {}, {ids[n / 2], hi}, p) == KAD_ERR_INVALID);
        if (n >= 2) EXPECT(run_plan(ids, {0}, {ids[1]}, p) == KAD_ERR_INVALID);   // erased one, re-used another
        EXPECT(run_plan(ids, {n}, {ids[0], ids[0]}, p, &msg) == KAD_ERR_INVALID &&
               msg.find("below S") != std::string::npos);                          // the erase list is checked first
        EXPECT(run_plan(ids, {}, {ids[0], lo, lo}, p, &msg) == KAD_ERR_INVALID &&
               msg.find("equal") != std::string::npos);                            // then distinctness
    }
    std::string err;
    EXPECT(kadplan::searches_check_erase(0, nullptr, 0, err) == KAD_OK);
    const uint32_t zero = 0;
    EXPECT(kadplan::searches_check_erase(0, &zero, 1, err) == KAD_ERR_INVALID);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("PASS\n");
    return 0;
}
