// The host parts of kad_sr_step and kad_sr_mark_entries (kad_search_step / kad_search_step_batch over kad_step.h's closed
// form, kadplan::sr_step_check, kadplan::sr_entries_plan; opendht_amd/csrc/kad_searches_plan.cpp) under AddressSanitizer and
// UndefinedBehaviorSanitizer: a stand-alone program, compiled together with the plan file by tests/test_sr_step_san.py.
// Every array is an exact-size copy, so a read past any input is a report, and the shifts of the 64-bit planes (n = 64, a
// pick at entry 63, room of 1 to 4) run under UBSan. Random lists of every length 0..64 in both search states and every
// mode are checked against searchStep's loops written out one entry at a time; then the checks, in their documented order.
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

bool can_get(uint8_t f) { return !(f & KAD_SN_NOGET) && (!(f & KAD_SN_BAD) || (f & KAD_SN_CANDIDATE)); }

uint32_t solicited_of(const std::vector<uint8_t>& fl) {
    uint32_t c = 0;
    for (uint8_t f : fl) c += !(f & KAD_SN_BAD) && (f & KAD_SN_PENDING);
    return c;
}

// Dht::searchStep (dht.cpp:1344-1464) on flag bytes, one entry at a time
kad_step_out loop_step(std::vector<uint8_t> fl, bool expired, uint32_t mode) {
    const uint32_t n = (uint32_t)fl.size();
    uint32_t bad = 0, lead = 0;
    for (uint8_t f : fl) bad += f & KAD_SN_BAD;
    while (lead < n && (fl[lead] & KAD_SN_BAD)) lead++;
    kad_step_out o = {0, 0, 0};
    if (expired) {
        o.bits = KAD_STEP_SKIPPED;
    } else {
        if (n - bad < KAD_SEARCH_NODES) o.bits |= KAD_STEP_SHORT;
        uint32_t i = 0;
        bool synced = true;
        for (uint8_t f : fl) {
            if (f & KAD_SN_BAD) continue;
            if (!(f & KAD_SN_SYNCED)) {
                synced = false;
                break;
            }
            if (++i == 8) break;
        }
        synced = synced && i > 0;
        if (synced) o.bits |= KAD_STEP_SYNCED;
        const bool done = synced && (mode & KAD_STEP_DONE_IF_SYNCED);
        if (done) o.bits |= KAD_STEP_DONE;
        if (solicited_of(fl) < 4 && !(mode & KAD_STEP_NO_SEND)) {
            bool sent;
            do {
                sent = false;
                if (!done && solicited_of(fl) < 4) {
                    for (uint32_t e = 0; e < n && !sent; e++)
                        if (can_get(fl[e])) {
                            fl[e] |= KAD_SN_PENDING | KAD_SN_NOGET;
                            o.picks |= 1ull << e;
                            sent = true;
                        }
                    if (!sent) o.bits |= KAD_STEP_EXHAUSTED;
                }
            } while (sent && solicited_of(fl) < 4);
        }
        if (lead >= std::min(n, 25u)) o.bits |= KAD_STEP_EXPIRE;
    }
    o.counts = n | (bad << 8) | (lead << 16) | (solicited_of(fl) << 24);
    return o;
}

bool same(const kad_step_out& a, const kad_step_out& b) { return a.picks == b.picks && a.counts == b.counts && a.bits == b.bits; }

}  // namespace

int main() {
    std::mt19937_64 rng(12345);
    const uint8_t profiles[5][8] = {
        {0, 0, 0, KAD_SN_NOGET, KAD_SN_PENDING | KAD_SN_NOGET, KAD_SN_BAD, KAD_SN_BAD | KAD_SN_CANDIDATE, KAD_SN_SYNCED},
        {KAD_SN_SYNCED, KAD_SN_SYNCED, KAD_SN_SYNCED | KAD_SN_NOGET, KAD_SN_SYNCED, 0, KAD_SN_BAD | KAD_SN_SYNCED, KAD_SN_SYNCED, KAD_SN_SYNCED},
        {KAD_SN_BAD, KAD_SN_BAD, KAD_SN_BAD | KAD_SN_REMOVABLE, KAD_SN_BAD | KAD_SN_CANDIDATE, KAD_SN_BAD, KAD_SN_BAD, 0, KAD_SN_BAD},
        {KAD_SN_NOGET, KAD_SN_NOGET, KAD_SN_NOGET, 0, KAD_SN_NOGET | KAD_SN_PENDING, KAD_SN_PENDING, KAD_SN_NOGET, KAD_SN_NOGET},
        {0, 0, 0, 0, 0, 0, 0, 0}};
    uint32_t seen = 0;
    for (uint32_t n = 0; n <= 64; n++) {
        for (uint32_t rep = 0; rep < 40; rep++) {
            std::vector<uint8_t> fl(n);  // exact size
            for (auto& f : fl) f = rep % 5 == 4 ? (uint8_t)(rng() & 63) : profiles[rep % 5][rng() & 7];
            for (uint32_t expired = 0; expired < 2; expired++)
                for (uint32_t mode = 0; mode < 16; mode++) {
                    kad_step_out got = {1, 2, 3};
                    EXPECT(kad_search_step(n, n ? fl.data() : nullptr, expired, mode, &got) == KAD_OK);
                    const kad_step_out want = loop_step(fl, expired != 0, mode);
                    EXPECT(same(got, want));
                    seen |= got.bits;
                }
        }
    }
    EXPECT(seen == 0x3Fu);
    {  // the batch entry over exact-size CSR arrays, lists of every length once
        std::vector<uint32_t> off = {0};
        std::vector<uint8_t> fl, sf, md;
        for (uint32_t n = 0; n <= 64; n++) {
            for (uint32_t e = 0; e < n; e++) fl.push_back((uint8_t)(rng() & 63));
            off.push_back((uint32_t)fl.size());
            sf.push_back(n % 7 == 3 ? KAD_SR_EXPIRED : 0);
            md.push_back((uint8_t)(n & 15));
        }
        std::vector<kad_step_out> out(65);
        EXPECT(kad_search_step_batch(65, off.data(), fl.data(), sf.data(), md.data(), out.data()) == KAD_OK);
        for (uint32_t k = 0; k < 65; k++)
            EXPECT(same(out[k], loop_step(std::vector<uint8_t>(fl.begin() + off[k], fl.begin() + off[k + 1]), sf[k] != 0, md[k])));
        EXPECT(kad_search_step_batch(65, off.data(), fl.data(), nullptr, nullptr, out.data()) == KAD_OK);
        std::vector<uint32_t> long_off = {0, 65};
        std::vector<uint8_t> long_fl(65, 0);
        EXPECT(kad_search_step_batch(1, long_off.data(), long_fl.data(), nullptr, nullptr, out.data()) == KAD_ERR_INVALID);
        kad_step_out one;
        EXPECT(kad_search_step(65, long_fl.data(), 0, 0, &one) == KAD_ERR_INVALID);
        EXPECT(kad_search_step(0, nullptr, 0, 0x10, &one) == KAD_ERR_INVALID);
        EXPECT(kad_search_step(1, nullptr, 0, 0, &one) == KAD_ERR_INVALID);
        EXPECT(kad_search_step(0, nullptr, 0, 0, nullptr) == KAD_ERR_INVALID);
    }
    {  // kad_sr_step's list checks, in order
        std::string msg;
        const std::vector<uint32_t> up = {0, 3, 7}, twice = {0, 3, 3}, down = {3, 0, 7}, out_of = {0, 3, 8};
        const std::vector<uint8_t> ok = {1, 15, 0}, wide = {0, 0, 16};
        EXPECT(kadplan::sr_step_check(8, 3, up.data(), ok.data(), msg) == KAD_OK);
        EXPECT(kadplan::sr_step_check(8, 3, up.data(), nullptr, msg) == KAD_OK);
        EXPECT(kadplan::sr_step_check(3, 3, nullptr, ok.data(), msg) == KAD_OK);
        EXPECT(kadplan::sr_step_check(0, 0, nullptr, nullptr, msg) == KAD_OK);
        EXPECT(kadplan::sr_step_check(8, 3, nullptr, wide.data(), msg) == KAD_ERR_INVALID && msg.find("m must be S") != std::string::npos);
        for (const auto* w : {&twice, &down, &out_of})
            EXPECT(kadplan::sr_step_check(8, 3, w->data(), wide.data(), msg) == KAD_ERR_INVALID && msg.find("ascending") != std::string::npos);
        EXPECT(kadplan::sr_step_check(8, 3, up.data(), wide.data(), msg) == KAD_ERR_INVALID && msg.find("search 2") != std::string::npos);
        EXPECT(kadplan::sr_step_check(3, 3, nullptr, wide.data(), msg) == KAD_ERR_INVALID && msg.find("mode bit") != std::string::npos);
    }
    {  // kad_sr_mark_entries' plan: the checks in order, then the sorted pairs and the way back
        std::string msg;
        kadplan::SrEntriesPlan plan;
        const uint32_t p = 300;
        std::vector<uint32_t> pw(p);
        std::vector<uint8_t> ids(20ull * p), clear(p), setb(p);
        for (uint32_t k = 0; k < p; k++) {
            pw[k] = (uint32_t)(rng() % 50);
            for (uint32_t b = 0; b < 20; b++) ids[20ull * k + b] = (uint8_t)rng();
            if (k % 9 == 0 && k) std::memcpy(&ids[20ull * k], &ids[20ull * (k - 1)], 20);  // the same ID in another search, mostly
            if (k % 9 == 0 && k && pw[k] == pw[k - 1]) pw[k] = (pw[k] + 1) % 50;
            clear[k] = (uint8_t)((rng() & 15) << 2);
            setb[k] = (uint8_t)(((rng() & 15) << 2) & ~clear[k]);
        }
        EXPECT(kadplan::sr_entries_plan(50, p, pw.data(), ids.data(), clear.data(), setb.data(), plan, msg) == KAD_OK);
        EXPECT(plan.pord.size() == p && plan.pkey.size() == p && plan.ptail.size() == 3ull * p);
        std::vector<uint8_t> hit(p, 0);
        for (uint32_t k = 0; k < p; k++) {
            const uint32_t a = plan.pord[k];
            EXPECT(a < p && !hit[a]);
            hit[a] = 1;
            EXPECT(plan.pw[k] == pw[a] && plan.pclear[k] == clear[a] && plan.pset[k] == setb[a]);
            uint64_t key = 0;
            for (uint32_t b = 0; b < 8; b++) key = key << 8 | ids[20ull * a + b];
            EXPECT(plan.pkey[k] == key);
            if (k) EXPECT(plan.pw[k - 1] <= plan.pw[k]);
        }
        EXPECT(kadplan::sr_entries_plan(50, p, pw.data(), ids.data(), nullptr, nullptr, plan, msg) == KAD_OK);
        EXPECT(std::all_of(plan.pclear.begin(), plan.pclear.end(), [](uint8_t v) { return v == 0; }));
        EXPECT(kadplan::sr_entries_plan(0, 0, nullptr, nullptr, nullptr, nullptr, plan, msg) == KAD_OK && plan.pord.empty());
        // every refusal, each with the later ones present too: the first in the documented order answers
        std::vector<uint32_t> w2 = {1, 1, 9};
        std::vector<uint8_t> i2(60, 7), c2 = {0x04, 0x08, 0x41}, s2 = {0x10, 0x08, 0x02};
        EXPECT(kadplan::sr_entries_plan(5, 3, w2.data(), i2.data(), c2.data(), s2.data(), plan, msg) == KAD_ERR_INVALID &&
               msg.find("pair 2: clear_bits") != std::string::npos);
        c2[2] = 0x04;
        EXPECT(kadplan::sr_entries_plan(5, 3, w2.data(), i2.data(), c2.data(), s2.data(), plan, msg) == KAD_ERR_INVALID &&
               msg.find("pair 2: set_bits") != std::string::npos);
        s2[2] = 0x20;
        EXPECT(kadplan::sr_entries_plan(5, 3, w2.data(), i2.data(), c2.data(), s2.data(), plan, msg) == KAD_ERR_INVALID &&
               msg.find("pair 1: a bit both") != std::string::npos);
        s2[1] = 0;
        EXPECT(kadplan::sr_entries_plan(5, 3, w2.data(), i2.data(), c2.data(), s2.data(), plan, msg) == KAD_ERR_INVALID &&
               msg.find("pair 2: search 9") != std::string::npos);
        w2[2] = 4;
        EXPECT(kadplan::sr_entries_plan(5, 3, w2.data(), i2.data(), c2.data(), s2.data(), plan, msg) == KAD_ERR_INVALID &&
               msg.find("are equal") != std::string::npos);
        w2[1] = 2;
        EXPECT(kadplan::sr_entries_plan(5, 3, w2.data(), i2.data(), c2.data(), s2.data(), plan, msg) == KAD_OK);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("PASS\n");
    return 0;
}
