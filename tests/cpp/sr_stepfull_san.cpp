// The host parts of kad_sr_step_full and kad_sr_mark_due (kad_search_step_full / kad_search_step_full_batch over
// kadstep::decide_full, kadplan::sr_step_full_check, kadplan::sr_due_plan; opendht_amd/csrc/kad_searches_plan.cpp) under
// AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, compiled together with the plan file by
// tests/test_sr_stepfull_san.py. Every array is an exact-size copy, so a read past any input is a report, and the shifts
// of the 64-bit planes (n = 64, a fourth or eighth counted entry at bit 63) run under UBSan. Random lists of every length
// 0..64 over all eight bits, in both search states and every valid mode, are checked against searchStep's three send loops
// written out one entry at a time; then the checks, in their documented order.
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

bool valid_mode(uint32_t m) {
    if (m & ~0x7Fu) return false;
    if ((m & KAD_STEP_DONE_IF_SYNCED) && (m & (KAD_STEP_LISTEN | KAD_STEP_ANNOUNCE))) return false;
    return !(m & KAD_STEP_PROBE_BLOCKS) || (m & KAD_STEP_ANNOUNCE);
}

// Dht::searchStep (dht.cpp:1344-1464) with searchSendAnnounceValue (:1237-1339) on flag bytes, one entry at a time
kad_step_full_out loop_step(std::vector<uint8_t> fl, bool expired, uint32_t mode) {
    const uint32_t n = (uint32_t)fl.size();
    uint32_t bad = 0, lead = 0;
    for (uint8_t f : fl) bad += f & KAD_SN_BAD;
    while (lead < n && (fl[lead] & KAD_SN_BAD)) lead++;
    kad_step_full_out o = {0, 0, 0, 0, 0};
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
        if (synced) {
            o.bits |= KAD_STEP_SYNCED;
            if (mode & KAD_STEP_LISTEN) {  // :1384-1428
                i = 0;
                for (uint32_t e = 0; e < n; e++) {
                    if (!(fl[e] & KAD_SN_SYNCED)) continue;
                    if (fl[e] & KAD_SN_LISTEN_DUE) {
                        o.listen |= 1ull << e;
                        fl[e] &= (uint8_t)~KAD_SN_LISTEN_DUE;
                    }
                    if (!(fl[e] & KAD_SN_CANDIDATE) && ++i == 4) break;
                }
            }
            if (mode & KAD_STEP_ANNOUNCE) {  // :1244-1338
                i = 0;
                for (uint32_t e = 0; e < n; e++) {
                    if (!((fl[e] & KAD_SN_SYNCED) && (fl[e] & KAD_SN_ANNOUNCE_DUE))) continue;
                    o.announce |= 1ull << e;
                    fl[e] = (uint8_t)((fl[e] | KAD_SN_PENDING | ((mode & KAD_STEP_PROBE_BLOCKS) ? KAD_SN_NOGET : 0u)) &
                                      ~KAD_SN_ANNOUNCE_DUE);
                    if (!(fl[e] & KAD_SN_CANDIDATE) && ++i == 8) break;
                }
            }
        }
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

bool same(const kad_step_full_out& a, const kad_step_full_out& b) {
    return a.picks == b.picks && a.listen == b.listen && a.announce == b.announce && a.counts == b.counts && a.bits == b.bits;
}

}  // namespace

int main() {
    std::mt19937_64 rng(4321);
    const uint8_t S = KAD_SN_SYNCED, G = KAD_SN_SYNCED | KAD_SN_NOGET, L = KAD_SN_LISTEN_DUE, A = KAD_SN_ANNOUNCE_DUE,
                  BC = KAD_SN_BAD | KAD_SN_CANDIDATE;
    const uint8_t profiles[3][8] = {
        {(uint8_t)(G | L), (uint8_t)(G | A), (uint8_t)(G | L | A), G, (uint8_t)(S | A), (uint8_t)(BC | G | L | A), (uint8_t)(BC | S | A), (uint8_t)(G | L)},
        {S, (uint8_t)(S | KAD_SN_PENDING | KAD_SN_NOGET), (uint8_t)(S | A), (uint8_t)(S | L), (uint8_t)(G | L | A), (uint8_t)(BC | G | L), BC, KAD_SN_BAD},
        {(uint8_t)(BC | G | L | A), (uint8_t)(BC | G | L | A), (uint8_t)(BC | G | L | A), (uint8_t)(G | L | A), (uint8_t)(BC | G | A), (uint8_t)(BC | G | L), (uint8_t)(G | A), (uint8_t)(G | L)}};
    uint32_t seen = 0;
    uint64_t listens = 0, announces = 0, top = 0;
    for (uint32_t n = 0; n <= 64; n++) {
        for (uint32_t rep = 0; rep < 24; rep++) {
            std::vector<uint8_t> fl(n);  // exact size
            for (auto& f : fl) f = rep % 4 == 3 ? (uint8_t)rng() : profiles[rep % 4][rng() & 7];
            if (rep == 0 && n) {  // candidates all along, the one entry that counts is the last: both walks reach n - 1
                std::fill(fl.begin(), fl.end(), (uint8_t)(BC | G | L | A));
                fl[n - 1] = (uint8_t)(G | L | A);
            }
            for (uint32_t expired = 0; expired < 2; expired++)
                for (uint32_t mode = 0; mode < 256; mode++) {
                    kad_step_full_out got = {1, 2, 3, 4, 5};
                    const int rc = kad_search_step_full(n, n ? fl.data() : nullptr, expired, mode, &got);
                    if (!valid_mode(mode)) {
                        EXPECT(rc == KAD_ERR_INVALID && got.picks == 1 && got.bits == 5);
                        continue;
                    }
                    EXPECT(rc == KAD_OK);
                    const kad_step_full_out want = loop_step(fl, expired != 0, mode);
                    EXPECT(same(got, want));
                    seen |= got.bits;
                    listens += got.listen != 0;
                    announces += got.announce != 0;
                    top += ((got.listen | got.announce) >> 63) & 1;
                    if (!(mode & (KAD_STEP_LISTEN | KAD_STEP_ANNOUNCE))) {  // kad_search_step's answer, zero masks
                        kad_step_out old = {9, 9, 9};
                        EXPECT(kad_search_step(n, n ? fl.data() : nullptr, expired, mode, &old) == KAD_OK);
                        EXPECT(old.picks == got.picks && old.counts == got.counts && old.bits == got.bits);
                        EXPECT(got.listen == 0 && got.announce == 0);
                    }
                }
        }
    }
    EXPECT(seen == 0x3Fu);
    EXPECT(listens && announces && top);  // both loops sent, and to entry 63
    {  // the batch entry over exact-size CSR arrays, lists of every length once, every valid mode in turn
        std::vector<uint32_t> modes;
        for (uint32_t m = 0; m < 256; m++)
            if (valid_mode(m)) modes.push_back(m);
        EXPECT(modes.size() == 56);
        std::vector<uint32_t> off = {0};
        std::vector<uint8_t> fl, sf, md;
        for (uint32_t n = 0; n <= 64; n++) {
            for (uint32_t e = 0; e < n; e++) fl.push_back(profiles[n % 3][rng() & 7]);
            off.push_back((uint32_t)fl.size());
            sf.push_back(n % 7 == 3 ? KAD_SR_EXPIRED : 0);
            md.push_back((uint8_t)modes[n % modes.size()]);
        }
        std::vector<kad_step_full_out> out(65);
        EXPECT(kad_search_step_full_batch(65, off.data(), fl.data(), sf.data(), md.data(), out.data()) == KAD_OK);
        for (uint32_t k = 0; k < 65; k++)
            EXPECT(same(out[k], loop_step(std::vector<uint8_t>(fl.begin() + off[k], fl.begin() + off[k + 1]), sf[k] != 0, md[k])));
        EXPECT(kad_search_step_full_batch(65, off.data(), fl.data(), nullptr, nullptr, out.data()) == KAD_OK);
        md[64] = KAD_STEP_PROBE_BLOCKS;
        out[0].bits = 0xABCDu;
        EXPECT(kad_search_step_full_batch(65, off.data(), fl.data(), sf.data(), md.data(), out.data()) == KAD_ERR_INVALID);
        EXPECT(out[0].bits == 0xABCDu);  // nothing written before every check passed
        std::vector<uint32_t> long_off = {0, 65};
        std::vector<uint8_t> long_fl(65, 0);
        EXPECT(kad_search_step_full_batch(1, long_off.data(), long_fl.data(), nullptr, nullptr, out.data()) == KAD_ERR_INVALID);
        kad_step_full_out one;
        EXPECT(kad_search_step_full(65, long_fl.data(), 0, 0, &one) == KAD_ERR_INVALID);
        EXPECT(kad_search_step_full(1, nullptr, 0, 0, &one) == KAD_ERR_INVALID);
        EXPECT(kad_search_step_full(0, nullptr, 0, 0, nullptr) == KAD_ERR_INVALID);
    }
    {  // kad_sr_step_full's list checks, in order
        std::string msg;
        const std::vector<uint32_t> up = {0, 3, 7}, twice = {0, 3, 3}, down = {3, 0, 7}, out_of = {0, 3, 8};
        const std::vector<uint8_t> ok = {0x71, 0x3B, 0x0F};
        EXPECT(kadplan::sr_step_full_check(8, 3, up.data(), ok.data(), msg) == KAD_OK);
        EXPECT(kadplan::sr_step_full_check(8, 3, up.data(), nullptr, msg) == KAD_OK);
        EXPECT(kadplan::sr_step_full_check(3, 3, nullptr, ok.data(), msg) == KAD_OK);
        EXPECT(kadplan::sr_step_full_check(0, 0, nullptr, nullptr, msg) == KAD_OK);
        EXPECT(kadplan::sr_step_check(3, 3, nullptr, ok.data(), msg) == KAD_ERR_INVALID);  // the old check refuses them
        for (uint8_t bad : {(uint8_t)0x80, (uint8_t)0x14, (uint8_t)0x24, (uint8_t)0x40, (uint8_t)0x50}) {
            const std::vector<uint8_t> wide = {0, 0, bad};
            EXPECT(kadplan::sr_step_full_check(8, 3, nullptr, wide.data(), msg) == KAD_ERR_INVALID && msg.find("m must be S") != std::string::npos);
            for (const auto* w : {&twice, &down, &out_of})
                EXPECT(kadplan::sr_step_full_check(8, 3, w->data(), wide.data(), msg) == KAD_ERR_INVALID && msg.find("ascending") != std::string::npos);
            EXPECT(kadplan::sr_step_full_check(8, 3, up.data(), wide.data(), msg) == KAD_ERR_INVALID && msg.find("search 2") != std::string::npos);
            EXPECT(kadplan::sr_step_full_check(3, 3, nullptr, wide.data(), msg) == KAD_ERR_INVALID && msg.find("invalid mode") != std::string::npos);
        }
    }
    {  // kad_sr_mark_due's plan: sr_entries_plan over 0xC0
        std::string msg;
        kadplan::SrEntriesPlan plan;
        const uint32_t p = 300;
        std::vector<uint32_t> pw(p);
        std::vector<uint8_t> ids(20ull * p), clear(p), setb(p);
        for (uint32_t k = 0; k < p; k++) {
            pw[k] = (uint32_t)(rng() % 50);
            for (uint32_t b = 0; b < 20; b++) ids[20ull * k + b] = (uint8_t)rng();
            clear[k] = (uint8_t)((rng() & 3) << 6);
            setb[k] = (uint8_t)(((rng() & 3) << 6) & ~clear[k]);
        }
        EXPECT(kadplan::sr_due_plan(50, p, pw.data(), ids.data(), clear.data(), setb.data(), plan, msg) == KAD_OK);
        EXPECT(plan.pord.size() == p && plan.pkey.size() == p && plan.ptail.size() == 3ull * p);
        std::vector<uint8_t> hit(p, 0);
        for (uint32_t k = 0; k < p; k++) {
            const uint32_t a = plan.pord[k];
            EXPECT(a < p && !hit[a]);
            hit[a] = 1;
            EXPECT(plan.pw[k] == pw[a] && plan.pclear[k] == clear[a] && plan.pset[k] == setb[a]);
            if (k) EXPECT(plan.pw[k - 1] <= plan.pw[k]);
        }
        EXPECT(kadplan::sr_entries_plan(50, p, pw.data(), ids.data(), clear.data(), setb.data(), plan, msg) == KAD_ERR_INVALID);
        EXPECT(kadplan::sr_due_plan(0, 0, nullptr, nullptr, nullptr, nullptr, plan, msg) == KAD_OK && plan.pord.empty());
        // every refusal, each with the later ones present too: the first in the documented order answers
        std::vector<uint32_t> w2 = {1, 1, 9};
        std::vector<uint8_t> i2(60, 7), c2 = {0x40, 0x80, 0x44}, s2 = {0x80, 0x80, 0x20};
        EXPECT(kadplan::sr_due_plan(5, 3, w2.data(), i2.data(), c2.data(), s2.data(), plan, msg) == KAD_ERR_INVALID &&
               msg.find("pair 2: clear_bits outside the due bits") != std::string::npos);
        c2[2] = 0x40;
        EXPECT(kadplan::sr_due_plan(5, 3, w2.data(), i2.data(), c2.data(), s2.data(), plan, msg) == KAD_ERR_INVALID &&
               msg.find("pair 2: set_bits outside the due bits") != std::string::npos);
        s2[2] = 0x80;
        EXPECT(kadplan::sr_due_plan(5, 3, w2.data(), i2.data(), c2.data(), s2.data(), plan, msg) == KAD_ERR_INVALID &&
               msg.find("pair 1: a bit both") != std::string::npos);
        s2[1] = 0;
        EXPECT(kadplan::sr_due_plan(5, 3, w2.data(), i2.data(), c2.data(), s2.data(), plan, msg) == KAD_ERR_INVALID &&
               msg.find("pair 2: search 9") != std::string::npos);
        w2[2] = 4;
        EXPECT(kadplan::sr_due_plan(5, 3, w2.data(), i2.data(), c2.data(), s2.data(), plan, msg) == KAD_ERR_INVALID &&
               msg.find("are equal") != std::string::npos);
        w2[1] = 2;
        EXPECT(kadplan::sr_due_plan(5, 3, w2.data(), i2.data(), c2.data(), s2.data(), plan, msg) == KAD_OK);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("PASS\n");
    return 0;
}
