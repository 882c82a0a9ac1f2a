// One round's host plan of kad_sr_try_insert_tick (kadplan::sr_round_plan, opendht_amd/csrc/kad_searches_plan.cpp) under
// AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, compiled together with the plan file by
// tests/test_sr_tick_san.py. Every array is an exact-size copy, so a read past any input is a report. Random rounds over
// sets of 0 to 1000 searches (sizes around the bitmap's word size included, intervals that start and end on word
// boundaries, runs over the whole set) are checked against the rules written out one search at a time; the same plan
// object is used for every round, as the engine does. Then the refusals, and the C entry with exact-size outputs.
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

struct Round {
    uint32_t S = 0;
    std::vector<uint32_t> lb, fwd, back;
    std::vector<uint8_t> stop, trim;
};

struct Plain {
    std::vector<uint8_t> kind;
    std::vector<uint32_t> pw, pc;
    std::vector<uint8_t> want;
};

bool far_stop(uint32_t v) { return v == KAD_SR_STOP_FAR || v == KAD_SR_STOP_FAR_EXPIRED; }
bool open_stop(uint32_t v) { return v == KAD_SR_STOP_KNOWN || v == KAD_SR_STOP_FAR_EXPIRED; }

// plan_insert_round, one search at a time
Plain plain_plan(const Round& in) {
    const uint32_t r = (uint32_t)in.stop.size();
    Plain out;
    out.kind.assign(r, KAD_SR_PLAN_SKIPPED);
    std::vector<uint8_t> marked(in.S + 1, 0);
    std::vector<int64_t> owner(in.S + 1, -1), want(in.S + 1, 0);
    int64_t up = in.S, down = -1;
    for (uint32_t k = 0; k < r; k++) {
        const uint32_t fs = in.stop[k] & 15u, bs = in.stop[k] >> 4;
        const int64_t l = in.lb[k], f = in.fwd[k], b = in.back[k];
        const bool ftrim = far_stop(fs) && (in.trim[k] & 1), btrim = far_stop(bs) && (in.trim[k] & 2);
        const bool fin_f = fs == KAD_SR_STOP_END || fs == KAD_SR_STOP_FAR, fin_b = bs == KAD_SR_STOP_END || bs == KAD_SR_STOP_FAR;
        if (f + b == 0 && fin_f && fin_b && !ftrim && !btrim) continue;
        const int64_t lo = l - b - (bs == KAD_SR_STOP_END ? 0 : 1), hi = l + f - (fs == KAD_SR_STOP_END ? 1 : 0);
        bool free = lo <= hi && hi < up && lo > down;
        for (int64_t s = lo; free && s <= hi; s++) free = !marked[s];
        if (free) {
            out.kind[k] = KAD_SR_PLAN_READY;
            for (int64_t s = l - b; s < l + f; s++) owner[s] = k, want[s] = 1;
            if (ftrim) owner[l + f] = k, want[l + f] = 0;
            if (btrim) owner[l - b - 1] = k, want[l - b - 1] = 0;
        } else {
            out.kind[k] = KAD_SR_PLAN_DEFERRED;
            if (lo <= hi) {
                if (open_stop(fs)) up = std::min(up, lo);
                if (open_stop(bs)) down = std::max(down, hi);
            }
        }
        for (int64_t s = lo; s <= hi; s++) marked[s] = 1;
    }
    for (uint32_t s = 0; s < in.S; s++)
        if (owner[s] >= 0) {
            out.pw.push_back(s);
            out.pc.push_back((uint32_t)owner[s]);
            out.want.push_back((uint8_t)want[s]);
        }
    return out;
}

int run(const Round& in0, kadplan::SrRoundPlan& plan, std::string* msg = nullptr) {
    const Round in(in0);  // exact-size copies
    const uint32_t r = (uint32_t)in.stop.size();
    std::string err;
    const int rc = kadplan::sr_round_plan(in.S, r, in.lb.data(), in.fwd.data(), in.back.data(), in.stop.data(),
                                          in.trim.data(), plan, err);
    EXPECT((rc == KAD_OK) == err.empty());
    if (msg) *msg = err;
    return rc;
}

void check(const Round& in, kadplan::SrRoundPlan& plan) {
    EXPECT(run(in, plan) == KAD_OK);
    const Plain want = plain_plan(in);
    EXPECT(plan.kind == want.kind);
    EXPECT(plan.pair_which == want.pw && plan.pair_cand == want.pc && plan.pair_want == want.want);
    // the C entry with outputs of exactly r and S entries
    const uint32_t r = (uint32_t)in.stop.size();
    std::vector<uint8_t> kind(r), pwant(in.S);
    std::vector<uint32_t> pw(in.S), pc(in.S);
    uint32_t n = 99;
    const Round c(in);
    EXPECT(kad_sr_plan_round(c.S, r, c.lb.data(), c.fwd.data(), c.back.data(), c.stop.data(), c.trim.data(), kind.data(),
                             pw.data(), pc.data(), pwant.data(), &n) == KAD_OK);
    EXPECT(n == want.pw.size() && kind == want.kind);
    pw.resize(n);
    pc.resize(n);
    pwant.resize(n);
    EXPECT(pw == want.pw && pc == want.pc && pwant == want.want);
}

// a verdict that is consistent with S searches: lb, the two runs and stops that name a search where they are not END
void push(Round& in, std::mt19937_64& rng, uint32_t l, uint32_t f, uint32_t b) {
    const uint32_t S = in.S;
    const uint32_t fs = l + f == S ? KAD_SR_STOP_END : 1u + (uint32_t)(rng() % 3), bs = l == b ? KAD_SR_STOP_END : 1u + (uint32_t)(rng() % 3);
    in.lb.push_back(l);
    in.fwd.push_back(f);
    in.back.push_back(b);
    in.stop.push_back((uint8_t)(fs | (bs << 4)));
    in.trim.push_back((uint8_t)(rng() % 4));
}

Round random_round(std::mt19937_64& rng, uint32_t S, uint32_t r, uint32_t longest) {
    Round in;
    in.S = S;
    for (uint32_t k = 0; k < r; k++) {
        const uint32_t l = (uint32_t)(rng() % (S + 1u));
        uint32_t f = (uint32_t)(rng() % (longest + 1u)), b = (uint32_t)(rng() % (longest + 1u));
        if (rng() % 3 == 0) f = b = 0;
        f = std::min(f, S - l);
        b = std::min(b, l);
        if (rng() % 16 == 0) f = S - l;  // runs off the end
        if (rng() % 16 == 0) b = l;
        push(in, rng, l, f, b);
    }
    return in;
}

}  // namespace

int main() {
    std::mt19937_64 rng(2718);
    kadplan::SrRoundPlan plan;  // one object for every round: the scratch of an earlier, larger set must not show
    for (uint32_t S : {1000u, 0u, 1u, 2u, 63u, 64u, 65u, 127u, 128u, 129u, 640u, 300u})
        for (uint32_t r : {0u, 1u, 2u, 17u, 400u})
            for (uint32_t longest : {0u, 1u, 3u, 70u, 1000u}) check(random_round(rng, S, r, longest), plan);
    {  // intervals on the words' boundaries, and the whole set for one candidate
        Round in;
        in.S = 256;
        push(in, rng, 64, 64, 0);    // accepting 64 .. 127
        push(in, rng, 129, 63, 0);   // 129 .. 191 plus its stoppers
        push(in, rng, 63, 0, 63);    // 0 .. 62, its forward stopper is 63
        push(in, rng, 200, 56, 0);   // runs off the end
        push(in, rng, 0, 256, 0);    // everything: meets all of them
        check(in, plan);
        Round all;
        all.S = 1000;
        push(all, rng, 500, 500, 500);
        push(all, rng, 7, 0, 0);
        check(all, plan);
        EXPECT(plan.kind[0] == KAD_SR_PLAN_READY && plan.pair_which.size() == 1000);
    }
    {  // the refusals: none reads past its input, none leaves a message out
        std::string msg;
        const uint32_t bad[][5] = {{9, 0, 0, 0, 0}, {5, 4, 0, 0, 0}, {2, 0, 3, 0, 0}, {7, 1, 0, 2, 2}, {0, 1, 0, 2, 2}, {3, 0, 0, 4, 0}, {3, 0, 0, 0, 5}};
        for (const auto& v : bad) {
            Round in;
            in.S = 8;
            in.lb = {1, v[0]};
            in.fwd = {0, v[1]};
            in.back = {0, v[2]};
            in.stop = {(uint8_t)(2 | 2 << 4), (uint8_t)(v[3] | v[4] << 4)};
            in.trim = {0, 3};
            EXPECT(run(in, plan, &msg) == KAD_ERR_INVALID && msg.find("candidate 1") != std::string::npos);
        }
        uint32_t n = 5;
        EXPECT(kad_sr_plan_round(8, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n) == KAD_OK && n == 0);
        EXPECT(kad_sr_plan_round(8, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == KAD_ERR_INVALID);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("PASS\n");
    return 0;
}
