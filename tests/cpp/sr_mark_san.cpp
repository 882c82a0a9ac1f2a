// The host plan of kad_sr_mark_nodes (kadplan::sr_mark_plan, opendht_amd/csrc/kad_searches_plan.cpp) under
// AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, compiled together with the plan file by
// tests/test_sr_mark_san.py. Every array is an exact-size copy, so a read past any input is a report; accepted inputs
// are checked for the sort orders and the permutations, rejected ones in the order the header documents: unknown bits
// (clear, set, pair), a bit both ways, equal node IDs, a pair's search out of range, equal pairs.
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

struct In {
    uint32_t S = 0;
    std::vector<uint8_t> ids, clear, set;  // q x 20, q, q
    bool null_clear = false, null_set = false;
    std::vector<uint32_t> pw;
    std::vector<uint8_t> pid, pfl;
};

int run(const In& in0, kadplan::SrMarkPlan& plan, std::string* msg = nullptr) {
    const In in(in0);  // exact-size copies
    const uint32_t q = (uint32_t)in.clear.size(), p = (uint32_t)in.pw.size();
    std::string err;
    const int rc = kadplan::sr_mark_plan(in.S, q, q ? in.ids.data() : nullptr, in.null_clear ? nullptr : in.clear.data(),
                                         in.null_set ? nullptr : in.set.data(), p, p ? in.pw.data() : nullptr,
                                         p ? in.pid.data() : nullptr, p ? in.pfl.data() : nullptr, plan, err);
    EXPECT((rc == KAD_OK) == err.empty());
    if (msg) *msg = err;
    return rc;
}

bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

uint32_t be32(const uint8_t* p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

// the plan of an accepted input: both sorts, both permutations, every word
void check_plan(const In& in, const kadplan::SrMarkPlan& pl) {
    const uint32_t q = (uint32_t)in.clear.size(), p = (uint32_t)in.pw.size();
    EXPECT(pl.ord.size() == q && pl.bkey.size() == q && pl.btail.size() == 3ull * q && pl.bop.size() == q);
    EXPECT(pl.pord.size() == p && pl.pw.size() == p && pl.pkey.size() == p && pl.ptail.size() == 3ull * p &&
           pl.pfl.size() == p);
    std::vector<uint8_t> seen(q, 0), pseen(p, 0);
    // the prefix directory: B = ceil(log2 q) within its limits, dir[s] = the keys whose top B bits are below s
    if (q == 0) {
        EXPECT(pl.dir.empty() && pl.dbits == 0);
    } else {
        const uint32_t B = pl.dbits, most = q <= kadplan::SR_MARK_SMALL_BATCH ? kadplan::SR_MARK_DIR_BITS_SMALL
                                                                              : kadplan::SR_MARK_DIR_BITS;
        EXPECT(B >= 1 && B <= most && ((1u << B) >= q || B == most) && (B == 1 || (1u << (B - 1)) < q));
        EXPECT(pl.dir.size() == ((size_t)1 << B) + 1 && pl.dir.front() == 0 && pl.dir.back() == q);
        if (B >= 1 && B <= 16 && pl.dir.size() == ((size_t)1 << B) + 1)
            for (size_t s = 0; s + 1 < pl.dir.size(); s++) {
                EXPECT(pl.dir[s] <= pl.dir[s + 1] && pl.dir[s + 1] <= q);
                for (uint32_t j = pl.dir[s]; j < pl.dir[s + 1] && j < q; j++) EXPECT((pl.bkey[j] >> (64 - B)) == s);
            }
    }
    for (uint32_t j = 0; j < q; j++) {
        const uint32_t a = pl.ord[j];
        EXPECT(a < q && !seen[a]);
        if (a >= q) return;
        seen[a] = 1;
        const uint8_t* id = in.ids.data() + 20ull * a;
        EXPECT(pl.bkey[j] == (((uint64_t)be32(id) << 32) | be32(id + 4)));
        for (int w = 0; w < 3; w++) EXPECT(pl.btail[3ull * j + w] == be32(id + 8 + 4 * w));
        EXPECT(pl.bop[j] == ((in.null_clear ? 0 : in.clear[a]) | ((in.null_set ? 0 : in.set[a]) << 2)));
        if (j) EXPECT(std::memcmp(in.ids.data() + 20ull * pl.ord[j - 1], id, 20) < 0);
    }
    for (uint32_t k = 0; k < p; k++) {
        const uint32_t a = pl.pord[k];
        EXPECT(a < p && !pseen[a]);
        if (a >= p) return;
        pseen[a] = 1;
        const uint8_t* id = in.pid.data() + 20ull * a;
        EXPECT(pl.pw[k] == in.pw[a] && pl.pfl[k] == in.pfl[a]);
        EXPECT(pl.pkey[k] == (((uint64_t)be32(id) << 32) | be32(id + 4)));
        for (int w = 0; w < 3; w++) EXPECT(pl.ptail[3ull * k + w] == be32(id + 8 + 4 * w));
        if (k) {
            const uint32_t b = pl.pord[k - 1];
            EXPECT(in.pw[b] < in.pw[a] ||
                   (in.pw[b] == in.pw[a] && std::memcmp(in.pid.data() + 20ull * b, id, 20) < 0));
        }
    }
}

}  // namespace

int main() {
    std::mt19937_64 g(4242);
    kadplan::SrMarkPlan plan;
    std::string msg;
    {  // nothing at all reads nothing
        In in;
        EXPECT(run(in, plan) == KAD_OK && plan.ord.empty() && plan.pord.empty());
        in.S = 9;
        EXPECT(run(in, plan) == KAD_OK);
    }
    const uint8_t masks[6][2] = {{3, 0}, {2, 1}, {0, 3}, {0, 0}, {1, 2}, {0, 2}};
    for (uint32_t S : {1u, 2u, 65u, 5000u}) {
        for (uint32_t q : {0u, 1u, 2u, 63u, 64u, 65u, 1000u, 4096u, 4097u}) {
            for (uint32_t p : {0u, 1u, 2u, 70u}) {
                In in;
                in.S = S;
                in.ids.resize(20ull * q);
                in.clear.resize(q);
                in.set.resize(q);
                for (uint32_t j = 0; j < q; j++) {
                    for (int b = 0; b < 20; b++) in.ids[20ull * j + b] = (uint8_t)g();
                    // runs of equal keys with distinct tails, zero keys, the all-zero ID once
                    if (j && (g() & 3) == 0) std::memcpy(&in.ids[20ull * j], &in.ids[20ull * (j - 1)], 8);
                    if ((g() & 15) == 0) std::memset(&in.ids[20ull * j], 0, 8);
                    const uint8_t* m = masks[g() % 6];
                    in.clear[j] = m[0];
                    in.set[j] = m[1];
                }
                if (q > 5) std::memset(&in.ids[20ull * 5], 0, 20);
                in.pw.resize(p);
                in.pid.resize(20ull * p);
                in.pfl.resize(p);
                for (uint32_t k = 0; k < p; k++) {
                    in.pw[k] = (uint32_t)(g() % S);
                    for (int b = 0; b < 20; b++) in.pid[20ull * k + b] = (uint8_t)g();
                    // the same ID in another search, and the same search with another ID
                    if (k && (g() & 1)) {
                        std::memcpy(&in.pid[20ull * k], &in.pid[20ull * (k - 1)], 20);
                        in.pw[k] = (in.pw[k - 1] + 1) % S;
                        if (S == 1) in.pid[20ull * k + 19] ^= 1;
                    }
                    in.pfl[k] = (uint8_t)(g() & 3);
                }
                // S == 1 with many pairs: make sure no two pairs are equal
                if (S <= 2)
                    for (uint32_t k = 0; k < p; k++) {
                        in.pid[20ull * k] = (uint8_t)k;
                        in.pid[20ull * k + 1] = (uint8_t)(k >> 8);
                    }
                EXPECT(run(in, plan) == KAD_OK);
                check_plan(in, plan);
                for (int nulls = 1; nulls < 4; nulls++) {
                    In n(in);
                    n.null_clear = nulls & 1;
                    n.null_set = (nulls & 2) != 0;
                    EXPECT(run(n, plan) == KAD_OK);
                    check_plan(n, plan);
                }
                // what later checks would refuse, present while an earlier one answers
                In late(in);
                if (q >= 2) std::memcpy(&late.ids[20ull * (q - 1)], &late.ids[0], 20);
                if (p) late.pw[p - 1] = S;
                if (q) {
                    In b(late);
                    b.clear[g() % q] |= (uint8_t)(4u << (g() % 6));
                    b.set[g() % q] = 0x40;
                    if (p) b.pfl[0] = 4;
                    EXPECT(run(b, plan, &msg) == KAD_ERR_INVALID && has(msg, "clear_bits"));
                    b.clear = late.clear;
                    EXPECT(run(b, plan, &msg) == KAD_ERR_INVALID && has(msg, "set_bits"));
                    b.null_clear = true;  // a NULL clear array is not read
                    EXPECT(run(b, plan, &msg) == KAD_ERR_INVALID && has(msg, "set_bits"));
                }
                if (p) {
                    In b(late);
                    b.pfl[g() % p] = (uint8_t)(4u << (g() % 6));
                    if (q) {
                        b.clear[0] = 1;
                        b.set[0] = 1;
                    }
                    EXPECT(run(b, plan, &msg) == KAD_ERR_INVALID && has(msg, "pair_flags"));
                }
                if (q) {
                    In b(late);
                    const uint32_t j = (uint32_t)(g() % q);
                    b.clear[j] = 3;
                    b.set[j] = 2;
                    EXPECT(run(b, plan, &msg) == KAD_ERR_INVALID && has(msg, "both cleared and set"));
                    b.null_set = true;  // nothing is set: accepted up to the later checks
                    const int rc = run(b, plan, &msg);
                    EXPECT(q >= 2 || p ? rc == KAD_ERR_INVALID : rc == KAD_OK);
                }
                if (q >= 2) {
                    EXPECT(run(late, plan, &msg) == KAD_ERR_INVALID && has(msg, "node IDs"));
                    In b(in);  // neighbours in the caller's order, and the first with the last
                    std::memcpy(&b.ids[20ull * 1], &b.ids[0], 20);
                    EXPECT(run(b, plan, &msg) == KAD_ERR_INVALID && has(msg, "node IDs"));
                }
                if (p) {
                    In b(in);
                    b.pw[p - 1] = S;
                    if (p >= 3) {  // two equal pairs as well: the range is reported first
                        b.pw[1] = b.pw[0];
                        std::memcpy(&b.pid[20], &b.pid[0], 20);
                    }
                    EXPECT(run(b, plan, &msg) == KAD_ERR_INVALID && has(msg, "not below S"));
                    b.pw[p - 1] = 0xFFFFFFFFu;
                    EXPECT(run(b, plan, &msg) == KAD_ERR_INVALID && has(msg, "not below S"));
                }
                if (p >= 2) {
                    In b(in);
                    const uint32_t a = (uint32_t)(g() % (p - 1));
                    b.pw[p - 1] = b.pw[a];
                    std::memcpy(&b.pid[20ull * (p - 1)], &b.pid[20ull * a], 20);
                    EXPECT(run(b, plan, &msg) == KAD_ERR_INVALID && has(msg, "are equal"));
                }
            }
        }
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("PASS\n");
    return 0;
}
