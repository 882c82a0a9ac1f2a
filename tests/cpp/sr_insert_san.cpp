// The list checks of kad_sr_insert (kadplan::sr_insert_check, opendht_amd/csrc/kad_searches_plan.cpp) under
// AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, compiled together with the plan file by
// tests/test_sr_insert_san.py. Every array is an exact-size copy, so a read past any input is a report; accepted and
// rejected inputs in the order the header documents: which, then the offsets, then the flag bytes.
#include <cstdint>
#include <cstdio>
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

int run(uint32_t S, const std::vector<uint32_t>& which, const std::vector<uint32_t>& off,
        const std::vector<uint8_t>* flags, std::string* msg = nullptr) {
    const std::vector<uint32_t> w(which), o(off);  // exact-size copies
    std::vector<uint8_t> f;
    if (flags) f = *flags;
    std::string err;
    const int rc = kadplan::sr_insert_check(S, (uint32_t)w.size(), w.data(), o.data(), flags ? f.data() : nullptr, err);
    EXPECT((rc == KAD_OK) == err.empty());
    if (msg) *msg = err;
    return rc;
}

bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

}  // namespace

int main() {
    std::mt19937_64 g(777);
    std::string err, msg;
    // m == 0 reads nothing
    EXPECT(kadplan::sr_insert_check(0, 0, nullptr, nullptr, nullptr, err) == KAD_OK);
    EXPECT(kadplan::sr_insert_check(5, 0, nullptr, nullptr, nullptr, err) == KAD_OK && err.empty());
    for (uint32_t S : {1u, 2u, 63u, 64u, 65u, 300u, 5000u}) {
        for (int round = 0; round < 40; round++) {
            std::vector<uint32_t> which;
            for (uint32_t s = 0; s < S; s++)
                if (round == 0 || (g() % 3) == 0) which.push_back(s);
            if (which.empty()) which.push_back(S - 1);
            const uint32_t m = (uint32_t)which.size();
            std::vector<uint32_t> off(m + 1, 0);
            for (uint32_t k = 0; k < m; k++) off[k + 1] = off[k] + (uint32_t)((g() & 3) ? g() % 4 : g() % 131);
            std::vector<uint8_t> flags(off[m]);
            for (auto& b : flags) b = (uint8_t)(g() & 1);
            EXPECT(run(S, which, off, &flags) == KAD_OK);
            EXPECT(run(S, which, off, nullptr) == KAD_OK);
            EXPECT(run(S, which, std::vector<uint32_t>(m + 1, 0), nullptr) == KAD_OK);  // every list empty
            // which: out of range, repeated, descending; reported before bad offsets and flags
            std::vector<uint32_t> bad_off(off);
            bad_off[0] = 1;
            std::vector<uint8_t> bad_flags(flags);
            if (!bad_flags.empty()) bad_flags[g() % bad_flags.size()] |= (uint8_t)(2u << (g() % 7));
            std::vector<uint32_t> w(which);
            w[m - 1] = S;
            EXPECT(run(S, w, bad_off, &bad_flags, &msg) == KAD_ERR_INVALID && has(msg, "below S"));
            w[m - 1] = 0xFFFFFFFFu;
            EXPECT(run(S, w, off, &flags, &msg) == KAD_ERR_INVALID && has(msg, "below S"));
            if (m >= 2) {
                w = which;
                w[m - 1] = w[m - 2];
                EXPECT(run(S, w, bad_off, &bad_flags, &msg) == KAD_ERR_INVALID && has(msg, "ascending"));
                w = which;
                std::swap(w[0], w[m - 1]);
                EXPECT(run(S, w, off, &flags, &msg) == KAD_ERR_INVALID && has(msg, "ascending"));
            }
            // offsets: not starting at 0, descending, too many; reported before bad flags
            EXPECT(run(S, which, bad_off, &bad_flags, &msg) == KAD_ERR_INVALID && has(msg, "start at 0"));
            if (off[m] > 0) {
                std::vector<uint32_t> o(off);
                uint32_t k = 1;
                while (o[k] == 0) k++;
                o[k - 1] = o[k] + 1;  // off[k-1] > off[k]
                if (k - 1 == 0) {
                    EXPECT(run(S, which, o, &bad_flags, &msg) == KAD_ERR_INVALID && has(msg, "start at 0"));
                } else {
                    EXPECT(run(S, which, o, &bad_flags, &msg) == KAD_ERR_INVALID && has(msg, "not ascending"));
                }
            }
            {
                std::vector<uint32_t> o(off);
                o[m] = 0x7FFFFFFFu;  // never read as a length: the flags stay NULL-sized
                EXPECT(run(S, which, o, nullptr, &msg) == KAD_ERR_INVALID && has(msg, "too many"));
                o[m] = 0xFFFFFFFFu;
                EXPECT(run(S, which, o, nullptr, &msg) == KAD_ERR_INVALID && has(msg, "too many"));
            }
            // flags: any bit other than KAD_SN_BAD, anywhere
            if (!flags.empty()) {
                EXPECT(run(S, which, off, &bad_flags, &msg) == KAD_ERR_INVALID && has(msg, "KAD_SN_BAD"));
                std::vector<uint8_t> f(flags);
                f.back() = 0x80;
                EXPECT(run(S, which, off, &f, &msg) == KAD_ERR_INVALID && has(msg, "KAD_SN_BAD"));
                f = flags;
                f.front() = KAD_SN_REMOVABLE;
                EXPECT(run(S, which, off, &f, &msg) == KAD_ERR_INVALID && has(msg, "KAD_SN_BAD"));
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
