// kad_maint_scan_host and kadmaint::kind_of (opendht_amd/csrc/kad_maint_host.cpp, kad_maint_kind.h) under ASan + UBSan:
// every array has exactly the size the call documents (heap vectors, so a read or write past the end is caught), for
// every B from 0 to 70, against the loops of Dht::bucketMaintenance written out here: the body of dht.cpp:2838-2850 run
// under all four outcomes of the two trials, and InfoHash::lowbit byte by byte.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../opendht_amd/csrc/kad_maint_kind.h"
#include "kadgpu.h"

static int lowbit_bytes(const uint8_t* h) {
    int i, j;
    for (i = 19; i >= 0; i--)
        if (h[i] != 0) break;
    if (i < 0) return -1;
    for (j = 7; j >= 0; j--)
        if ((h[i] & (0x80 >> j)) != 0) break;
    return 8 * i + j;
}

static bool body(const std::vector<uint32_t>& w, uint32_t b, bool t1, bool t2) {
    const uint32_t B = (uint32_t)w.size();
    uint32_t q = b;
    if (b + 1 != B && (w[q] == 0 || t1)) q = b + 1;
    if (b != 0 && (w[q] == 0 || t2)) {
        const uint32_t r = b - 1;
        if (w[r] != 0) q = r;
    }
    return w[q] != 0;
}

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            return 1;                                                  \
        }                                                              \
    } while (0)

int main() {
    std::mt19937_64 rng(0x6D61696E74ull);
    const int64_t now = 1000000000000000ll;
    uint64_t records = 0;
    for (uint32_t B = 0; B <= 70; B++) {
        for (int rep = 0; rep < 6; rep++) {
            std::vector<uint32_t> w(B), off(B + 1, 0);
            std::vector<uint8_t> first(20ull * B);
            std::vector<int64_t> tm(B);
            for (uint32_t b = 0; b < B; b++) {
                w[b] = (rng() % 3 == 0) ? 0u : (uint32_t)(rng() % 40);
                off[b + 1] = off[b] + w[b];
                const unsigned r = (unsigned)(rng() % 4);
                tm[b] = r == 0 ? INT64_MIN : r == 1 ? now - KAD_MAINT_STALE_NS : r == 2 ? now - KAD_MAINT_STALE_NS - 1 : now;
                // firsts with their lowest set bit anywhere, the all-zero one included
                uint8_t* f = first.data() + 20ull * b;
                const unsigned bit = (unsigned)(rng() % 161);
                for (unsigned x = 0; x < 20; x++) f[x] = bit ? (uint8_t)rng() : 0;
                if (bit) {
                    const unsigned p = bit - 1;
                    f[p / 8] = (uint8_t)((f[p / 8] | (0x80 >> (p % 8))) & (0xFF00 >> (p % 8 + 1)));
                    for (unsigned x = p / 8 + 1; x < 20; x++) f[x] = 0;
                    CHECK(lowbit_bytes(f) == (int)p);
                }
                CHECK(kadmaint::lowbit(kadmaint::first_of(f)) == lowbit_bytes(f));
            }
            // the expected records
            std::vector<kad_maint_rec> want;
            kad_maint_totals wt = {0, 0, 0, 0, 0, 0, 0xFFFFFFFFu, 0};
            const uint32_t fb = B ? (uint32_t)(rng() % (B + 1)) * (rep & 1) : 0;
            for (uint32_t b = fb; b < B; b++) {
                const bool stale = tm[b] < now - KAD_MAINT_STALE_NS;
                if (!(stale || w[b] == 0)) continue;
                uint32_t k = (stale ? 1u : 0u) | (w[b] == 0 ? 2u : 0u);
                if (b + 1 < B) k |= 4u | (w[b + 1] == 0 ? 8u : 0u);
                if (b > 0) k |= 16u | (w[b - 1] == 0 ? 32u : 0u);
                int yes = 0;
                for (int o = 0; o < 4; o++) yes += body(w, b, o & 1, o & 2) ? 1 : 0;
                const uint32_t cls = yes == 4 ? 2u : yes ? 1u : 0u;
                const int b1 = lowbit_bytes(first.data() + 20ull * b);
                const int b2 = b + 1 < B ? lowbit_bytes(first.data() + 20ull * (b + 1)) : -1;
                k |= cls << 6 | (uint32_t)((b1 > b2 ? b1 : b2) + 1) << 8;
                want.push_back({b, k});
                wt.candidates++;
                wt.stale += stale;
                wt.empty += w[b] == 0;
                wt.sure += cls == 2;
                wt.maybe += cls == 1;
                wt.never += cls == 0;
                if (cls == 2 && wt.first_sure == 0xFFFFFFFFu) wt.first_sure = b;
            }
            // exact-size outputs at several caps
            const uint32_t count = (uint32_t)want.size();
            for (uint32_t cap : {0u, 1u, count ? count - 1 : 0u, count, count + 1}) {
                std::vector<kad_maint_rec> out(cap);
                std::vector<kad_maint_totals> tot(1);
                std::memset(tot.data(), 0xAA, sizeof(kad_maint_totals));
                const int rc = kad_maint_scan_host(B, B ? off.data() : nullptr, B ? first.data() : nullptr,
                                                   (rep % 3 == 2) ? nullptr : tm.data(), now, fb, tot.data(),
                                                   cap ? out.data() : nullptr, cap);
                CHECK(rc == KAD_OK);
                if (rep % 3 == 2) continue;  // no times: every bucket stale; checked by the Python model tests
                CHECK(std::memcmp(tot.data(), &wt, sizeof wt) == 0);
                const uint32_t m = cap < count ? cap : count;
                CHECK(m == 0 || std::memcmp(out.data(), want.data(), 8ull * m) == 0);
                records += m;
            }
            if (B) {
                std::vector<kad_maint_totals> tot(1);
                CHECK(kad_maint_scan_host(B, off.data(), first.data(), tm.data(), now, B + 1, tot.data(), nullptr, 0) ==
                      KAD_ERR_INVALID);
                CHECK(kad_maint_scan_host(B, off.data(), first.data(), tm.data(), INT64_MIN + KAD_MAINT_STALE_NS - 1, 0,
                                          tot.data(), nullptr, 0) == KAD_ERR_INVALID);
                CHECK(kad_maint_scan_host(B, off.data(), first.data(), tm.data(), INT64_MIN + KAD_MAINT_STALE_NS, 0,
                                          tot.data(), nullptr, 0) == KAD_OK);
            }
        }
    }
    CHECK(records > 5000);
    std::printf("PASS %llu records\n", (unsigned long long)records);
    return 0;
}
