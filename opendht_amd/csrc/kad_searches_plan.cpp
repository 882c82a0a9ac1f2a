// Host plan of a device search set; see kad_searches_plan.h.
#include "kad_searches_plan.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../include/kadgpu.h"

namespace kadplan {
namespace {

int fail(std::string& err, int code, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

uint32_t be32(const uint8_t* p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

uint64_t top64(const uint8_t* p) { return ((uint64_t)be32(p) << 32) | be32(p + 4); }

// InfoHash::xorCmp (infohash.h): <0 if a is closer to self than b, 0 if equal, >0 otherwise.
int xor_cmp(const uint8_t* self, const uint8_t* a, const uint8_t* b) {
    for (uint32_t i = 0; i < KAD_HASH_LEN; i++) {
        const uint8_t x = a[i] ^ self[i], y = b[i] ^ self[i];
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}

}  // namespace

void search_trim(uint32_t n, const uint8_t* node_flags, uint32_t search_flags, uint32_t* full, uint32_t* t) {
    uint32_t f, tt;
    if (search_flags & KAD_SR_EXPIRED) {  // trim to SEARCH_NODES nodes (dht.cpp:992-997)
        f = n >= KAD_SEARCH_NODES;
        tt = f ? KAD_SEARCH_NODES : n;
    } else {  // trim to SEARCH_NODES nodes, not counting bad nodes (dht.cpp:998-1006)
        uint32_t bad = 0;
        for (uint32_t i = 0; i < n; i++) bad += (node_flags[i] & KAD_SN_BAD) ? 1u : 0u;
        f = n - bad >= KAD_SEARCH_NODES;
        tt = n;
        while (tt - bad > KAD_SEARCH_NODES) {
            --tt;
            if (node_flags[tt] & KAD_SN_BAD) --bad;
        }
    }
    *full = f;
    *t = tt;
}

int searches_check_ids(uint32_t S, const uint8_t* ids, std::string& err) {
    for (uint32_t s = 1; s < S; s++)
        if (std::memcmp(ids + 20ull * (s - 1), ids + 20ull * s, KAD_HASH_LEN) >= 0)
            return fail(err, KAD_ERR_INVALID, "search IDs not strictly ascending at %u", s);
    return KAD_OK;
}

int searches_plan(uint32_t m, uint32_t cap, const uint8_t* ids, const uint8_t* flags, const uint32_t* off,
                  const uint8_t* node_ids, const uint8_t* node_flags, SearchesPlan& out, std::string& err) {
    for (uint32_t s = 0; s < m; s++) {
        if (off[s + 1] < off[s]) return fail(err, KAD_ERR_INVALID, "list offsets not ascending at %u", s);
        const uint8_t* self = ids + 20ull * s;
        for (uint32_t j = off[s] + 1; j < off[s + 1]; j++)
            if (xor_cmp(self, node_ids + 20ull * (j - 1), node_ids + 20ull * j) >= 0)
                return fail(err, KAD_ERR_INVALID, "list %u not strictly ascending in distance at entry %u", s,
                            j - off[s]);
    }
    for (uint32_t s = 0; s < m; s++)
        if (off[s + 1] - off[s] > cap)
            return fail(err, KAD_ERR_UNSUPPORTED, "list %u holds %u entries, cap is %u", s, off[s + 1] - off[s], cap);
    out.rec.assign((size_t)m * SREC_WORDS, 0u);
    out.mkey.assign((size_t)m * cap, 0ull);
    out.mtail.assign((size_t)m * cap * 3, 0u);
    out.mflag.assign((size_t)m * cap, 0);
    for (uint32_t s = 0; s < m; s++) {
        const uint32_t n = off[s + 1] - off[s];
        const uint8_t* nid = node_ids + 20ull * off[s];
        const uint8_t* nfl = node_flags + off[s];
        for (uint32_t j = 0; j < n; j++) {
            const size_t e = (size_t)s * cap + j;
            out.mkey[e] = top64(nid + 20ull * j);
            for (int k = 0; k < 3; k++) out.mtail[3 * e + k] = be32(nid + 20ull * j + 8 + 4 * k);
            out.mflag[e] = nfl[j];
        }
        uint32_t full = 0, t = 0;
        search_trim(n, nfl, flags[s], &full, &t);
        uint32_t* r = out.rec.data() + (size_t)s * SREC_WORDS;
        const uint64_t k = top64(ids + 20ull * s);
        std::memcpy(r, &k, 8);
        for (int w = 0; w < 3; w++) r[2 + w] = be32(ids + 20ull * s + 8 + 4 * w);
        r[SREC_N] = n;
        if (t) {
            const uint64_t tk = top64(nid + 20ull * (t - 1));
            std::memcpy(r + SREC_THR, &tk, 8);
            for (int w = 0; w < 3; w++) r[SREC_THR + 2 + w] = be32(nid + 20ull * (t - 1) + 8 + 4 * w);
        }
        r[SREC_T] = t;
        r[SREC_BITS] = (full ? SREC_FULL : 0u) | ((flags[s] & KAD_SR_EXPIRED) ? SREC_EXPIRED : 0u);
    }
    return KAD_OK;
}

}  // namespace kadplan

extern "C" int kad_search_trim(uint32_t n, const uint8_t* node_flags, uint32_t search_flags, uint32_t* full,
                               uint32_t* t) {
    if ((n && !node_flags) || !full || !t) return KAD_ERR_INVALID;
    kadplan::search_trim(n, node_flags, search_flags, full, t);
    return KAD_OK;
}
