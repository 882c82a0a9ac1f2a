// Host plan of a device search set; see kad_searches_plan.h.
#include "kad_searches_plan.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/kadgpu.h"
#include "kad_step.h"

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

int searches_check_erase(uint32_t S, const uint32_t* erase, uint32_t n_erase, std::string& err) {
    for (uint32_t k = 0; k < n_erase; k++)
        if (erase[k] >= S || (k && erase[k] <= erase[k - 1]))
            return fail(err, KAD_ERR_INVALID, "erased searches must be strictly ascending and below S (entry %u)", k);
    return KAD_OK;
}

int searches_apply_plan(uint32_t S, const uint8_t* ids, const uint32_t* erase, uint32_t n_erase, const uint8_t* ins_ids,
                        uint32_t n_ins, SearchesApplyPlan& out, std::string& err) {
    if (int rc = searches_check_erase(S, erase, n_erase, err)) return rc;
    std::vector<uint32_t> ord(n_ins);  // the insert slots in ascending ID order
    for (uint32_t j = 0; j < n_ins; j++) ord[j] = j;
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
        return std::memcmp(ins_ids + 20ull * a, ins_ids + 20ull * b, KAD_HASH_LEN) < 0;
    });
    for (uint32_t k = 1; k < n_ins; k++)
        if (std::memcmp(ins_ids + 20ull * ord[k - 1], ins_ids + 20ull * ord[k], KAD_HASH_LEN) == 0)
            return fail(err, KAD_ERR_INVALID, "inserted search IDs %u and %u are equal", ord[k - 1], ord[k]);
    const size_t S2 = (size_t)S - n_erase + n_ins;
    out.src.clear();
    out.src.reserve(S2);
    out.ids.resize(20 * S2);
    out.remap.assign(S, KAD_NO_NODE);
    out.new_index.assign(n_ins, 0u);
    uint32_t e = 0, k = 0;
    auto emit = [&](const uint8_t* id, uint32_t word) {
        std::memcpy(&out.ids[20 * out.src.size()], id, KAD_HASH_LEN);
        out.src.push_back(word);
    };
    auto emit_new = [&]() {
        out.new_index[ord[k]] = (uint32_t)out.src.size();
        emit(ins_ids + 20ull * ord[k], SRC_NEW | ord[k]);
        k++;
    };
    for (uint32_t s = 0; s < S; s++) {
        if (e < n_erase && erase[e] == s) {
            e++;
            continue;
        }
        const uint8_t* id = ids + 20ull * s;
        int c = 1;
        while (k < n_ins && (c = std::memcmp(ins_ids + 20ull * ord[k], id, KAD_HASH_LEN)) < 0) emit_new();
        if (k < n_ins && c == 0)
            return fail(err, KAD_ERR_INVALID, "inserted search ID %u equals the kept search %u", ord[k], s);
        out.remap[s] = (uint32_t)out.src.size();
        emit(id, s);
    }
    while (k < n_ins) emit_new();
    return KAD_OK;
}

int sr_insert_check(uint32_t S, uint32_t m, const uint32_t* which, const uint32_t* off, const uint8_t* cand_flags,
                    std::string& err) {
    if (m == 0) return KAD_OK;
    for (uint32_t k = 0; k < m; k++)
        if (which[k] >= S || (k && which[k] <= which[k - 1]))
            return fail(err, KAD_ERR_INVALID, "listed searches must be strictly ascending and below S (entry %u)", k);
    if (off[0] != 0) return fail(err, KAD_ERR_INVALID, "candidate offsets must start at 0");
    for (uint32_t k = 0; k < m; k++)
        if (off[k + 1] < off[k]) return fail(err, KAD_ERR_INVALID, "candidate offsets not ascending at %u", k);
    if (off[m] >= 0x7FFFFFFFu) return fail(err, KAD_ERR_INVALID, "too many candidates");
    for (uint32_t j = 0; cand_flags && j < off[m]; j++)
        if (cand_flags[j] & ~KAD_SN_BAD)
            return fail(err, KAD_ERR_INVALID, "candidate %u: only KAD_SN_BAD may be set", j);
    return KAD_OK;
}

namespace {

// bits lo .. hi (inclusive) of the bitmap, a word at a time
bool any_marked(const uint64_t* w, uint32_t lo, uint32_t hi) {
    const uint32_t a = lo >> 6, b = hi >> 6;
    const uint64_t first = ~0ull << (lo & 63u), last = ~0ull >> (63u - (hi & 63u));
    if (a == b) return (w[a] & first & last) != 0;
    if (w[a] & first) return true;
    for (uint32_t i = a + 1; i < b; i++)
        if (w[i]) return true;
    return (w[b] & last) != 0;
}

void mark(uint64_t* w, uint32_t lo, uint32_t hi) {
    const uint32_t a = lo >> 6, b = hi >> 6;
    const uint64_t first = ~0ull << (lo & 63u), last = ~0ull >> (63u - (hi & 63u));
    if (a == b) {
        w[a] |= first & last;
        return;
    }
    w[a] |= first;
    for (uint32_t i = a + 1; i < b; i++) w[i] = ~0ull;
    w[b] |= last;
}

}  // namespace

int sr_round_plan(uint32_t S, uint32_t r, const uint32_t* lb, const uint32_t* fwd, const uint32_t* back,
                  const uint8_t* stop, const uint8_t* trim, SrRoundPlan& out, std::string& err) {
    for (uint32_t k = 0; k < r; k++) {
        const uint32_t fs = stop[k] & 15u, bs = stop[k] >> 4;
        if (fs > KAD_SR_STOP_FAR_EXPIRED || bs > KAD_SR_STOP_FAR_EXPIRED)
            return fail(err, KAD_ERR_INVALID, "candidate %u: unknown stop code", k);
        if (lb[k] > S || fwd[k] > S - lb[k] || back[k] > lb[k])
            return fail(err, KAD_ERR_INVALID, "candidate %u: verdict outside the %u searches", k, S);
        if ((fs != KAD_SR_STOP_END && lb[k] + fwd[k] >= S) || (bs != KAD_SR_STOP_END && back[k] >= lb[k]))
            return fail(err, KAD_ERR_INVALID, "candidate %u: a stop without a search that refused", k);
    }
    out.kind.assign(r, SR_PLAN_SKIPPED);
    out.pair_which.clear();
    out.pair_cand.clear();
    out.pair_want.clear();
    out.ready.clear();
    out.marked.assign(((size_t)S + 63) / 64 + 1, 0ull);
    uint64_t* marked = out.marked.data();
    int64_t block_up = S, block_down = -1;  // searches >= block_up and <= block_down are blocked
    auto is_far = [](uint32_t v) { return v == KAD_SR_STOP_FAR || v == KAD_SR_STOP_FAR_EXPIRED; };
    auto is_open = [](uint32_t v) { return v == KAD_SR_STOP_KNOWN || v == KAD_SR_STOP_FAR_EXPIRED; };
    auto final_stop = [](uint32_t v) { return v == KAD_SR_STOP_END || v == KAD_SR_STOP_FAR; };
    for (uint32_t k = 0; k < r; k++) {
        const uint32_t fs = stop[k] & 15u, bs = stop[k] >> 4;
        const bool ftrim = is_far(fs) && (trim[k] & 1u), btrim = is_far(bs) && (trim[k] & 2u);
        if (fwd[k] + back[k] == 0 && final_stop(fs) && final_stop(bs) && !ftrim && !btrim) continue;
        const int64_t lo = (int64_t)lb[k] - back[k] - (bs == KAD_SR_STOP_END ? 0 : 1);
        const int64_t hi = (int64_t)lb[k] + fwd[k] - (fs == KAD_SR_STOP_END ? 1 : 0);
        if (lo <= hi && hi < block_up && lo > block_down && !any_marked(marked, (uint32_t)lo, (uint32_t)hi)) {
            out.kind[k] = SR_PLAN_READY;
            out.ready.push_back(k);
        } else {
            out.kind[k] = SR_PLAN_DEFERRED;
            if (lo <= hi) {
                if (is_open(fs)) block_up = std::min(block_up, lo);
                if (is_open(bs)) block_down = std::max(block_down, hi);
            }
        }
        // a later candidate is ready only inside (block_down, block_up), and the blocks only tighten: the part of T
        // outside them is never asked for again
        const int64_t mlo = std::max(lo, block_down + 1), mhi = std::min(hi, block_up - 1);
        if (mlo <= mhi) mark(marked, (uint32_t)mlo, (uint32_t)mhi);
    }
    // the ready candidates' T are disjoint: ascending by their first accepting search is ascending by search throughout
    std::sort(out.ready.begin(), out.ready.end(),
              [&](uint32_t a, uint32_t b) { return lb[a] - back[a] < lb[b] - back[b] || (lb[a] - back[a] == lb[b] - back[b] && a < b); });
    for (uint32_t k : out.ready) {
        const uint32_t fs = stop[k] & 15u, bs = stop[k] >> 4;
        auto put = [&](uint32_t s, uint8_t want) {
            out.pair_which.push_back(s);
            out.pair_cand.push_back(k);
            out.pair_want.push_back(want);
        };
        if (is_far(bs) && (trim[k] & 2u)) put(lb[k] - back[k] - 1, 0);
        for (uint32_t s = lb[k] - back[k]; s < lb[k] + fwd[k]; s++) put(s, 1);
        if (is_far(fs) && (trim[k] & 1u)) put(lb[k] + fwd[k], 0);
    }
    return KAD_OK;
}

int sr_mark_plan(uint32_t S, uint32_t q, const uint8_t* node_ids, const uint8_t* clear_bits, const uint8_t* set_bits,
                 uint32_t p, const uint32_t* pair_which, const uint8_t* pair_ids, const uint8_t* pair_flags,
                 SrMarkPlan& out, std::string& err) {
    constexpr uint8_t known = KAD_SN_BAD | KAD_SN_REMOVABLE;
    for (uint32_t j = 0; clear_bits && j < q; j++)
        if (clear_bits[j] & ~known) return fail(err, KAD_ERR_INVALID, "node %u: unknown bit in clear_bits", j);
    for (uint32_t j = 0; set_bits && j < q; j++)
        if (set_bits[j] & ~known) return fail(err, KAD_ERR_INVALID, "node %u: unknown bit in set_bits", j);
    for (uint32_t k = 0; k < p; k++)
        if (pair_flags[k] & ~known) return fail(err, KAD_ERR_INVALID, "pair %u: unknown bit in pair_flags", k);
    for (uint32_t j = 0; clear_bits && set_bits && j < q; j++)
        if (clear_bits[j] & set_bits[j]) return fail(err, KAD_ERR_INVALID, "node %u: a bit both cleared and set", j);
    out.ord.resize(q);
    for (uint32_t j = 0; j < q; j++) out.ord[j] = j;
    // big-endian bytes: memcmp order is (key, tail) order
    std::sort(out.ord.begin(), out.ord.end(), [&](uint32_t a, uint32_t b) {
        return std::memcmp(node_ids + 20ull * a, node_ids + 20ull * b, KAD_HASH_LEN) < 0;
    });
    for (uint32_t j = 1; j < q; j++)
        if (std::memcmp(node_ids + 20ull * out.ord[j - 1], node_ids + 20ull * out.ord[j], KAD_HASH_LEN) == 0)
            return fail(err, KAD_ERR_INVALID, "node IDs %u and %u are equal", out.ord[j - 1], out.ord[j]);
    for (uint32_t k = 0; k < p; k++)
        if (pair_which[k] >= S) return fail(err, KAD_ERR_INVALID, "pair %u: search %u not below S", k, pair_which[k]);
    out.pord.resize(p);
    for (uint32_t k = 0; k < p; k++) out.pord[k] = k;
    std::sort(out.pord.begin(), out.pord.end(), [&](uint32_t a, uint32_t b) {
        if (pair_which[a] != pair_which[b]) return pair_which[a] < pair_which[b];
        return std::memcmp(pair_ids + 20ull * a, pair_ids + 20ull * b, KAD_HASH_LEN) < 0;
    });
    for (uint32_t k = 1; k < p; k++) {
        const uint32_t a = out.pord[k - 1], b = out.pord[k];
        if (pair_which[a] == pair_which[b] && std::memcmp(pair_ids + 20ull * a, pair_ids + 20ull * b, KAD_HASH_LEN) == 0)
            return fail(err, KAD_ERR_INVALID, "pairs %u and %u are equal", a, b);
    }
    out.bkey.resize(q);
    out.btail.resize(3ull * q);
    out.bop.resize(q);
    for (uint32_t j = 0; j < q; j++) {
        const uint32_t a = out.ord[j];
        const uint8_t* id = node_ids + 20ull * a;
        out.bkey[j] = top64(id);
        for (int w = 0; w < 3; w++) out.btail[3ull * j + w] = be32(id + 8 + 4 * w);
        out.bop[j] = (uint8_t)((clear_bits ? clear_bits[a] : 0) | ((set_bits ? set_bits[a] : 0) << 2));
    }
    out.dir.clear();
    out.dbits = 0;
    if (q) {
        const uint32_t most = q <= SR_MARK_SMALL_BATCH ? SR_MARK_DIR_BITS_SMALL : SR_MARK_DIR_BITS;
        uint32_t B = 1;
        while (B < most && (1u << B) < q) B++;
        out.dbits = B;
        out.dir.assign(((size_t)1 << B) + 1, 0u);
        for (uint32_t j = 0; j < q; j++) out.dir[(size_t)(out.bkey[j] >> (64 - B)) + 1]++;
        for (size_t s = 1; s < out.dir.size(); s++) out.dir[s] += out.dir[s - 1];
    }
    out.pw.resize(p);
    out.pkey.resize(p);
    out.ptail.resize(3ull * p);
    out.pfl.resize(p);
    for (uint32_t k = 0; k < p; k++) {
        const uint32_t a = out.pord[k];
        const uint8_t* id = pair_ids + 20ull * a;
        out.pw[k] = pair_which[a];
        out.pkey[k] = top64(id);
        for (int w = 0; w < 3; w++) out.ptail[3ull * k + w] = be32(id + 8 + 4 * w);
        out.pfl[k] = pair_flags[a];
    }
    return KAD_OK;
}

namespace {
// sr_entries_plan and sr_due_plan: the same plan over the bits `known`, named `what` in the errors
int entries_plan_over(uint8_t known, const char* what, uint32_t S, uint32_t p, const uint32_t* pair_which,
                      const uint8_t* pair_ids, const uint8_t* clear_bits, const uint8_t* set_bits, SrEntriesPlan& out,
                      std::string& err) {
    for (uint32_t k = 0; clear_bits && k < p; k++)
        if (clear_bits[k] & ~known) return fail(err, KAD_ERR_INVALID, "pair %u: clear_bits outside the %s bits", k, what);
    for (uint32_t k = 0; set_bits && k < p; k++)
        if (set_bits[k] & ~known) return fail(err, KAD_ERR_INVALID, "pair %u: set_bits outside the %s bits", k, what);
    for (uint32_t k = 0; clear_bits && set_bits && k < p; k++)
        if (clear_bits[k] & set_bits[k]) return fail(err, KAD_ERR_INVALID, "pair %u: a bit both cleared and set", k);
    for (uint32_t k = 0; k < p; k++)
        if (pair_which[k] >= S) return fail(err, KAD_ERR_INVALID, "pair %u: search %u not below S", k, pair_which[k]);
    out.pord.resize(p);
    for (uint32_t k = 0; k < p; k++) out.pord[k] = k;
    std::sort(out.pord.begin(), out.pord.end(), [&](uint32_t a, uint32_t b) {
        if (pair_which[a] != pair_which[b]) return pair_which[a] < pair_which[b];
        return std::memcmp(pair_ids + 20ull * a, pair_ids + 20ull * b, KAD_HASH_LEN) < 0;
    });
    for (uint32_t k = 1; k < p; k++) {
        const uint32_t a = out.pord[k - 1], b = out.pord[k];
        if (pair_which[a] == pair_which[b] && std::memcmp(pair_ids + 20ull * a, pair_ids + 20ull * b, KAD_HASH_LEN) == 0)
            return fail(err, KAD_ERR_INVALID, "pairs %u and %u are equal", a, b);
    }
    out.pw.resize(p);
    out.pkey.resize(p);
    out.ptail.resize(3ull * p);
    out.pclear.resize(p);
    out.pset.resize(p);
    for (uint32_t k = 0; k < p; k++) {
        const uint32_t a = out.pord[k];
        const uint8_t* id = pair_ids + 20ull * a;
        out.pw[k] = pair_which[a];
        out.pkey[k] = top64(id);
        for (int w = 0; w < 3; w++) out.ptail[3ull * k + w] = be32(id + 8 + 4 * w);
        out.pclear[k] = clear_bits ? clear_bits[a] : (uint8_t)0;
        out.pset[k] = set_bits ? set_bits[a] : (uint8_t)0;
    }
    return KAD_OK;
}
}  // namespace

int sr_entries_plan(uint32_t S, uint32_t p, const uint32_t* pair_which, const uint8_t* pair_ids, const uint8_t* clear_bits,
                    const uint8_t* set_bits, SrEntriesPlan& out, std::string& err) {
    return entries_plan_over((uint8_t)kadstep::ENTRY_BITS, "step", S, p, pair_which, pair_ids, clear_bits, set_bits, out, err);
}

int sr_due_plan(uint32_t S, uint32_t p, const uint32_t* pair_which, const uint8_t* pair_ids, const uint8_t* clear_bits,
                const uint8_t* set_bits, SrEntriesPlan& out, std::string& err) {
    return entries_plan_over((uint8_t)kadstep::DUE_BITS, "due", S, p, pair_which, pair_ids, clear_bits, set_bits, out, err);
}

int sr_step_check(uint32_t S, uint32_t m, const uint32_t* which, const uint8_t* mode, std::string& err) {
    if (!which && m != S) return fail(err, KAD_ERR_INVALID, "which == NULL steps every search: m must be S");
    for (uint32_t k = 0; which && k < m; k++)
        if (which[k] >= S || (k && which[k] <= which[k - 1]))
            return fail(err, KAD_ERR_INVALID, "stepped searches must be strictly ascending and below S");
    for (uint32_t k = 0; mode && k < m; k++)
        if (mode[k] & ~kadstep::MODE_BITS) return fail(err, KAD_ERR_INVALID, "search %u: unknown mode bit", k);
    return KAD_OK;
}

int sr_step_full_check(uint32_t S, uint32_t m, const uint32_t* which, const uint8_t* mode, std::string& err) {
    if (int rc = sr_step_check(S, m, which, nullptr, err)) return rc;
    for (uint32_t k = 0; mode && k < m; k++)
        if (!kadstep::full_mode_ok(mode[k])) return fail(err, KAD_ERR_INVALID, "search %u: invalid mode 0x%02x", k, mode[k]);
    return KAD_OK;
}

}  // namespace kadplan

namespace {
// the flag bytes of a list of n <= 64 entries four at a time, as the kernel's words hold them: entry 4i + b is byte b
// of w[i], zero from n on
void flag_words(uint32_t n, const uint8_t* node_flags, uint32_t (&w)[16]) {
    for (uint32_t i = 0; i < 16; i++) w[i] = 0;
    for (uint32_t e = 0; e < n; e++) w[e / 4u] |= (uint32_t)node_flags[e] << (8u * (e % 4u));
}

bool step_mode_ok(uint32_t mode) { return !(mode & ~kadstep::MODE_BITS); }

// kad_search_step_batch and kad_search_step_full_batch: `step` on every list of the CSR, after every list and mode passed
template <class Out>
int step_lists(uint32_t m, const uint32_t* off, const uint8_t* node_flags, const uint8_t* search_flags, const uint8_t* mode,
               Out* out, bool (*mode_ok)(uint32_t), int (*step)(uint32_t, const uint8_t*, uint32_t, uint32_t, Out*)) {
    if (m == 0) return KAD_OK;
    if (!off || !out || (off[m] && !node_flags)) return KAD_ERR_INVALID;
    for (uint32_t k = 0; k < m; k++)
        if (off[k + 1] < off[k] || off[k + 1] - off[k] > 64u || (mode && !mode_ok(mode[k]))) return KAD_ERR_INVALID;
    for (uint32_t k = 0; k < m; k++)
        if (int rc = step(off[k + 1] - off[k], node_flags + off[k], search_flags ? search_flags[k] : 0u, mode ? mode[k] : 0u,
                          out + k))
            return rc;
    return KAD_OK;
}
}  // namespace

extern "C" int kad_search_step_full(uint32_t n, const uint8_t* node_flags, uint32_t search_flags, uint32_t mode,
                                    kad_step_full_out* out) {
    if ((n && !node_flags) || !out || n > 64u || !kadstep::full_mode_ok(mode)) return KAD_ERR_INVALID;
    uint32_t w[16];
    flag_words(n, node_flags, w);
    kadstep::PlanesFull P;
    for (uint32_t i = 0; i < 16; i++) kadstep::add_word_full(P, w[i], i);
    const kadstep::DecisionFull d = kadstep::decide_full(P, n, (search_flags & KAD_SR_EXPIRED) != 0, mode);
    out->picks = d.picks;
    out->listen = d.listen;
    out->announce = d.announce;
    out->counts = d.counts;
    out->bits = d.bits;
    return KAD_OK;
}

extern "C" int kad_search_step_full_batch(uint32_t m, const uint32_t* off, const uint8_t* node_flags,
                                          const uint8_t* search_flags, const uint8_t* mode, kad_step_full_out* out) {
    return step_lists(m, off, node_flags, search_flags, mode, out, kadstep::full_mode_ok, kad_search_step_full);
}

extern "C" int kad_search_step(uint32_t n, const uint8_t* node_flags, uint32_t search_flags, uint32_t mode,
                               kad_step_out* out) {
    if ((n && !node_flags) || !out || n > 64u || !step_mode_ok(mode)) return KAD_ERR_INVALID;
    uint32_t w[16];
    flag_words(n, node_flags, w);
    kadstep::Planes P;
    for (uint32_t i = 0; i < 16; i++) kadstep::add_word(P, w[i], i);
    const kadstep::Decision d = kadstep::decide(P, n, (search_flags & KAD_SR_EXPIRED) != 0, mode);
    out->picks = d.picks;
    out->counts = d.counts;
    out->bits = d.bits;
    return KAD_OK;
}

extern "C" int kad_search_step_batch(uint32_t m, const uint32_t* off, const uint8_t* node_flags,
                                     const uint8_t* search_flags, const uint8_t* mode, kad_step_out* out) {
    return step_lists(m, off, node_flags, search_flags, mode, out, step_mode_ok, kad_search_step);
}

extern "C" int kad_search_trim(uint32_t n, const uint8_t* node_flags, uint32_t search_flags, uint32_t* full,
                               uint32_t* t) {
    if ((n && !node_flags) || !full || !t) return KAD_ERR_INVALID;
    kadplan::search_trim(n, node_flags, search_flags, full, t);
    return KAD_OK;
}

extern "C" int kad_sr_plan_round(uint32_t S, uint32_t r, const uint32_t* lb, const uint32_t* fwd, const uint32_t* back,
                                 const uint8_t* stop, const uint8_t* trim, uint8_t* out_kind, uint32_t* out_pair_which,
                                 uint32_t* out_pair_cand, uint8_t* out_pair_want, uint32_t* out_n_pairs) {
    if (!out_n_pairs || (r && (!lb || !fwd || !back || !stop || !trim || !out_kind))) return KAD_ERR_INVALID;
    if (S && r && (!out_pair_which || !out_pair_cand || !out_pair_want)) return KAD_ERR_INVALID;
    *out_n_pairs = 0;
    kadplan::SrRoundPlan plan;
    std::string err;
    try {
        if (int rc = kadplan::sr_round_plan(S, r, lb, fwd, back, stop, trim, plan, err)) return rc;
    } catch (const std::bad_alloc&) {
        return KAD_ERR_NOMEM;
    }
    const size_t n = plan.pair_which.size();
    if (r) std::memcpy(out_kind, plan.kind.data(), r);
    if (n) {
        std::memcpy(out_pair_which, plan.pair_which.data(), 4 * n);
        std::memcpy(out_pair_cand, plan.pair_cand.data(), 4 * n);
        std::memcpy(out_pair_want, plan.pair_want.data(), n);
    }
    *out_n_pairs = (uint32_t)n;
    return KAD_OK;
}
