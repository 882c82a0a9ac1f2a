// Dht::searchStep's decision on one search's list (dht.cpp:1344-1464), DESIGN.md §7.19: written once, over bit planes
// of the member flag bytes, for the host (kad_search_step) and for step_lane of kad_searches.hip (the body of step_kernel
// and step_full_kernel), which call the same functions. Plain C++ without a loop over the entries: popcounts,
// trailing-zero counts and a fixed number of lowest-bit removals. No HIP call and no header beyond <cstdint>, so the CPU
// sanitizer build compiles it alone.
// decide_full adds the listen loop and the announce probes of a synced search over two more planes and
// hands the get loop to decide; kad_search_step_full and step_lane<WIDE, true> call it.
#pragma once

#include <cstdint>

#include "../../include/kadgpu.h"

#if defined(__HIPCC__)
#define KAD_STEP_HD __host__ __device__ __forceinline__
#else
#define KAD_STEP_HD inline
#endif

namespace kadstep {

constexpr uint32_t TARGET_NODES = 8;                // dht.h: Search::isSynced looks at the first 8 live nodes
constexpr uint32_t MAX_REQUESTED_SEARCH_NODES = 4;  // dht.h:316, searchSendGetValues' alpha
constexpr uint32_t SEARCH_MAX_BAD_NODES = 25;       // dht.h:324
constexpr uint32_t MODE_BITS = KAD_STEP_APPLY | KAD_STEP_NO_SEND | KAD_STEP_DONE_IF_SYNCED | KAD_STEP_NO_EXPIRE;
constexpr uint32_t ENTRY_BITS = KAD_SN_CANDIDATE | KAD_SN_PENDING | KAD_SN_SYNCED | KAD_SN_NOGET;

// bit e of a plane = that bit of entry e's flag byte
struct Planes {
    uint64_t bad = 0, cand = 0, pend = 0, sync = 0, noget = 0;
};

struct Decision {
    uint64_t picks;
    uint32_t counts;  // n | bad << 8 | lead_bad << 16 | solicited << 24
    uint32_t bits;    // KAD_STEP_SKIPPED .. KAD_STEP_EXPIRE
};

// bit `b` of the four bytes of w as four adjacent bits (byte 0 first)
KAD_STEP_HD uint64_t gather4(uint32_t w, uint32_t b) {
    return (uint64_t)((((w >> b) & 0x01010101u) * 0x01020408u) >> 24) & 15ull;
}

// four adjacent bits as the lowest bit of four bytes (bit 0 to byte 0)
KAD_STEP_HD uint32_t spread4(uint32_t p4) { return ((p4 & 15u) * 0x00204081u) & 0x01010101u; }

// the flag bytes of entries 4i .. 4i+3, little-endian in w, added to the planes (i < 16)
KAD_STEP_HD void add_word(Planes& P, uint32_t w, uint32_t i) {
    const uint32_t sh = 4u * i;
    P.bad |= gather4(w, 0) << sh;
    P.cand |= gather4(w, 2) << sh;
    P.pend |= gather4(w, 3) << sh;
    P.sync |= gather4(w, 4) << sh;
    P.noget |= gather4(w, 5) << sh;
}

KAD_STEP_HD uint32_t pop64(uint64_t v) { return (uint32_t)__builtin_popcountll(v); }

// v without its k lowest set bits, k <= 8
KAD_STEP_HD uint64_t drop_lowest(uint64_t v, uint32_t k) {
#if defined(__clang__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 8; i++)
        if (i < k) v &= v - 1;
    return v;
}

// The step of a list of n <= 64 entries; planes may hold anything at or past n.
KAD_STEP_HD Decision decide(Planes P, uint32_t n, bool expired, uint32_t mode) {
    const uint64_t valid = n >= 64u ? ~0ull : (1ull << n) - 1ull;
    const uint64_t bad = P.bad & valid, good = ~P.bad & valid;
    const uint32_t n_bad = pop64(bad);
    const uint32_t lead = ~bad ? (uint32_t)__builtin_ctzll(~bad) : 64u;  // <= n: bit n of ~bad is set when n < 64
    uint32_t solicited = pop64(good & P.pend);
    Decision d = {0ull, 0u, 0u};
    if (expired) {  // :1346
        d.bits = KAD_STEP_SKIPPED;
    } else {
        if (n - n_bad < KAD_SEARCH_NODES) d.bits |= KAD_STEP_SHORT;  // :1354
        // Search::isSynced (:1467-1478): the first TARGET_NODES entries that are not BAD all carry SYNCED
        const uint64_t first = good & ~drop_lowest(good, TARGET_NODES);
        const bool synced = good && !(first & ~P.sync);
        if (synced) d.bits |= KAD_STEP_SYNCED;
        const bool done = synced && (mode & KAD_STEP_DONE_IF_SYNCED);
        if (done) d.bits |= KAD_STEP_DONE;  // setDone (:1434-1435) makes :1173 return
        if (solicited < MAX_REQUESTED_SEARCH_NODES && !(mode & KAD_STEP_NO_SEND) && !done) {  // :1438-1446
            // gg: the picks that raise currentlySolicitedNodeCount. An entry that is not BAD and already PENDING (a
            // request for another query is in flight) is counted before it is picked, and its pick adds nothing.
            const uint64_t gettable = ~P.noget & (~P.bad | P.cand) & valid, gg = gettable & good & ~P.pend;
            const uint32_t room = MAX_REQUESTED_SEARCH_NODES - solicited;
            if (pop64(gg) < room) {  // the loop ends on a searchSendGetValues that finds no node
                d.picks = gettable;
                d.bits |= KAD_STEP_EXHAUSTED;
            } else {  // it ends right after the room-th pick that counts
                const uint64_t at = drop_lowest(gg, room - 1u);  // its lowest bit is that pick
                d.picks = gettable & (at ^ (at - 1ull));
            }
            solicited += pop64(d.picks & gg);
        }
        if (lead >= (n < SEARCH_MAX_BAD_NODES ? n : SEARCH_MAX_BAD_NODES)) d.bits |= KAD_STEP_EXPIRE;  // :1451-1452
    }
    d.counts = n | (n_bad << 8) | (lead << 16) | (solicited << 24);
    return d;
}

// ---- the whole searchStep: the listen loop (:1384-1428) and the announce probes (:1244-1338) before the get loop, §7.20
constexpr uint32_t LISTEN_NODES = 4;  // dht.h: the listen loop ends after the fourth synced non-candidate node
constexpr uint32_t FULL_MODE_BITS = MODE_BITS | KAD_STEP_LISTEN | KAD_STEP_ANNOUNCE | KAD_STEP_PROBE_BLOCKS;
constexpr uint32_t DUE_BITS = KAD_SN_LISTEN_DUE | KAD_SN_ANNOUNCE_DUE;

// DONE_IF_SYNCED says "no listeners, no announces"; PROBE_BLOCKS speaks of the announce probes
KAD_STEP_HD bool full_mode_ok(uint32_t mode) {
    if (mode & ~FULL_MODE_BITS) return false;
    if ((mode & KAD_STEP_DONE_IF_SYNCED) && (mode & (KAD_STEP_LISTEN | KAD_STEP_ANNOUNCE))) return false;
    return !(mode & KAD_STEP_PROBE_BLOCKS) || (mode & KAD_STEP_ANNOUNCE);
}

// Planes with the two due bits beside them
struct PlanesFull {
    Planes p;
    uint64_t ldue = 0, adue = 0;
};

struct DecisionFull {
    uint64_t picks, listen, announce;
    uint32_t counts;  // as Decision; solicited after all three loops
    uint32_t bits;
};

KAD_STEP_HD void add_word_full(PlanesFull& P, uint32_t w, uint32_t i) {
    add_word(P.p, w, i);
    P.ldue |= gather4(w, 6) << (4u * i);
    P.adue |= gather4(w, 7) << (4u * i);
}

// the byte mask that gives entries 4i .. 4i+3 of a flag word `bits` where they are in mask
KAD_STEP_HD uint32_t mask_bytes(uint64_t mask, uint32_t i, uint32_t bits) {
    return spread4((uint32_t)(mask >> (4u * i))) * bits;
}

// Everything up to and including the k-th set bit of v (1 <= k <= 8); all ones if v has fewer than k.
KAD_STEP_HD uint64_t reach_of(uint64_t v, uint32_t k) {
    const uint64_t at = drop_lowest(v, k - 1u);  // its lowest bit is the k-th
    return at ? at ^ (at - 1ull) : ~0ull;
}

// The step of a list of n <= 64 entries with its listen and announce sends; mode passes full_mode_ok. Bits are read
// literally: an entry with SYNCED and BAD but without CANDIDATE is the caller's inconsistency and is not repaired.
KAD_STEP_HD DecisionFull decide_full(PlanesFull F, uint32_t n, bool expired, uint32_t mode) {
    Planes P = F.p;
    const uint64_t valid = n >= 64u ? ~0ull : (1ull << n) - 1ull;
    const uint64_t good = ~P.bad & valid;
    uint64_t listen = 0ull, announce = 0ull;
    const uint64_t first = good & ~drop_lowest(good, TARGET_NODES);
    if (!expired && good && !(first & ~P.sync)) {  // Search::isSynced, as decide has it
        const uint64_t sync = P.sync & valid;
        if (mode & KAD_STEP_LISTEN)  // every synced non-candidate counts towards 4, due or not
            listen = sync & F.ldue & reach_of(sync & ~P.cand, LISTEN_NODES);
        if (mode & KAD_STEP_ANNOUNCE) {  // only the probed non-candidates count towards 8
            const uint64_t A = sync & F.adue;
            announce = A & reach_of(A & ~P.cand, TARGET_NODES);
        }
    }
    P.pend |= announce;  // the probe is a get request: getStatus[probe_query] is pending (:1330)
    if (mode & KAD_STEP_PROBE_BLOCKS) P.noget |= announce;
    const Decision d = decide(P, n, expired, mode & MODE_BITS);
    return {d.picks, listen, announce, d.counts, d.bits};
}

}  // namespace kadstep
