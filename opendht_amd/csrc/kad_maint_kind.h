// Dht::bucketMaintenance's decision on one bucket (dht.cpp:2832-2850), DESIGN.md §7.21: written once, for the host twin
// (kad_maint_scan_host, kad_maint_host.cpp) and for the kernels of kad_maint.h, which call the same kind_of. Plain C++,
// no HIP call and no header beyond <cstdint>, so the CPU sanitizer build compiles it alone.
#pragma once

#include <cstdint>

#include "../../include/kadgpu.h"

#if defined(__HIPCC__)
#define KAD_MAINT_HD __host__ __device__ __forceinline__
#else
#define KAD_MAINT_HD inline
#endif

namespace kadmaint {

// A Bucket::first as numbers: bits 0..63, then three 32-bit words (the device's fkey / ftail entry).
struct First {
    uint64_t hi;
    uint32_t t2, t3, t4;
};

KAD_MAINT_HD First first_of(const uint8_t* b) {
    First f;
    f.hi = 0;
    for (int x = 0; x < 8; x++) f.hi = (f.hi << 8) | b[x];
    f.t2 = ((uint32_t)b[8] << 24) | ((uint32_t)b[9] << 16) | ((uint32_t)b[10] << 8) | b[11];
    f.t3 = ((uint32_t)b[12] << 24) | ((uint32_t)b[13] << 16) | ((uint32_t)b[14] << 8) | b[15];
    f.t4 = ((uint32_t)b[16] << 24) | ((uint32_t)b[17] << 16) | ((uint32_t)b[18] << 8) | b[19];
    return f;
}

// InfoHash::lowbit (infohash.h:84-95): the position of the lowest set bit counted from the most significant one, -1 for
// the all-zero ID.
KAD_MAINT_HD int lowbit(const First& f) {
    if (f.t4) return 159 - __builtin_ctz(f.t4);
    if (f.t3) return 127 - __builtin_ctz(f.t3);
    if (f.t2) return 95 - __builtin_ctz(f.t2);
    if (f.hi) return 63 - __builtin_ctzll(f.hi);
    return -1;
}

// The time test of :2833 (strict). now_ns >= INT64_MIN + KAD_MAINT_STALE_NS (the entry points check it).
KAD_MAINT_HD bool is_stale(int64_t time_ns, int64_t now_ns) { return time_ns < now_ns - KAD_MAINT_STALE_NS; }

// A bucket passes :2833.
KAD_MAINT_HD bool is_candidate(bool stale, uint32_t n) { return stale || n == 0; }

// The kind word of a candidate bucket b: n, n_next, n_prev the node counts of b, std::next(b), std::prev(b) (read only
// where has_next / has_prev), first_b and first_next their firsts (first_next only with has_next).
KAD_MAINT_HD uint32_t kind_of(bool stale, uint32_t n, bool has_next, uint32_t n_next, bool has_prev, uint32_t n_prev,
                              const First& first_b, const First& first_next) {
    const bool empty = n == 0, next_empty = has_next && n_next == 0, prev_empty = has_prev && n_prev == 0;
    uint32_t k = (stale ? KAD_MAINT_STALE : 0u) | (empty ? KAD_MAINT_EMPTY : 0u) | (has_next ? KAD_MAINT_HAS_NEXT : 0u) |
                 (next_empty ? KAD_MAINT_NEXT_EMPTY : 0u) | (has_prev ? KAD_MAINT_HAS_PREV : 0u) |
                 (prev_empty ? KAD_MAINT_PREV_EMPTY : 0u);
    // q after :2842-2843 is b (no next), next (b empty) or either (a trial decides); a q ends in a node iff it has
    // nodes or :2844-2848 can move it to a prev that has some
    const bool prev_nodes = has_prev && n_prev != 0;
    const bool via_b = !empty || prev_nodes, via_next = (has_next && n_next != 0) || prev_nodes;
    const bool q_b = !has_next || !empty, q_next = has_next;
    const bool all = (!q_b || via_b) && (!q_next || via_next), any = (q_b && via_b) || (q_next && via_next);
    k |= (all ? KAD_MAINT_SURE : any ? KAD_MAINT_MAYBE : KAD_MAINT_NEVER) << KAD_MAINT_CLASS_SHIFT;
    // RoutingTable::randomId's bit (routing_table.cpp:30-32)
    const int b1 = lowbit(first_b), b2 = has_next ? lowbit(first_next) : -1;
    k |= (uint32_t)((b1 > b2 ? b1 : b2) + 1) << KAD_MAINT_BIT_SHIFT;
    return k;
}

// One candidate's share of the totals.
KAD_MAINT_HD uint32_t class_of(uint32_t kind) { return (kind >> KAD_MAINT_CLASS_SHIFT) & 3u; }

}  // namespace kadmaint
