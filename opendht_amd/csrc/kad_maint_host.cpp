// kad_maint_scan_host: Dht::bucketMaintenance's scan (kad_table_maintenance) over host arrays, without a
// GPU. The same kind_of as the kernels (kad_maint_kind.h), the same checks, the same record bytes.
#include <cstdint>

#include "../../include/kadgpu.h"
#include "kad_maint_kind.h"

extern "C" int kad_maint_scan_host(uint32_t B, const uint32_t* off, const uint8_t* first, const int64_t* time_ns,
                                   int64_t now_ns, uint32_t first_bucket, kad_maint_totals* totals, kad_maint_rec* out,
                                   uint32_t cap) {
    if (B && (!off || !first)) return KAD_ERR_INVALID;
    if (!totals) return KAD_ERR_INVALID;
    if (!out && cap) return KAD_ERR_INVALID;
    if (now_ns < INT64_MIN + KAD_MAINT_STALE_NS) return KAD_ERR_INVALID;
    if (first_bucket > B) return KAD_ERR_INVALID;
    kad_maint_totals r = {0, 0, 0, 0, 0, 0, 0xFFFFFFFFu, 0};
    for (uint32_t b = first_bucket; b < B; b++) {
        const uint32_t n = off[b + 1] - off[b];
        const bool stale = kadmaint::is_stale(time_ns ? time_ns[b] : INT64_MIN, now_ns);
        if (!kadmaint::is_candidate(stale, n)) continue;
        const bool has_next = b + 1 < B, has_prev = b > 0;
        const kadmaint::First fb = kadmaint::first_of(first + 20ull * b);
        const kadmaint::First fn = has_next ? kadmaint::first_of(first + 20ull * (b + 1)) : fb;
        const uint32_t kind = kadmaint::kind_of(stale, n, has_next, has_next ? off[b + 2] - off[b + 1] : 0u, has_prev,
                                                has_prev ? off[b] - off[b - 1] : 0u, fb, fn);
        if (r.candidates < cap) {
            out[r.candidates].bucket = b;
            out[r.candidates].kind = kind;
        }
        r.candidates++;
        r.stale += stale ? 1u : 0u;
        r.empty += n == 0 ? 1u : 0u;
        const uint32_t c = kadmaint::class_of(kind);
        if (c == KAD_MAINT_SURE) {
            if (r.first_sure == 0xFFFFFFFFu) r.first_sure = b;
            r.sure++;
        } else if (c == KAD_MAINT_MAYBE) {
            r.maybe++;
        } else {
            r.never++;
        }
    }
    *totals = r;
    return KAD_OK;
}
