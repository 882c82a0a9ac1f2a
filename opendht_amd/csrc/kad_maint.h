// Bucket::time on the device and Dht::bucketMaintenance's scan (kad_table_set/patch/get_bucket_times,
// kad_table_touch_buckets, kad_table_maintenance). Included by kad_engine.hip (the kernels read
// kad_table's private arrays); the decision on one bucket is kadmaint::kind_of of kad_maint_kind.h, which the host twin
// (kad_maint_host.cpp) calls as well.
//
//   touch_kernel        Dht::onReportedAddr x q: one lane per ID, load_target and locate_bucket, one 8-byte store of
//                       `now` to the bucket's time and one 4-byte store of the bucket when asked
//   btime_patch_kernel  one lane per listed bucket (the host has removed earlier duplicates)
//   btime_gather_kernel kad_table_apply's splits: the new bucket's time from its source bucket
//   maint_count_kernel  one lane per bucket from first_bucket on: its time and directory words, for a candidate the
//                       firsts and the kind; the tile's candidate bits (one ballot per wave) and its counts
//   maint_scan_kernel   one workgroup: the exclusive scan of the tiles' candidate counts (sw_scan) and the totals
//   maint_write_kernel  the ordered records from the bits and the tile bases, one 8-byte store each
//
// Nothing is shared between calls: the bits and partials live in a stream-ordered allocation of the call's own (the
// sweep's pool), no workgroup waits for another and no result depends on the order they run (first_sure is a minimum
// over the tiles' partials, not an atomic).
#ifndef KAD_MAINT_H
#define KAD_MAINT_H

#include "kad_maint_kind.h"

namespace {

__global__ __launch_bounds__(BLOCK) void touch_kernel(DevTable T, const uint8_t* __restrict__ ids, uint32_t q,
                                                      int64_t now_ns, int64_t* __restrict__ btime,
                                                      uint32_t* __restrict__ out_bucket) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= q) return;
    const uint32_t b = locate_bucket(T, load_target(ids, i));  // < T.B (the host refuses B == 0)
    btime[b] = now_ns;
    if (out_bucket) out_bucket[i] = b;
}

__global__ __launch_bounds__(BLOCK) void btime_patch_kernel(const uint32_t* __restrict__ buckets,
                                                            const int64_t* __restrict__ time_ns, uint32_t m, uint32_t B,
                                                            int64_t* __restrict__ btime) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= m) return;
    const uint32_t b = buckets[j];
    if (b < B) btime[b] = time_ns[j];
}

__global__ __launch_bounds__(BLOCK) void btime_gather_kernel(const uint32_t* __restrict__ src, uint32_t B1, uint32_t B0,
                                                             const int64_t* __restrict__ btime0,
                                                             int64_t* __restrict__ btime1) {
    const uint32_t c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= B1) return;
    const uint32_t a = src[c];
    btime1[c] = a < B0 ? btime0[a] : INT64_MIN;
}

// Bucket b < B of the table: does it pass :2833, and with what kind? (dir has B + 1 entries, fkey / ftail B.)
__device__ __forceinline__ bool mt_bucket(const uint2* __restrict__ dir, const uint64_t* __restrict__ fkey,
                                          const uint32_t* __restrict__ ftail, const int64_t* __restrict__ btime,
                                          uint32_t B, uint32_t b, int64_t now_ns, uint32_t& kind) {
    const uint32_t s = dir[b].x & ~WIDE, e = dir[b + 1].x & ~WIDE;
    const bool stale = kadmaint::is_stale(btime ? btime[b] : INT64_MIN, now_ns);
    if (!kadmaint::is_candidate(stale, e - s)) return false;
    const bool has_next = b + 1 < B, has_prev = b > 0;
    const uint32_t n_next = has_next ? (dir[b + 2].x & ~WIDE) - e : 0u, n_prev = has_prev ? s - (dir[b - 1].x & ~WIDE) : 0u;
    const uint32_t* fa = ftail + 3ull * b;
    const kadmaint::First fb{fkey[b], fa[0], fa[1], fa[2]};
    kadmaint::First fn = fb;
    if (has_next) fn = kadmaint::First{fkey[b + 1], fa[3], fa[4], fa[5]};
    kind = kadmaint::kind_of(stale, e - s, has_next, n_next, has_prev, n_prev, fb, fn);
    return true;
}

// Per tile t of BLOCK buckets: bits[4 t + w] = wave w's candidate ballot; part[2 t] = candidates, stale, empty, sure;
// part[2 t + 1] = maybe, first_sure (NONE: no SURE bucket in the tile), 0, 0.
__global__ __launch_bounds__(BLOCK) void maint_count_kernel(const uint2* __restrict__ dir,
                                                            const uint64_t* __restrict__ fkey,
                                                            const uint32_t* __restrict__ ftail,
                                                            const int64_t* __restrict__ btime, uint32_t B,
                                                            uint32_t first_bucket, int64_t now_ns,
                                                            unsigned long long* __restrict__ bits,
                                                            uint4* __restrict__ part) {
    __shared__ uint32_t red[6][4];
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t kind = 0;
    bool cand = false;
    if (j < B - first_bucket) cand = mt_bucket(dir, fkey, ftail, btime, B, first_bucket + j, now_ns, kind);
    const uint32_t cls = kadmaint::class_of(kind);
    const unsigned long long cm = __ballot(cand), sm = __ballot(cand && (kind & KAD_MAINT_STALE)),
                             em = __ballot(cand && (kind & KAD_MAINT_EMPTY)),
                             su = __ballot(cand && cls == KAD_MAINT_SURE), ma = __ballot(cand && cls == KAD_MAINT_MAYBE);
    const uint32_t wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) {
        bits[blockIdx.x * 4 + wid] = cm;
        red[0][wid] = (uint32_t)__popcll(cm);
        red[1][wid] = (uint32_t)__popcll(sm);
        red[2][wid] = (uint32_t)__popcll(em);
        red[3][wid] = (uint32_t)__popcll(su);
        red[4][wid] = (uint32_t)__popcll(ma);
        red[5][wid] = su ? first_bucket + j + (uint32_t)__ffsll((long long)su) - 1u : NONE;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        auto sum = [&](int k) { return red[k][0] + red[k][1] + red[k][2] + red[k][3]; };
        part[2 * blockIdx.x] = make_uint4(sum(0), sum(1), sum(2), sum(3));
        part[2 * blockIdx.x + 1] = make_uint4(sum(4), min(min(red[5][0], red[5][1]), min(red[5][2], red[5][3])), 0u, 0u);
    }
}

// One workgroup: exc[t] = the candidates of the tiles before t, and the totals.
__global__ __launch_bounds__(BLOCK) void maint_scan_kernel(const uint4* __restrict__ part, uint32_t NT,
                                                           uint32_t* __restrict__ exc,
                                                           kad_maint_totals* __restrict__ totals) {
    __shared__ uint32_t lds[4];
    __shared__ uint32_t red[4][4];
    __shared__ uint32_t fmin[4];
    uint32_t stale = 0, empty = 0, sure = 0, maybe = 0, fs = NONE;
    const uint32_t cand = sw_scan(NT, exc, lds, [&](uint32_t i) {
        const uint4 p = part[2 * i], r = part[2 * i + 1];
        stale += p.y; empty += p.z; sure += p.w; maybe += r.x;
        fs = min(fs, r.y);
        return p.x;
    });
    const uint32_t st = sw_block_sum(stale, red[0]), em = sw_block_sum(empty, red[1]), su = sw_block_sum(sure, red[2]),
                   ma = sw_block_sum(maybe, red[3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) fs = min(fs, (uint32_t)__shfl_xor(fs, o, 64));
    if ((threadIdx.x & 63u) == 0) fmin[threadIdx.x >> 6] = fs;
    __syncthreads();
    if (threadIdx.x == 0) {
        kad_maint_totals r;
        r.candidates = cand; r.stale = st; r.empty = em; r.sure = su; r.maybe = ma; r.never = cand - su - ma;
        r.first_sure = min(min(fmin[0], fmin[1]), min(fmin[2], fmin[3])); r.reserved = 0;
        *totals = r;
    }
}

// Tile blockIdx.x's records, in bucket order from exc[tile]; record k is written only if k < cap.
__global__ __launch_bounds__(BLOCK) void maint_write_kernel(const uint2* __restrict__ dir,
                                                            const uint64_t* __restrict__ fkey,
                                                            const uint32_t* __restrict__ ftail,
                                                            const int64_t* __restrict__ btime, uint32_t B,
                                                            uint32_t first_bucket, int64_t now_ns,
                                                            const unsigned long long* __restrict__ bits,
                                                            const uint32_t* __restrict__ exc,
                                                            kad_maint_rec* __restrict__ out, uint32_t cap) {
    __shared__ uint32_t lds[4];
    const uint32_t base = exc[blockIdx.x];
    if (base >= cap) return;  // block-uniform
    const uint32_t bit = (uint32_t)(bits[blockIdx.x * 4 + (threadIdx.x >> 6)] >> (threadIdx.x & 63u)) & 1u;
    uint32_t total;
    const uint32_t o = base + block_exclusive_scan(bit, lds, total);
    if (!bit || o >= cap) return;
    const uint32_t b = first_bucket + blockIdx.x * BLOCK + threadIdx.x;  // < B: the bit is set
    uint32_t kind = 0;
    (void)mt_bucket(dir, fkey, ftail, btime, B, b, now_ns, kind);
    reinterpret_cast<uint2*>(out)[o] = make_uint2(b, kind);
}

// The bucket times of a table that has none yet: every bucket at INT64_MIN.
int btime_ensure(kad_table* t) {
    if (t->btime || t->d.B == 0) return KAD_OK;
    const std::vector<int64_t> init(t->d.B, INT64_MIN);
    return dev_upload(&t->btime, init.data(), init.size(), t->owned, t->bytes);
}

// Waits for the table's last asynchronous touch (whatever stream it ran on).
int btime_settle(const kad_table* t) {
    if (t->bt_async) HIP_TRY(hipEventSynchronize(t->bt_ev));
    return KAD_OK;
}

// kad_table_apply's hook (declared before table_apply): the times of the new bucket list, in a new array listed in
// `fresh`. The source of a new bucket is the old bucket with the largest first not greater than its own.
int btime_carry_split(const kad_table* t, const uint8_t* first0, uint32_t B0, const uint8_t* first1, uint32_t B1,
                      int64_t** out, std::vector<void*>& fresh, uint64_t& freshb, std::vector<void*>& tmp, uint64_t& tmpb) {
    std::vector<uint32_t> src(B1);
    uint32_t a = 0;
    for (uint32_t c = 0; c < B1; c++) {
        while (a + 1 < B0 && std::memcmp(first0 + 20ull * (a + 1), first1 + 20ull * c, 20) <= 0) a++;
        src[c] = a;
    }
    uint32_t* dsrc;
    if (int rc = dev_upload(&dsrc, src.data(), src.size(), tmp, tmpb)) return rc;
    if (int rc = dev_upload(out, nullptr, B1, fresh, freshb)) return rc;
    if (int rc = btime_settle(t)) return rc;
    hipLaunchKernelGGL(btime_gather_kernel, dim3(grid_for(B1)), dim3(BLOCK), 0, 0, dsrc, B1, B0, t->btime, *out);
    HIP_TRY(hipGetLastError());
    return KAD_OK;
}

int maint_check(const kad_table* t, int64_t now_ns, uint32_t first_bucket, const kad_maint_totals* totals,
                const kad_maint_rec* out, uint32_t cap) {
    if (!t) return set_err(KAD_ERR_INVALID, "NULL table");
    if (!totals) return set_err(KAD_ERR_INVALID, "NULL totals");
    if (!out && cap) return set_err(KAD_ERR_INVALID, "NULL list with a non-zero cap");
    if (now_ns < INT64_MIN + KAD_MAINT_STALE_NS) return set_err(KAD_ERR_INVALID, "now_ns is within 10 minutes of INT64_MIN");
    if (first_bucket > t->d.B) return set_err(KAD_ERR_INVALID, "first_bucket %u: the table has %u buckets", first_bucket, t->d.B);
    return KAD_OK;
}

// The scan enqueued on s: count, scan, write; the partials are freed in stream order.
int maint_run(const kad_table* t, int64_t now_ns, uint32_t first_bucket, kad_maint_totals* totals, kad_maint_rec* out,
              uint32_t cap, hipStream_t s) {
    const DevTable& d = t->d;
    const uint32_t NT = (uint32_t)(((uint64_t)(d.B - first_bucket) + BLOCK - 1) / BLOCK);
    const size_t o_bits = 32ull * NT, o_exc = o_bits + 32ull * NT, bytes = o_exc + 4ull * NT + 16;
    void* mem = nullptr;
    hipMemPool_t pool = sweep_pool(t->device);
    const hipError_t e = pool ? hipMallocFromPoolAsync(&mem, bytes, pool, s) : hipMallocAsync(&mem, bytes, s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(KAD_ERR_NOMEM, "maintenance: hipMallocAsync(%zu) failed: %s", bytes, hipGetErrorString(e));
    }
    uint8_t* m = static_cast<uint8_t*>(mem);
    uint4* part = reinterpret_cast<uint4*>(m);
    unsigned long long* bits = reinterpret_cast<unsigned long long*>(m + o_bits);
    uint32_t* exc = reinterpret_cast<uint32_t*>(m + o_exc);
    if (NT)
        hipLaunchKernelGGL(maint_count_kernel, dim3(NT), dim3(BLOCK), 0, s, d.dir, d.fkey, d.ftail, t->btime, d.B,
                           first_bucket, now_ns, bits, part);
    hipLaunchKernelGGL(maint_scan_kernel, dim3(1), dim3(BLOCK), 0, s, part, NT, exc, totals);
    if (NT && cap)
        hipLaunchKernelGGL(maint_write_kernel, dim3(NT), dim3(BLOCK), 0, s, d.dir, d.fkey, d.ftail, t->btime, d.B,
                           first_bucket, now_ns, bits, exc, out, cap);
    const hipError_t le = hipGetLastError();
    (void)hipFreeAsync(mem, s);
    if (le != hipSuccess) return set_err(KAD_ERR_HIP, "maintenance: launch failed: %s", hipGetErrorString(le));
    return KAD_OK;
}

}  // namespace

extern "C" {

int kad_table_set_bucket_times(kad_table* t, const int64_t* time_ns) {
    if (!t) return set_err(KAD_ERR_INVALID, "NULL table");
    if (t->d.B == 0 || (!time_ns && !t->btime)) return KAD_OK;  // no times yet: every bucket is at INT64_MIN already
    DeviceGuard g(t->device);
    if (int rc = btime_settle(t)) return rc;
    if (!time_ns) {
        const std::vector<int64_t> init(t->d.B, INT64_MIN);
        HIP_TRY(hipMemcpy(t->btime, init.data(), 8ull * t->d.B, hipMemcpyHostToDevice));
        return KAD_OK;
    }
    if (!t->btime) return dev_upload(&t->btime, time_ns, t->d.B, t->owned, t->bytes);
    HIP_TRY(hipMemcpy(t->btime, time_ns, 8ull * t->d.B, hipMemcpyHostToDevice));
    return KAD_OK;
}

int kad_table_patch_bucket_times(kad_table* t, uint32_t m, const uint32_t* buckets, const int64_t* time_ns) {
    if (!t) return set_err(KAD_ERR_INVALID, "NULL table");
    if (m && (!buckets || !time_ns)) return set_err(KAD_ERR_INVALID, "NULL list");
    for (uint32_t j = 0; j < m; j++)
        if (buckets[j] >= t->d.B)
            return set_err(KAD_ERR_INVALID, "bucket %u (entry %u): the table has %u buckets", buckets[j], j, t->d.B);
    if (m == 0) return KAD_OK;
    // the later entry of a bucket listed twice wins: keep each bucket's last entry, so the lanes write distinct words
    std::vector<std::pair<uint32_t, uint32_t>> order(m);
    for (uint32_t j = 0; j < m; j++) order[j] = {buckets[j], j};
    std::sort(order.begin(), order.end());
    std::vector<uint32_t> hb;
    std::vector<int64_t> ht;
    for (uint32_t k = 0; k < m; k++)
        if (k + 1 == m || order[k + 1].first != order[k].first) {
            hb.push_back(order[k].first);
            ht.push_back(time_ns[order[k].second]);
        }
    DeviceGuard g(t->device);
    if (int rc = btime_ensure(t)) return rc;
    if (int rc = btime_settle(t)) return rc;
    std::vector<void*> tmp;
    uint64_t tmpb = 0;
    uint32_t* db = nullptr;
    int64_t* dt = nullptr;
    int rc = dev_upload(&db, hb.data(), hb.size(), tmp, tmpb);
    if (rc == KAD_OK) rc = dev_upload(&dt, ht.data(), ht.size(), tmp, tmpb);
    if (rc == KAD_OK) {
        hipLaunchKernelGGL(btime_patch_kernel, dim3(grid_for(hb.size())), dim3(BLOCK), 0, 0, db, dt, (uint32_t)hb.size(),
                           t->d.B, t->btime);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess)
            rc = set_err(KAD_ERR_HIP, "patch_bucket_times: kernel failed");
    }
    for (void* p : tmp) (void)hipFree(p);
    return rc;
}

int kad_table_get_bucket_times(const kad_table* t, int64_t* out) {
    if (!t) return set_err(KAD_ERR_INVALID, "NULL table");
    if (t->d.B == 0) return KAD_OK;
    if (!out) return set_err(KAD_ERR_INVALID, "NULL buffer");
    if (!t->btime) {
        std::fill(out, out + t->d.B, INT64_MIN);
        return KAD_OK;
    }
    DeviceGuard g(t->device);
    if (int rc = btime_settle(t)) return rc;
    HIP_TRY(hipMemcpy(out, t->btime, 8ull * t->d.B, hipMemcpyDeviceToHost));
    return KAD_OK;
}

int kad_table_touch_buckets(kad_table* t, const uint8_t* ids, uint32_t q, int64_t now_ns, uint32_t* out_bucket,
                            void* stream) {
    if (!t) return set_err(KAD_ERR_INVALID, "NULL table");
    if (t->d.B == 0) return set_err(KAD_ERR_INVALID, "touch_buckets needs a RoutingTable (buckets)");
    if (q == 0) return KAD_OK;
    if (!ids) return set_err(KAD_ERR_INVALID, "NULL buffer");
    DeviceGuard g(t->device);
    if (int rc = btime_ensure(t)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (!t->bt_ev) HIP_TRY(hipEventCreateWithFlags(&t->bt_ev, hipEventDisableTiming));
    if (t->bt_async) HIP_TRY(hipStreamWaitEvent(s, t->bt_ev, 0));  // after the last touch, whatever stream it ran on
    hipLaunchKernelGGL(touch_kernel, dim3(grid_for(q)), dim3(BLOCK), 0, s, t->d, ids, q, now_ns, t->btime, out_bucket);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(t->bt_ev, s));
    t->bt_async = true;
    return KAD_OK;
}

int kad_table_touch_buckets_host(kad_table* t, const uint8_t* ids, uint32_t q, int64_t now_ns, uint32_t* out_bucket) {
    if (!t) return set_err(KAD_ERR_INVALID, "NULL table");
    if (t->d.B == 0) return set_err(KAD_ERR_INVALID, "touch_buckets needs a RoutingTable (buckets)");
    if (q == 0) return KAD_OK;
    if (!ids) return set_err(KAD_ERR_INVALID, "NULL buffer");
    DeviceGuard g(t->device);
    uint8_t* buf = nullptr;
    const size_t o_out = (20ull * q + 15) & ~size_t(15);
    if (hipMalloc((void**)&buf, o_out + 4ull * q) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(KAD_ERR_NOMEM, "touch host: out of device memory");
    }
    int rc = KAD_OK;
    if (hipMemcpy(buf, ids, 20ull * q, hipMemcpyHostToDevice) != hipSuccess) rc = set_err(KAD_ERR_HIP, "touch host: H2D failed");
    if (rc == KAD_OK)
        rc = kad_table_touch_buckets(t, buf, q, now_ns, out_bucket ? reinterpret_cast<uint32_t*>(buf + o_out) : nullptr, nullptr);
    if (rc == KAD_OK && hipStreamSynchronize(nullptr) != hipSuccess) rc = set_err(KAD_ERR_HIP, "touch host: kernel failed");
    if (rc == KAD_OK && out_bucket && hipMemcpy(out_bucket, buf + o_out, 4ull * q, hipMemcpyDeviceToHost) != hipSuccess)
        rc = set_err(KAD_ERR_HIP, "touch host: D2H failed");
    (void)hipFree(buf);
    return rc;
}

int kad_table_maintenance(const kad_table* t, int64_t now_ns, uint32_t first_bucket, kad_maint_totals* totals,
                          kad_maint_rec* out, uint32_t cap, void* stream) {
    if (int rc = maint_check(t, now_ns, first_bucket, totals, out, cap)) return rc;
    if (((uintptr_t)totals & 3) || ((uintptr_t)out & 7))
        return set_err(KAD_ERR_INVALID, "device buffers must be aligned (totals 4 bytes, records 8)");
    DeviceGuard g(t->device);
    return maint_run(t, now_ns, first_bucket, totals, out, cap, (hipStream_t)stream);
}

int kad_table_maintenance_host(const kad_table* t, int64_t now_ns, uint32_t first_bucket, kad_maint_totals* totals,
                               kad_maint_rec* out, uint32_t cap) {
    if (int rc = maint_check(t, now_ns, first_bucket, totals, out, cap)) return rc;
    DeviceGuard g(t->device);
    cap = std::min(cap, t->d.B - first_bucket);
    uint8_t* buf = nullptr;
    hipStream_t s = nullptr;
    auto done = [&](int r) {
        if (s) (void)hipStreamDestroy(s);
        if (buf) (void)hipFree(buf);
        return r;
    };
    const size_t o_rec = sizeof(kad_maint_totals);
    if (hipMalloc((void**)&buf, o_rec + 8ull * cap) != hipSuccess) {
        (void)hipGetLastError();
        return done(set_err(KAD_ERR_NOMEM, "maintenance host: out of device memory"));
    }
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess)
        return done(set_err(KAD_ERR_HIP, "maintenance host: no stream"));
    if (t->bt_async && hipStreamWaitEvent(s, t->bt_ev, 0) != hipSuccess)
        return done(set_err(KAD_ERR_HIP, "maintenance host: wait failed"));
    kad_maint_totals r;
    int rc = maint_run(t, now_ns, first_bucket, reinterpret_cast<kad_maint_totals*>(buf),
                       cap ? reinterpret_cast<kad_maint_rec*>(buf + o_rec) : nullptr, cap, s);
    if (rc == KAD_OK && hipMemcpyAsync(&r, buf, sizeof(r), hipMemcpyDeviceToHost, s) != hipSuccess)
        rc = set_err(KAD_ERR_HIP, "maintenance host: D2H failed");
    const hipError_t e = hipStreamSynchronize(s);
    if (rc == KAD_OK && e != hipSuccess) rc = set_err(KAD_ERR_HIP, "maintenance host: %s", hipGetErrorString(e));
    if (rc != KAD_OK) return done(rc);
    const uint32_t mr = std::min(r.candidates, cap);
    if (mr && hipMemcpy(out, buf + o_rec, 8ull * mr, hipMemcpyDeviceToHost) != hipSuccess)
        return done(set_err(KAD_ERR_HIP, "maintenance host: D2H failed"));
    *totals = r;
    return done(KAD_OK);
}

}  // extern "C"

#endif  // KAD_MAINT_H
