// Whole-table sweep (kad_table_sweep, kad_table_sweep_host; the list half of kad_table_expire): Dht::getNodesStats
// (dht.cpp:2470-2495) and the scan of Dht::expireBuckets (dht.cpp:942-956) as one streaming pass over the status
// bytes and the bucket directory. Included by kad_engine.hip (the kernels read kad_table's private arrays).
//
//   sweep_count_kernel   one workgroup per tile of SW_TILE status bytes, 16 bytes per lane in one load: the tile's
//                        good / dubious / expired / incoming counts (wave shuffles, then LDS; written as the tile's
//                        partial, no atomic) and the tile's EXPIRED bits, one 16-bit word per lane
//   sweep_bucket_kernel  one lane per bucket: its two directory entries and the EXPIRED bits of its nodes; the
//                        tile's changed / empty counts and its changed bits (one ballot per wave)
//   sweep_scan_kernel    one workgroup: exclusive scans of the tiles' expired and changed counts, and the totals
//   sweep_write_kernel   the ordered lists from the bits and the tile bases (a block scan per tile)
//
// The status bytes and the directory are read once; the write pass reads the bit maps (an eighth of a byte per
// node). Nothing is shared between calls: the partials and bit maps live in a stream-ordered allocation of the call's
// own, so sweeps of one table on several streams do not meet, and no workgroup waits for another.
#ifndef KAD_SWEEP_H
#define KAD_SWEEP_H

namespace {

constexpr uint32_t SW_TILE = BLOCK * 16;  // status bytes per workgroup
constexpr uint32_t SW_SCAN_ITEMS = 8;     // tile counts per lane and round of the one-workgroup scan
constexpr size_t SWEEP_POOL_KEEP = 32u << 20;  // what the engine's pool keeps after a kad_table_expire that took more

// Bits 1, 9, 17, 25 of w (the EXPIRED bit of four status bytes) as a nibble.
__device__ __forceinline__ uint32_t sw_expired_nibble(uint32_t w) {
    return ((((w >> 1) & 0x01010101u) * 0x01020408u) >> 24) & 0xFu;
}

// Sum of v over the workgroup in lane 0 of wave 0 (red: 4 words of LDS per call site, synchronised here).
__device__ __forceinline__ uint32_t sw_block_sum(uint32_t v, uint32_t* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(BLOCK) void sweep_count_kernel(const uint8_t* __restrict__ status, uint32_t n,
                                                            const int64_t* __restrict__ time_ns,
                                                            const int64_t* __restrict__ reply_ns,
                                                            unsigned short* __restrict__ nbits,
                                                            uint4* __restrict__ part) {
    __shared__ uint32_t red[4][4];
    __shared__ uint4 sst[BLOCK];
    const uint32_t tile0 = blockIdx.x * SW_TILE, i0 = tile0 + 16u * threadIdx.x;
    uint32_t w[4] = {0, 0, 0, 0};
    uint32_t valid = 0;
    if (i0 < n) {
        valid = min(16u, n - i0);
        if (valid == 16u) {
            const uint4 v = reinterpret_cast<const uint4*>(status)[i0 >> 4];
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {  // the last lane of the table: the array ends with the table
            for (uint32_t k = 0; k < valid; k++) w[k >> 2] |= (uint32_t)status[i0 + k] << (8 * (k & 3));
        }
    }
    uint32_t good = 0, expired = 0, neither = 0, bits = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        good += __popc(w[k] & 0x01010101u);
        expired += __popc(w[k] & 0x02020202u);
        neither += __popc(~(w[k] | (w[k] >> 1)) & 0x01010101u);
        bits |= sw_expired_nibble(w[k]) << (4 * k);
    }
    neither -= 16u - valid;  // the padding bytes are zero
    nbits[blockIdx.x * BLOCK + threadIdx.x] = (unsigned short)bits;
    uint32_t incoming = 0;
    if (time_ns) {  // grid-uniform: lane j of round k takes node tile0 + k * BLOCK + j (coalesced 8-byte loads)
        sst[threadIdx.x] = make_uint4(w[0], w[1], w[2], w[3]);
        __syncthreads();
        const uint8_t* sb = reinterpret_cast<const uint8_t*>(sst);
#pragma unroll 4
        for (uint32_t k = 0; k < 16; k++) {
            const uint32_t j = k * BLOCK + threadIdx.x, i = tile0 + j;
            if (i < n && (sb[j] & KAD_STATUS_GOOD)) incoming += time_ns[i] > reply_ns[i] ? 1u : 0u;
        }
    }
    const uint32_t g = sw_block_sum(good, red[0]), d = sw_block_sum(neither, red[1]),
                   e = sw_block_sum(expired, red[2]), in = sw_block_sum(incoming, red[3]);
    if (threadIdx.x == 0) part[blockIdx.x] = make_uint4(g, d, e, in);
}

// Does any node of [s, e), s < e, have its EXPIRED bit set? Whole tiles inside the range answer from their count.
__device__ __forceinline__ bool sw_any_expired(const unsigned short* __restrict__ nbits, const uint4* __restrict__ part,
                                               uint32_t s, uint32_t e) {
    const uint32_t us = s >> 4, ue = (e - 1) >> 4;
    const uint32_t lo = 0xFFFFu << (s & 15u), hi = (2u << ((e - 1) & 15u)) - 1u;
    if (us == ue) return (nbits[us] & lo & hi) != 0;
    if ((nbits[us] & lo) || (nbits[ue] & hi)) return true;
    uint32_t u = us + 1;
    while (u < ue) {
        if ((u % BLOCK) == 0 && u + BLOCK <= ue) {
            if (part[u / BLOCK].z) return true;
            u += BLOCK;
        } else {
            if (nbits[u]) return true;
            u++;
        }
    }
    return false;
}

__global__ __launch_bounds__(BLOCK) void sweep_bucket_kernel(const uint2* __restrict__ dir, uint32_t B,
                                                             const unsigned short* __restrict__ nbits,
                                                             const uint4* __restrict__ part,
                                                             unsigned long long* __restrict__ bbits,
                                                             uint2* __restrict__ bcnt) {
    __shared__ uint32_t red[2][4];
    const uint32_t b = blockIdx.x * BLOCK + threadIdx.x;
    bool changed = false, empty = false;
    if (b < B) {
        const uint32_t s = dir[b].x & ~WIDE, e = dir[b + 1].x & ~WIDE;
        empty = s >= e;
        if (!empty) changed = sw_any_expired(nbits, part, s, e);
    }
    const unsigned long long cm = __ballot(changed), em = __ballot(empty);
    const uint32_t wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) {
        bbits[blockIdx.x * 4 + wid] = cm;
        red[0][wid] = (uint32_t)__popcll(cm);
        red[1][wid] = (uint32_t)__popcll(em);
    }
    __syncthreads();
    if (threadIdx.x == 0)
        bcnt[blockIdx.x] = make_uint2(red[0][0] + red[0][1] + red[0][2] + red[0][3], red[1][0] + red[1][1] + red[1][2] + red[1][3]);
}

// One workgroup's exclusive scan of m counts, 2048 per round with the carry of the rounds before: exc[i] = the sum of
// count(j) for j < i; returns the total. count(i) also adds whatever else entry i carries to the caller's sums.
template <class Count>
__device__ __forceinline__ uint32_t sw_scan(uint32_t m, uint32_t* __restrict__ exc, uint32_t* lds, Count count) {
    uint32_t carry = 0;
    for (uint32_t c = 0; c < m; c += BLOCK * SW_SCAN_ITEMS) {
        const uint32_t base = c + threadIdx.x * SW_SCAN_ITEMS;
        uint32_t v[SW_SCAN_ITEMS], s = 0;
#pragma unroll
        for (uint32_t k = 0; k < SW_SCAN_ITEMS; k++) {
            v[k] = base + k < m ? count(base + k) : 0u;
            s += v[k];
        }
        uint32_t total;
        uint32_t ex = carry + block_exclusive_scan(s, lds, total);
#pragma unroll
        for (uint32_t k = 0; k < SW_SCAN_ITEMS; k++) {
            if (base + k < m) exc[base + k] = ex;
            ex += v[k];
        }
        carry += total;
    }
    return carry;
}

// One workgroup: texc[t] = expired nodes of the tiles before t, bexc[t] = changed buckets of the bucket tiles before
// t, and the totals.
__global__ __launch_bounds__(BLOCK) void sweep_scan_kernel(const uint4* __restrict__ part, uint32_t NT,
                                                           uint32_t* __restrict__ texc, const uint2* __restrict__ bcnt,
                                                           uint32_t NBT, uint32_t* __restrict__ bexc, uint32_t flags,
                                                           kad_sweep_totals* __restrict__ totals) {
    __shared__ uint32_t lds[4];
    __shared__ uint32_t red[4][4];
    uint32_t good = 0, dubious = 0, incoming = 0, empty = 0;
    const uint32_t expired = sw_scan(NT, texc, lds, [&](uint32_t i) {
        const uint4 p = part[i];
        good += p.x; dubious += p.y; incoming += p.w;
        return p.z;
    });
    const uint32_t changed = sw_scan(NBT, bexc, lds, [&](uint32_t i) {
        const uint2 p = bcnt[i];
        empty += p.y;
        return p.x;
    });
    const uint32_t g = sw_block_sum(good, red[0]), d = sw_block_sum(dubious, red[1]),
                   in = sw_block_sum(incoming, red[2]), em = sw_block_sum(empty, red[3]);
    if (threadIdx.x == 0) {
        kad_sweep_totals r;
        r.good = g; r.dubious = d; r.expired = expired; r.incoming = in;
        r.changed_buckets = changed; r.empty_buckets = em; r.flags = flags; r.reserved = 0;
        *totals = r;
    }
}

// Blocks [0, NTw): the expired nodes of node tile blockIdx.x; blocks [NTw, NTw + NBTw): the changed buckets of
// bucket tile blockIdx.x - NTw. Entry k of a list is written only if k < cap.
__global__ __launch_bounds__(BLOCK) void sweep_write_kernel(const unsigned short* __restrict__ nbits,
                                                            const uint32_t* __restrict__ texc, uint32_t NTw,
                                                            uint32_t index_base, uint32_t* __restrict__ out_nodes,
                                                            uint32_t cap_nodes,
                                                            const unsigned long long* __restrict__ bbits,
                                                            const uint32_t* __restrict__ bexc,
                                                            uint32_t* __restrict__ out_buckets, uint32_t cap_buckets) {
    __shared__ uint32_t lds[4];
    uint32_t total;
    if (blockIdx.x < NTw) {
        const uint32_t base = texc[blockIdx.x];
        if (base >= cap_nodes) return;  // block-uniform
        uint32_t m = nbits[blockIdx.x * BLOCK + threadIdx.x];
        uint32_t o = base + block_exclusive_scan((uint32_t)__popc(m), lds, total);
        const uint32_t i0 = blockIdx.x * SW_TILE + 16u * threadIdx.x + index_base;
        while (m) {
            const uint32_t k = (uint32_t)__ffs((int)m) - 1u;
            m &= m - 1u;
            if (o < cap_nodes) out_nodes[o] = i0 + k;
            o++;
        }
    } else {
        const uint32_t bt = blockIdx.x - NTw, base = bexc[bt];
        if (base >= cap_buckets) return;  // block-uniform
        const uint32_t bit = (uint32_t)(bbits[bt * 4 + (threadIdx.x >> 6)] >> (threadIdx.x & 63u)) & 1u;
        const uint32_t o = base + block_exclusive_scan(bit, lds, total);
        if (bit && o < cap_buckets) out_buckets[o] = bt * BLOCK + threadIdx.x;
    }
}

// The partials and bit maps of one sweep: one stream-ordered allocation, freed in stream order by sweep_release.
struct SweepTmp {
    void* mem = nullptr;
    uint32_t NT = 0, NBT = 0;
    uint4* part = nullptr;               // NT: good, dubious, expired, incoming of every node tile
    unsigned long long* bbits = nullptr; // NBT x 4: the changed bits of every bucket tile
    uint2* bcnt = nullptr;               // NBT: changed, empty
    uint32_t* texc = nullptr;            // NT
    uint32_t* bexc = nullptr;            // NBT
    unsigned short* nbits = nullptr;     // NT x BLOCK: the EXPIRED bits of 16 nodes each
};

// A memory pool of the engine's own per device that keeps what it is given back (release threshold: never), so a
// sweep's allocation is a pool lookup, not a trip to the driver. NULL: use the device's default pool.
hipMemPool_t sweep_pool(int dev) {
    static std::mutex mu;
    static hipMemPool_t pools[64] = {};
    static bool tried[64] = {};
    if (dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    if (!tried[dev]) {
        tried[dev] = true;
        hipMemPoolProps p{};
        p.allocType = hipMemAllocationTypePinned;
        p.handleTypes = hipMemHandleTypeNone;
        p.location.type = hipMemLocationTypeDevice;
        p.location.id = dev;
        if (hipMemPoolCreate(&pools[dev], &p) != hipSuccess) {
            (void)hipGetLastError();
            pools[dev] = nullptr;
        } else {
            uint64_t keep = ~0ull;
            (void)hipMemPoolSetAttribute(pools[dev], hipMemPoolAttrReleaseThreshold, &keep);
        }
    }
    return pools[dev];
}

void sweep_release(SweepTmp& w, hipStream_t s) {
    if (w.mem) (void)hipFreeAsync(w.mem, s);
    w.mem = nullptr;
}

// The count passes and the totals (device word block `totals`), enqueued on s. The caller releases w.
int sweep_count(const kad_table* t, uint32_t flags, kad_sweep_totals* totals, hipStream_t s, SweepTmp& w) {
    const DevTable& d = t->d;
    w.NT = (uint32_t)(((uint64_t)d.n + SW_TILE - 1) / SW_TILE);
    w.NBT = (uint32_t)(((uint64_t)d.B + BLOCK - 1) / BLOCK);
    const size_t o_bbits = 16ull * w.NT, o_bcnt = o_bbits + 32ull * w.NBT, o_texc = o_bcnt + 8ull * w.NBT,
                 o_bexc = o_texc + 4ull * w.NT, o_nbits = o_bexc + 4ull * w.NBT,
                 bytes = o_nbits + 2ull * BLOCK * w.NT + 16;
    hipMemPool_t pool = sweep_pool(t->device);
    const hipError_t e = pool ? hipMallocFromPoolAsync(&w.mem, bytes, pool, s) : hipMallocAsync(&w.mem, bytes, s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        w.mem = nullptr;
        return set_err(KAD_ERR_NOMEM, "sweep: hipMallocAsync(%zu) failed: %s", bytes, hipGetErrorString(e));
    }
    uint8_t* m = static_cast<uint8_t*>(w.mem);
    w.part = reinterpret_cast<uint4*>(m);
    w.bbits = reinterpret_cast<unsigned long long*>(m + o_bbits);
    w.bcnt = reinterpret_cast<uint2*>(m + o_bcnt);
    w.texc = reinterpret_cast<uint32_t*>(m + o_texc);
    w.bexc = reinterpret_cast<uint32_t*>(m + o_bexc);
    w.nbits = reinterpret_cast<unsigned short*>(m + o_nbits);
    const bool inc = (flags & KAD_SWEEP_INCOMING) != 0;
    if (w.NT)
        hipLaunchKernelGGL(sweep_count_kernel, dim3(w.NT), dim3(BLOCK), 0, s, d.status, d.n, inc ? t->time_ns : nullptr,
                           inc ? t->reply_ns : nullptr, w.nbits, w.part);
    if (w.NBT)
        hipLaunchKernelGGL(sweep_bucket_kernel, dim3(w.NBT), dim3(BLOCK), 0, s, d.dir, d.B, w.nbits, w.part, w.bbits,
                           w.bcnt);
    hipLaunchKernelGGL(sweep_scan_kernel, dim3(1), dim3(BLOCK), 0, s, w.part, w.NT, w.texc, w.bcnt, w.NBT, w.bexc, flags,
                       totals);
    HIP_TRY(hipGetLastError());
    return KAD_OK;
}

// The ordered lists of a counted sweep (either may be NULL: not wanted).
int sweep_write(const kad_table* t, const SweepTmp& w, uint32_t* expired_nodes, uint32_t cap_nodes,
                uint32_t* changed_buckets, uint32_t cap_buckets, hipStream_t s) {
    const uint32_t NTw = expired_nodes && cap_nodes ? w.NT : 0, NBTw = changed_buckets && cap_buckets ? w.NBT : 0;
    if (NTw + NBTw == 0) return KAD_OK;
    hipLaunchKernelGGL(sweep_write_kernel, dim3(NTw + NBTw), dim3(BLOCK), 0, s, w.nbits, w.texc, NTw, t->d.index_base,
                       expired_nodes, cap_nodes, w.bbits, w.bexc, changed_buckets, cap_buckets);
    HIP_TRY(hipGetLastError());
    return KAD_OK;
}

// The argument checks of both entry points, answered from the handle's host fields alone.
int sweep_check(const kad_table* t, uint32_t flags, const kad_sweep_totals* totals, const uint32_t* expired_nodes,
                uint32_t cap_nodes, const uint32_t* changed_buckets, uint32_t cap_buckets) {
    if (!t) return set_err(KAD_ERR_INVALID, "NULL table");
    if (!totals) return set_err(KAD_ERR_INVALID, "NULL totals");
    if (flags & ~KAD_SWEEP_INCOMING) return set_err(KAD_ERR_INVALID, "unknown sweep flags 0x%x", flags);
    if ((!expired_nodes && cap_nodes) || (!changed_buckets && cap_buckets))
        return set_err(KAD_ERR_INVALID, "NULL list with a non-zero cap");
    if ((flags & KAD_SWEEP_INCOMING) && !t->time_ns)
        return set_err(KAD_ERR_INVALID, "KAD_SWEEP_INCOMING: kad_table_set_times was not called");
    return KAD_OK;
}

int sweep_run(const kad_table* t, uint32_t flags, kad_sweep_totals* totals, uint32_t* expired_nodes, uint32_t cap_nodes,
              uint32_t* changed_buckets, uint32_t cap_buckets, hipStream_t s) {
    SweepTmp w;
    int rc = sweep_count(t, flags, totals, s, w);
    if (rc == KAD_OK) rc = sweep_write(t, w, expired_nodes, cap_nodes, changed_buckets, cap_buckets, s);
    sweep_release(w, s);
    return rc;
}

}  // namespace

extern "C" {

int kad_table_sweep(const kad_table* t, uint32_t flags, kad_sweep_totals* totals, uint32_t* expired_nodes,
                    uint32_t cap_nodes, uint32_t* changed_buckets, uint32_t cap_buckets, void* stream) {
    if (int rc = sweep_check(t, flags, totals, expired_nodes, cap_nodes, changed_buckets, cap_buckets)) return rc;
    if (((uintptr_t)totals | (uintptr_t)expired_nodes | (uintptr_t)changed_buckets) & 3)
        return set_err(KAD_ERR_INVALID, "device buffers must be 4-byte aligned");
    DeviceGuard g(t->device);
    return sweep_run(t, flags, totals, expired_nodes, cap_nodes, changed_buckets, cap_buckets, (hipStream_t)stream);
}

int kad_table_sweep_host(const kad_table* t, uint32_t flags, kad_sweep_totals* totals, uint32_t* expired_nodes,
                         uint32_t cap_nodes, uint32_t* changed_buckets, uint32_t cap_buckets) {
    if (int rc = sweep_check(t, flags, totals, expired_nodes, cap_nodes, changed_buckets, cap_buckets)) return rc;
    DeviceGuard g(t->device);
    // buffers and a stream of the call's own, ordered after the table's last asynchronous status refresh (as
    // kad_rt_triage_batch_host). One allocation: the totals, then the node list, then the bucket list.
    cap_nodes = std::min(cap_nodes, t->d.n);
    cap_buckets = std::min(cap_buckets, t->d.B);
    uint8_t* buf = nullptr;
    hipStream_t s = nullptr;
    auto done = [&](int r) {
        if (s) (void)hipStreamDestroy(s);
        if (buf) (void)hipFree(buf);
        return r;
    };
    const size_t o_nodes = sizeof(kad_sweep_totals), o_buckets = o_nodes + 4ull * cap_nodes;
    if (hipMalloc((void**)&buf, o_buckets + 4ull * cap_buckets) != hipSuccess) {
        (void)hipGetLastError();
        return done(set_err(KAD_ERR_NOMEM, "sweep host: out of device memory"));
    }
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess)
        return done(set_err(KAD_ERR_HIP, "sweep host: no stream"));
    if (t->mut_async && hipStreamWaitEvent(s, t->mut_ev, 0) != hipSuccess)
        return done(set_err(KAD_ERR_HIP, "sweep host: wait failed"));
    kad_sweep_totals r;
    int rc = sweep_run(t, flags, reinterpret_cast<kad_sweep_totals*>(buf), cap_nodes ? (uint32_t*)(buf + o_nodes) : nullptr,
                       cap_nodes, cap_buckets ? (uint32_t*)(buf + o_buckets) : nullptr, cap_buckets, s);
    if (rc == KAD_OK && hipMemcpyAsync(&r, buf, sizeof(r), hipMemcpyDeviceToHost, s) != hipSuccess)
        rc = set_err(KAD_ERR_HIP, "sweep host: D2H failed");
    hipError_t e = hipStreamSynchronize(s);
    if (rc == KAD_OK && e != hipSuccess) rc = set_err(KAD_ERR_HIP, "sweep host: %s", hipGetErrorString(e));
    if (rc != KAD_OK) return done(rc);
    const uint32_t mn = std::min(r.expired, cap_nodes), mb = std::min(r.changed_buckets, cap_buckets);
    if ((mn && hipMemcpy(expired_nodes, buf + o_nodes, 4ull * mn, hipMemcpyDeviceToHost) != hipSuccess) ||
        (mb && hipMemcpy(changed_buckets, buf + o_buckets, 4ull * mb, hipMemcpyDeviceToHost) != hipSuccess))
        return done(set_err(KAD_ERR_HIP, "sweep host: D2H failed"));
    *totals = r;
    return done(KAD_OK);
}

}  // extern "C"

#endif  // KAD_SWEEP_H
