// kad_searches.hip — trySearchInsert verdicts over a device set of live searches.
// Dht::onNewNode ends with trySearchInsert(node) (dht.cpp:816-849): lower_bound(node->id) in the family's
// std::map<InfoHash, Sp<Search>>, then Search::insertNode (dht.cpp:961-1047) forwards and backwards until the first
// search that refuses. On a node with many live searches nearly every candidate is refused by both neighbours; the
// verdict of a whole tick is one launch here, and the host touches only the searches that accept.
//
// Layout, one family's set of S searches with a slab of `cap` members each:
//   rec    S x 64 bytes  the probe record (kad_searches_plan.h): search ID, threshold ID entry[t-1], n, t, full and
//                        expired bits. A probe of a search is this one line.
//   skey   S x u64       (sets of up to LDS_KEYS searches) the search IDs' top 64 bits, dense, staged in LDS for the
//                        lower bound; ties on the key are resolved from the records' tails
//   rdx    2^B + 1 words (larger sets; B = ceil(log2 S), at most 24): the lower bound of every B-bit key prefix. The
//                        binary search then runs over the one or two records of the candidate's prefix, which are the
//                        neighbours the walks read anyway, instead of log2 S dependent probes of a key array
//   mkey   S x cap x u64, mtail S x cap x 3 words, mflag S x cap bytes: the members. Read only when a candidate passes
//                        the threshold, when the search is not full, or when members lie past the trim position.
// One lane per candidate. A refused candidate costs the lower-bound probes plus the two records beside lb. A walk
// over a run of accepting searches is serial in its lane (no wave-cooperative path).
//
// kad_sr_refill is Dht::refill (dht.cpp:1647-1668) over the same set: the count-14 NodeCache rows
// of the listed searches, then Search::insertNode on every row node in walk order, applied to the slabs and records
// in place by refill_kernel, one wave per search with one list entry per lane.
//
// kad_sr_insert is Search::insertNode on candidates of the caller, any number per listed search and
// each with its own KAD_SN_BAD bit, applied in place by insert_kernel in the same one-wave-per-search form: the accepted
// inserts of a trySearchInsert tick without an upload of the touched lists.
//
// kad_sr_try_insert_tick is a whole tick of trySearchInsert in one call: the candidates stay resident in
// the call's scratch, tick_verdict_kernel gives the verdicts of the candidates that remain plus the stoppers' trim bits,
// the host plans the round (kadplan::sr_round_plan), tick_gather_kernel lays the ready pairs' candidates out as the CSR
// insert_kernel reads, and insert_kernel applies them; round after round until nothing waits.
//
// kad_sr_mark_nodes carries node status changes (Node::setExpired, a reply, the candidate bit) to the
// flag bytes of every list that holds the node: mark_scan_kernel streams the member keys against the tick's sorted batch
// of node IDs, mark_pairs_kernel sets single (search, node) entries, mark_fix_kernel derives the changed searches'
// records again.
//
// kad_sr_step is Dht::searchStep's decision (dht.cpp:1344-1464) on every listed search: step_kernel
// reads a search's flag bytes and n, one lane per search, and answers which entries get a request and whether the search
// is synced or expires (kad_step.h, shared with the host's kad_search_step); with KAD_STEP_APPLY the sends are written to
// the flag bytes and step_expire_kernel empties the searches that expire. kad_sr_mark_entries (entries_kernel) sets and
// clears the step bits of single entries when replies arrive.
//
// kad_sr_step_full is the same step with the two send loops that precede the get loop: the listen
// requests and the announce probes of a synced search, from two more bits of the flag byte (kad_sr_mark_due sets them).
// step_full_kernel and step_kernel are one body (step_lane), here over seven planes and kadstep::decide_full, and the two
// calls are one host body (step_call); step_expire_kernel is shared.
//
// kad_searches_apply changes the membership (Dht::search dht.cpp:1673-1735, Dht::expireSearches
// :1060-1074) and the slab size: the host plans one source word per new search, searches_relayout_kernel gathers the
// records and slabs into new arrays beside the old ones, searches_rdx_kernel rebuilds the prefix directory, and the
// handle's arrays are swapped once everything succeeded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/kadgpu.h"
#include "kad_internal.h"
#include "kad_searches_plan.h"
#include "kad_step.h"

// tests/test_refill_abi.py, test_searches_abi.py and test_searches_apply_abi.py hand the argument checks a zeroed
// buffer for a set: it must read as a set of no searches (S == 0, cap == 0, no pointer followed before the checks end,
// rf_ms == 0); tests/test_sr_insert_abi.py does the same (in_ms == 0), and tests/test_sr_mark_abi.py (no mark scratch,
// mk_ms == 0), tests/test_sr_tick_abi.py (S == 0 answers before anything else of the set is read) and
// tests/test_sr_step_abi.py and tests/test_sr_stepfull_abi.py (no step events).
struct kad_searches {
    int device = 0;
    uint32_t S = 0, cap = 0;
    uint32_t* rec = nullptr;
    uint64_t* skey = nullptr;
    uint64_t* mkey = nullptr;
    uint32_t* mtail = nullptr;
    uint8_t* mflag = nullptr;
    uint32_t* rdx = nullptr;
    uint32_t rshift = 0;  // 64 - B
    uint64_t bytes = 0;
    std::vector<uint8_t> h_ids;  // S x 20: a patch checks its lists against the search IDs
    hipEvent_t rf_ev[2] = {nullptr, nullptr};  // around the last kad_sr_refill's refill kernel
    float rf_ms = 0.f;
    hipEvent_t in_ev[2] = {nullptr, nullptr};  // around the last kad_sr_insert's insert kernel
    float in_ms = 0.f;
    // kad_sr_mark_nodes' scratch, allocated by the first call and again when the set outgrew it: the count of changed
    // searches, their (search, count word) pairs, the dirty bitmap and the changed list, for mk_cap searches
    uint8_t* mk_buf = nullptr;
    uint32_t mk_cap = 0;
    uint64_t mk_bytes = 0;
    hipEvent_t mk_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // around the last call's scan and fix kernels
    float mk_ms[2] = {0.f, 0.f};
    // around a kad_sr_try_insert_tick round's verdict kernel, and around its gather and insert kernels
    hipEvent_t tk_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t sp_ev[2] = {nullptr, nullptr};  // around the last kad_sr_step's or kad_sr_step_full's kernels
};

namespace {

using kadgpu_internal::set_error;
using kadplan::SREC_BITS;
using kadplan::SREC_EXPIRED;
using kadplan::SREC_FULL;
using kadplan::SREC_N;
using kadplan::SREC_T;
using kadplan::SREC_THR;
using kadplan::SREC_WORDS;

constexpr int BLOCK = 256;
constexpr uint32_t LDS_KEYS = 4096;   // 32 KB of search keys per workgroup
constexpr uint32_t MAX_GRID = 2048;   // grid-stride beyond: the LDS staging is paid per workgroup
constexpr uint32_t ACCEPT = 0xFFu;
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

#define SR_HIP_TRY(expr)                                                                            \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return set_error(KAD_ERR_HIP, (std::string(#expr " failed: ") + hipGetErrorString(e_)).c_str()); \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// What a call that changes the set holds while it runs: the set's device made current, the call's one device allocation
// and its host staging buffer (a new[] array handed over, or none), both released when the scope ends.
struct CallScratch {
    DeviceGuard g;
    uint8_t* buf = nullptr;
    uint8_t* h;
    explicit CallScratch(int dev, uint8_t* host = nullptr) : g(dev), h(host) {}
    CallScratch(const CallScratch&) = delete;
    CallScratch& operator=(const CallScratch&) = delete;
    ~CallScratch() {
        if (buf) (void)hipFree(buf);
        delete[] h;
    }
    // Waits for everything enqueued before the call (queries enqueued before it read the old set), then allocates
    // `bytes` of device memory. KAD_OK, or the error set with `what` as its prefix.
    int open(size_t bytes, const char* what) {
        if (hipDeviceSynchronize() != hipSuccess)
            return set_error(KAD_ERR_HIP, (std::string(what) + ": device in error").c_str());
        if (hipMalloc((void**)&buf, bytes) != hipSuccess) {
            (void)hipGetLastError();
            buf = nullptr;
            return set_error(KAD_ERR_NOMEM, (std::string(what) + ": out of device memory").c_str());
        }
        return KAD_OK;
    }
};

// the handle's timing events, created by the first call that needs them
template <size_t N>
bool have_events(hipEvent_t (&ev)[N]) {
    for (hipEvent_t& e : ev)
        if (!e && hipEventCreate(&e) != hipSuccess) return false;
    return true;
}

float elapsed_or_zero(hipEvent_t ev0, hipEvent_t ev1) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev0, ev1) != hipSuccess) {
        (void)hipGetLastError();
        ms = 0.f;
    }
    return ms;
}

struct DevSearches {
    const u32x4_t* rec;
    const uint64_t* skey;
    const uint64_t* mkey;
    const uint32_t* mtail;
    const uint32_t* rdx;
    uint32_t S, cap, rshift;
};

struct Rec {
    u32x4_t r0, r1, r2, r3;
};

__device__ __forceinline__ Rec load_rec(const DevSearches& D, uint32_t s) {
    const u32x4_t* r = D.rec + 4ull * s;
    return Rec{r[0], r[1], r[2], r[3]};
}

struct Cand {
    uint64_t hi;
    uint32_t t2, t3, t4;
};

__device__ __forceinline__ Cand load_cand(const uint8_t* ids, uint32_t i) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(ids + 20ull * i);
    const uint32_t w0 = __builtin_nontemporal_load(p), w1 = __builtin_nontemporal_load(p + 1),
                   w2 = __builtin_nontemporal_load(p + 2), w3 = __builtin_nontemporal_load(p + 3),
                   w4 = __builtin_nontemporal_load(p + 4);
    Cand c;
    c.hi = ((uint64_t)__builtin_bswap32(w0) << 32) | __builtin_bswap32(w1);
    c.t2 = __builtin_bswap32(w2);
    c.t3 = __builtin_bswap32(w3);
    c.t4 = __builtin_bswap32(w4);
    return c;
}

// (a2, a3, a4) < (b2, b3, b4) as 96-bit numbers
__device__ __forceinline__ bool tail_less(uint32_t a2, uint32_t a3, uint32_t a4, uint32_t b2, uint32_t b3,
                                          uint32_t b4) {
    if (a2 != b2) return a2 < b2;
    if (a3 != b3) return a3 < b3;
    return a4 < b4;
}

// x among the members [a, e) of search s (e <= n <= cap): keys eight at a time, none predicated (an index past the
// range is clamped to its last entry), a member's tail only when its key equals the candidate's.
__device__ __forceinline__ bool member(const DevSearches& D, uint32_t s, uint32_t a, uint32_t e, const Cand& x) {
    const uint64_t* mk = D.mkey + (uint64_t)s * D.cap;
    const uint32_t* mt = D.mtail + 3ull * s * D.cap;
    for (uint32_t c = a; c < e; c += 8) {
        uint64_t k[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) k[u] = mk[min(c + u, e - 1u)];
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) {
            if (c + u < e && k[u] == x.hi) {
                const uint32_t* tl = mt + 3ull * (c + u);
                if (tl[0] == x.t2 && tl[1] == x.t3 && tl[2] == x.t4) return true;
            }
        }
    }
    return false;
}

// accept(s, x) with R = the record of s: ACCEPT, or the stop code of the refusal.
__device__ __forceinline__ uint32_t probe(const DevSearches& D, uint32_t s, const Rec& R, const Cand& x) {
    const u32x4_t r0 = R.r0, r1 = R.r1, r2 = R.r2, r3 = R.r3;
    const uint64_t ihi = ((uint64_t)r0.y << 32) | r0.x;
    const uint32_t n = r1.y, t = r2.w, bits = r3.x;
    if (bits & SREC_FULL) {  // t >= KAD_SEARCH_NODES: the threshold entry[t-1] exists
        const uint64_t thi = ((uint64_t)r1.w << 32) | r1.z;
        // XOR distances to the search ID: the u64 key first, the 96-bit tail only on equality
        const uint64_t dx = x.hi ^ ihi, dt = thi ^ ihi;
        bool closer;
        if (dx != dt) {
            closer = dx < dt;
        } else {
            closer = tail_less(x.t2 ^ r0.z, x.t3 ^ r0.w, x.t4 ^ r1.x, r2.x ^ r0.z, r2.y ^ r0.w, r2.z ^ r1.x);
        }
        if (!closer) {
            const bool is_thr = x.hi == thi && x.t2 == r2.x && x.t3 == r2.y && x.t4 == r2.z;
            if (is_thr || (n > t && member(D, s, t, n, x))) return KAD_SR_STOP_KNOWN;
            return (bits & SREC_EXPIRED) ? KAD_SR_STOP_FAR_EXPIRED : KAD_SR_STOP_FAR;
        }
        // strictly closer than entry[t-1]: only entries before it can have x's ID
        return member(D, s, 0, t - 1u, x) ? KAD_SR_STOP_KNOWN : ACCEPT;
    }
    return (n && member(D, s, 0, n, x)) ? KAD_SR_STOP_KNOWN : ACCEPT;
}

template <bool LDS>
__global__ __launch_bounds__(BLOCK) void try_insert_kernel(DevSearches D, const uint8_t* __restrict__ ids, uint32_t q,
                                                           uint32_t* __restrict__ out_lb, uint32_t* __restrict__ out_fwd,
                                                           uint32_t* __restrict__ out_back,
                                                           uint8_t* __restrict__ out_stop) {
    __shared__ uint64_t sk[LDS ? LDS_KEYS : 1];
    if (LDS) {
        for (uint32_t j = threadIdx.x; j < D.S; j += BLOCK) sk[j] = D.skey[j];
        __syncthreads();
    }
    for (uint64_t i0 = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i0 < q; i0 += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t i = (uint32_t)i0;
        uint32_t lb = 0, fwd = 0, back = 0, fstop = KAD_SR_STOP_END, bstop = KAD_SR_STOP_END;
        if (D.S) {  // kernel-uniform
            const Cand x = load_cand(ids, i);
            // lower_bound over the 160-bit search IDs: the keys, a record's tail only on a key tie
            uint32_t lo = 0, hi = D.S;
            if (!LDS) {  // the searches of the candidate's key prefix
                const uint32_t p = (uint32_t)(x.hi >> D.rshift);
                lo = D.rdx[p];
                hi = D.rdx[p + 1];
            }
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                // large sets compare against the record itself: within a prefix the probed records are the
                // neighbours the walks read next, and a dense key array would be one more dependent random line
                const u32x4_t* r = D.rec + 4ull * mid;
                u32x4_t r0 = {};
                if (!LDS) r0 = r[0];
                const uint64_t k = LDS ? sk[mid] : (((uint64_t)r0.y << 32) | r0.x);
                bool less = k < x.hi;
                if (k == x.hi) {
                    if (LDS) r0 = r[0];
                    less = tail_less(r0.z, r0.w, r[1].x, x.t2, x.t3, x.t4);
                }
                if (less)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            lb = lo;
            // both neighbours' records in flight together: the common candidate is refused by each at once
            Rec rf = load_rec(D, min(lb, D.S - 1u)), rb = load_rec(D, max(lb, 1u) - 1u);
            for (uint32_t s = lb; s < D.S;) {  // insert forward (dht.cpp:826-836)
                const uint32_t v = probe(D, s, rf, x);
                if (v != ACCEPT) {
                    fstop = v;
                    break;
                }
                fwd++;
                if (++s < D.S) rf = load_rec(D, s);
            }
            for (uint32_t s = lb; s > 0;) {  // insert backward (dht.cpp:837-847)
                const uint32_t v = probe(D, --s, rb, x);
                if (v != ACCEPT) {
                    bstop = v;
                    break;
                }
                back++;
                if (s > 0) rb = load_rec(D, s - 1u);
            }
        }
        if (out_lb) __builtin_nontemporal_store(lb, out_lb + i);
        __builtin_nontemporal_store(fwd, out_fwd + i);
        __builtin_nontemporal_store(back, out_back + i);
        __builtin_nontemporal_store((uint8_t)(fstop | (bstop << 4)), out_stop + i);
    }
}

int launch(const kad_searches* ss, const uint8_t* ids, uint32_t q, uint32_t* out_lb, uint32_t* out_fwd,
           uint32_t* out_back, uint8_t* out_stop, hipStream_t s) {
    const DevSearches D{reinterpret_cast<const u32x4_t*>(ss->rec), ss->skey, ss->mkey, ss->mtail, ss->rdx, ss->S, ss->cap,
                        ss->rshift};
    const uint32_t blocks = (q + BLOCK - 1) / BLOCK, grid = blocks < MAX_GRID ? blocks : MAX_GRID;
    if (ss->S <= LDS_KEYS)
        hipLaunchKernelGGL(try_insert_kernel<true>, dim3(grid), dim3(BLOCK), 0, s, D, ids, q, out_lb, out_fwd, out_back,
                           out_stop);
    else
        hipLaunchKernelGGL(try_insert_kernel<false>, dim3(grid), dim3(BLOCK), 0, s, D, ids, q, out_lb, out_fwd,
                           out_back, out_stop);
    SR_HIP_TRY(hipGetLastError());
    return KAD_OK;
}

// ---- kad_sr_try_insert_tick's verdicts ------------------------------------------------------------
// try_insert_kernel's walk over a subset of the candidates resident in the call's scratch: lane i takes candidate
// rem[i] (NULL: candidate i, the first round). A FAR / FAR_EXPIRED refusal also reads, from the stopper's record the
// walk holds in registers, whether the refusal cuts that search's list (full and t < n): the round's plan needs nothing
// else about the searches. One 16-byte store per candidate: {lb, fwd, back, fstop | bstop << 4 | trim << 8}.
__device__ __forceinline__ uint32_t refusal_trims(const Rec& R, uint32_t v) {
    return (v == KAD_SR_STOP_FAR || v == KAD_SR_STOP_FAR_EXPIRED) && (R.r3.x & SREC_FULL) && R.r2.w < R.r1.y ? 1u : 0u;
}

template <bool LDS>
__global__ __launch_bounds__(BLOCK) void tick_verdict_kernel(DevSearches D, const uint8_t* __restrict__ ids,
                                                             const uint32_t* __restrict__ rem, uint32_t r,
                                                             u32x4_t* __restrict__ out) {
    __shared__ uint64_t sk[LDS ? LDS_KEYS : 1];
    if (LDS) {
        for (uint32_t j = threadIdx.x; j < D.S; j += BLOCK) sk[j] = D.skey[j];
        __syncthreads();
    }
    for (uint64_t i0 = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i0 < r; i0 += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t i = (uint32_t)i0;
        const Cand x = load_cand(ids, rem ? rem[i] : i);
        // lower_bound over the 160-bit search IDs, as try_insert_kernel (D.S > 0 here)
        uint32_t lo = 0, hi = D.S;
        if (!LDS) {
            const uint32_t p = (uint32_t)(x.hi >> D.rshift);
            lo = D.rdx[p];
            hi = D.rdx[p + 1];
        }
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            const u32x4_t* rr = D.rec + 4ull * mid;
            u32x4_t r0 = {};
            if (!LDS) r0 = rr[0];
            const uint64_t k = LDS ? sk[mid] : (((uint64_t)r0.y << 32) | r0.x);
            bool less = k < x.hi;
            if (k == x.hi) {
                if (LDS) r0 = rr[0];
                less = tail_less(r0.z, r0.w, rr[1].x, x.t2, x.t3, x.t4);
            }
            if (less)
                lo = mid + 1;
            else
                hi = mid;
        }
        const uint32_t lb = lo;
        uint32_t fwd = 0, back = 0, fstop = KAD_SR_STOP_END, bstop = KAD_SR_STOP_END, trim = 0;
        Rec rf = load_rec(D, min(lb, D.S - 1u)), rb = load_rec(D, max(lb, 1u) - 1u);
        for (uint32_t s = lb; s < D.S;) {  // insert forward (dht.cpp:826-836)
            const uint32_t v = probe(D, s, rf, x);
            if (v != ACCEPT) {
                fstop = v;
                trim = refusal_trims(rf, v);
                break;
            }
            fwd++;
            if (++s < D.S) rf = load_rec(D, s);
        }
        for (uint32_t s = lb; s > 0;) {  // insert backward (dht.cpp:837-847)
            const uint32_t v = probe(D, --s, rb, x);
            if (v != ACCEPT) {
                bstop = v;
                trim |= refusal_trims(rb, v) << 1;
                break;
            }
            back++;
            if (s > 0) rb = load_rec(D, s - 1u);
        }
        const u32x4_t v = {lb, fwd, back, fstop | (bstop << 4) | (trim << 8)};
        __builtin_nontemporal_store(v, out + i);
    }
}

// ---- kad_sr_refill: Dht::refill over the set ------------------------------------------------------
// One wave per listed search, one list entry per lane (cap <= 64). An entry lives in its lane's registers as the XOR
// distance of its ID to the search ID plus its flag byte; Search::insertNode (dht.cpp:961-1047) is then ballots,
// popcounts and one-lane shifts, and the slab and the record are written once at the end.
constexpr uint32_t REFILL_MAX_CAP = 64;
constexpr uint32_t REFILL_WAVES = BLOCK / 64;

struct Ent {
    uint32_t k0, k1, d2, d3, d4, fl;  // distance words, k1 the most significant; fl the flag byte
};

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

__device__ __forceinline__ uint32_t word_from(uint32_t v, uint32_t src_lane) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src_lane << 2), (int)v);
}

// every lane takes the entry of its lane src (a one-lane shift of the list)
__device__ __forceinline__ Ent ent_from(const Ent& e, uint32_t src) {
    return Ent{word_from(e.k0, src), word_from(e.k1, src), word_from(e.d2, src),
               word_from(e.d3, src), word_from(e.d4, src), word_from(e.fl, src)};
}

// the entry of one lane, wave-uniform
__device__ __forceinline__ Ent ent_of_lane(const Ent& e, uint32_t l) {
    return Ent{(uint32_t)__builtin_amdgcn_readlane((int)e.k0, (int)l), (uint32_t)__builtin_amdgcn_readlane((int)e.k1, (int)l),
               (uint32_t)__builtin_amdgcn_readlane((int)e.d2, (int)l), (uint32_t)__builtin_amdgcn_readlane((int)e.d3, (int)l),
               (uint32_t)__builtin_amdgcn_readlane((int)e.d4, (int)l), (uint32_t)__builtin_amdgcn_readlane((int)e.fl, (int)l)};
}

__device__ __forceinline__ bool ent_same(const Ent& a, const Ent& b) {
    return a.k0 == b.k0 && a.k1 == b.k1 && a.d2 == b.d2 && a.d3 == b.d3 && a.d4 == b.d4;
}

// a closer than b: the u64 key first, the tail only on equality
__device__ __forceinline__ bool ent_closer(const Ent& a, const Ent& b) {
    const uint64_t ka = ((uint64_t)a.k1 << 32) | a.k0, kb = ((uint64_t)b.k1 << 32) | b.k0;
    if (ka != kb) return ka < kb;
    return tail_less(a.d2, a.d3, a.d4, b.d2, b.d3, b.d4);
}

// The index of the 15th entry that is not BAD, n if there is none: where the trim loop (dht.cpp:1002-1006) and the
// pop loop (:1031-1035) of a live search both stop. goodm: the ballot of the entries that are not BAD.
__device__ __forceinline__ uint32_t fifteenth_good(uint64_t goodm, uint32_t lane, uint32_t n) {
    const bool hit = ((goodm >> lane) & 1ull) && __popcll(goodm & ((1ull << lane) - 1ull)) == (int)KAD_SEARCH_NODES;
    const uint64_t b = __ballot(hit);
    return b ? (uint32_t)__builtin_ctzll(b) : n;
}

// kad_search_trim over the wave (n <= 64)
__device__ __forceinline__ void wave_trim(bool expired, uint32_t n, uint64_t goodm, uint32_t lane, bool& full,
                                          uint32_t& t) {
    if (expired) {
        full = n >= KAD_SEARCH_NODES;
        t = full ? KAD_SEARCH_NODES : n;
    } else {
        full = (uint32_t)__popcll(goodm) >= KAD_SEARCH_NODES;
        t = fifteenth_good(goodm, lane, n);
    }
}

__global__ __launch_bounds__(BLOCK) void refill_targets_kernel(const uint32_t* __restrict__ rec,
                                                               const uint32_t* __restrict__ which, uint32_t m,
                                                               uint32_t* __restrict__ targets) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m) return;
    const uint32_t* r = rec + (uint64_t)SREC_WORDS * which[i];
    uint32_t* t = targets + 5ull * i;  // the search ID as its 20 bytes
    t[0] = __builtin_bswap32(r[1]);
    t[1] = __builtin_bswap32(r[0]);
    t[2] = __builtin_bswap32(r[2]);
    t[3] = __builtin_bswap32(r[3]);
    t[4] = __builtin_bswap32(r[4]);
}

struct DevRefill {
    uint32_t* rec;
    uint64_t* mkey;
    uint32_t* mtail;
    uint8_t* mflag;
    uint32_t cap;
    const uint64_t* nkey;  // the NodeCache table's node IDs
    const uint32_t* ntail;
    uint32_t nn, index_base;
};

__global__ __launch_bounds__(BLOCK) void refill_kernel(DevRefill D, const uint32_t* __restrict__ which, uint32_t m,
                                                       const uint32_t* __restrict__ rows,
                                                       const uint8_t* __restrict__ cnts,
                                                       uint16_t* __restrict__ out_ins, uint8_t* __restrict__ out_status) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = rfl(blockIdx.x * REFILL_WAVES + (threadIdx.x >> 6));
    if (i >= m) return;
    const uint32_t s = rfl(which[i]);
    const uint32_t cnt = D.nn ? min(rfl(cnts[i]), KAD_SEARCH_NODES) : 0u;
    // the row's node IDs one per lane, the record and the slab: all loads in flight together
    Ent c = {};
    if (lane < cnt) {
        const uint32_t j = min(rows[KAD_SEARCH_NODES * (uint64_t)i + lane] - D.index_base, D.nn - 1u);
        const uint64_t k = D.nkey[j];
        const uint32_t* tl = D.ntail + 3ull * j;
        c = Ent{(uint32_t)k, (uint32_t)(k >> 32), tl[0], tl[1], tl[2], 0u};
    }
    uint32_t* r = D.rec + (uint64_t)SREC_WORDS * s;
    const uint32_t s0 = rfl(r[0]), s1 = rfl(r[1]), s2 = rfl(r[2]), s3 = rfl(r[3]), s4 = rfl(r[4]);
    uint32_t n = min(rfl(r[SREC_N]), D.cap);
    bool expired = (rfl(r[SREC_BITS]) & SREC_EXPIRED) != 0;
    const uint64_t e0 = (uint64_t)s * D.cap + lane;
    Ent e = {};
    if (lane < n) {
        const uint64_t k = D.mkey[e0];
        const uint32_t* tl = D.mtail + 3ull * e0;
        e = Ent{(uint32_t)k ^ s0, (uint32_t)(k >> 32) ^ s1, tl[0] ^ s2, tl[1] ^ s3, tl[2] ^ s4, D.mflag[e0]};
    }
    c.k0 ^= s0;
    c.k1 ^= s1;
    c.d2 ^= s2;
    c.d3 ^= s3;
    c.d4 ^= s4;

    uint32_t ins = 0;
    bool dirty = false, overflow = false;
    // Lanes at or beyond n hold stale entries by design (a trim or a pop only lowers n): every ballot below masks with
    // lane < n, a shift up writes lane n before n grows, and the final store writes zeros past n.
    for (uint32_t j = 0; j < cnt; j++) {  // sr.insertNode(row[j], now), dht.cpp:1659-1663
        const Ent x = ent_of_lane(c, j);
        const bool valid = lane < n;  // n <= cap here
        if (__ballot(valid && ent_same(e, x))) continue;  // found (:972-984)
        const uint32_t pos = (uint32_t)__popcll(__ballot(valid && ent_closer(e, x)));
        bool full;
        uint32_t t;
        wave_trim(expired, n, __ballot(valid && !(e.fl & KAD_SN_BAD)), lane, full, t);
        if (full) {  // :1009-1013
            if (t < n) {
                n = t;
                dirty = true;
            }
            if (pos >= t) continue;
        }
        // insert at pos; a list of cap = 64 entries holds its 65th, wave-uniform, until the pops and the erase
        Ent sp = {};
        bool has_sp = false;
        const Ent up = ent_from(e, (lane - 1u) & 63u);
        if (n == 64u) {
            sp = pos == 64u ? x : ent_of_lane(e, 63u);
            has_sp = true;
        }
        if (lane == pos)
            e = x;
        else if (lane > pos)
            e = up;
        n++;
        dirty = true;
        if (expired) {  // a good node revives the search; bad = size - 1, so nothing is popped (:1026-1029)
            expired = false;
        } else {  // the pop loop (:1031-1035): back to the 15th entry that is not BAD
            const uint64_t goodm = __ballot(lane < min(n, 64u) && !(e.fl & KAD_SN_BAD));
            const uint32_t g = (uint32_t)__popcll(goodm);
            if (g > KAD_SEARCH_NODES)
                n = fifteenth_good(goodm, lane, n);
            else if (has_sp && g == KAD_SEARCH_NODES && !(sp.fl & KAD_SN_BAD))
                n = 64u;
            if (n <= 64u) has_sp = false;
        }
        // removeExpiredNode (dht.h:628-640): the REMOVABLE entry with the greatest index
        const uint64_t rm = __ballot(lane < min(n, 64u) && (e.fl & KAD_SN_REMOVABLE));
        if (has_sp && (sp.fl & KAD_SN_REMOVABLE)) {
            n = 64u;
            has_sp = false;
        } else if (rm) {
            const uint32_t at = 63u - (uint32_t)__builtin_clzll(rm);
            Ent dn = ent_from(e, (lane + 1u) & 63u);
            if (has_sp && lane == 63u) dn = sp;
            if (lane >= at) e = dn;
            n--;
            has_sp = false;
        }
        ins |= 1u << j;
        if (n > D.cap) {
            overflow = true;
            break;
        }
    }

    if (dirty && !overflow) {  // the slab and the record as kad_searches_create derives them from the new list
        const bool in = lane < n;
        if (lane < D.cap) {
            D.mkey[e0] = in ? ((uint64_t)(e.k1 ^ s1) << 32) | (e.k0 ^ s0) : 0ull;
            uint32_t* tl = D.mtail + 3ull * e0;
            tl[0] = in ? e.d2 ^ s2 : 0u;
            tl[1] = in ? e.d3 ^ s3 : 0u;
            tl[2] = in ? e.d4 ^ s4 : 0u;
            D.mflag[e0] = in ? (uint8_t)e.fl : (uint8_t)0;
        }
        bool full;
        uint32_t t;
        wave_trim(expired, n, __ballot(in && !(e.fl & KAD_SN_BAD)), lane, full, t);
        if (lane + 1u == t || (t == 0 && lane == 0)) {  // the threshold entry[t-1], zero for t == 0
            r[SREC_THR] = t ? e.k0 ^ s0 : 0u;
            r[SREC_THR + 1] = t ? e.k1 ^ s1 : 0u;
            r[SREC_THR + 2] = t ? e.d2 ^ s2 : 0u;
            r[SREC_THR + 3] = t ? e.d3 ^ s3 : 0u;
            r[SREC_THR + 4] = t ? e.d4 ^ s4 : 0u;
        }
        if (lane == 0) {
            r[SREC_N] = n;
            r[SREC_T] = t;
            r[SREC_BITS] = (full ? SREC_FULL : 0u) | (expired ? SREC_EXPIRED : 0u);
        }
    }
    if (lane == 0) {
        out_ins[i] = overflow ? (uint16_t)0 : (uint16_t)ins;
        out_status[i] = overflow ? (uint8_t)KAD_SR_REFILL_OVERFLOW : (uint8_t)KAD_SR_REFILL_OK;
    }
}

// ---- kad_sr_insert: Search::insertNode on candidates of the caller --------------------------------
// refill_kernel's insert step for any number of candidates per search, each with its own KAD_SN_BAD bit: one wave per
// listed search, one list entry per lane, the candidates of search which[i] at off[i] .. off[i+1] of the uploaded CSR.
// They are loaded one per lane, 64 at a time, the next chunk's loads issued before the current chunk's inserts; the
// candidate of a step is broadcast from its lane (v_readlane with a wave-uniform lane number).
struct DevInsert {
    uint32_t* rec;
    uint64_t* mkey;
    uint32_t* mtail;
    uint8_t* mflag;
    uint32_t cap, m;
    const uint32_t* which;  // m
    const uint32_t* off;    // m + 1
    const uint8_t* ids;     // off[m] x 20 B
    const uint8_t* flags;   // off[m]
    uint8_t* out_ins;       // off[m]
    uint8_t* out_status;    // m
};

// candidate `at` of [.., end) as an entry of the search with ID words s0..s4 (load_cand's byte order): its XOR distance
// and KAD_SN_BAD; zero past the end
__device__ __forceinline__ Ent load_cand_ent(const DevInsert& D, uint32_t at, uint32_t end, uint32_t s0, uint32_t s1,
                                             uint32_t s2, uint32_t s3, uint32_t s4) {
    Ent c = {};
    if (at < end) {
        const Cand x = load_cand(D.ids, at);
        c = Ent{(uint32_t)x.hi ^ s0, (uint32_t)(x.hi >> 32) ^ s1, x.t2 ^ s2, x.t3 ^ s3, x.t4 ^ s4,
                (uint32_t)__builtin_nontemporal_load(D.flags + at) & KAD_SN_BAD};
    }
    return c;
}

__global__ __launch_bounds__(BLOCK) void insert_kernel(DevInsert D) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = rfl(blockIdx.x * REFILL_WAVES + (threadIdx.x >> 6));
    if (i >= D.m) return;
    const uint32_t s = rfl(D.which[i]), a = rfl(D.off[i]), b = rfl(D.off[i + 1]);
    if (a >= b) {  // an empty list: the search is untouched
        if (lane == 0) D.out_status[i] = (uint8_t)KAD_SR_INSERT_OK;
        return;
    }
    // the record, the slab and the first chunk of candidates: all loads in flight together
    uint32_t* r = D.rec + (uint64_t)SREC_WORDS * s;
    const uint32_t s0 = rfl(r[0]), s1 = rfl(r[1]), s2 = rfl(r[2]), s3 = rfl(r[3]), s4 = rfl(r[4]);
    uint32_t n = min(rfl(r[SREC_N]), D.cap);
    bool expired = (rfl(r[SREC_BITS]) & SREC_EXPIRED) != 0;
    const uint64_t e0 = (uint64_t)s * D.cap + lane;
    Ent e = {};
    if (lane < n) {
        const uint64_t k = D.mkey[e0];
        const uint32_t* tl = D.mtail + 3ull * e0;
        e = Ent{(uint32_t)k ^ s0, (uint32_t)(k >> 32) ^ s1, tl[0] ^ s2, tl[1] ^ s3, tl[2] ^ s4, D.mflag[e0]};
    }
    Ent c = load_cand_ent(D, a + lane, b, s0, s1, s2, s3, s4);

    bool dirty = false, overflow = false;
    // Lanes at or beyond n hold stale entries by design, as in refill_kernel: every ballot masks with lane < n.
    for (uint32_t base = a; base < b && !overflow; base += 64u) {
        const uint32_t cnt = min(b - base, 64u);
        const Ent nx = load_cand_ent(D, base + 64u + lane, b, s0, s1, s2, s3, s4);  // in flight during the inserts
        uint64_t insm = 0;
        for (uint32_t j = 0; j < cnt; j++) {  // s.insertNode(x, now), dht.cpp:961-1047
            const Ent x = ent_of_lane(c, j);
            const bool valid = lane < n;  // n <= cap here
            if (__ballot(valid && ent_same(e, x))) continue;  // found (:972-984), a repeated candidate included
            const uint32_t pos = (uint32_t)__popcll(__ballot(valid && ent_closer(e, x)));
            bool full;
            uint32_t t;
            wave_trim(expired, n, __ballot(valid && !(e.fl & KAD_SN_BAD)), lane, full, t);
            if (full) {  // :1009-1013
                if (t < n) {
                    n = t;
                    dirty = true;
                }
                if (pos >= t) continue;
            }
            // insert at pos; a list of cap = 64 entries holds its 65th, wave-uniform, until the pops and the erase
            Ent sp = {};
            bool has_sp = false;
            const Ent up = ent_from(e, (lane - 1u) & 63u);
            if (n == 64u) {
                sp = pos == 64u ? x : ent_of_lane(e, 63u);
                has_sp = true;
            }
            if (lane == pos)
                e = x;
            else if (lane > pos)
                e = up;
            n++;
            dirty = true;
            if (expired) {
                if (x.fl & KAD_SN_BAD)  // bad stays 0 and the search expired: the pops cut to SEARCH_NODES entries
                    n = min(n, KAD_SEARCH_NODES);
                else  // a good node revives the search; bad = size - 1, so nothing is popped (:1026-1029)
                    expired = false;
            } else {  // the pop loop (:1031-1035): back to the 15th entry that is not BAD, the new one counted
                const uint64_t goodm = __ballot(lane < min(n, 64u) && !(e.fl & KAD_SN_BAD));
                const uint32_t g = (uint32_t)__popcll(goodm);
                if (g > KAD_SEARCH_NODES)
                    n = fifteenth_good(goodm, lane, n);
                else if (has_sp && g == KAD_SEARCH_NODES && !(sp.fl & KAD_SN_BAD))
                    n = 64u;
            }
            if (n <= 64u) has_sp = false;
            // removeExpiredNode (dht.h:628-640): the REMOVABLE entry with the greatest index; never the new one, whose
            // node.time = now comes first
            const uint64_t rm = __ballot(lane < min(n, 64u) && (e.fl & KAD_SN_REMOVABLE));
            if (has_sp && (sp.fl & KAD_SN_REMOVABLE)) {
                n = 64u;
                has_sp = false;
            } else if (rm) {
                const uint32_t at = 63u - (uint32_t)__builtin_clzll(rm);
                Ent dn = ent_from(e, (lane + 1u) & 63u);
                if (has_sp && lane == 63u) dn = sp;
                if (lane >= at) e = dn;
                n--;
                has_sp = false;
            }
            insm |= 1ull << j;
            if (n > D.cap) {
                overflow = true;
                break;
            }
        }
        if (!overflow && lane < cnt) __builtin_nontemporal_store((uint8_t)((insm >> lane) & 1ull), D.out_ins + base + lane);
        c = nx;
    }
    if (overflow)  // the search stays as it was: every result byte of its list is 0
        for (uint32_t at = a + lane; at < b; at += 64u) __builtin_nontemporal_store((uint8_t)0, D.out_ins + at);

    if (dirty && !overflow) {  // the slab and the record as kad_searches_create derives them from the new list
        const bool in = lane < n;
        if (lane < D.cap) {
            D.mkey[e0] = in ? ((uint64_t)(e.k1 ^ s1) << 32) | (e.k0 ^ s0) : 0ull;
            uint32_t* tl = D.mtail + 3ull * e0;
            tl[0] = in ? e.d2 ^ s2 : 0u;
            tl[1] = in ? e.d3 ^ s3 : 0u;
            tl[2] = in ? e.d4 ^ s4 : 0u;
            D.mflag[e0] = in ? (uint8_t)e.fl : (uint8_t)0;
        }
        bool full;
        uint32_t t;
        wave_trim(expired, n, __ballot(in && !(e.fl & KAD_SN_BAD)), lane, full, t);
        if (lane + 1u == t || (t == 0 && lane == 0)) {  // the threshold entry[t-1], zero for t == 0
            r[SREC_THR] = t ? e.k0 ^ s0 : 0u;
            r[SREC_THR + 1] = t ? e.k1 ^ s1 : 0u;
            r[SREC_THR + 2] = t ? e.d2 ^ s2 : 0u;
            r[SREC_THR + 3] = t ? e.d3 ^ s3 : 0u;
            r[SREC_THR + 4] = t ? e.d4 ^ s4 : 0u;
        }
        if (lane == 0) {
            r[SREC_N] = n;
            r[SREC_T] = t;
            r[SREC_BITS] = (full ? SREC_FULL : 0u) | (expired ? SREC_EXPIRED : 0u);
        }
    }
    if (lane == 0) D.out_status[i] = overflow ? (uint8_t)KAD_SR_INSERT_OVERFLOW : (uint8_t)KAD_SR_INSERT_OK;
}

// kad_sr_try_insert_tick's round inserts: the pairs of a round never share a search, so pair i is the
// one candidate of its search. Its ID and BAD bit are gathered by position from the candidates resident in the call's
// scratch into the CSR insert_kernel reads (off[i] = i), and insert_kernel runs unmodified over it.
__global__ __launch_bounds__(BLOCK) void tick_gather_kernel(const uint8_t* __restrict__ ids,
                                                            const uint8_t* __restrict__ flags,
                                                            const uint32_t* __restrict__ pos, uint32_t m,
                                                            uint32_t* __restrict__ off, uint32_t* __restrict__ gids,
                                                            uint8_t* __restrict__ gflags) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i > m) return;
    off[i] = i;  // m + 1 offsets
    if (i == m) return;
    const uint32_t j = pos[i];
    const uint32_t* p = reinterpret_cast<const uint32_t*>(ids + 20ull * j);
    uint32_t* g = gids + 5ull * i;
    g[0] = p[0];
    g[1] = p[1];
    g[2] = p[2];
    g[3] = p[3];
    g[4] = p[4];
    gflags[i] = flags[j];
}

// ---- kad_sr_mark_nodes: node status changes over the set -----------------------------------------
// A node's isExpired() or time changed: every list that holds it carries a stale flag byte. mark_scan_kernel streams
// the S x cap member keys once, one entry per lane, against the sorted batch of changed IDs; mark_pairs_kernel sets the
// exact byte of single (search, node) pairs (the per-search `candidate` bit); mark_fix_kernel derives the records of the
// searches whose bytes changed again. An entry that a pair names belongs to the pair alone: the scan counts its hit and
// leaves the byte to mark_pairs_kernel, so every byte is written at most once, by one lane, and "changed" compares the
// byte before the call with the one after it.
constexpr uint32_t MARK_LDS_KEYS = kadplan::SR_MARK_SMALL_BATCH;  // 32 KB of batch keys per workgroup, and next to
constexpr uint32_t MARK_LDS_DIR = (1u << kadplan::SR_MARK_DIR_BITS_SMALL) + 1;  // them 4 KB of directory; larger batches
constexpr uint32_t MARK_UNROLL = 4;  // are read through L2. Member keys in flight per lane.
constexpr uint32_t MARK_FIX_GRID = 1024;  // wave-stride beyond
constexpr uint32_t MARK_HEAD_BYTES = 16;

struct DevMark {
    uint32_t* rec;
    const uint64_t* mkey;
    const uint32_t* mtail;
    uint8_t* mflag;
    uint32_t S, cap, total;  // total = S x cap < 2^31
    uint32_t q;              // the batch, ascending by (key, tail)
    const uint64_t* bkey;
    const uint32_t* btail;
    const uint8_t* bop;      // clear | set << 2
    const uint32_t* dir;     // 2^B + 1 words: the lower bound of every B-bit key prefix among the batch keys
    uint32_t dshift;         // 64 - B
    uint32_t p;              // the pairs, ascending by (search, ID)
    const uint32_t* pw;
    const uint64_t* pkey;
    const uint32_t* ptail;
    const uint8_t* pfl;
    uint32_t* hits;          // q, by batch position; NULL when the caller does not ask for them
    uint8_t* found;          // p, by pair position
    uint32_t* head;          // the number of changed searches
    uint32_t* bitmap;        // one bit per search: some byte of it changed
    uint32_t* list;          // the changed searches in the order they were first marked
};

// search s changed: the lane that flips its bit appends it to the list
__device__ __forceinline__ void mark_dirty(const DevMark& D, uint32_t s) {
    const uint32_t bit = 1u << (s & 31u);
    if (!(atomicOr(D.bitmap + (s >> 5), bit) & bit)) D.list[atomicAdd(D.head, 1u)] = s;
}

// a pair names entry (k, t0..t2) of search s
__device__ __forceinline__ bool pair_owns(const DevMark& D, uint32_t s, uint64_t k, uint32_t t0, uint32_t t1,
                                          uint32_t t2) {
    uint32_t lo = 0, hi = D.p;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (D.pw[mid] < s)
            lo = mid + 1;
        else
            hi = mid;
    }
    for (; lo < D.p && D.pw[lo] == s; lo++) {
        const uint32_t* tl = D.ptail + 3ull * lo;
        if (D.pkey[lo] == k && tl[0] == t0 && tl[1] == t1 && tl[2] == t2) return true;
    }
    return false;
}

// member entry i with key k against the batch: sk / sd are the staged keys and directory of the LDS form
template <bool LDS>
__device__ __forceinline__ void mark_one(const DevMark& D, const uint64_t* sk, const uint16_t* sd, uint32_t i, uint64_t k) {
    // the batch keys of the member key's prefix, then the lower bound among them: for keys spread like hashes a
    // bucket holds one key or none, so the common lane reads two directory words and at most one key
    const uint32_t p = (uint32_t)(k >> D.dshift);
    uint32_t lo = LDS ? (uint32_t)sd[p] : D.dir[p];
    const uint32_t end = LDS ? (uint32_t)sd[p + 1] : D.dir[p + 1];
    uint32_t hi = end;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((LDS ? sk[mid] : D.bkey[mid]) < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo >= end || (LDS ? sk[lo] : D.bkey[lo]) != k) return;  // the common lane: 8 bytes of HBM, nothing else
    // a key hit: the run of equal keys against the member's tail, then the index against n (a zero key of the
    // batch meets the padding of every slab here)
    const uint32_t* tl = D.mtail + 3ull * i;
    const uint32_t t0 = tl[0], t1 = tl[1], t2 = tl[2];
    for (uint32_t j = lo; j < D.q && (LDS ? sk[j] : D.bkey[j]) == k; j++) {
        const uint32_t* bt = D.btail + 3ull * j;
        if (bt[0] != t0 || bt[1] != t1 || bt[2] != t2) continue;
        const uint32_t s = i / D.cap, e = i - s * D.cap;
        if (e < min(D.rec[(uint64_t)SREC_WORDS * s + SREC_N], D.cap)) {
            if (D.hits) atomicAdd(D.hits + j, 1u);
            if (!(D.p && pair_owns(D, s, k, t0, t1, t2))) {
                const uint32_t f = D.mflag[i], op = D.bop[j], nf = (f & ~(op & 3u)) | (op >> 2);
                if (nf != f) {
                    D.mflag[i] = (uint8_t)nf;
                    mark_dirty(D, s);
                }
            }
        }
        break;  // the batch IDs are distinct
    }
}

template <bool LDS>
__global__ __launch_bounds__(BLOCK) void mark_scan_kernel(DevMark D) {
    __shared__ uint64_t sk[LDS ? MARK_LDS_KEYS : 1];
    __shared__ uint16_t sd[LDS ? MARK_LDS_DIR + 1 : 2];  // a batch of up to 4096 keys: its bounds fit 16 bits
    if (LDS) {
        for (uint32_t j = threadIdx.x; j < D.q; j += BLOCK) sk[j] = D.bkey[j];
        for (uint32_t j = threadIdx.x; j <= (1u << (64u - D.dshift)); j += BLOCK) sd[j] = (uint16_t)D.dir[j];
        __syncthreads();
    }
    const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
    for (uint64_t i0 = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i0 < D.total; i0 += MARK_UNROLL * stride) {
        uint64_t k[MARK_UNROLL];  // all loads of the step in flight together, none predicated
#pragma unroll
        for (uint32_t u = 0; u < MARK_UNROLL; u++) {
            const uint64_t iu = i0 + u * stride;
            k[u] = __builtin_nontemporal_load(D.mkey + (iu < D.total ? iu : (uint64_t)D.total - 1u));
        }
#pragma unroll
        for (uint32_t u = 0; u < MARK_UNROLL; u++) {
            const uint64_t iu = i0 + u * stride;
            if (iu < D.total) mark_one<LDS>(D, sk, sd, (uint32_t)iu, k[u]);
        }
    }
}

__global__ __launch_bounds__(BLOCK) void mark_pairs_kernel(DevMark D) {
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= D.p) return;
    const uint32_t s = D.pw[k], n = min(D.rec[(uint64_t)SREC_WORDS * s + SREC_N], D.cap);
    const uint64_t x = D.pkey[k];
    const uint32_t* xt = D.ptail + 3ull * k;
    const uint32_t x0 = xt[0], x1 = xt[1], x2 = xt[2];
    const uint64_t* mk = D.mkey + (uint64_t)s * D.cap;
    const uint32_t* mt = D.mtail + 3ull * s * D.cap;
    uint32_t at = n;
    // member()'s walk: keys eight at a time, none predicated, a tail only on a key hit
    for (uint32_t c = 0; c < n && at == n; c += 8) {
        uint64_t v[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) v[u] = mk[min(c + u, n - 1u)];
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) {
            if (at == n && c + u < n && v[u] == x) {
                const uint32_t* tl = mt + 3ull * (c + u);
                if (tl[0] == x0 && tl[1] == x1 && tl[2] == x2) at = c + u;
            }
        }
    }
    D.found[k] = at < n ? (uint8_t)1 : (uint8_t)0;
    if (at < n) {
        uint8_t* f = D.mflag + (uint64_t)s * D.cap + at;
        const uint8_t want = D.pfl[k];
        if (*f != want) {
            *f = want;
            mark_dirty(D, s);
        }
    }
}

// One wave per changed search, one entry per lane: t, SREC_FULL and the threshold from the new flag bytes as
// refill_kernel's tail writes them, and the count word n | bad << 8 | lead_bad << 16 | bits << 24. res[w] (w < n_res)
// pairs the search with its count word in the call's own buffer, which travels back with the other outputs; all[w] is
// the same pair in the handle's scratch, for a call that changed more searches than that.
__global__ __launch_bounds__(BLOCK) void mark_fix_kernel(DevMark D, uint64_t* __restrict__ all,
                                                         uint32_t* __restrict__ out_head, uint64_t* __restrict__ res,
                                                         uint32_t n_res) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = rfl(blockIdx.x * REFILL_WAVES + (threadIdx.x >> 6)), waves = gridDim.x * REFILL_WAVES;
    const uint32_t n_changed = min(rfl(D.head[0]), D.S);
    if (wave == 0 && lane == 0) *out_head = n_changed;
    for (uint32_t w = wave; w < n_changed; w += waves) {
        const uint32_t s = min(rfl(D.list[w]), D.S - 1u);
        uint32_t* r = D.rec + (uint64_t)SREC_WORDS * s;
        const uint32_t n = min(rfl(r[SREC_N]), D.cap);
        const bool expired = (rfl(r[SREC_BITS]) & SREC_EXPIRED) != 0;
        const uint64_t e0 = (uint64_t)s * D.cap + lane;
        const bool in = lane < n;
        const uint32_t fl = in ? D.mflag[e0] : 0u;
        const uint64_t badm = __ballot(in && (fl & KAD_SN_BAD)), goodm = __ballot(in && !(fl & KAD_SN_BAD));
        bool full;
        uint32_t t;
        wave_trim(expired, n, goodm, lane, full, t);
        if (lane + 1u == t || (t == 0 && lane == 0)) {  // the threshold entry[t-1], zero for t == 0
            uint64_t k = 0;
            uint32_t t0 = 0, t1 = 0, t2 = 0;
            if (t) {
                k = D.mkey[e0];
                const uint32_t* tl = D.mtail + 3ull * e0;
                t0 = tl[0];
                t1 = tl[1];
                t2 = tl[2];
            }
            r[SREC_THR] = (uint32_t)k;
            r[SREC_THR + 1] = (uint32_t)(k >> 32);
            r[SREC_THR + 2] = t0;
            r[SREC_THR + 3] = t1;
            r[SREC_THR + 4] = t2;
        }
        if (lane == 0) {
            const uint32_t bits = (full ? SREC_FULL : 0u) | (expired ? SREC_EXPIRED : 0u);
            const uint32_t bad = (uint32_t)__popcll(badm);
            const uint32_t lead = min(~badm ? (uint32_t)__builtin_ctzll(~badm) : 64u, n);
            const uint32_t cw = n | (bad << 8) | (lead << 16) | (bits << 24);
            r[SREC_T] = t;
            r[SREC_BITS] = bits;
            all[w] = ((uint64_t)cw << 32) | s;
            if (w < n_res) res[w] = ((uint64_t)cw << 32) | s;
        }
    }
}

// ---- kad_sr_mark_entries and kad_sr_step: Dht::searchStep over the set ---------------------------
// The four step bits of single (search, node) entries: mark_pairs_kernel's walk, then (f & ~clear) | set on the one byte.
// The pairs of a call are distinct, so every byte has one writer; no record depends on these bits.
struct DevEntries {
    const uint32_t* rec;
    const uint64_t* mkey;
    const uint32_t* mtail;
    uint8_t* mflag;
    uint32_t cap, p;
    const uint32_t* pw;  // the pairs: search, key, tail, the bits to clear and to set
    const uint64_t* pkey;
    const uint32_t* ptail;
    const uint8_t* pclear;
    const uint8_t* pset;
    uint8_t* found;
};

__global__ __launch_bounds__(BLOCK) void entries_kernel(DevEntries D) {
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= D.p) return;
    const uint32_t s = D.pw[k], n = min(D.rec[(uint64_t)SREC_WORDS * s + SREC_N], D.cap);
    const uint64_t x = D.pkey[k];
    const uint32_t* xt = D.ptail + 3ull * k;
    const uint32_t x0 = xt[0], x1 = xt[1], x2 = xt[2];
    const uint64_t* mk = D.mkey + (uint64_t)s * D.cap;
    const uint32_t* mt = D.mtail + 3ull * s * D.cap;
    uint32_t at = n;
    // member()'s walk: keys eight at a time, none predicated, a tail only on a key hit
    for (uint32_t c = 0; c < n && at == n; c += 8) {
        uint64_t v[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) v[u] = mk[min(c + u, n - 1u)];
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) {
            if (at == n && c + u < n && v[u] == x) {
                const uint32_t* tl = mt + 3ull * (c + u);
                if (tl[0] == x0 && tl[1] == x1 && tl[2] == x2) at = c + u;
            }
        }
    }
    D.found[k] = at < n ? (uint8_t)1 : (uint8_t)0;
    if (at < n) {
        uint8_t* f = D.mflag + (uint64_t)s * D.cap + at;
        const uint8_t have = *f, want = (uint8_t)((have & ~D.pclear[k]) | D.pset[k]);
        if (want != have) *f = want;
    }
}

// One lane per stepped search, step_kernel and step_full_kernel alike (step_lane): n and the expired bit from the record,
// the flag bytes of the entries below n as words (WIDE, cap a multiple of 16: every slab starts on a 16-byte boundary and
// is read as 16-byte units; otherwise byte by byte, as a slab then starts anywhere), the words turned into kadstep's
// planes, the decision, the result stored. With KAD_STEP_APPLY the entries a loop sent to are rewritten; a search that
// expires is appended to a list instead, and step_expire_kernel empties it.
struct DevStep {
    uint32_t* rec;
    uint64_t* mkey;
    uint32_t* mtail;
    uint8_t* mflag;
    uint32_t S, cap, m;
    const uint32_t* which;  // m, NULL: search i
    const uint8_t* mode;    // m, NULL: all zero
    u32x4_t* out;           // m units, 2 m for step_full_kernel
    uint32_t* n_exp;      // the number of searches to expire, and the searches: room for m
    uint32_t* exp_list;
};

// the flag bytes of entries 4k .. 4k+3 in w[k]; zero from n on (the slab's padding is zero)
template <bool WIDE>
__device__ __forceinline__ void load_flag_words(const uint8_t* fl, uint32_t n, uint32_t (&w)[16]) {
    if (WIDE) {
        const u32x4_t* fu = reinterpret_cast<const u32x4_t*>(fl);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            u32x4_t u = {0u, 0u, 0u, 0u};
            if (16u * k < n) u = fu[k];
            w[4 * k] = u.x;
            w[4 * k + 1] = u.y;
            w[4 * k + 2] = u.z;
            w[4 * k + 3] = u.w;
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            uint32_t v = 0;
#pragma unroll
            for (uint32_t b = 0; b < 4; b++)
                if (4u * k + b < n) v |= (uint32_t)fl[4u * k + b] << (8u * b);
            w[k] = v;
        }
    }
}

// the bytes of v stored back for the entries in `touched` (all below n): WIDE the 16-byte units that hold one, otherwise
// those bytes alone
template <bool WIDE>
__device__ __forceinline__ void store_flag_words(uint8_t* fl, uint64_t touched, const uint32_t (&v)[16]) {
    if (WIDE) {
        u32x4_t* fu = reinterpret_cast<u32x4_t*>(fl);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            if ((touched >> (16u * k)) & 0xFFFFull) {
                const u32x4_t u = {v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]};
                fu[k] = u;
            }
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
#pragma unroll
            for (uint32_t b = 0; b < 4; b++)
                if ((touched >> (4u * k + b)) & 1ull) fl[4u * k + b] = (uint8_t)(v[k] >> (8u * b));
        }
    }
}

// FULL (kad_sr_step_full): all eight bits of the flag bytes as kadstep's seven planes, decide_full's three
// send loops, a 32-byte result as two 16-byte stores (D.out holds 2 m units). Otherwise (kad_sr_step, §7.19) five planes,
// decide's get loop and one 16-byte store. With KAD_STEP_APPLY an entry picked by any loop is rewritten: PENDING for a get
// request or a probe, NOGET for a get request (and for a probe under PROBE_BLOCKS), LISTEN_DUE and ANNOUNCE_DUE cleared
// where that loop sent. Without listens and probes that is PENDING | NOGET on the picks.
template <bool WIDE, bool FULL>
__device__ __forceinline__ void step_lane(const DevStep& D) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= D.m) return;
    const uint32_t s = D.which ? min(D.which[i], D.S - 1u) : i;
    const uint32_t mode = D.mode ? (uint32_t)D.mode[i] : 0u;
    const uint32_t* r = D.rec + (uint64_t)SREC_WORDS * s;
    const uint32_t n = min(r[SREC_N], D.cap);
    const bool expired = (r[SREC_BITS] & SREC_EXPIRED) != 0;
    uint8_t* fl = D.mflag + (uint64_t)s * D.cap;
    uint32_t w[16];
    load_flag_words<WIDE>(fl, n, w);
    kadstep::DecisionFull d;
    if (FULL) {
        kadstep::PlanesFull P;
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) kadstep::add_word_full(P, w[k], k);
        d = kadstep::decide_full(P, n, expired, mode);
    } else {
        kadstep::Planes P;
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) kadstep::add_word(P, w[k], k);
        const kadstep::Decision g = kadstep::decide(P, n, expired, mode);
        d = {g.picks, 0ull, 0ull, g.counts, g.bits};
    }
    if (mode & KAD_STEP_APPLY) {
        const uint64_t pend = d.picks | d.announce, noget = d.picks | ((mode & KAD_STEP_PROBE_BLOCKS) ? d.announce : 0ull);
        const uint64_t touched = pend | d.listen;  // all below n
        if ((d.bits & KAD_STEP_EXPIRE) && !(mode & KAD_STEP_NO_EXPIRE)) {
            D.exp_list[min(atomicAdd(D.n_exp, 1u), D.m - 1u)] = s;
        } else if (touched) {
            uint32_t v[16];
#pragma unroll
            for (uint32_t k = 0; k < 16; k++)
                v[k] = (w[k] | kadstep::mask_bytes(pend, k, KAD_SN_PENDING) | kadstep::mask_bytes(noget, k, KAD_SN_NOGET)) &
                       ~kadstep::mask_bytes(d.listen, k, KAD_SN_LISTEN_DUE) &
                       ~kadstep::mask_bytes(d.announce, k, KAD_SN_ANNOUNCE_DUE);
            store_flag_words<WIDE>(fl, touched, v);
        }
    }
    if (FULL) {
        const u32x4_t o0 = {(uint32_t)d.picks, (uint32_t)(d.picks >> 32), (uint32_t)d.listen, (uint32_t)(d.listen >> 32)};
        const u32x4_t o1 = {(uint32_t)d.announce, (uint32_t)(d.announce >> 32), d.counts, d.bits};
        __builtin_nontemporal_store(o0, D.out + 2ull * i);
        __builtin_nontemporal_store(o1, D.out + 2ull * i + 1ull);
    } else {
        const u32x4_t o = {(uint32_t)d.picks, (uint32_t)(d.picks >> 32), d.counts, d.bits};
        __builtin_nontemporal_store(o, D.out + i);
    }
}

template <bool WIDE>
__global__ __launch_bounds__(BLOCK) void step_kernel(DevStep D) {
    step_lane<WIDE, false>(D);
}

template <bool WIDE>
__global__ __launch_bounds__(BLOCK) void step_full_kernel(DevStep D) {
    step_lane<WIDE, true>(D);
}

// Search::expire() (dht.cpp:649-653) on the listed searches, one wave per search: the slab all zero and the record's
// words from n on what kad_searches_create derives for an empty expired list. The search ID stays.
__global__ __launch_bounds__(BLOCK) void step_expire_kernel(DevStep D) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = rfl(blockIdx.x * REFILL_WAVES + (threadIdx.x >> 6)), waves = gridDim.x * REFILL_WAVES;
    const uint32_t n_exp = min(rfl(D.n_exp[0]), D.m);
    for (uint32_t x = wave; x < n_exp; x += waves) {
        const uint32_t s = min(rfl(D.exp_list[x]), D.S - 1u);
        if (lane < D.cap) {
            const uint64_t e0 = (uint64_t)s * D.cap + lane;
            D.mkey[e0] = 0ull;
            uint32_t* tl = D.mtail + 3ull * e0;
            tl[0] = 0u;
            tl[1] = 0u;
            tl[2] = 0u;
            D.mflag[e0] = (uint8_t)0;
        }
        if (lane < SREC_WORDS - SREC_N)
            D.rec[(uint64_t)SREC_WORDS * s + SREC_N + lane] = SREC_N + lane == SREC_BITS ? SREC_EXPIRED : 0u;
    }
}

// kad_sr_step (Out = kad_step_out, 16 bytes a search) and kad_sr_step_full (kad_step_full_out, 32 bytes): the checks of
// `check`, the call's scratch, the step kernel of Out's width, the expire pass, the copy back and the counts of Stats.
// `what` opens every message; `unsupported` is the whole text for slabs of more than 64 entries.
template <class Out, class Stats>
int step_call(kad_searches* ss, uint32_t m, const uint32_t* which, const uint8_t* mode, Out* out, Stats* out_stats,
              int (*check)(uint32_t, uint32_t, const uint32_t*, const uint8_t*, std::string&), const char* what,
              const char* unsupported) {
    constexpr bool FULL = sizeof(Out) == 32;
    static_assert(sizeof(Out) == (FULL ? 32 : 16), "one 16-byte store per search, or two");
    if (!ss || !out) return set_error(KAD_ERR_INVALID, "NULL search set or output");
    std::string err;
    if (int rc = check(ss->S, m, which, mode, err)) return set_error(rc, err.c_str());
    Stats st = {};
    if (m == 0) {
        if (out_stats) *out_stats = st;
        return KAD_OK;
    }
    if (ss->cap > REFILL_MAX_CAP) return set_error(KAD_ERR_UNSUPPORTED, unsupported);
    bool any_apply = false;
    for (uint32_t k = 0; mode && k < m && !any_apply; k++) any_apply = (mode[k] & KAD_STEP_APPLY) != 0;
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    auto msg = [what](const char* text) { return std::string(what) + ": " + text; };
    // the call's scratch, one allocation: the listed searches and the modes (one upload each, when given), the results
    // (one copy back), the count of searches to expire and their list
    const size_t o_mode = which ? 4ull * m : 0, o_out = up16(o_mode + (mode ? m : 0)), o_head = o_out + sizeof(Out) * m,
                 o_list = o_head + 16, total = o_list + 4ull * m;
    CallScratch cs(ss->device);
    if (int rc = cs.open(total, what)) return rc;
    uint8_t* const buf = cs.buf;
    if (!have_events(ss->sp_ev)) return set_error(KAD_ERR_HIP, msg("no events").c_str());
    if ((which && hipMemcpy(buf, which, 4ull * m, hipMemcpyHostToDevice) != hipSuccess) ||
        (mode && hipMemcpy(buf + o_mode, mode, m, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemsetAsync(buf + o_head, 0, 16, nullptr) != hipSuccess)
        return set_error(KAD_ERR_HIP, msg("H2D failed").c_str());
    const DevStep D{ss->rec, ss->mkey, ss->mtail, ss->mflag, ss->S, ss->cap, m,
                    which ? (const uint32_t*)buf : nullptr, mode ? buf + o_mode : nullptr, (u32x4_t*)(buf + o_out),
                    (uint32_t*)(buf + o_head), (uint32_t*)(buf + o_list)};
    const bool wide = ss->cap % 16 == 0;
    void (*const kernel)(DevStep) = FULL ? (wide ? step_full_kernel<true> : step_full_kernel<false>)
                                         : (wide ? step_kernel<true> : step_kernel<false>);
    (void)hipEventRecord(ss->sp_ev[0], nullptr);
    hipLaunchKernelGGL(kernel, dim3((m + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, nullptr, D);
    hipError_t le = hipGetLastError();
    if (le == hipSuccess && any_apply) {  // the grid is sized without the count: the waves stride over what the head says
        const uint32_t blocks = (m + REFILL_WAVES - 1) / REFILL_WAVES, grid = blocks < MARK_FIX_GRID ? blocks : MARK_FIX_GRID;
        hipLaunchKernelGGL(step_expire_kernel, dim3(grid), dim3(BLOCK), 0, nullptr, D);
        le = hipGetLastError();
    }
    (void)hipEventRecord(ss->sp_ev[1], nullptr);
    if (le != hipSuccess) return set_error(KAD_ERR_HIP, (msg("launch failed: ") + hipGetErrorString(le)).c_str());
    const hipError_t ce = hipMemcpy(out, buf + o_out, sizeof(Out) * m, hipMemcpyDeviceToHost);
    if (ce != hipSuccess) return set_error(KAD_ERR_HIP, (msg("D2H failed: ") + hipGetErrorString(ce)).c_str());
    st.kernel_ms = elapsed_or_zero(ss->sp_ev[0], ss->sp_ev[1]);
    if (out_stats) {
        for (uint32_t k = 0; k < m; k++) {
            st.synced += (out[k].bits & KAD_STEP_SYNCED) ? 1u : 0u;
            st.expired += (out[k].bits & KAD_STEP_EXPIRE) ? 1u : 0u;
            st.skipped += (out[k].bits & KAD_STEP_SKIPPED) ? 1u : 0u;
            st.picks += (uint32_t)__builtin_popcountll(out[k].picks);
            if constexpr (FULL) {
                st.listens += (uint32_t)__builtin_popcountll(out[k].listen);
                st.announces += (uint32_t)__builtin_popcountll(out[k].announce);
            }
        }
        *out_stats = st;
    }
    return KAD_OK;
}

// ---- kad_searches_apply: add and erase searches, grow the slabs -----------------------------------
// The new set is written beside the old one: every record and slab is gathered from src[s'] (kadplan::SRC_NEW: an
// inserted search, zero-filled, its record from the 20 uploaded ID bytes). A streaming gather, read once with
// non-temporal loads and written once; one thread per unit of the four arrays taken one after the other, so
// neighbouring lanes write neighbouring units. WIDE (old and new cap multiples of 16: every slab starts on a 16-byte
// boundary) moves 16-byte units throughout. Otherwise a key is one 8-byte unit, a tail three words, and the flag bytes,
// whose per-search slabs then start at any byte, are assembled into the words of the new array taken as a whole.
constexpr uint32_t SRC_EXPIRED = 0x40000000u;  // with SRC_NEW: the inserted search is KAD_SR_EXPIRED
constexpr uint32_t SRC_SLOT = SRC_EXPIRED - 1u;
constexpr uint32_t RELAYOUT_GRID = 4096;  // grid-stride beyond

struct DevRelayout {
    const u32x4_t* rec;  // the old set
    const uint64_t* mkey;
    const uint32_t* mtail;
    const uint8_t* mflag;
    u32x4_t* nrec;  // the new one
    uint64_t* nskey;  // NULL for a set with a prefix directory
    uint64_t* nmkey;
    uint32_t* nmtail;
    uint8_t* nmflag;
    const uint32_t* src;
    const uint32_t* ins_ids;  // n_ins x 5 words, the inserted IDs as their bytes
    uint32_t S2, cap, cap2;
};

// unit j (16 bytes) of the record kad_searches_create derives for an empty search
__device__ __forceinline__ u32x4_t empty_rec_unit(const uint32_t* id, uint32_t j, bool expired) {
    u32x4_t v = {0u, 0u, 0u, 0u};
    if (j == 0) {
        v.x = __builtin_bswap32(id[1]);
        v.y = __builtin_bswap32(id[0]);
        v.z = __builtin_bswap32(id[2]);
        v.w = __builtin_bswap32(id[3]);
    } else if (j == 1) {
        v.x = __builtin_bswap32(id[4]);
    } else if (j == 3) {
        v.x = expired ? SREC_EXPIRED : 0u;
    }
    return v;
}

// unit j of per_new of the slab of new search s: the old search's unit, zero past its per_old units or for a new one
template <class T>
__device__ __forceinline__ T gather_unit(const T* old, uint32_t w, uint32_t j, uint32_t per_old) {
    T v = {};
    if (!(w & kadplan::SRC_NEW) && j < per_old) v = __builtin_nontemporal_load(old + (uint64_t)w * per_old + j);
    return v;
}

template <bool WIDE>
__global__ __launch_bounds__(BLOCK) void searches_relayout_kernel(DevRelayout D) {
    const uint32_t cap = D.cap, cap2 = D.cap2;
    const uint32_t kn = WIDE ? cap2 / 2 : cap2, ko = WIDE ? cap / 2 : cap;             // key units per search
    const uint32_t tn = WIDE ? cap2 / 4 * 3 : cap2, to = WIDE ? cap / 4 * 3 : cap;     // tail units
    const uint64_t fbytes = (uint64_t)D.S2 * cap2;
    const uint64_t n_rec = 4ull * D.S2, n_key = (uint64_t)D.S2 * kn, n_tail = (uint64_t)D.S2 * tn,
                   n_flag = WIDE ? fbytes / 16 : (fbytes + 3) / 4;
    const uint64_t total = n_rec + n_key + n_tail + n_flag;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (uint64_t)gridDim.x * BLOCK) {
        if (i < n_rec) {
            const uint32_t s = (uint32_t)(i >> 2), j = (uint32_t)i & 3u, w = D.src[s];
            u32x4_t v;
            if (w & kadplan::SRC_NEW)
                v = empty_rec_unit(D.ins_ids + 5ull * (w & SRC_SLOT), j, (w & SRC_EXPIRED) != 0);
            else
                v = __builtin_nontemporal_load(D.rec + 4ull * w + j);
            D.nrec[i] = v;
            if (j == 0 && D.nskey) D.nskey[s] = ((uint64_t)v.y << 32) | v.x;
        } else if (i - n_rec < n_key) {
            const uint32_t l = (uint32_t)(i - n_rec), s = l / kn, j = l - s * kn, w = D.src[s];
            if (WIDE)
                reinterpret_cast<u32x4_t*>(D.nmkey)[l] = gather_unit(reinterpret_cast<const u32x4_t*>(D.mkey), w, j, ko);
            else
                D.nmkey[l] = gather_unit(D.mkey, w, j, ko);
        } else if (i - n_rec - n_key < n_tail) {
            const uint32_t l = (uint32_t)(i - n_rec - n_key), s = l / tn, j = l - s * tn, w = D.src[s];
            if (WIDE) {
                reinterpret_cast<u32x4_t*>(D.nmtail)[l] =
                    gather_unit(reinterpret_cast<const u32x4_t*>(D.mtail), w, j, to);
            } else {
                const bool in = !(w & kadplan::SRC_NEW) && j < to;
                const uint32_t* o = D.mtail + 3ull * ((uint64_t)(in ? w : 0u) * cap + (in ? j : 0u));
                uint32_t t0 = 0, t1 = 0, t2 = 0;
                if (in) {
                    t0 = __builtin_nontemporal_load(o);
                    t1 = __builtin_nontemporal_load(o + 1);
                    t2 = __builtin_nontemporal_load(o + 2);
                }
                uint32_t* d = D.nmtail + 3ull * l;
                d[0] = t0;
                d[1] = t1;
                d[2] = t2;
            }
        } else {
            const uint32_t l = (uint32_t)(i - n_rec - n_key - n_tail);
            if (WIDE) {
                const uint32_t fn = cap2 / 16, s = l / fn, j = l - s * fn;
                reinterpret_cast<u32x4_t*>(D.nmflag)[l] =
                    gather_unit(reinterpret_cast<const u32x4_t*>(D.mflag), D.src[s], j, cap / 16);
            } else {  // word l of the new flag array: bytes 4l .. 4l+3, each of its own search and entry
                const uint32_t b0 = 4u * l;  // below S' x cap' < 2^31
                uint32_t s = b0 / cap2, j = b0 - s * cap2, word = 0;
                const uint32_t nb = fbytes - b0 < 4 ? (uint32_t)(fbytes - b0) : 4u;
                for (uint32_t k = 0; k < nb; k++) {
                    const uint32_t w = D.src[s];
                    if (!(w & kadplan::SRC_NEW) && j < cap)
                        word |= (uint32_t)__builtin_nontemporal_load(D.mflag + (uint64_t)w * cap + j) << (8 * k);
                    if (++j == cap2) {
                        j = 0;
                        s++;
                    }
                }
                if (nb == 4)
                    reinterpret_cast<uint32_t*>(D.nmflag)[l] = word;
                else  // the array's last bytes
                    for (uint32_t k = 0; k < nb; k++) D.nmflag[b0 + k] = (uint8_t)(word >> (8 * k));
            }
        }
    }
}

// The prefix directory of a large set from the new records: rdx[p] = the number of search keys whose top B bits are
// below p, p = 0 .. 2^B, by a lower bound over the ascending keys.
__global__ __launch_bounds__(BLOCK) void searches_rdx_kernel(const u32x4_t* __restrict__ rec, uint32_t S, uint32_t rshift,
                                                             uint32_t slots, uint32_t* __restrict__ rdx) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= slots) return;
    uint32_t lo = 0, hi = S;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const u32x4_t r0 = rec[4ull * mid];
        const uint64_t k = ((uint64_t)r0.y << 32) | r0.x;
        if ((uint32_t)(k >> rshift) < p)
            lo = mid + 1;
        else
            hi = mid;
    }
    rdx[p] = lo;
}

// The arrays of a set of S searches with slabs of cap entries: their sizes and the directory's B (0: dense skey).
struct Layout {
    size_t b_rec, b_skey, b_mkey, b_mtail, b_mflag, b_rdx;
    uint32_t B;
    Layout(uint32_t S, uint32_t cap) {
        B = 0;
        if (S > LDS_KEYS) {
            B = 1;
            while (B < 24 && (1u << B) < S) B++;
        }
        b_rec = 64ull * S;
        b_skey = B ? 0 : 8ull * S;
        b_mkey = 8ull * S * cap;
        b_mtail = 12ull * S * cap;
        b_mflag = (size_t)S * cap;
        b_rdx = B ? 4ull * ((1ull << B) + 1) : 0;
    }
    uint64_t bytes() const { return b_rec + b_skey + b_mkey + b_mtail + b_mflag + b_rdx; }
};

void free_device(kad_searches* ss) {
    if (ss->rec) (void)hipFree(ss->rec);
    if (ss->skey) (void)hipFree(ss->skey);
    if (ss->mkey) (void)hipFree(ss->mkey);
    if (ss->mtail) (void)hipFree(ss->mtail);
    if (ss->mflag) (void)hipFree(ss->mflag);
    if (ss->rdx) (void)hipFree(ss->rdx);
    ss->rdx = nullptr;
    ss->rec = nullptr;
    ss->skey = nullptr;
    ss->mkey = nullptr;
    ss->mtail = nullptr;
    ss->mflag = nullptr;
}

int check_lists(uint32_t m, const uint8_t* flags, const uint32_t* off, const uint8_t* node_ids,
                const uint8_t* node_flags) {
    if (!off || (m && !flags)) return set_error(KAD_ERR_INVALID, "NULL argument");
    if (m && off[m] > 0 && (!node_ids || !node_flags)) return set_error(KAD_ERR_INVALID, "NULL node arrays");
    return KAD_OK;
}

void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

}  // namespace

extern "C" {

int kad_searches_create(kad_searches** out, int device, uint32_t S, uint32_t cap, const uint8_t* ids,
                        const uint8_t* flags, const uint32_t* off, const uint8_t* node_ids, const uint8_t* node_flags) {
    if (!out) return set_error(KAD_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (S && !ids) return set_error(KAD_ERR_INVALID, "NULL argument");
    if (int rc = check_lists(S, flags, off, node_ids, node_flags)) return rc;
    if (cap < KAD_SEARCH_NODES) return set_error(KAD_ERR_INVALID, "cap below KAD_SEARCH_NODES");
    if ((uint64_t)S * cap >= 0x7FFFFFFFull) return set_error(KAD_ERR_INVALID, "search set too large");
    std::string err;
    if (int rc = kadplan::searches_check_ids(S, ids, err)) return set_error(rc, err.c_str());
    kadplan::SearchesPlan plan;
    if (int rc = kadplan::searches_plan(S, cap, ids, flags, off, node_ids, node_flags, plan, err))
        return set_error(rc, err.c_str());
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        (void)hipGetLastError();
        return set_error(KAD_ERR_NO_DEVICE, "no such device");
    }
    kad_searches* ss = new kad_searches;
    ss->device = device;
    ss->S = S;
    ss->cap = cap;
    if (S) ss->h_ids.assign(ids, ids + 20ull * S);
    if (S == 0) {
        *out = ss;
        return KAD_OK;
    }
    DeviceGuard g(device);
    std::vector<uint64_t> skey(S);
    for (uint32_t s = 0; s < S; s++) std::memcpy(&skey[s], plan.rec.data() + (size_t)s * SREC_WORDS, 8);
    // the prefix directory of large sets: rdx[p] = the number of search keys whose top B bits are below p
    std::vector<uint32_t> rdx;
    const Layout L(S, cap);
    if (L.B) {
        ss->rshift = 64 - L.B;
        rdx.assign((1ull << L.B) + 1, 0u);
        for (uint32_t s = 0; s < S; s++) rdx[(size_t)(skey[s] >> ss->rshift) + 1]++;
        for (size_t p = 1; p < rdx.size(); p++) rdx[p] += rdx[p - 1];
    }
    const size_t b_rec = L.b_rec, b_skey = L.b_skey, b_mkey = L.b_mkey, b_mtail = L.b_mtail, b_mflag = L.b_mflag,
                 b_rdx = L.b_rdx;
    if (hipMalloc((void**)&ss->rec, b_rec) != hipSuccess ||
        (b_skey && hipMalloc((void**)&ss->skey, b_skey) != hipSuccess) ||
        hipMalloc((void**)&ss->mkey, b_mkey) != hipSuccess || hipMalloc((void**)&ss->mtail, b_mtail) != hipSuccess ||
        hipMalloc((void**)&ss->mflag, b_mflag) != hipSuccess ||
        (b_rdx && hipMalloc((void**)&ss->rdx, b_rdx) != hipSuccess)) {
        (void)hipGetLastError();
        free_device(ss);
        delete ss;
        return set_error(KAD_ERR_NOMEM, "search set: out of device memory");
    }
    ss->bytes = b_rec + b_skey + b_mkey + b_mtail + b_mflag + b_rdx;
    if (hipMemcpy(ss->rec, plan.rec.data(), b_rec, hipMemcpyHostToDevice) != hipSuccess ||
        (b_skey && hipMemcpy(ss->skey, skey.data(), b_skey, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(ss->mkey, plan.mkey.data(), b_mkey, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ss->mtail, plan.mtail.data(), b_mtail, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ss->mflag, plan.mflag.data(), b_mflag, hipMemcpyHostToDevice) != hipSuccess ||
        (b_rdx && hipMemcpy(ss->rdx, rdx.data(), b_rdx, hipMemcpyHostToDevice) != hipSuccess)) {
        free_device(ss);
        delete ss;
        return set_error(KAD_ERR_HIP, "search set: upload failed");
    }
    *out = ss;
    return KAD_OK;
}

int kad_searches_patch(kad_searches* ss, uint32_t m, const uint32_t* which, const uint8_t* flags, const uint32_t* off,
                       const uint8_t* node_ids, const uint8_t* node_flags) {
    if (!ss || (m && !which)) return set_error(KAD_ERR_INVALID, "NULL argument");
    if (int rc = check_lists(m, flags, off, node_ids, node_flags)) return rc;
    for (uint32_t k = 0; k < m; k++)
        if (which[k] >= ss->S || (k && which[k] <= which[k - 1]))
            return set_error(KAD_ERR_INVALID, "patched searches must be strictly ascending and below S");
    if (m == 0) return KAD_OK;
    std::vector<uint8_t> pid(20ull * m);
    for (uint32_t k = 0; k < m; k++) std::memcpy(&pid[20ull * k], &ss->h_ids[20ull * which[k]], 20);
    kadplan::SearchesPlan plan;
    std::string err;
    if (int rc = kadplan::searches_plan(m, ss->cap, pid.data(), flags, off, node_ids, node_flags, plan, err))
        return set_error(rc, err.c_str());
    DeviceGuard g(ss->device);
    SR_HIP_TRY(hipDeviceSynchronize());  // queries enqueued before the call read the old set
    const uint32_t cap = ss->cap;
    // runs of consecutive searches travel as one copy per array
    for (uint32_t a = 0; a < m;) {
        uint32_t e = a + 1;
        while (e < m && which[e] == which[e - 1] + 1) e++;
        const uint64_t s0 = which[a], len = e - a;
        SR_HIP_TRY(hipMemcpy(ss->rec + s0 * SREC_WORDS, plan.rec.data() + (size_t)a * SREC_WORDS, 64ull * len,
                             hipMemcpyHostToDevice));
        SR_HIP_TRY(hipMemcpy(ss->mkey + s0 * cap, plan.mkey.data() + (size_t)a * cap, 8ull * len * cap,
                             hipMemcpyHostToDevice));
        SR_HIP_TRY(hipMemcpy(ss->mtail + 3ull * s0 * cap, plan.mtail.data() + 3ull * a * cap, 12ull * len * cap,
                             hipMemcpyHostToDevice));
        SR_HIP_TRY(hipMemcpy(ss->mflag + s0 * cap, plan.mflag.data() + (size_t)a * cap, len * cap,
                             hipMemcpyHostToDevice));
        a = e;
    }
    return KAD_OK;
}

int kad_searches_apply(kad_searches* ss, const uint32_t* erase, uint32_t n_erase, const uint8_t* ins_ids,
                       const uint8_t* ins_flags, uint32_t n_ins, uint32_t new_cap, uint32_t* remap, uint32_t* new_index) {
    if (!ss) return set_error(KAD_ERR_INVALID, "NULL search set");
    if ((n_erase && !erase) || (n_ins && !ins_ids)) return set_error(KAD_ERR_INVALID, "NULL argument");
    std::string err;
    if (int rc = kadplan::searches_check_erase(ss->S, erase, n_erase, err)) return set_error(rc, err.c_str());
    if (new_cap && new_cap < ss->cap) return set_error(KAD_ERR_INVALID, "new_cap below cap: slabs do not shrink");
    for (uint32_t j = 0; ins_flags && j < n_ins; j++)
        if (ins_flags[j] & ~KAD_SR_EXPIRED) return set_error(KAD_ERR_INVALID, "unknown search flag");
    const uint32_t S = ss->S, cap = ss->cap, cap2 = new_cap ? new_cap : cap;
    const bool members = n_erase || n_ins;
    kadplan::SearchesApplyPlan plan;
    try {
        if (members) {
            if (int rc = kadplan::searches_apply_plan(S, ss->h_ids.data(), erase, n_erase, ins_ids, n_ins, plan, err))
                return set_error(rc, err.c_str());
        } else if (cap2 != cap) {  // larger slabs alone: every search stays where it is, and so do the IDs
            plan.src.resize(S);
            std::iota(plan.src.begin(), plan.src.end(), 0u);
            plan.remap = plan.src;
        }
    } catch (const std::bad_alloc&) {
        return set_error(KAD_ERR_NOMEM, "searches apply: out of host memory");
    }
    const uint64_t S2 = (uint64_t)S - n_erase + n_ins;
    // the limit also keeps an insert slot clear of SRC_NEW and SRC_EXPIRED in its source word (n_ins <= S' < 2^31 / cap')
    if (S2 * cap2 >= 0x7FFFFFFFull || n_ins > SRC_SLOT) return set_error(KAD_ERR_INVALID, "search set too large");
    if (!members && cap2 == cap) {
        for (uint32_t s = 0; remap && s < S; s++) remap[s] = s;
        return KAD_OK;
    }
    for (uint32_t j = 0; ins_flags && j < n_ins; j++)
        if (ins_flags[j] & KAD_SR_EXPIRED) plan.src[plan.new_index[j]] |= SRC_EXPIRED;
    DeviceGuard g(ss->device);
    SR_HIP_TRY(hipDeviceSynchronize());  // queries enqueued before the call read the old set
    kad_searches nw;  // the new arrays, beside the old ones until the last device step succeeded
    const Layout L((uint32_t)S2, cap2);
    uint8_t* scratch = nullptr;  // src, then the inserted IDs
    auto fail = [&](int code, const char* what) {
        (void)hipGetLastError();
        if (scratch) (void)hipFree(scratch);
        free_device(&nw);
        return set_error(code, what);
    };
    if (S2) {
        if (hipMalloc((void**)&nw.rec, L.b_rec) != hipSuccess ||
            (L.b_skey && hipMalloc((void**)&nw.skey, L.b_skey) != hipSuccess) ||
            hipMalloc((void**)&nw.mkey, L.b_mkey) != hipSuccess || hipMalloc((void**)&nw.mtail, L.b_mtail) != hipSuccess ||
            hipMalloc((void**)&nw.mflag, L.b_mflag) != hipSuccess ||
            (L.b_rdx && hipMalloc((void**)&nw.rdx, L.b_rdx) != hipSuccess) ||
            hipMalloc((void**)&scratch, 4ull * S2 + 20ull * n_ins) != hipSuccess)
            return fail(KAD_ERR_NOMEM, "searches apply: out of device memory");
        if (hipMemcpy(scratch, plan.src.data(), 4ull * S2, hipMemcpyHostToDevice) != hipSuccess ||
            (n_ins && hipMemcpy(scratch + 4ull * S2, ins_ids, 20ull * n_ins, hipMemcpyHostToDevice) != hipSuccess))
            return fail(KAD_ERR_HIP, "searches apply: upload failed");
        const DevRelayout D{reinterpret_cast<const u32x4_t*>(ss->rec), ss->mkey, ss->mtail, ss->mflag,
                            reinterpret_cast<u32x4_t*>(nw.rec), nw.skey, nw.mkey, nw.mtail, nw.mflag,
                            reinterpret_cast<const uint32_t*>(scratch),
                            reinterpret_cast<const uint32_t*>(scratch + 4ull * S2), (uint32_t)S2, cap, cap2};
        const bool wide = cap % 16 == 0 && cap2 % 16 == 0;
        // units: 4 per record, then keys, tails and flags as the kernel counts them
        const uint64_t e = S2 * cap2, units = 4 * S2 + (wide ? e / 2 + e / 4 * 3 + e / 16 : 2 * e + (e + 3) / 4);
        const uint64_t blocks = (units + BLOCK - 1) / BLOCK;
        const dim3 grid((uint32_t)(blocks < RELAYOUT_GRID ? blocks : RELAYOUT_GRID));
        if (wide)
            hipLaunchKernelGGL(searches_relayout_kernel<true>, grid, dim3(BLOCK), 0, nullptr, D);
        else
            hipLaunchKernelGGL(searches_relayout_kernel<false>, grid, dim3(BLOCK), 0, nullptr, D);
        if (hipGetLastError() != hipSuccess) return fail(KAD_ERR_HIP, "searches apply: relayout launch failed");
        if (L.B) {
            const uint32_t slots = (1u << L.B) + 1;
            hipLaunchKernelGGL(searches_rdx_kernel, dim3((slots + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, nullptr,
                               reinterpret_cast<const u32x4_t*>(nw.rec), (uint32_t)S2, 64 - L.B, slots, nw.rdx);
            if (hipGetLastError() != hipSuccess) return fail(KAD_ERR_HIP, "searches apply: directory launch failed");
        }
        if (hipDeviceSynchronize() != hipSuccess) return fail(KAD_ERR_HIP, "searches apply: relayout failed");
        (void)hipFree(scratch);
    }
    free_device(ss);  // the old arrays; the new ones take their place
    ss->rec = nw.rec;
    ss->skey = nw.skey;
    ss->mkey = nw.mkey;
    ss->mtail = nw.mtail;
    ss->mflag = nw.mflag;
    ss->rdx = nw.rdx;
    ss->S = (uint32_t)S2;
    ss->cap = cap2;
    ss->rshift = L.B ? 64 - L.B : 0;
    ss->bytes = L.bytes();
    if (members) ss->h_ids.swap(plan.ids);
    if (remap && S) std::memcpy(remap, plan.remap.data(), 4ull * S);
    if (new_index && n_ins) std::memcpy(new_index, plan.new_index.data(), 4ull * n_ins);
    return KAD_OK;
}

int kad_searches_info(const kad_searches* ss, uint32_t* S, uint32_t* cap, uint64_t* device_bytes) {
    if (!ss) return set_error(KAD_ERR_INVALID, "NULL search set");
    if (S) *S = ss->S;
    if (cap) *cap = ss->cap;
    if (device_bytes) *device_bytes = ss->bytes + ss->mk_bytes;  // the mark scratch from its first use on
    return KAD_OK;
}

int kad_searches_export(const kad_searches* ss, uint8_t* ids, uint8_t* flags, uint32_t* n, uint8_t* node_ids,
                        uint8_t* node_flags, uint8_t* full, uint32_t* t) {
    if (!ss) return set_error(KAD_ERR_INVALID, "NULL search set");
    const uint32_t S = ss->S, cap = ss->cap;
    if (S == 0) return KAD_OK;
    DeviceGuard g(ss->device);
    SR_HIP_TRY(hipDeviceSynchronize());
    std::vector<uint32_t> rec((size_t)S * SREC_WORDS);
    SR_HIP_TRY(hipMemcpy(rec.data(), ss->rec, 64ull * S, hipMemcpyDeviceToHost));
    for (uint32_t s = 0; s < S; s++) {
        const uint32_t* r = rec.data() + (size_t)s * SREC_WORDS;
        if (ids) {
            uint8_t* p = ids + 20ull * s;
            put_be32(p, r[1]);
            put_be32(p + 4, r[0]);
            for (int w = 0; w < 3; w++) put_be32(p + 8 + 4 * w, r[2 + w]);
        }
        if (flags) flags[s] = (r[SREC_BITS] & SREC_EXPIRED) ? (uint8_t)KAD_SR_EXPIRED : 0;
        if (n) n[s] = r[SREC_N];
        if (full) full[s] = (r[SREC_BITS] & SREC_FULL) ? 1 : 0;
        if (t) t[s] = r[SREC_T];
    }
    if (node_ids) {
        const size_t e = (size_t)S * cap;
        std::vector<uint64_t> mk(e);
        std::vector<uint32_t> mt(3 * e);
        SR_HIP_TRY(hipMemcpy(mk.data(), ss->mkey, 8ull * e, hipMemcpyDeviceToHost));
        SR_HIP_TRY(hipMemcpy(mt.data(), ss->mtail, 12ull * e, hipMemcpyDeviceToHost));
        for (size_t j = 0; j < e; j++) {
            uint8_t* p = node_ids + 20ull * j;
            put_be32(p, (uint32_t)(mk[j] >> 32));
            put_be32(p + 4, (uint32_t)mk[j]);
            for (int w = 0; w < 3; w++) put_be32(p + 8 + 4 * w, mt[3 * j + w]);
        }
    }
    if (node_flags) SR_HIP_TRY(hipMemcpy(node_flags, ss->mflag, (size_t)S * cap, hipMemcpyDeviceToHost));
    return KAD_OK;
}

int kad_searches_destroy(kad_searches* ss) {
    if (!ss) return KAD_OK;
    if (ss->S || ss->rf_ev[0] || ss->in_ev[0] || ss->mk_ev[0] || ss->mk_buf || ss->tk_ev[0] || ss->sp_ev[0]) {  // apply can empty a set that holds events
        DeviceGuard g(ss->device);
        (void)hipDeviceSynchronize();
        for (hipEvent_t e : ss->sp_ev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ss->tk_ev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ss->rf_ev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ss->in_ev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ss->mk_ev)
            if (e) (void)hipEventDestroy(e);
        if (ss->mk_buf) (void)hipFree(ss->mk_buf);
        free_device(ss);
    }
    delete ss;
    return KAD_OK;
}

int kad_sr_try_insert_batch(const kad_searches* ss, const uint8_t* ids, uint32_t q, uint32_t* out_lb,
                            uint32_t* out_fwd, uint32_t* out_back, uint8_t* out_stop, void* stream) {
    if (!ss) return set_error(KAD_ERR_INVALID, "NULL search set");
    if (!ids || !out_fwd || !out_back || !out_stop) return set_error(KAD_ERR_INVALID, "NULL buffer");
    if (q == 0) return KAD_OK;
    if (((uintptr_t)ids | (uintptr_t)out_lb | (uintptr_t)out_fwd | (uintptr_t)out_back) & 3)
        return set_error(KAD_ERR_INVALID, "device buffers must be 4-byte aligned");
    DeviceGuard g(ss->device);
    return launch(ss, ids, q, out_lb, out_fwd, out_back, out_stop, (hipStream_t)stream);
}

int kad_sr_refill(kad_searches* ss, const kad_table* nc, uint32_t m, const uint32_t* which, uint32_t* out_rows,
                  uint8_t* out_cnt, uint16_t* out_inserted, uint8_t* out_status) {
    if (!ss || !nc) return set_error(KAD_ERR_INVALID, "NULL argument");
    if (m && (!which || !out_cnt || !out_inserted || !out_status)) return set_error(KAD_ERR_INVALID, "NULL argument");
    for (uint32_t k = 0; k < m; k++)
        if (which[k] >= ss->S || (k && which[k] <= which[k - 1]))
            return set_error(KAD_ERR_INVALID, "patched searches must be strictly ascending and below S");
    const kadgpu_internal::TableIds T = kadgpu_internal::table_ids(nc);
    if (!T.sorted) return set_error(KAD_ERR_NOT_SORTED, "NodeCache query needs a KAD_TABLE_SORTED table");
    if (T.device != ss->device) return set_error(KAD_ERR_INVALID, "search set and NodeCache table on different devices");
    if (m == 0) return KAD_OK;
    if (ss->cap > REFILL_MAX_CAP)
        return set_error(KAD_ERR_UNSUPPORTED, "kad_sr_refill handles slabs of up to 64 entries");
    DeviceGuard g(ss->device);
    SR_HIP_TRY(hipDeviceSynchronize());  // queries enqueued before the call read the old set
    // the call's scratch, one allocation: which, the targets, then the outputs in the order of the one copy back
    const size_t o_tgt = 4ull * m, o_rows = o_tgt + 20ull * m, o_ins = o_rows + 4ull * KAD_SEARCH_NODES * m,
                 o_cnt = o_ins + 2ull * m, o_st = o_cnt + m, total = o_st + m;
    // the host side of the one copy back (rows if asked for, masks, counts, statuses), taken before anything runs: a
    // failure up to the refill kernel's launch leaves the set unchanged
    const size_t o_back = out_rows ? o_rows : o_ins;
    uint8_t* h = new (std::nothrow) uint8_t[total - o_back];
    if (!h) return set_error(KAD_ERR_NOMEM, "refill: out of host memory");
    uint8_t* buf = nullptr;
    if (hipMalloc((void**)&buf, total) != hipSuccess) {
        (void)hipGetLastError();
        delete[] h;
        return set_error(KAD_ERR_NOMEM, "refill: out of device memory");
    }
    auto done = [&](int r) {
        (void)hipFree(buf);
        delete[] h;
        return r;
    };
    if (!have_events(ss->rf_ev)) return done(set_error(KAD_ERR_HIP, "refill: no events"));
    if (hipMemcpy(buf, which, 4ull * m, hipMemcpyHostToDevice) != hipSuccess)
        return done(set_error(KAD_ERR_HIP, "refill: H2D failed"));
    uint32_t* d_which = (uint32_t*)buf;
    uint32_t* d_rows = (uint32_t*)(buf + o_rows);
    hipLaunchKernelGGL(refill_targets_kernel, dim3((m + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, nullptr, ss->rec, d_which, m,
                       (uint32_t*)(buf + o_tgt));
    if (hipGetLastError() != hipSuccess) return done(set_error(KAD_ERR_HIP, "refill: target launch failed"));
    if (int rc = kad_nc_closest_batch(nc, buf + o_tgt, m, KAD_SEARCH_NODES, d_rows, buf + o_cnt, nullptr)) return done(rc);
    const DevRefill D{ss->rec, ss->mkey, ss->mtail, ss->mflag, ss->cap, T.key, T.tail, T.n, T.index_base};
    (void)hipEventRecord(ss->rf_ev[0], nullptr);
    hipLaunchKernelGGL(refill_kernel, dim3((m + REFILL_WAVES - 1) / REFILL_WAVES), dim3(BLOCK), 0, nullptr, D, d_which, m,
                       d_rows, buf + o_cnt, (uint16_t*)(buf + o_ins), buf + o_st);
    const hipError_t le = hipGetLastError();
    (void)hipEventRecord(ss->rf_ev[1], nullptr);
    if (le != hipSuccess)
        return done(set_error(KAD_ERR_HIP, (std::string("refill: launch failed: ") + hipGetErrorString(le)).c_str()));
    const hipError_t ce = hipMemcpy(h, buf + o_back, total - o_back, hipMemcpyDeviceToHost);
    if (ce != hipSuccess)
        return done(set_error(KAD_ERR_HIP, (std::string("refill: D2H failed: ") + hipGetErrorString(ce)).c_str()));
    ss->rf_ms = elapsed_or_zero(ss->rf_ev[0], ss->rf_ev[1]);
    if (out_rows) std::memcpy(out_rows, h, o_ins - o_rows);
    std::memcpy(out_inserted, h + (o_ins - o_back), 2ull * m);
    std::memcpy(out_cnt, h + (o_cnt - o_back), m);
    std::memcpy(out_status, h + (o_st - o_back), m);
    return done(KAD_OK);
}

int kad_sr_refill_kernel_ms(const kad_searches* ss, float* out_ms) {
    if (!ss || !out_ms) return set_error(KAD_ERR_INVALID, "NULL argument");
    *out_ms = ss->rf_ms;
    return KAD_OK;
}

int kad_sr_insert(kad_searches* ss, uint32_t m, const uint32_t* which, const uint32_t* off, const uint8_t* cand_ids,
                  const uint8_t* cand_flags, uint8_t* out_inserted, uint8_t* out_status) {
    if (!ss) return set_error(KAD_ERR_INVALID, "NULL search set");
    if (m && (!which || !off || !out_status)) return set_error(KAD_ERR_INVALID, "NULL argument");
    if (m && off[m] > 0 && (!cand_ids || !out_inserted)) return set_error(KAD_ERR_INVALID, "NULL candidate arrays");
    std::string err;
    if (int rc = kadplan::sr_insert_check(ss->S, m, which, off, cand_flags, err)) return set_error(rc, err.c_str());
    if (m == 0) return KAD_OK;
    if (ss->cap > REFILL_MAX_CAP)
        return set_error(KAD_ERR_UNSUPPORTED, "kad_sr_insert handles slabs of up to 64 entries");
    const size_t T = off[m];
    // the call's scratch, one allocation: which, off, the candidate IDs and flags as one upload, then the result bytes
    // and the statuses as one copy back
    const size_t o_off = 4ull * m, o_ids = o_off + 4ull * (m + 1), o_fl = o_ids + 20ull * T, o_ins = o_fl + T,
                 o_st = o_ins + T, total = o_st + m;
    uint8_t* h = new (std::nothrow) uint8_t[total];
    if (!h) return set_error(KAD_ERR_NOMEM, "insert: out of host memory");
    std::memcpy(h, which, 4ull * m);
    std::memcpy(h + o_off, off, 4ull * (m + 1));
    if (T) std::memcpy(h + o_ids, cand_ids, 20ull * T);
    if (T && cand_flags)
        std::memcpy(h + o_fl, cand_flags, T);
    else
        std::memset(h + o_fl, 0, T);
    CallScratch cs(ss->device, h);
    if (int rc = cs.open(total, "insert")) return rc;
    uint8_t* const buf = cs.buf;
    if (!have_events(ss->in_ev)) return set_error(KAD_ERR_HIP, "insert: no events");
    if (hipMemcpy(buf, h, o_ins, hipMemcpyHostToDevice) != hipSuccess)
        return set_error(KAD_ERR_HIP, "insert: H2D failed");
    const DevInsert D{ss->rec, ss->mkey, ss->mtail, ss->mflag, ss->cap, m, (const uint32_t*)buf,
                      (const uint32_t*)(buf + o_off), buf + o_ids, buf + o_fl, buf + o_ins, buf + o_st};
    (void)hipEventRecord(ss->in_ev[0], nullptr);
    hipLaunchKernelGGL(insert_kernel, dim3((m + REFILL_WAVES - 1) / REFILL_WAVES), dim3(BLOCK), 0, nullptr, D);
    const hipError_t le = hipGetLastError();
    (void)hipEventRecord(ss->in_ev[1], nullptr);
    if (le != hipSuccess)
        return set_error(KAD_ERR_HIP, (std::string("insert: launch failed: ") + hipGetErrorString(le)).c_str());
    const hipError_t ce = hipMemcpy(h + o_ins, buf + o_ins, total - o_ins, hipMemcpyDeviceToHost);
    if (ce != hipSuccess)
        return set_error(KAD_ERR_HIP, (std::string("insert: D2H failed: ") + hipGetErrorString(ce)).c_str());
    ss->in_ms = elapsed_or_zero(ss->in_ev[0], ss->in_ev[1]);
    if (T) std::memcpy(out_inserted, h + o_ins, T);
    std::memcpy(out_status, h + o_st, m);
    return KAD_OK;
}

int kad_sr_insert_kernel_ms(const kad_searches* ss, float* out_ms) {
    if (!ss || !out_ms) return set_error(KAD_ERR_INVALID, "NULL argument");
    *out_ms = ss->in_ms;
    return KAD_OK;
}

int kad_sr_try_insert_tick(kad_searches* ss, const uint8_t* cand_ids, const uint8_t* cand_flags, uint32_t q,
                           uint32_t max_rounds, uint8_t* out_kind, uint32_t* out_round, uint32_t* out_lb,
                           uint32_t* out_fwd, uint32_t* out_back, uint8_t* out_stop, uint8_t* out_trim,
                           uint32_t* out_overflow, uint32_t* out_n_overflow, kad_sr_tick_stats* out_stats) {
    if (!ss) return set_error(KAD_ERR_INVALID, "NULL search set");
    if (q && (!cand_ids || !out_kind || !out_round || !out_lb || !out_fwd || !out_back || !out_stop || !out_trim))
        return set_error(KAD_ERR_INVALID, "NULL candidate or output array");
    if (!out_overflow || !out_n_overflow) return set_error(KAD_ERR_INVALID, "NULL overflow outputs");
    for (uint32_t j = 0; cand_flags && j < q; j++)
        if (cand_flags[j] & ~KAD_SN_BAD) return set_error(KAD_ERR_INVALID, "candidate flags: only KAD_SN_BAD may be set");
    kad_sr_tick_stats st = {};
    *out_n_overflow = 0;
    if (q == 0 || ss->S == 0) {  // no search refuses, none accepts
        for (uint32_t j = 0; j < q; j++) {
            out_kind[j] = (uint8_t)KAD_SR_TICK_SKIPPED;
            out_round[j] = out_lb[j] = out_fwd[j] = out_back[j] = 0;
            out_stop[j] = out_trim[j] = 0;
        }
        st.skipped = q;
        if (out_stats) *out_stats = st;
        return KAD_OK;
    }
    if (ss->cap > REFILL_MAX_CAP)
        return set_error(KAD_ERR_UNSUPPORTED, "kad_sr_try_insert_tick handles slabs of up to 64 entries");
    const uint32_t S = ss->S;
    // a round's pairs never share a search: at most S, sent in slices of P
    const uint64_t want_p = 2ull * q + 1024;
    const uint32_t P = (uint32_t)(want_p < S ? want_p : S);
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    // the call's scratch, one allocation: the candidates' IDs and flags (uploaded once), the positions that remain, the
    // verdicts, then per slice of pairs the searches and positions (one upload), the CSR insert_kernel reads and the
    // result and status bytes (one copy back)
    const size_t o_fl = up16(20ull * q), o_rem = up16(o_fl + q), o_ver = up16(o_rem + 4ull * q), o_pw = o_ver + 16ull * q,
                 o_off = up16(o_pw + 8ull * P), o_gid = up16(o_off + 4ull * (P + 1)), o_gfl = up16(o_gid + 20ull * P),
                 o_ins = up16(o_gfl + P), total = o_ins + 2ull * P;
    std::vector<uint32_t> h_ver, lb, fwd, back, rem, h_pairs;
    std::vector<uint8_t> stop, trim, h_res;
    kadplan::SrRoundPlan plan;
    try {
        h_ver.resize(4ull * q);
        lb.resize(q);
        fwd.resize(q);
        back.resize(q);
        stop.resize(q);
        trim.resize(q);
        rem.resize(q);
        h_pairs.resize(2ull * P);
        h_res.resize(2ull * P);
        plan.kind.reserve(q);
        plan.marked.reserve(((size_t)S + 63) / 64 + 1);
    } catch (const std::bad_alloc&) {
        return set_error(KAD_ERR_NOMEM, "tick: out of host memory");
    }
    CallScratch cs(ss->device);
    uint32_t n_rem = q, n_over = 0;
    auto done = [&](int r) {  // on every path: what was applied so far stands in the stats and the overflow count
        st.left = n_rem;
        st.overflowed = n_over;
        *out_n_overflow = n_over;
        if (out_stats) *out_stats = st;
        return r;
    };
    std::memset(out_kind, (int)KAD_SR_TICK_LEFT, q);
    if (int rc = cs.open(total, "tick")) return done(rc);
    uint8_t* const buf = cs.buf;
    if (!have_events(ss->tk_ev)) return done(set_error(KAD_ERR_HIP, "tick: no events"));
    if (hipMemcpy(buf, cand_ids, 20ull * q, hipMemcpyHostToDevice) != hipSuccess ||
        (cand_flags ? hipMemcpy(buf + o_fl, cand_flags, q, hipMemcpyHostToDevice)
                    : hipMemset(buf + o_fl, 0, q)) != hipSuccess)
        return done(set_error(KAD_ERR_HIP, "tick: H2D failed"));
    const DevSearches V{reinterpret_cast<const u32x4_t*>(ss->rec), ss->skey, ss->mkey, ss->mtail, ss->rdx, S, ss->cap,
                        ss->rshift};
    uint32_t* d_rem = (uint32_t*)(buf + o_rem);
    uint32_t* d_pw = (uint32_t*)(buf + o_pw);
    for (uint32_t j = 0; j < q; j++) rem[j] = j;
    std::string err;
    while (n_rem && n_over == 0 && (max_rounds == 0 || st.rounds < max_rounds)) {
        const uint32_t r = n_rem, round = ++st.rounds;
        if (round > 1 && hipMemcpy(d_rem, rem.data(), 4ull * r, hipMemcpyHostToDevice) != hipSuccess)
            return done(set_error(KAD_ERR_HIP, "tick: H2D of the remaining candidates failed"));
        const uint32_t blocks = (r + BLOCK - 1) / BLOCK, grid = blocks < MAX_GRID ? blocks : MAX_GRID;
        (void)hipEventRecord(ss->tk_ev[0], nullptr);
        if (S <= LDS_KEYS)
            hipLaunchKernelGGL(tick_verdict_kernel<true>, dim3(grid), dim3(BLOCK), 0, nullptr, V, buf,
                               round > 1 ? d_rem : nullptr, r, (u32x4_t*)(buf + o_ver));
        else
            hipLaunchKernelGGL(tick_verdict_kernel<false>, dim3(grid), dim3(BLOCK), 0, nullptr, V, buf,
                               round > 1 ? d_rem : nullptr, r, (u32x4_t*)(buf + o_ver));
        hipError_t le = hipGetLastError();
        (void)hipEventRecord(ss->tk_ev[1], nullptr);
        if (le != hipSuccess)
            return done(set_error(KAD_ERR_HIP, (std::string("tick: verdict launch failed: ") + hipGetErrorString(le)).c_str()));
        le = hipMemcpy(h_ver.data(), buf + o_ver, 16ull * r, hipMemcpyDeviceToHost);
        if (le != hipSuccess)
            return done(set_error(KAD_ERR_HIP, (std::string("tick: D2H of the verdicts failed: ") + hipGetErrorString(le)).c_str()));
        st.verdict_ms += elapsed_or_zero(ss->tk_ev[0], ss->tk_ev[1]);
        for (uint32_t k = 0; k < r; k++) {
            lb[k] = h_ver[4ull * k];
            fwd[k] = h_ver[4ull * k + 1];
            back[k] = h_ver[4ull * k + 2];
            stop[k] = (uint8_t)h_ver[4ull * k + 3];
            trim[k] = (uint8_t)((h_ver[4ull * k + 3] >> 8) & 3u);
        }
        try {
            if (kadplan::sr_round_plan(S, r, lb.data(), fwd.data(), back.data(), stop.data(), trim.data(), plan, err))
                return done(set_error(KAD_ERR_HIP, ("tick: verdict out of range: " + err).c_str()));
        } catch (const std::bad_alloc&) {
            return done(set_error(KAD_ERR_NOMEM, "tick: out of host memory"));
        }
        // the round's outputs stand before its inserts run: whatever happens then, they describe what was applied
        uint32_t n_next = 0;
        for (uint32_t k = 0; k < r; k++) {
            const uint32_t j = rem[k];
            if (plan.kind[k] == kadplan::SR_PLAN_DEFERRED) {
                n_next++;
                continue;
            }
            const bool ready = plan.kind[k] == kadplan::SR_PLAN_READY;
            out_kind[j] = ready ? (uint8_t)KAD_SR_TICK_APPLIED : (uint8_t)KAD_SR_TICK_SKIPPED;
            out_round[j] = round;
            out_lb[j] = lb[k];
            out_fwd[j] = fwd[k];
            out_back[j] = back[k];
            out_stop[j] = stop[k];
            out_trim[j] = trim[k];
            (ready ? st.applied : st.skipped)++;
        }
        n_rem = n_next;  // what waits for the next round, or stays LEFT
        const size_t n_pairs = plan.pair_which.size();
        for (size_t a = 0; a < n_pairs; a += P) {
            const uint32_t m = (uint32_t)(n_pairs - a < P ? n_pairs - a : P);
            for (uint32_t i = 0; i < m; i++) {
                h_pairs[i] = plan.pair_which[a + i];
                h_pairs[m + i] = rem[plan.pair_cand[a + i]];
            }
            if (hipMemcpy(d_pw, h_pairs.data(), 8ull * m, hipMemcpyHostToDevice) != hipSuccess)
                return done(set_error(KAD_ERR_HIP, "tick: H2D of the pairs failed"));
            const DevInsert D{ss->rec, ss->mkey, ss->mtail, ss->mflag, ss->cap, m, d_pw, (const uint32_t*)(buf + o_off),
                              buf + o_gid, buf + o_gfl, buf + o_ins, buf + o_ins + m};
            (void)hipEventRecord(ss->tk_ev[2], nullptr);
            hipLaunchKernelGGL(tick_gather_kernel, dim3(m / BLOCK + 1), dim3(BLOCK), 0, nullptr, buf, buf + o_fl, d_pw + m,
                               m, (uint32_t*)(buf + o_off), (uint32_t*)(buf + o_gid), buf + o_gfl);
            le = hipGetLastError();
            if (le == hipSuccess) {
                hipLaunchKernelGGL(insert_kernel, dim3((m + REFILL_WAVES - 1) / REFILL_WAVES), dim3(BLOCK), 0, nullptr, D);
                le = hipGetLastError();
            }
            (void)hipEventRecord(ss->tk_ev[3], nullptr);
            if (le != hipSuccess)
                return done(set_error(KAD_ERR_HIP, (std::string("tick: insert launch failed: ") + hipGetErrorString(le)).c_str()));
            le = hipMemcpy(h_res.data(), buf + o_ins, 2ull * m, hipMemcpyDeviceToHost);
            if (le != hipSuccess)
                return done(set_error(KAD_ERR_HIP, (std::string("tick: D2H of the results failed: ") + hipGetErrorString(le)).c_str()));
            st.insert_ms += elapsed_or_zero(ss->tk_ev[2], ss->tk_ev[3]);
            st.pairs += m;
            for (uint32_t i = 0; i < m; i++) {
                if (h_res[m + i] == KAD_SR_INSERT_OVERFLOW) {
                    out_overflow[n_over++] = plan.pair_which[a + i];  // the pairs ascend by search
                } else if (h_res[i] != plan.pair_want[a + i]) {
                    char msg[160];
                    std::snprintf(msg, sizeof msg, "tick: round %u, search %u answered %u to candidate %u against its verdict",
                                  round, plan.pair_which[a + i], (unsigned)h_res[i], rem[plan.pair_cand[a + i]]);
                    return done(set_error(KAD_ERR_HIP, msg));
                }
            }
        }
        n_next = 0;
        for (uint32_t k = 0; k < r; k++)
            if (plan.kind[k] == kadplan::SR_PLAN_DEFERRED) rem[n_next++] = rem[k];
    }
    return done(KAD_OK);
}

int kad_sr_mark_nodes(kad_searches* ss, uint32_t q, const uint8_t* node_ids, const uint8_t* clear_bits,
                      const uint8_t* set_bits, uint32_t p, const uint32_t* pair_which, const uint8_t* pair_ids,
                      const uint8_t* pair_flags, uint32_t* out_hits, uint8_t* out_pair_found, uint32_t* out_changed,
                      uint8_t* out_counts, uint32_t* out_n_changed) {
    if (!ss || !out_changed || !out_n_changed) return set_error(KAD_ERR_INVALID, "NULL argument");
    if (q && !node_ids) return set_error(KAD_ERR_INVALID, "NULL node_ids");
    if (p && (!pair_which || !pair_ids || !pair_flags)) return set_error(KAD_ERR_INVALID, "NULL pair arrays");
    kadplan::SrMarkPlan plan;
    std::string err;
    try {
        if (int rc = kadplan::sr_mark_plan(ss->S, q, node_ids, clear_bits, set_bits, p, pair_which, pair_ids, pair_flags,
                                           plan, err))
            return set_error(rc, err.c_str());
    } catch (const std::bad_alloc&) {
        return set_error(KAD_ERR_NOMEM, "mark: out of host memory");
    }
    if (q > KAD_SR_MARK_MAX_NODES) return set_error(KAD_ERR_UNSUPPORTED, "kad_sr_mark_nodes takes up to 2^20 nodes a call");
    if (ss->cap > REFILL_MAX_CAP)
        return set_error(KAD_ERR_UNSUPPORTED, "kad_sr_mark_nodes handles slabs of up to 64 entries");
    *out_n_changed = 0;
    if (out_hits && q) std::memset(out_hits, 0, 4ull * q);
    if (out_pair_found && p) std::memset(out_pair_found, 0, p);
    if ((q == 0 && p == 0) || ss->S == 0) return KAD_OK;
    const uint32_t S = ss->S;
    // The call's buffer. Up: batch keys, pair keys, batch tails, pair tails, pair searches, the batch's prefix directory,
    // ops, pair bytes, as one copy. Back, as one copy: the count of changed searches, the hits, the first n_res (search,
    // count word) pairs and the found bytes. More than n_res changed searches (batch nodes held by many searches each)
    // take a second copy, of all pairs, from the handle's scratch.
    const uint64_t want_res = 2ull * q + p + 64;
    const uint32_t n_res = (uint32_t)(want_res < S ? want_res : S);
    const size_t n_dir = plan.dir.size();
    const size_t o_pkey = 8ull * q, o_btail = o_pkey + 8ull * p, o_ptail = o_btail + 12ull * q, o_pw = o_ptail + 12ull * p,
                 o_dir = o_pw + 4ull * p, o_bop = o_dir + 4ull * n_dir, o_pfl = o_bop + q, o_out = (o_pfl + p + 7) & ~(size_t)7, o_hits = o_out + 8,
                 o_res = (o_hits + 4ull * q + 7) & ~(size_t)7, o_found = o_res + 8ull * n_res, total = o_found + p;
    uint8_t* h = new (std::nothrow) uint8_t[total];
    if (!h) return set_error(KAD_ERR_NOMEM, "mark: out of host memory");
    if (q) {
        std::memcpy(h, plan.bkey.data(), 8ull * q);
        std::memcpy(h + o_btail, plan.btail.data(), 12ull * q);
        std::memcpy(h + o_bop, plan.bop.data(), q);
        std::memcpy(h + o_dir, plan.dir.data(), 4ull * n_dir);
    }
    if (p) {
        std::memcpy(h + o_pkey, plan.pkey.data(), 8ull * p);
        std::memcpy(h + o_ptail, plan.ptail.data(), 12ull * p);
        std::memcpy(h + o_pw, plan.pw.data(), 4ull * p);
        std::memcpy(h + o_pfl, plan.pfl.data(), p);
    }
    DeviceGuard g(ss->device);
    uint8_t* buf = nullptr;
    auto done = [&](int r) {
        if (buf) (void)hipFree(buf);
        delete[] h;
        return r;
    };
    if (hipDeviceSynchronize() != hipSuccess)  // queries enqueued before the call read the old set
        return done(set_error(KAD_ERR_HIP, "mark: device in error"));
    const size_t b_bitmap = 4ull * ((S + 31) / 32), b_scratch = MARK_HEAD_BYTES + 8ull * S + b_bitmap + 4ull * S;
    if (ss->mk_cap < S) {  // first use, or kad_searches_apply made the set larger since
        uint8_t* nb = nullptr;
        if (hipMalloc((void**)&nb, b_scratch) != hipSuccess) {
            (void)hipGetLastError();
            return done(set_error(KAD_ERR_NOMEM, "mark: out of device memory"));
        }
        if (ss->mk_buf) (void)hipFree(ss->mk_buf);
        ss->mk_buf = nb;
        ss->mk_cap = S;
        ss->mk_bytes = b_scratch;
    }
    if (hipMalloc((void**)&buf, total) != hipSuccess) {
        (void)hipGetLastError();
        buf = nullptr;
        return done(set_error(KAD_ERR_NOMEM, "mark: out of device memory"));
    }
    if (!have_events(ss->mk_ev)) return done(set_error(KAD_ERR_HIP, "mark: no events"));
    // the scratch is laid out for mk_cap searches; only the part of the current S is used
    const size_t cap_bitmap = 4ull * (((size_t)ss->mk_cap + 31) / 32);
    // the count, the (search, count word) pairs of the last call, the bitmap, the list
    uint32_t* d_head = (uint32_t*)ss->mk_buf;
    uint64_t* d_all = (uint64_t*)(ss->mk_buf + MARK_HEAD_BYTES);
    uint32_t* d_bitmap = (uint32_t*)(ss->mk_buf + MARK_HEAD_BYTES + 8ull * ss->mk_cap);
    uint32_t* d_list = (uint32_t*)(ss->mk_buf + MARK_HEAD_BYTES + 8ull * ss->mk_cap + cap_bitmap);
    if (hipMemcpy(buf, h, o_out, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemsetAsync(d_head, 0, MARK_HEAD_BYTES, nullptr) != hipSuccess ||
        hipMemsetAsync(d_bitmap, 0, b_bitmap, nullptr) != hipSuccess ||
        hipMemsetAsync(buf + o_out, 0, total - o_out, nullptr) != hipSuccess)
        return done(set_error(KAD_ERR_HIP, "mark: H2D failed"));
    const DevMark D{ss->rec, ss->mkey, ss->mtail, ss->mflag, S, ss->cap, S * ss->cap, q, (const uint64_t*)buf,
                    (const uint32_t*)(buf + o_btail), buf + o_bop, (const uint32_t*)(buf + o_dir), 64u - plan.dbits, p,
                    (const uint32_t*)(buf + o_pw),
                    (const uint64_t*)(buf + o_pkey), (const uint32_t*)(buf + o_ptail), buf + o_pfl,
                    out_hits ? (uint32_t*)(buf + o_hits) : nullptr, buf + o_found, d_head, d_bitmap, d_list};
    hipError_t le = hipSuccess;
    (void)hipEventRecord(ss->mk_ev[0], nullptr);
    if (q) {
        const uint32_t blocks = (D.total + BLOCK - 1) / BLOCK, grid = blocks < MAX_GRID ? blocks : MAX_GRID;
        if (q <= MARK_LDS_KEYS)
            hipLaunchKernelGGL(mark_scan_kernel<true>, dim3(grid), dim3(BLOCK), 0, nullptr, D);
        else
            hipLaunchKernelGGL(mark_scan_kernel<false>, dim3(grid), dim3(BLOCK), 0, nullptr, D);
        le = hipGetLastError();
    }
    (void)hipEventRecord(ss->mk_ev[1], nullptr);
    if (le == hipSuccess && p) {
        hipLaunchKernelGGL(mark_pairs_kernel, dim3((p + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, nullptr, D);
        le = hipGetLastError();
    }
    (void)hipEventRecord(ss->mk_ev[2], nullptr);
    if (le == hipSuccess) {  // the grid is sized without the count: the waves stride over what the head word says
        const uint32_t blocks = (S + REFILL_WAVES - 1) / REFILL_WAVES, grid = blocks < MARK_FIX_GRID ? blocks : MARK_FIX_GRID;
        hipLaunchKernelGGL(mark_fix_kernel, dim3(grid), dim3(BLOCK), 0, nullptr, D, d_all, (uint32_t*)(buf + o_out),
                           (uint64_t*)(buf + o_res), n_res);
        le = hipGetLastError();
    }
    (void)hipEventRecord(ss->mk_ev[3], nullptr);
    if (le != hipSuccess)
        return done(set_error(KAD_ERR_HIP, (std::string("mark: launch failed: ") + hipGetErrorString(le)).c_str()));
    const hipError_t ce = hipMemcpy(h + o_out, buf + o_out, total - o_out, hipMemcpyDeviceToHost);
    if (ce != hipSuccess)
        return done(set_error(KAD_ERR_HIP, (std::string("mark: D2H failed: ") + hipGetErrorString(ce)).c_str()));
    if (hipEventElapsedTime(&ss->mk_ms[0], ss->mk_ev[0], ss->mk_ev[1]) != hipSuccess ||
        hipEventElapsedTime(&ss->mk_ms[1], ss->mk_ev[2], ss->mk_ev[3]) != hipSuccess) {
        (void)hipGetLastError();
        ss->mk_ms[0] = ss->mk_ms[1] = 0.f;
    }
    uint32_t n_changed;
    std::memcpy(&n_changed, h + o_out, 4);
    if (n_changed > S) return done(set_error(KAD_ERR_HIP, "mark: changed count out of range"));
    std::vector<uint64_t> res;  // count word << 32 | search: the search is what the sort goes by
    try {
        res.resize(n_changed);
        if (n_changed <= n_res) {
            if (n_changed) std::memcpy(res.data(), h + o_res, 8ull * n_changed);
        } else {
            if (hipMemcpy(res.data(), d_all, 8ull * n_changed, hipMemcpyDeviceToHost) != hipSuccess)
                return done(set_error(KAD_ERR_HIP, "mark: D2H of the changed list failed"));
        }
    } catch (const std::bad_alloc&) {
        return done(set_error(KAD_ERR_NOMEM, "mark: out of host memory"));
    }
    std::sort(res.begin(), res.end(), [](uint64_t a, uint64_t b) { return (uint32_t)a < (uint32_t)b; });
    for (uint32_t k = 0; k < n_changed; k++) {
        out_changed[k] = (uint32_t)res[k];
        if (out_counts) {
            const uint32_t c = (uint32_t)(res[k] >> 32);
            out_counts[4ull * k] = (uint8_t)c;
            out_counts[4ull * k + 1] = (uint8_t)(c >> 8);
            out_counts[4ull * k + 2] = (uint8_t)(c >> 16);
            out_counts[4ull * k + 3] = (uint8_t)(c >> 24);
        }
    }
    if (out_hits)
        for (uint32_t j = 0; j < q; j++) std::memcpy(out_hits + plan.ord[j], h + o_hits + 4ull * j, 4);
    if (out_pair_found)
        for (uint32_t k = 0; k < p; k++) out_pair_found[plan.pord[k]] = h[o_found + k];
    *out_n_changed = n_changed;
    return done(KAD_OK);
}

int kad_sr_mark_kernel_ms(const kad_searches* ss, float* out_scan_ms, float* out_fix_ms) {
    if (!ss || !out_scan_ms || !out_fix_ms) return set_error(KAD_ERR_INVALID, "NULL argument");
    *out_scan_ms = ss->mk_ms[0];
    *out_fix_ms = ss->mk_ms[1];
    return KAD_OK;
}

namespace {
// kad_sr_mark_entries and kad_sr_mark_due: one body, the bits that may be named decided by `plan_fn`
using EntriesPlanFn = int (*)(uint32_t, uint32_t, const uint32_t*, const uint8_t*, const uint8_t*, const uint8_t*,
                              kadplan::SrEntriesPlan&, std::string&);

int mark_entry_bits(kad_searches* ss, uint32_t p, const uint32_t* pair_which, const uint8_t* pair_ids,
                    const uint8_t* clear_bits, const uint8_t* set_bits, uint8_t* out_found, EntriesPlanFn plan_fn,
                    const char* unsupported) {
    if (!ss) return set_error(KAD_ERR_INVALID, "NULL search set");
    if (p && (!pair_which || !pair_ids)) return set_error(KAD_ERR_INVALID, "NULL pair arrays");
    kadplan::SrEntriesPlan plan;
    std::string err;
    try {
        if (int rc = plan_fn(ss->S, p, pair_which, pair_ids, clear_bits, set_bits, plan, err))
            return set_error(rc, err.c_str());
    } catch (const std::bad_alloc&) {
        return set_error(KAD_ERR_NOMEM, "mark entries: out of host memory");
    }
    if (p == 0 || ss->S == 0) return KAD_OK;
    if (ss->cap > REFILL_MAX_CAP)
        return set_error(KAD_ERR_UNSUPPORTED, unsupported);
    // the call's buffer, one upload: keys, tails, searches, the two op bytes; then the found bytes, one copy back
    const size_t o_tail = 8ull * p, o_pw = o_tail + 12ull * p, o_clear = o_pw + 4ull * p, o_set = o_clear + p,
                 o_found = o_set + p, total = o_found + p;
    uint8_t* h = new (std::nothrow) uint8_t[total];
    if (!h) return set_error(KAD_ERR_NOMEM, "mark entries: out of host memory");
    std::memcpy(h, plan.pkey.data(), 8ull * p);
    std::memcpy(h + o_tail, plan.ptail.data(), 12ull * p);
    std::memcpy(h + o_pw, plan.pw.data(), 4ull * p);
    std::memcpy(h + o_clear, plan.pclear.data(), p);
    std::memcpy(h + o_set, plan.pset.data(), p);
    CallScratch cs(ss->device, h);
    if (int rc = cs.open(total, "mark entries")) return rc;
    uint8_t* const buf = cs.buf;
    if (hipMemcpy(buf, h, o_found, hipMemcpyHostToDevice) != hipSuccess)
        return set_error(KAD_ERR_HIP, "mark entries: H2D failed");
    const DevEntries D{ss->rec, ss->mkey, ss->mtail, ss->mflag, ss->cap, p, (const uint32_t*)(buf + o_pw),
                       (const uint64_t*)buf, (const uint32_t*)(buf + o_tail), buf + o_clear, buf + o_set, buf + o_found};
    hipLaunchKernelGGL(entries_kernel, dim3((p + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, nullptr, D);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess)
        return set_error(KAD_ERR_HIP, (std::string("mark entries: launch failed: ") + hipGetErrorString(le)).c_str());
    const hipError_t ce = hipMemcpy(h + o_found, buf + o_found, p, hipMemcpyDeviceToHost);
    if (ce != hipSuccess)
        return set_error(KAD_ERR_HIP, (std::string("mark entries: D2H failed: ") + hipGetErrorString(ce)).c_str());
    if (out_found)
        for (uint32_t k = 0; k < p; k++) out_found[plan.pord[k]] = h[o_found + k];
    return KAD_OK;
}
}  // namespace

int kad_sr_mark_entries(kad_searches* ss, uint32_t p, const uint32_t* pair_which, const uint8_t* pair_ids,
                        const uint8_t* clear_bits, const uint8_t* set_bits, uint8_t* out_found) {
    return mark_entry_bits(ss, p, pair_which, pair_ids, clear_bits, set_bits, out_found, kadplan::sr_entries_plan,
                           "kad_sr_mark_entries handles slabs of up to 64 entries");
}

int kad_sr_mark_due(kad_searches* ss, uint32_t p, const uint32_t* pair_which, const uint8_t* pair_ids,
                    const uint8_t* clear_bits, const uint8_t* set_bits, uint8_t* out_found) {
    return mark_entry_bits(ss, p, pair_which, pair_ids, clear_bits, set_bits, out_found, kadplan::sr_due_plan,
                           "kad_sr_mark_due handles slabs of up to 64 entries");
}

int kad_sr_step(kad_searches* ss, uint32_t m, const uint32_t* which, const uint8_t* mode, kad_step_out* out,
                kad_sr_step_stats* out_stats) {
    return step_call(ss, m, which, mode, out, out_stats, kadplan::sr_step_check, "step",
                     "kad_sr_step handles slabs of up to 64 entries");
}

int kad_sr_step_full(kad_searches* ss, uint32_t m, const uint32_t* which, const uint8_t* mode, kad_step_full_out* out,
                     kad_sr_step_full_stats* out_stats) {
    return step_call(ss, m, which, mode, out, out_stats, kadplan::sr_step_full_check, "step full",
                     "kad_sr_step_full handles slabs of up to 64 entries");
}

int kad_sr_try_insert_batch_host(const kad_searches* ss, const uint8_t* ids, uint32_t q, uint32_t* out_lb,
                                 uint32_t* out_fwd, uint32_t* out_back, uint8_t* out_stop) {
    if (!ss) return set_error(KAD_ERR_INVALID, "NULL search set");
    if (!ids || !out_fwd || !out_back || !out_stop) return set_error(KAD_ERR_INVALID, "NULL buffer");
    if (q == 0) return KAD_OK;
    DeviceGuard g(ss->device);
    // one allocation: ids, then the lb, fwd and back words, then the stop bytes
    uint8_t* buf = nullptr;
    hipStream_t s = nullptr;
    auto done = [&](int r) {
        if (s) (void)hipStreamDestroy(s);
        if (buf) (void)hipFree(buf);
        return r;
    };
    const size_t o_lb = 20ull * q, o_fwd = o_lb + 4ull * q, o_back = o_fwd + 4ull * q, o_stop = o_back + 4ull * q;
    if (hipMalloc((void**)&buf, o_stop + q) != hipSuccess) {
        (void)hipGetLastError();
        return done(set_error(KAD_ERR_NOMEM, "try_insert host batch: out of device memory"));
    }
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess)
        return done(set_error(KAD_ERR_HIP, "try_insert host batch: no stream"));
    if (hipMemcpyAsync(buf, ids, 20ull * q, hipMemcpyHostToDevice, s) != hipSuccess)
        return done(set_error(KAD_ERR_HIP, "try_insert host batch: H2D failed"));
    int rc = launch(ss, buf, q, (uint32_t*)(buf + o_lb), (uint32_t*)(buf + o_fwd), (uint32_t*)(buf + o_back),
                    buf + o_stop, s);
    if (rc == KAD_OK &&
        ((out_lb && hipMemcpyAsync(out_lb, buf + o_lb, 4ull * q, hipMemcpyDeviceToHost, s) != hipSuccess) ||
         hipMemcpyAsync(out_fwd, buf + o_fwd, 4ull * q, hipMemcpyDeviceToHost, s) != hipSuccess ||
         hipMemcpyAsync(out_back, buf + o_back, 4ull * q, hipMemcpyDeviceToHost, s) != hipSuccess ||
         hipMemcpyAsync(out_stop, buf + o_stop, q, hipMemcpyDeviceToHost, s) != hipSuccess))
        rc = set_error(KAD_ERR_HIP, "try_insert host batch: D2H failed");
    const hipError_t e = hipStreamSynchronize(s);
    if (rc == KAD_OK && e != hipSuccess)
        rc = set_error(KAD_ERR_HIP, (std::string("try_insert host batch: ") + hipGetErrorString(e)).c_str());
    return done(rc);
}

}  // extern "C"
