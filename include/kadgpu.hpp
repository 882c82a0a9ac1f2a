/*
 * kadgpu.hpp — C++11 host shim over the kadgpu C ABI, with OpenDHT's own signatures.
 *
 * Drop-in for the reference path (OpenDHT 1.2.1):
 *   RoutingTable::findClosestNodes(const InfoHash, time_point, size_t)   routing_table.h:48
 *   RoutingTable::findBucket(const InfoHash&)                            routing_table.h:50-51
 *   NodeCache::getCachedNodes(const InfoHash&, sa_family_t, size_t)      node_cache.h:32
 *   Dht::findClosestNodes(id, af, count) -- the accessor SURVEY.md §0.3 asks for, equal to
 *   buckets(af).findClosestNodes(id, scheduler.time(), count)             dht.h:437-438
 *
 * The shim is generic over the reference's types, so it compiles against OpenDHT's own headers
 * without modifying them (and against test doubles of the same shape):
 *   RoutingTableT : iterable of Buckets in ascending `first` order (std::list<Bucket>)
 *   Bucket        : `first` (20 contiguous bytes via .data()), `nodes` (iterable of shared_ptr<NodeT>)
 *   NodeT         : `id` (20 bytes via .data()), `bool isGood(time_point) const`, `bool isExpired() const`
 *   NodeMapT      : std::map<InfoHash, std::weak_ptr<NodeT>> (one NodeCache family, node_cache.h:42-50)
 *
 * A mirror holds the table's node IDs, bucket directory and every node's liveness (Node::time,
 * reply_time, isExpired(); node.h:39-40, 67) on the device. findClosestNodes(id, now, count) evaluates
 * Node::isGood(now) for the `now` it is given, as the reference does per call (routing_table.cpp:77):
 * when `now` moves, kad_table_refresh_status re-derives the status on the device and rebuilds only what
 * flipped. Results come back as the same shared_ptr<NodeT> objects the table holds, in the reference's
 * order. What the mirror cannot observe must be reported:
 *   - liveness changes of a node (Node::received, setExpired, reset, a search writing node->time):
 *     nodeUpdated(node) before the next query (or syncTimes() to re-read every node);
 *   - table mutations (Dht::onNewNode / expireBuckets / split): nodeRemoved / nodeReplaced / nodeAdded /
 *     bucketSplit, then flush(now): kad_table_apply replays them on the device copy; or re-snapshot.
 */
#ifndef KADGPU_HPP
#define KADGPU_HPP

#include <sys/socket.h>  // AF_INET (sa_family_t), as OpenDHT's sockaddr.h

#include <algorithm>
#include <array>
#include <chrono>
#include <climits>
#include <cstdint>
#include <functional>
#include <unordered_map>
#include <cstring>
#include <iterator>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "kadgpu.h"

namespace kadgpu {

class Error : public std::runtime_error {
public:
    Error(int code, const std::string& what) : std::runtime_error(what), code_(code) {}
    int code() const { return code_; }

private:
    int code_;
};

inline void check(int rc, const char* where) {
    if (rc != KAD_OK) throw Error(rc, std::string(where) + ": " + kad_last_error());
}

/* RAII owner of one device table (kad_table_create / kad_table_destroy). */
class DeviceTable {
public:
    DeviceTable() {}
    DeviceTable(int device, const std::vector<uint8_t>& ids, const std::vector<uint8_t>& status,
                const std::vector<uint8_t>& bucket_first, const std::vector<uint32_t>& bucket_offset,
                uint32_t index_base = 0, bool sorted = false) {
        const uint32_t n = (uint32_t)(ids.size() / KAD_HASH_LEN);
        const uint32_t B = (uint32_t)(bucket_first.size() / KAD_HASH_LEN);
        check(kad_table_create(&t_, device, n, ids.data(), status.data(), B, B ? bucket_first.data() : nullptr,
                               B ? bucket_offset.data() : nullptr, index_base, sorted ? KAD_TABLE_SORTED : 0u),
              "kad_table_create");
    }
    ~DeviceTable() { reset(); }
    DeviceTable(const DeviceTable&) = delete;
    DeviceTable& operator=(const DeviceTable&) = delete;
    DeviceTable(DeviceTable&& o) : t_(o.t_) { o.t_ = nullptr; }
    DeviceTable& operator=(DeviceTable&& o) {
        if (this != &o) { reset(); t_ = o.t_; o.t_ = nullptr; }
        return *this;
    }
    void reset() {
        if (t_) kad_table_destroy(t_);
        t_ = nullptr;
    }
    kad_table* get() const { return t_; }
    explicit operator bool() const { return t_ != nullptr; }

    /* Resident query service for single requests (kad_table_serve); idle_us = 0 turns it off. */
    void serve(uint32_t idle_us) const { check(kad_table_serve(t_, idle_us), "kad_table_serve"); }

    /* Host-buffer batch queries (synchronous). Rows of `count` indices, KAD_NO_NODE padded. */
    void findClosestNodesBatch(const uint8_t* targets, size_t q, size_t count, std::vector<uint32_t>& idx,
                               std::vector<uint8_t>& cnt) const {
        idx.resize(q * count);
        cnt.resize(q);
        if (q) check(kad_rt_closest_batch_host(t_, targets, (uint32_t)q, (uint32_t)count, idx.data(), cnt.data()),
                     "kad_rt_closest_batch_host");
    }
    void getCachedNodesBatch(const uint8_t* targets, size_t q, size_t count, std::vector<uint32_t>& idx,
                             std::vector<uint8_t>& cnt) const {
        idx.resize(q * count);
        cnt.resize(q);
        if (q) check(kad_nc_closest_batch_host(t_, targets, (uint32_t)q, (uint32_t)count, idx.data(), cnt.data()),
                     "kad_nc_closest_batch_host");
    }

    /* Storage-responsibility verdicts on host buffers (kad_rt_responsible_batch_host): one byte per target. */
    void responsibleBatch(const uint8_t* self_id, const uint8_t* targets, size_t q, size_t count, size_t min_nodes,
                          std::vector<uint8_t>& far) const {
        far.resize(q);
        if (q) check(kad_rt_responsible_batch_host(t_, self_id, targets, (uint32_t)q, (uint32_t)count,
                                                   (uint32_t)min_nodes, far.data()),
                     "kad_rt_responsible_batch_host");
    }

    /* onNewNode triage verdicts on host buffers (kad_rt_triage_batch_host); self_id may be NULL. */
    void triageBatch(const uint8_t* self_id, const uint8_t* ids, size_t q, uint32_t flags, std::vector<uint8_t>& verdict,
                     std::vector<uint32_t>& node, std::vector<uint32_t>& bucket) const {
        verdict.resize(q);
        node.resize(q);
        bucket.resize(q);
        if (q) check(kad_rt_triage_batch_host(t_, self_id, ids, (uint32_t)q, flags, verdict.data(), node.data(),
                                              bucket.data()),
                     "kad_rt_triage_batch_host");
    }

    /* The whole-table sweep on host buffers (kad_table_sweep_host): the totals alone. */
    kad_sweep_totals sweepTotals(uint32_t flags) const {
        kad_sweep_totals tot;
        check(kad_table_sweep_host(t_, flags, &tot, nullptr, 0, nullptr, 0), "kad_table_sweep_host");
        return tot;
    }

    /* Node liveness (kad_table_set_times / kad_table_patch_times) and the device-side isGood(now)
     * refresh (kad_table_refresh_status, incremental). */
    void setTimes(const std::vector<int64_t>& time_ns, const std::vector<int64_t>& reply_ns,
                  const std::vector<uint8_t>& expired) {
        check(kad_table_set_times(t_, time_ns.data(), reply_ns.data(), expired.data()), "kad_table_set_times");
    }
    void patchTimes(const std::vector<uint32_t>& nodes, const std::vector<int64_t>& time_ns,
                    const std::vector<int64_t>& reply_ns, const std::vector<uint8_t>& expired) {
        if (!nodes.empty())
            check(kad_table_patch_times(t_, (uint32_t)nodes.size(), nodes.data(), time_ns.data(), reply_ns.data(),
                                        expired.data()), "kad_table_patch_times");
    }
    void patchStatus(const std::vector<uint32_t>& nodes, const std::vector<uint8_t>& status) {
        if (!nodes.empty())
            check(kad_table_patch_status(t_, (uint32_t)nodes.size(), nodes.data(), status.data()),
                  "kad_table_patch_status");
    }
    void refreshStatus(int64_t now_ns) {
        check(kad_table_refresh_status(t_, now_ns, nullptr), "kad_table_refresh_status");
    }

private:
    kad_table* t_ = nullptr;
};

/* One candidate's onNewNode triage (kad_rt_triage_batch): verdict = KAD_NN_* kind | KAD_NN_MYBUCKET, node = the
 * mirror's node index the kind names (KAD_NO_NODE if none), bucket = findBucket(id) (KAD_NO_NODE for KAD_NN_NONE). */
struct NewNodeVerdict {
    uint8_t verdict;
    uint32_t node;
    uint32_t bucket;
};

/* Dht::getNodesStats' counts (dht.cpp:2470-2495) plus the expired nodes (what expireBuckets would remove). `cached`
 * (Bucket::cached) is host state and stays with the caller. */
struct NodesStats {
    unsigned good, dubious, incoming, expired;
};

/* What RoutingTableMirror::expireBuckets removed from the mirror: the nodes (erase them from the host's lists) and the
 * indices of the buckets that held them (sendCachedPing for each, dht.cpp:953-954). */
template <class NodePtrT>
struct Expired {
    std::vector<NodePtrT> removed;
    std::vector<uint32_t> buckets;
};

/* time_point -> int64 nanoseconds of its clock, time_point::min()/max() -> INT64_MIN/MAX (Node::time and
 * reply_time start at time_point::min(), node.h:39-40). */
template <class TimePoint>
inline int64_t to_ns(TimePoint tp) {
    if (tp == TimePoint::min()) return INT64_MIN;
    if (tp == TimePoint::max()) return INT64_MAX;
    return (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(tp.time_since_epoch()).count();
}

/* Status byte of a node at `now`: Node::isGood(now) | Node::isExpired() << 1 (node.cpp:34-40, node.h:67). */
template <class NodePtr, class TimePoint>
inline uint8_t status_of(const NodePtr& n, TimePoint now) {
    return (uint8_t)((n->isGood(now) ? KAD_STATUS_GOOD : 0u) | (n->isExpired() ? KAD_STATUS_EXPIRED : 0u));
}

template <class T>
inline const uint8_t* id_bytes(const T& id) {
    static_assert(sizeof(id) == KAD_HASH_LEN, "InfoHash must be 20 contiguous bytes");
    return reinterpret_cast<const uint8_t*>(id.data());
}

/* Bucket::time (routing_table.h:34) in ns where the bucket type has the member; a table type without it (a caller
 * that does not use the bucket times) mirrors none. */
template <class B>
inline auto bucket_time_ns(const B& b, int) -> decltype(to_ns(b.time)) { return to_ns(b.time); }
template <class B>
inline int64_t bucket_time_ns(const B&, long) { return INT64_MIN; }
template <class B>
inline auto has_bucket_time(int) -> decltype((void)std::declval<const B&>().time, std::true_type()) { return std::true_type(); }
template <class B>
inline std::false_type has_bucket_time(long) { return std::false_type(); }

/* What RoutingTableMirror::bucketMaintenance's loop (dht.cpp:2832-2850) came to: found = a node came out; then bucket =
 * the index of b, q = the index of the bucket the node was drawn from, id = randomId(b), node = q->randomNode(). The
 * `want` decision (:2852-2866), the request and the scheduler edit stay with the caller. */
template <class NodePtrT>
struct MaintenancePick {
    using InfoHashT = typename std::decay<decltype(std::declval<const NodePtrT&>()->id)>::type;
    bool found;
    uint32_t bucket;
    uint32_t q;
    InfoHashT id;
    NodePtrT node;
};

/* Device mirror of one RoutingTable (one address family). */
template <class RoutingTableT>
class RoutingTableMirror {
public:
    using BucketT = typename std::decay<decltype(*std::declval<const RoutingTableT&>().begin())>::type;
    using NodePtr = typename std::decay<decltype(*std::declval<const BucketT&>().nodes.begin())>::type;

    RoutingTableMirror() {}

    template <class TimePoint>
    RoutingTableMirror(const RoutingTableT& rt, TimePoint now, int device = 0) {
        snapshot(rt, now, device);
    }

    /* Snapshot `rt`: nodes grouped by bucket in list order, their liveness, status at `now`. */
    template <class TimePoint>
    void snapshot(const RoutingTableT& rt, TimePoint now, int device = 0) {
        std::vector<uint8_t> ids, status, first;
        std::vector<uint32_t> off;
        std::vector<int64_t> btime;
        nodes_.clear();
        for (const auto& b : rt) {
            off.push_back((uint32_t)nodes_.size());
            btime.push_back(bucket_time_ns(b, 0));
            first.insert(first.end(), id_bytes(b.first), id_bytes(b.first) + KAD_HASH_LEN);
            for (const auto& n : b.nodes) {
                nodes_.push_back(n);
                ids.insert(ids.end(), id_bytes(n->id), id_bytes(n->id) + KAD_HASH_LEN);
                status.push_back(status_of(n, now));
            }
        }
        off.push_back((uint32_t)nodes_.size());
        buckets_ = (uint32_t)(off.size() - 1);
        table_ = DeviceTable(device, ids, status, first, off);
        if (decltype(has_bucket_time<BucketT>(0))::value && buckets_)  // every Bucket::time, where the table has them
            check(kad_table_set_bucket_times(table_.get(), btime.data()), "kad_table_set_bucket_times");
        first_.swap(first);
        off_.swap(off);
        reindex();
        syncTimes();
        now_ns_ = to_ns(now);
        refresh_ = false;
    }

    /* RoutingTable::findClosestNodes(id, now, count) (routing_table.h:48, routing_table.cpp:67-111). */
    template <class InfoHashT, class TimePoint>
    std::vector<NodePtr> findClosestNodes(const InfoHashT& id, TimePoint now, size_t count = KAD_TARGET_NODES) const {
        std::vector<std::vector<NodePtr>> r = findClosestNodesBatch(&id, 1, now, count);
        return std::move(r[0]);
    }

    /* Batched form: one result vector per target, all at the same `now`. */
    template <class InfoHashT, class TimePoint>
    std::vector<std::vector<NodePtr>> findClosestNodesBatch(const InfoHashT* ids, size_t q, TimePoint now,
                                                            size_t count = KAD_TARGET_NODES) const {
        if (q <= hostBatchLimit() && count <= host_count_) {  // a few requests: the host path (no device round trip)
            std::vector<std::vector<NodePtr>> out(q);
            for (size_t i = 0; i < q; i++) out[i] = findClosestNodesHost(ids[i], now, count);
            return out;
        }
        advance(to_ns(now));
        std::vector<std::vector<NodePtr>> out(q);
        // any size_t count, as routing_table.h:48: a result never holds more than the table's nodes
        count = std::min(count, nodes_.size());
        if (count == 0 || q == 0) return out;
        std::vector<uint8_t> targets(q * KAD_HASH_LEN);
        for (size_t i = 0; i < q; i++) std::memcpy(&targets[i * KAD_HASH_LEN], id_bytes(ids[i]), KAD_HASH_LEN);
        std::vector<uint32_t> idx;
        std::vector<uint8_t> cnt;
        table_.findClosestNodesBatch(targets.data(), q, count, idx, cnt);
        for (size_t i = 0; i < q; i++) {
            size_t m = cnt[i];
            if (count > 255)  // the count byte saturates: the row's padding gives the length
                for (m = 0; m < count && idx[i * count + m] != KAD_NO_NODE; m++) {}
            out[i].reserve(m);
            for (size_t j = 0; j < m; j++) out[i].push_back(nodes_[idx[i * count + j]]);
        }
        return out;
    }
    template <class InfoHashT, class TimePoint>
    std::vector<std::vector<NodePtr>> findClosestNodesBatch(const std::vector<InfoHashT>& ids, TimePoint now,
                                                            size_t count = KAD_TARGET_NODES) const {
        return findClosestNodesBatch(ids.data(), ids.size(), now, count);
    }

    /* The storage-responsibility question of Dht::maintainStorage (dht.cpp:2909-2937: count = TARGET_NODES,
     * min_nodes = 1) and Dht::onAnnounce (dht.cpp:3352-3358: count = SEARCH_NODES, min_nodes = TARGET_NODES), per id:
     * 1 when findClosestNodes(id, now, count) returns at least max(min_nodes, 1) nodes and
     * id.xorCmp(nodes.back()->id, myid) < 0 (the last of them is closer to id than we are), else 0. A few requests
     * take the host path (findClosestNodesHost and a host xor compare), batches kad_rt_responsible_batch_host:
     * one byte per id comes back instead of a row. */
    template <class InfoHashT, class TimePoint>
    std::vector<uint8_t> isTooFarBatch(const InfoHashT* ids, size_t q, const InfoHashT& myid, TimePoint now,
                                       size_t count = KAD_TARGET_NODES, size_t min_nodes = 1) const {
        std::vector<uint8_t> out(q, 0);
        const size_t need = std::max<size_t>(min_nodes, 1);
        auto far_of = [&](const InfoHashT& id, const std::vector<NodePtr>& r) -> uint8_t {
            if (r.size() < need) return 0;
            const uint8_t* t = id_bytes(id);
            const uint8_t* a = id_bytes(r.back()->id);
            const uint8_t* me = id_bytes(myid);
            for (unsigned k = 0; k < KAD_HASH_LEN; k++) {  // InfoHash::xorCmp (infohash.h:131-146)
                const uint8_t da = a[k] ^ t[k], dm = me[k] ^ t[k];
                if (da != dm) return da < dm ? (uint8_t)KAD_RESP_FAR : (uint8_t)0;
            }
            return 0;
        };
        if (q <= hostBatchLimit() && count <= host_count_) {
            for (size_t i = 0; i < q; i++) out[i] = far_of(ids[i], findClosestNodesHost(ids[i], now, count));
            return out;
        }
        if (std::min(count, nodes_.size()) > KAD_MAX_COUNT) {  // any size_t count: rows, then the compare here
            const std::vector<std::vector<NodePtr>> r = findClosestNodesBatch(ids, q, now, count);
            for (size_t i = 0; i < q; i++) out[i] = far_of(ids[i], r[i]);
            return out;
        }
        advance(to_ns(now));
        count = std::min(count, nodes_.size());
        if (count == 0 || q == 0) return out;
        if (count < need) return out;  // fewer nodes than min_nodes can ever come back
        std::vector<uint8_t> targets(q * KAD_HASH_LEN);
        for (size_t i = 0; i < q; i++) std::memcpy(&targets[i * KAD_HASH_LEN], id_bytes(ids[i]), KAD_HASH_LEN);
        table_.responsibleBatch(id_bytes(myid), targets.data(), q, count, min_nodes, out);
        return out;
    }
    template <class InfoHashT, class TimePoint>
    std::vector<uint8_t> isTooFarBatch(const std::vector<InfoHashT>& ids, const InfoHashT& myid, TimePoint now,
                                       size_t count = KAD_TARGET_NODES, size_t min_nodes = 1) const {
        return isTooFarBatch(ids.data(), ids.size(), myid, now, count, min_nodes);
    }

    /* What Dht::onNewNode(node, 0) (dht.cpp:867-936) would do with each candidate ID, taken alone against the table
     * as mirrored and the statuses at `now`: KNOWN / REPLACE / INSERT / SPLIT / FULL (or NONE without a bucket), the
     * node the kind names (the known node, the expired node to replace, the dubious node to ping; node(v.node)
     * gives its pointer) and the bucket index. myid NULL: no bucket is "mine". The host-only parts stay with the
     * caller: trySearchInsert for every kind but KNOWN, mybucket_grow_time when KAD_NN_MYBUCKET is set, b->cached
     * for FULL, and isPendingMessage() of the ping candidate (walk on from it in the bucket when it has one). One
     * kad_rt_triage_batch_host call, after the same refresh isTooFarBatch takes. */
    template <class InfoHashT, class TimePoint>
    std::vector<NewNodeVerdict> onNewNodeBatch(const InfoHashT* ids, size_t q, const InfoHashT* myid, TimePoint now,
                                               bool is_bootstrap) const {
        std::vector<NewNodeVerdict> out(q);
        if (q == 0) return out;
        advance(to_ns(now));
        std::vector<uint8_t> cand(q * KAD_HASH_LEN), verdict;
        std::vector<uint32_t> node, bucket;
        for (size_t i = 0; i < q; i++) std::memcpy(&cand[i * KAD_HASH_LEN], id_bytes(ids[i]), KAD_HASH_LEN);
        table_.triageBatch(myid ? id_bytes(*myid) : nullptr, cand.data(), q, is_bootstrap ? KAD_NN_BOOTSTRAP : 0u, verdict,
                           node, bucket);
        for (size_t i = 0; i < q; i++) out[i] = NewNodeVerdict{verdict[i], node[i], bucket[i]};
        return out;
    }
    /* Dht::getNodesStats (dht.cpp:2470-2495) over the mirrored table at `now`: one kad_table_sweep_host call with
     * KAD_SWEEP_INCOMING, after the same refresh isTooFarBatch takes. No walk of the lists. */
    template <class TimePoint>
    NodesStats nodesStats(TimePoint now) const {
        NodesStats st{0, 0, 0, 0};
        if (nodes_.empty()) return st;
        advance(to_ns(now));
        const kad_sweep_totals tot = table_.sweepTotals(KAD_SWEEP_INCOMING);
        st.good = tot.good;
        st.dubious = tot.dubious;
        st.incoming = tot.incoming;
        st.expired = tot.expired;
        return st;
    }

    /* Dht::expireBuckets (dht.cpp:942-956) on the mirror: every node whose isExpired() holds (as reported through
     * nodeUpdated / syncTimes) leaves the device table in one kad_table_expire call, which keeps the node times and
     * wire records of the others attached: no syncTimes() follows, unlike flush(). Returns the removed nodes and the
     * buckets that held them; the host erases the former from its own lists and calls sendCachedPing for the latter.
     * Pending un-flushed ops are flushed first. */
    template <class TimePoint>
    Expired<NodePtr> expireBuckets(TimePoint now) {
        Expired<NodePtr> out;
        flush(now);
        if (nodes_.empty()) return out;
        advance(to_ns(now));
        std::vector<uint32_t> remap(nodes_.size()), removed(nodes_.size()), buckets(buckets_ ? buckets_ : 1);
        uint32_t nr = 0, nb = 0;
        check(kad_table_expire(table_.get(), remap.data(), removed.data(), (uint32_t)removed.size(), &nr, buckets.data(),
                               buckets_, &nb),
              "kad_table_expire");
        if (nr == 0) return out;
        kad_table_info inf;
        check(kad_table_get_info(table_.get(), &inf), "kad_table_get_info");
        out.removed.reserve(nr);
        for (uint32_t j = 0; j < nr; j++) out.removed.push_back(nodes_[removed[j] - inf.index_base]);
        out.buckets.assign(buckets.begin(), buckets.begin() + nb);
        std::vector<NodePtr> next(inf.n_nodes);
        for (size_t i = 0; i < nodes_.size(); i++)
            if (remap[i] != KAD_NO_NODE) next[remap[i]] = nodes_[i];
        nodes_.swap(next);
        buckets_ = inf.n_buckets;
        first_.assign((size_t)KAD_HASH_LEN * buckets_, 0);
        off_.assign(buckets_ + 1, 0);
        check(kad_table_export(table_.get(), nullptr, nullptr, buckets_ ? first_.data() : nullptr, off_.data()),
              "kad_table_export");
        reindex();
        expire_calls_++;
        return out;
    }
    /* Dht::onReportedAddr's bucket write (dht.cpp:3177-3178) for the replies of one tick: findBucket(id)->time = now
     * for every ID in one kad_table_touch_buckets_host call (reportedAddr(addr) stays with the caller). The host's own
     * Bucket::time is not written: the device copy is the one bucketMaintenance reads. Pending ops are flushed first.
     * A table without buckets throws (the reference dereferences end()). */
    template <class InfoHashT, class TimePoint>
    void onReportedAddrBatch(const InfoHashT* ids, size_t q, TimePoint now) {
        flush(now);
        if (q == 0 && buckets_) return;
        std::vector<uint8_t> raw(q * KAD_HASH_LEN);
        for (size_t i = 0; i < q; i++) std::memcpy(&raw[i * KAD_HASH_LEN], id_bytes(ids[i]), KAD_HASH_LEN);
        check(kad_table_touch_buckets_host(table_.get(), raw.data(), (uint32_t)q, to_ns(now), nullptr),
              "kad_table_touch_buckets_host");
    }
    template <class InfoHashT, class TimePoint>
    void onReportedAddrBatch(const std::vector<InfoHashT>& ids, TimePoint now) {
        onReportedAddrBatch(ids.data(), ids.size(), now);
    }
    /* A single reply: findBucket over the host's copy of the bucket directory, then one patched word
     * (kad_table_patch_bucket_times), as the other single requests stay off the launch path. */
    template <class InfoHashT, class TimePoint>
    void onReportedAddr(const InfoHashT& id, TimePoint now) {
        flush(now);
        if (buckets_ == 0) throw Error(KAD_ERR_INVALID, "onReportedAddr: the table has no buckets");
        const uint32_t b = bucket_of(id_bytes(id));
        const int64_t t = to_ns(now);
        check(kad_table_patch_bucket_times(table_.get(), 1, &b, &t), "kad_table_patch_bucket_times");
    }
    /* Dht::connectivityChanged's `b.time = time_point::min()` for every bucket (dht.cpp:2391). */
    void resetBucketTimes() {
        if (table_) check(kad_table_set_bucket_times(table_.get(), nullptr), "kad_table_set_bucket_times");
    }
    /* The device's bucket times (kad_table_get_bucket_times), one per bucket. */
    std::vector<int64_t> bucketTimes() const {
        std::vector<int64_t> t(buckets_);
        if (buckets_) check(kad_table_get_bucket_times(table_.get(), t.data()), "kad_table_get_bucket_times");
        return t;
    }
    /* Dht::bucketMaintenance's loop (dht.cpp:2832-2850) without the walk over every bucket: the device lists the buckets
     * that pass :2833 (kad_table_maintenance_host, kMaintenanceCap records per call, resumed behind the last one), and
     * the reference's loop body runs over those only, drawing from `rd` what the reference draws, in its order and
     * with its distributions: randomId's bytes (routing_table.cpp:27-45), the two short-circuited rand_trial(1/8)
     * draws, randomNode's index (routing_table.cpp:15-25). Stops at the first bucket that yields a node. With the same
     * `rd` it returns what the reference's loop reaches and leaves `rd` in the same state (the reference draws
     * randomId and randomNode from routing_table.cpp's own generator and the trials from the Dht's; here all come
     * from the one `rd`). `rt` is the mirrored table: every reported mutation is flushed first, and the mirror's own
     * directory and node list stand in for it, so it is not walked. neighbourhoodMaintenance has no scan and stays on
     * the host. */
    static constexpr uint32_t kMaintenanceCap = 1024;
    template <class TimePoint, class Rng>
    MaintenancePick<NodePtr> bucketMaintenance(RoutingTableT& rt, TimePoint now, Rng& rd, uint32_t cap = kMaintenanceCap) {
        (void)rt;
        flush(now);
        MaintenancePick<NodePtr> out{};
        out.found = false;
        out.bucket = out.q = KAD_NO_NODE;
        if (buckets_ == 0 || cap == 0) return out;
        std::bernoulli_distribution rand_trial(1. / 8.);
        std::uniform_int_distribution<uint8_t> rand_byte;
        std::vector<kad_maint_rec> rec(cap);
        uint32_t fb = 0;
        for (;;) {
            kad_maint_totals tot;
            check(kad_table_maintenance_host(table_.get(), to_ns(now), fb, &tot, rec.data(), cap),
                  "kad_table_maintenance_host");
            maint_calls_++;
            const uint32_t m = tot.candidates < cap ? tot.candidates : cap;
            for (uint32_t k = 0; k < m; k++) {
                const uint32_t b = rec[k].bucket, kind = rec[k].kind;
                typename MaintenancePick<NodePtr>::InfoHashT id{};
                uint8_t* o = const_cast<uint8_t*>(id_bytes(id));
                const uint8_t* f = &first_[(size_t)KAD_HASH_LEN * b];
                const unsigned bit = (kind >> KAD_MAINT_BIT_SHIFT) & 0xFFu;
                if (bit >= 8 * KAD_HASH_LEN) {
                    std::memcpy(o, f, KAD_HASH_LEN);
                } else {
                    const unsigned bb = bit / 8;
                    std::memcpy(o, f, bb);
                    o[bb] = (uint8_t)(f[bb] & (0xFF00 >> (bit % 8)));
                    o[bb] = (uint8_t)(o[bb] | (rand_byte(rd) >> (bit % 8)));
                    for (unsigned i = bb + 1; i < KAD_HASH_LEN; i++) o[i] = rand_byte(rd);
                }
                bool q_empty = (kind & KAD_MAINT_EMPTY) != 0;
                uint32_t q = b;
                if ((kind & KAD_MAINT_HAS_NEXT) && (q_empty || rand_trial(rd))) {
                    q = b + 1;
                    q_empty = (kind & KAD_MAINT_NEXT_EMPTY) != 0;
                }
                if ((kind & KAD_MAINT_HAS_PREV) && (q_empty || rand_trial(rd)) && !(kind & KAD_MAINT_PREV_EMPTY)) {
                    q = b - 1;
                    q_empty = false;
                }
                if (q_empty) continue;  // q->randomNode() is null: the loop goes on
                std::uniform_int_distribution<unsigned> rand_node(0, off_[q + 1] - off_[q] - 1);
                const unsigned nn = rand_node(rd);
                out.found = true;
                out.bucket = b;
                out.q = q;
                out.id = id;
                out.node = nodes_[off_[q] + nn];
                return out;
            }
            if (tot.candidates <= cap) return out;
            fb = rec[m - 1].bucket + 1;
        }
    }
    /* Bookkeeping for tests: kad_table_maintenance_host calls made by bucketMaintenance. */
    size_t maintenanceCalls() const { return maint_calls_; }

    /* Bookkeeping for tests: full liveness uploads (syncTimes) and expireBuckets calls that removed nodes. */
    size_t syncTimesCalls() const { return sync_calls_; }
    size_t expireCalls() const { return expire_calls_; }

    /* The mirrored node of a NewNodeVerdict's index. */
    const NodePtr& node(uint32_t index) const { return nodes_[index]; }

    /* A mirrored node's time / reply_time / expired_ changed (Node::received, setExpired, reset,
     * Search::insertNode writing node->time): re-read at the next query. */
    void nodeUpdated(const NodePtr& n) { updated_.push_back(index_of(n)); }
    /* Re-read every mirrored node's liveness (kad_table_set_times); status re-derived at the next query. */
    void syncTimes() {
        std::vector<int64_t> t(nodes_.size()), r(nodes_.size());
        std::vector<uint8_t> e(nodes_.size());
        for (size_t i = 0; i < nodes_.size(); i++) {
            t[i] = to_ns(nodes_[i]->time);
            r[i] = to_ns(nodes_[i]->reply_time);
            e[i] = nodes_[i]->isExpired() ? 1 : 0;
        }
        if (!nodes_.empty()) table_.setTimes(t, r, e);
        sync_calls_++;
        updated_.clear();
        refresh_ = true;
    }

    /* Incremental mirror (kad_table_apply): record the mutations the Dht makes to the host table, in
     * the order it makes them, then flush(now). Nodes named by nodeRemoved / nodeReplaced must be in
     * the last snapshot or flush (flush in between otherwise). */
    void nodeRemoved(const NodePtr& n) {  // Dht::expireBuckets remove_if (dht.cpp:942-956)
        op(KAD_OP_REMOVE, index_of(n), 0);
    }
    void nodeReplaced(const NodePtr& old, const NodePtr& n) {  // onNewNode: `n = node` (dht.cpp:917-921)
        op(KAD_OP_REPLACE, index_of(old), slot(n));
    }
    void nodeAdded(const NodePtr& n) {  // onNewNode: b->nodes.emplace_front(node) (dht.cpp:934)
        op(KAD_OP_INSERT, slot(n), 0);
    }
    void bucketSplit(size_t bucket_index) {  // RoutingTable::split (routing_table.cpp:137-163)
        op(KAD_OP_SPLIT, (uint32_t)bucket_index, 0);
        buckets_++;
    }
    template <class TimePoint>
    void flush(TimePoint now) {
        if (ops_.empty()) return;
        std::vector<uint8_t> ids, status;
        for (const auto& n : added_) {
            ids.insert(ids.end(), id_bytes(n->id), id_bytes(n->id) + KAD_HASH_LEN);
            status.push_back(status_of(n, now));
        }
        std::vector<uint32_t> remap(nodes_.size()), idx(added_.size());
        check(kad_table_apply(table_.get(), ops_.data(), (uint32_t)(ops_.size() / 3), ids.data(), status.data(),
                              (uint32_t)added_.size(), remap.data(), idx.data()),
              "kad_table_apply");
        kad_table_info inf;
        check(kad_table_get_info(table_.get(), &inf), "kad_table_get_info");
        std::vector<NodePtr> next(inf.n_nodes);
        for (size_t i = 0; i < nodes_.size(); i++)
            if (remap[i] != KAD_NO_NODE) next[remap[i]] = nodes_[i];
        for (size_t s = 0; s < added_.size(); s++)
            if (idx[s] != KAD_NO_NODE) next[idx[s]] = added_[s];
        nodes_.swap(next);
        buckets_ = inf.n_buckets;
        first_.assign((size_t)KAD_HASH_LEN * buckets_, 0);
        off_.assign(buckets_ + 1, 0);
        check(kad_table_export(table_.get(), nullptr, nullptr, buckets_ ? first_.data() : nullptr, off_.data()),
              "kad_table_export");
        ops_.clear();
        added_.clear();
        reindex();
        syncTimes();  // kad_table_apply drops the node times (the layout moved)
        now_ns_ = to_ns(now);
        refresh_ = true;
    }

    /* RoutingTable::findClosestNodes(id, now, count) on the host, over the mirror's bucket directory and the
     * table's own Node objects (isGood(now) read from them, as routing_table.cpp:77 does): the closed form of
     * routing_table.cpp:67-111 -- findBucket by binary search over the bucket firsts, the window W(r) grown ring
     * by ring until it holds `count` good nodes or the whole table, its good nodes ordered by (XOR distance,
     * index) -- no pass over the table and no device round trip. For a few single requests it answers faster
     * than a launch or the resident service (the crossover, tools/crossover.cpp); batches go to the device. */
    template <class InfoHashT, class TimePoint>
    std::vector<NodePtr> findClosestNodesHost(const InfoHashT& id, TimePoint now, size_t count = KAD_TARGET_NODES) const {
        std::vector<NodePtr> out;
        const uint32_t B = (uint32_t)(off_.size() ? off_.size() - 1 : 0);
        if (B == 0 || count == 0) return out;
        const uint8_t* t = id_bytes(id);
        // findBucket (routing_table.cpp:113-127): the last bucket whose first is <= t, the first if none
        uint32_t lo = 0, hi = B;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) / 2;
            if (std::memcmp(&first_[(size_t)KAD_HASH_LEN * mid], t, KAD_HASH_LEN) <= 0) lo = mid + 1; else hi = mid;
        }
        const uint32_t b = lo ? lo - 1 : 0;
        // the window: W(0) = [b-1, b], each round one bucket more on either side (routing_table.cpp:89-104)
        struct Cand { uint32_t idx; const uint8_t* id; };
        std::vector<Cand> cand;
        size_t good = 0;
        auto take = [&](uint32_t x) {
            for (uint32_t j = off_[x]; j < off_[x + 1]; j++)
                if (nodes_[j]->isGood(now)) { cand.push_back(Cand{j, id_bytes(nodes_[j]->id)}); good++; }
        };
        uint32_t wl = b ? b - 1 : 0, wh = b;
        for (uint32_t x = wl; x <= wh; x++) take(x);
        while (good < count && !(wl == 0 && wh == B - 1)) {
            if (wh + 1 < B) take(++wh);
            if (wl > 0) take(--wl);
        }
        auto closer = [&](const Cand& a, const Cand& c) {  // InfoHash::xorCmp (infohash.h:131-146), then index
            for (unsigned k = 0; k < KAD_HASH_LEN; k++) {
                const uint8_t da = a.id[k] ^ t[k], dc = c.id[k] ^ t[k];
                if (da != dc) return da < dc;
            }
            return a.idx < c.idx;
        };
        const size_t m = std::min(count, cand.size());
        std::partial_sort(cand.begin(), cand.begin() + m, cand.end(), closer);
        out.reserve(m);
        for (size_t k = 0; k < m; k++) out.push_back(nodes_[cand[k].idx]);
        return out;
    }
    /* Batches of at most q requests with count <= max_count take the host path (0: never; kHostPathAuto, the
       default: q from the table size, below).
       The two paths read liveness differently: the host path evaluates isGood(now) on the table's own Node objects
       (as routing_table.cpp:77 does), the device path the liveness mirrored through nodeUpdated / syncTimes. They
       agree when every change is reported (the mirror's contract); a change that is not reported shows up only in
       the answers of device batches (more than hostBatchLimit() requests, or count above max_count). */
    static constexpr size_t kHostPathAuto = ~size_t(0);
    void setHostPath(size_t q, size_t max_count = 64) {
        host_q_ = q;
        host_count_ = max_count;
    }
    /* The largest batch the host path answers: set by setHostPath, else the crossover measured on MI355X
       (tools/crossover.cpp, profiles/r04/r04j/crossover.json: the host path beats both device paths up to 32
       requests on tables of up to 10k nodes, 16 at 100k, 8 at 1M). */
    size_t hostBatchLimit() const {
        if (host_q_ != kHostAuto) return host_q_;
        const size_t n = nodes_.size();
        return n <= 20000 ? 32 : n <= 200000 ? 16 : 8;
    }

    size_t bucketCount() const { return buckets_; }
    size_t nodeCount() const { return nodes_.size(); }
    const DeviceTable& table() const { return table_; }
    /* Single findClosestNodes calls answered by the resident query service (kad_table_serve); 0 turns it off. */
    void serve(uint32_t idle_us = 2000) const { table_.serve(idle_us); }

private:
    // status at the query's `now`: reported liveness changes first, then the device refresh
    void advance(int64_t now_ns) const {
        if (nodes_.empty()) {  // nothing to evaluate (and no times on the device)
            now_ns_ = now_ns;
            return;
        }
        if (!updated_.empty()) {
            std::vector<int64_t> t, r;
            std::vector<uint8_t> e;
            for (uint32_t i : updated_) {
                t.push_back(to_ns(nodes_[i]->time));
                r.push_back(to_ns(nodes_[i]->reply_time));
                e.push_back(nodes_[i]->isExpired() ? 1 : 0);
            }
            table_.patchTimes(updated_, t, r, e);
            updated_.clear();
            refresh_ = true;
        }
        if (refresh_ || now_ns != now_ns_) {
            table_.refreshStatus(now_ns);
            now_ns_ = now_ns;
            refresh_ = false;
        }
    }
    void reindex() {
        index_.clear();
        for (size_t i = 0; i < nodes_.size(); i++) index_[nodes_[i].get()] = (uint32_t)i;
    }
    // findBucket (routing_table.cpp:113-127) over the host directory: the last bucket whose first is <= t, the first
    // if none (buckets_ > 0)
    uint32_t bucket_of(const uint8_t* t) const {
        uint32_t lo = 0, hi = buckets_;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) / 2;
            if (std::memcmp(&first_[(size_t)KAD_HASH_LEN * mid], t, KAD_HASH_LEN) <= 0) lo = mid + 1; else hi = mid;
        }
        return lo ? lo - 1 : 0;
    }
    void op(uint32_t kind, uint32_t a, uint32_t b) {
        ops_.push_back(kind);
        ops_.push_back(a);
        ops_.push_back(b);
    }
    uint32_t index_of(const NodePtr& n) const {
        auto it = index_.find(n.get());
        if (it == index_.end()) throw Error(KAD_ERR_INVALID, "node not in the mirrored snapshot (flush first)");
        return it->second;
    }
    uint32_t slot(const NodePtr& n) {
        added_.push_back(n);
        return (uint32_t)(added_.size() - 1);
    }

    mutable DeviceTable table_;
    std::vector<NodePtr> nodes_;
    std::unordered_map<const void*, uint32_t> index_;
    uint32_t buckets_ = 0;
    std::vector<uint8_t> first_;  // the bucket directory on the host (the host path)
    std::vector<uint32_t> off_;
    static constexpr size_t kHostAuto = ~size_t(0);
    size_t host_q_ = kHostAuto, host_count_ = 64;  // small batches take the host path (hostBatchLimit)
    std::vector<uint32_t> ops_;
    std::vector<NodePtr> added_;
    mutable std::vector<uint32_t> updated_;
    mutable int64_t now_ns_ = INT64_MIN;
    mutable bool refresh_ = false;
    size_t sync_calls_ = 0, expire_calls_ = 0, maint_calls_ = 0;
};

/* Device mirror of one NodeCache family map (node_cache.h:42-50: std::map<InfoHash, weak_ptr<Node>>). */
template <class NodeMapT>
class NodeCacheFamilyMirror {
public:
    using WeakPtr = typename std::decay<decltype(std::declval<const NodeMapT&>().begin()->second)>::type;
    using NodePtr = decltype(std::declval<const WeakPtr&>().lock());

    NodeCacheFamilyMirror() {}
    explicit NodeCacheFamilyMirror(const NodeMapT& m, int device = 0) { snapshot(m, device); }

    /* Snapshot: map order (ascending ID); dead weak_ptrs and expired nodes are walked over but never
     * emitted (node_cache.cpp:60-62), so both get the "expired" status bit. */
    void snapshot(const NodeMapT& m, int device = 0) {
        std::vector<uint8_t> status;
        ids_.clear();
        nodes_.clear();
        for (const auto& kv : m) {
            NodePtr n = kv.second.lock();
            ids_.insert(ids_.end(), id_bytes(kv.first), id_bytes(kv.first) + KAD_HASH_LEN);
            status.push_back(status_of(n));
            nodes_.push_back(kv.second);
        }
        table_ = DeviceTable(device, ids_, status, std::vector<uint8_t>(), std::vector<uint32_t>(), 0, true);
        reindex();
    }

    /* Bring the device copy in line with the host map after NodeMap::getNode emplaced new IDs or erased
     * dead entries, or clearBadNodes erased them (node_cache.cpp:79-115): a sorted diff of the map against
     * the mirrored IDs, then one kad_nc_apply (a device merge, no re-snapshot). An entry whose weak_ptr now
     * names another Node (getNode recreated it) or whose expiry changed gets its status patched. */
    void sync(const NodeMapT& m) {
        std::vector<uint32_t> erase, changed;
        std::vector<uint8_t> ins, ist, chst;
        std::vector<WeakPtr> added;
        size_t i = 0;
        auto it = m.begin();
        const size_t n = nodes_.size();
        while (i < n || it != m.end()) {
            const int c = i == n ? 1 : it == m.end() ? -1 : std::memcmp(&ids_[i * KAD_HASH_LEN], id_bytes(it->first), KAD_HASH_LEN);
            if (c < 0) {
                erase.push_back((uint32_t)i++);
            } else if (c > 0) {
                ins.insert(ins.end(), id_bytes(it->first), id_bytes(it->first) + KAD_HASH_LEN);
                ist.push_back(status_of(it->second.lock()));
                added.push_back(it->second);
                ++it;
            } else {
                const bool same = !nodes_[i].owner_before(it->second) && !it->second.owner_before(nodes_[i]);
                if (!same) {
                    nodes_[i] = it->second;
                    changed.push_back((uint32_t)i);
                    chst.push_back(status_of(it->second.lock()));
                }
                ++i;
                ++it;
            }
        }
        if (!changed.empty()) table_.patchStatus(changed, chst);
        if (erase.empty() && added.empty()) {
            if (!changed.empty()) reindex();
            return;
        }
        std::vector<uint32_t> remap(n ? n : 1), idx(added.empty() ? 1 : added.size());
        check(kad_nc_apply(table_.get(), erase.data(), (uint32_t)erase.size(), ins.data(), ist.data(),
                           (uint32_t)added.size(), remap.data(), idx.data()), "kad_nc_apply");
        const size_t n1 = n - erase.size() + added.size();
        std::vector<WeakPtr> next(n1);
        std::vector<uint8_t> ids1(n1 * KAD_HASH_LEN);
        for (size_t k = 0; k < n; k++)
            if (remap[k] != KAD_NO_NODE) {
                next[remap[k]] = nodes_[k];
                std::memcpy(&ids1[remap[k] * KAD_HASH_LEN], &ids_[k * KAD_HASH_LEN], KAD_HASH_LEN);
            }
        for (size_t k = 0; k < added.size(); k++) {
            next[idx[k]] = added[k];
            std::memcpy(&ids1[idx[k] * KAD_HASH_LEN], &ins[k * KAD_HASH_LEN], KAD_HASH_LEN);
        }
        nodes_.swap(next);
        ids_.swap(ids1);
        reindex();
    }

    /* NodeCache::getCachedNodes(id, af, count) for this family (node_cache.cpp:36-66). */
    template <class InfoHashT>
    std::vector<NodePtr> getCachedNodes(const InfoHashT& id, size_t count) const {
        std::vector<std::vector<NodePtr>> r = getCachedNodesBatch(&id, 1, count);
        return std::move(r[0]);
    }
    /* Batched form. A returned node found dead or expired on the host (the reference skips it without
     * counting it) is marked expired on the device and its queries re-run, so results stay exact without
     * a notification for deaths and expiries; an expired node that comes back (Node::received with a
     * reply, reset(), clearBadNodes) must be reported with nodeUpdated. */
    template <class InfoHashT>
    std::vector<std::vector<NodePtr>> getCachedNodesBatch(const InfoHashT* ids, size_t q, size_t count) const {
        std::vector<std::vector<NodePtr>> out(q);
        // any size_t count, as node_cache.h:32: a result never holds more than the map's nodes
        count = std::min(count, nodes_.size());
        if (count == 0 || q == 0) return out;
        std::vector<size_t> todo(q);
        for (size_t i = 0; i < q; i++) todo[i] = i;
        while (!todo.empty()) {
            std::vector<uint8_t> targets(todo.size() * KAD_HASH_LEN);
            for (size_t k = 0; k < todo.size(); k++)
                std::memcpy(&targets[k * KAD_HASH_LEN], id_bytes(ids[todo[k]]), KAD_HASH_LEN);
            std::vector<uint32_t> idx, stale;
            std::vector<uint8_t> cnt;
            table_.getCachedNodesBatch(targets.data(), todo.size(), count, idx, cnt);
            std::vector<size_t> again;
            for (size_t k = 0; k < todo.size(); k++) {
                std::vector<NodePtr>& o = out[todo[k]];
                o.clear();
                bool ok = true;
                size_t m = cnt[k];
                if (count > 255)  // the count byte saturates: the row's padding gives the length
                    for (m = 0; m < count && idx[k * count + m] != KAD_NO_NODE; m++) {}
                for (size_t j = 0; j < m; j++) {
                    const uint32_t x = idx[k * count + j];
                    NodePtr n = nodes_[x].lock();
                    if (!n || n->isExpired()) { stale.push_back(x); ok = false; continue; }
                    o.push_back(std::move(n));
                }
                if (!ok) again.push_back(todo[k]);
            }
            if (!stale.empty()) {
                std::sort(stale.begin(), stale.end());
                stale.erase(std::unique(stale.begin(), stale.end()), stale.end());
                table_.patchStatus(stale, std::vector<uint8_t>(stale.size(), (uint8_t)KAD_STATUS_EXPIRED));
            }
            todo.swap(again);
        }
        return out;
    }
    template <class InfoHashT>
    std::vector<std::vector<NodePtr>> getCachedNodesBatch(const std::vector<InfoHashT>& ids, size_t count) const {
        return getCachedNodesBatch(ids.data(), ids.size(), count);
    }
    /* A cached node's isExpired() changed (setExpired, Node::received with a reply, reset()). */
    void nodeUpdated(const NodePtr& n) {
        auto it = index_.find(n.get());
        if (it == index_.end()) return;  // not in this family's map
        table_.patchStatus(std::vector<uint32_t>{it->second},
                           std::vector<uint8_t>{(uint8_t)(n->isExpired() ? KAD_STATUS_EXPIRED : 0u)});
    }
    size_t size() const { return nodes_.size(); }
    /* The device table and the node behind one of its indices (SearchesMirror::refillBatch). */
    const DeviceTable& table() const { return table_; }
    NodePtr nodeAt(uint32_t idx) const { return idx < nodes_.size() ? nodes_[idx].lock() : NodePtr(); }
    /* A node of a device result was found dead or expired on the host: mark it on the device, as
     * getCachedNodesBatch does. */
    void markStale(const std::vector<uint32_t>& idx) const {
        if (!idx.empty()) table_.patchStatus(idx, std::vector<uint8_t>(idx.size(), (uint8_t)KAD_STATUS_EXPIRED));
    }

private:
    static uint8_t status_of(const NodePtr& n) {
        return (uint8_t)((!n || n->isExpired()) ? KAD_STATUS_EXPIRED : 0u);
    }
    void reindex() {
        index_.clear();
        for (size_t i = 0; i < nodes_.size(); i++)
            if (NodePtr n = nodes_[i].lock()) index_[n.get()] = (uint32_t)i;
    }

    mutable DeviceTable table_;
    std::vector<uint8_t> ids_;  // the mirrored map's keys, in map order
    std::vector<WeakPtr> nodes_;
    std::unordered_map<const void*, uint32_t> index_;
};

/* Device mirror of a whole NodeCache (cache_4 and cache_6, node_cache.h:49-50). */
template <class NodeMapT>
class NodeCacheMirror {
public:
    using NodePtr = typename NodeCacheFamilyMirror<NodeMapT>::NodePtr;

    void snapshot(const NodeMapT& cache4, const NodeMapT& cache6, int device = 0) {
        v4_.snapshot(cache4, device);
        v6_.snapshot(cache6, device);
    }
    /* NodeCache::getCachedNodes(const InfoHash&, sa_family_t, size_t) (node_cache.h:32, node_cache.cpp:36-66). */
    template <class InfoHashT>
    std::vector<NodePtr> getCachedNodes(const InfoHashT& id, sa_family_t sa_f, size_t count) const {
        return family(sa_f).getCachedNodes(id, count);
    }
    void nodeUpdated(const NodePtr& n) {
        v4_.nodeUpdated(n);
        v6_.nodeUpdated(n);
    }
    /* After NodeCache::getNode / clearBadNodes changed the maps (inserted or erased entries). */
    void sync(const NodeMapT& cache4, const NodeMapT& cache6) {
        v4_.sync(cache4);
        v6_.sync(cache6);
    }
    const NodeCacheFamilyMirror<NodeMapT>& family(sa_family_t sa_f) const { return sa_f == AF_INET ? v4_ : v6_; }
    NodeCacheFamilyMirror<NodeMapT>& family(sa_family_t sa_f) { return sa_f == AF_INET ? v4_ : v6_; }

private:
    NodeCacheFamilyMirror<NodeMapT> v4_, v6_;
};

/* One candidate's trySearchInsert verdict (kad_sr_try_insert_batch): the searches [lb - back, lb + fwd) in map
 * order would take it; stop = fstop | bstop << 4 (KAD_SR_STOP_*), why each walk ended. */
struct SearchInsertVerdict {
    uint32_t lb, fwd, back;
    uint8_t stop;
};

/* One search's Dht::refill on the device (SearchesMirror::refillBatch): the getCachedNodes result in walk order, bit j
 * of inserted = insertNode(nodes[j], now) returned true on the device copy, and overflow = the device copy was not
 * refilled (its list outgrew the slab, or a node of the row was found dead or expired on the host): the host's own
 * insertNode loop over `nodes` stands, and the search is reported to sync(). The name follows KAD_SR_REFILL_OVERFLOW;
 * read it as "handed back to the host", whichever of the two reasons applies. */
template <class NodePtr>
struct RefillResult {
    std::vector<NodePtr> nodes;
    uint16_t inserted;
    bool overflow;  // handed back: the host's walk stands and sync() overwrites the device copy
};

/* One search's inserts on the device (SearchesMirror::insertBatch): inserted[j] = insertNode(nodes[j], now) returned
 * true on the device copy, and overflow = the device copy was not touched (its list outgrew the slab, or one of its
 * candidates is removable at `now`): the host's own insertNode loop stands, and the search is reported to sync(). As
 * for RefillResult, read overflow as "handed back to the host". */
struct InsertResult {
    std::vector<uint8_t> inserted;
    bool overflow;
};

/* One candidate of SearchesMirror::trySearchInsertTick (kad_sr_try_insert_tick): kind is KAD_SR_TICK_LEFT, _SKIPPED or
 * _APPLIED; for the last two, round is the round that decided it and lb / fwd / back / stop / trim that round's verdict:
 * the searches [lb - back, lb + fwd) in map order took the candidate, stop = fstop | bstop << 4 (KAD_SR_STOP_*) says why
 * each walk ended, and trim bit 0 / bit 1 says that the forward / backward stopper's refusal cut its list. lb_id is the
 * ID of search lb (the map's lower_bound of the node's ID), at_end is set when lb is past the last search. */
template <class InfoHashT>
struct TickVerdict {
    uint8_t kind;
    uint32_t round, lb, fwd, back;
    uint8_t stop, trim;
    bool at_end;
    InfoHashT lb_id;
};

/* A tick of SearchesMirror::trySearchInsertTick: one verdict per candidate, and the searches the device left untouched
 * because their slab is too small (their candidates stay APPLIED; the host's replay stands and the searches are reported
 * to sync(changed, now)). */
template <class InfoHashT>
struct TickResult {
    std::vector<TickVerdict<InfoHashT>> verdicts;
    std::vector<InfoHashT> overflowed;
};

/* One search whose flag bytes SearchesMirror::markNodes changed, with the counts of its list after the change: n,
 * Search::getNumberOfBadNodes(), getNumberOfConsecutiveBadNodes() (dht.cpp:583-597), and whether it is full (at least
 * SEARCH_NODES entries that are not bad) and expired. Dht::searchStep's expiry test is lead_bad >= min(n,
 * SEARCH_MAX_BAD_NODES) (:1451), its refill test n - bad < SEARCH_NODES (:1354). */
template <class InfoHashT>
struct MarkedSearch {
    InfoHashT id;
    uint8_t n, bad, lead_bad;
    bool full, expired;
};

/* One search stepped by SearchesMirror::stepBatch (kad_sr_step): the nodes that get a get request, in list order, the
 * counts of its list (solicited as it is after the picks) and the KAD_STEP_* result bits. */
template <class InfoHashT, class NodePtrT>
struct SteppedSearch {
    InfoHashT id;
    std::vector<NodePtrT> picks;
    uint8_t n, bad, lead_bad, solicited;
    uint32_t bits;
};

/* One search stepped by SearchesMirror::stepBatchFull (kad_sr_step_full): SteppedSearch with the nodes that get the
 * listen requests due on them and the nodes that get the announce probe, each in list order. */
template <class InfoHashT, class NodePtrT>
struct FullySteppedSearch {
    InfoHashT id;
    std::vector<NodePtrT> picks, listen, announce;
    uint8_t n, bad, lead_bad, solicited;
    uint32_t bits;
};

/* Device mirror of one family's live searches (Dht::searches(af), dht.h) over a map shaped like
 * std::map<InfoHash, std::shared_ptr<Search>>. Reads of a search: id, expired, nodes[i].node->id, nodes[i].isBad().
 * The map must outlive the mirror or the next snapshot. */
template <class SearchMapT>
class SearchesMirror {
public:
    SearchesMirror() {}
    ~SearchesMirror() { reset(); }
    SearchesMirror(const SearchesMirror&) = delete;
    SearchesMirror& operator=(const SearchesMirror&) = delete;
    SearchesMirror(SearchesMirror&& o) noexcept { swap(o); }
    SearchesMirror& operator=(SearchesMirror&& o) noexcept {
        if (this != &o) {
            reset();
            swap(o);
        }
        return *this;
    }

    /* Snapshot every search of `map`. cap: slab entries per search, grown to the longest list. */
    void snapshot(const SearchMapT& map, int device = 0, uint32_t cap = 32) { snapshotAt(map, NoTime(), device, cap); }
    /* The same with KAD_SN_REMOVABLE set on the entries removeExpiredNode(now) would erase (node->isExpired() &&
     * node->time + Node::NODE_EXPIRE_TIME < now, dht.h:628-640): what refillBatch at `now` needs. Chosen only for a
     * std::chrono time point: snapshot(map, 0, 14) with plain integers stays the overload above. */
    template <class TimePoint, class = typename TimePoint::duration>
    void snapshot(const SearchMapT& map, TimePoint now, int device = 0, uint32_t cap = 32) {
        snapshotAt(map, At<TimePoint>{now}, device, cap);
    }

private:
    template <class When>
    void snapshotAt(const SearchMapT& map, const When& when, int device, uint32_t cap) {
        std::vector<uint8_t> ids, flags, nid, nfl;
        std::vector<uint32_t> off(1, 0u);
        for (const auto& kv : map) {
            ids.insert(ids.end(), id_bytes(kv.first), id_bytes(kv.first) + KAD_HASH_LEN);
            append(*kv.second, flags, off, nid, nfl, when);
            cap = std::max<uint32_t>(cap, off.back() - off[off.size() - 2]);
        }
        kad_searches* ss = nullptr;
        check(kad_searches_create(&ss, device, (uint32_t)flags.size(), cap, ids.data(), flags.data(), off.data(),
                                  nid.data(), nfl.data()), "kad_searches_create");
        reset();
        ss_ = ss;
        map_ = &map;
        ids_.swap(ids);
        device_ = device;
        cap_ = cap;
        at_.assign(size(), when.ns());
    }

public:
    /* The searches with these IDs changed their list or flags (the host's inserts, a node turning bad, expiry):
     * one kad_searches_patch. A search added to or erased from the map is reported to update() (KAD_ERR_INVALID
     * here for an ID that is not mirrored); a list that outgrew the slabs takes a new snapshot by itself. */
    template <class InfoHashT>
    void sync(const std::vector<InfoHashT>& changed) { syncAt(changed, NoTime()); }
    /* The same with KAD_SN_REMOVABLE evaluated at `now` (see snapshot). */
    template <class InfoHashT, class TimePoint, class = typename TimePoint::duration>
    void sync(const std::vector<InfoHashT>& changed, TimePoint now) { syncAt(changed, At<TimePoint>{now}); }

    /* The host's map lost the searches `erased` (Dht::expireSearches dht.cpp:1060-1074, or a done search re-used under
     * a new ID :1695-1711) and gained `added` (Dht::search :1691-1693), both already applied to the map: one
     * kad_searches_apply, which moves the kept searches on the device and uploads nothing but the new IDs. The new
     * searches enter empty; those of `added` whose host list already holds nodes then take one sync. An ID in `erased`
     * that is not mirrored, an ID in `added` that is mirrored and not in `erased`, or one that is not in the map:
     * KAD_ERR_INVALID, and the mirror is unchanged. Dht::search goes on with refillBatch on the new IDs (:1728). */
    template <class InfoHashT>
    void update(const std::vector<InfoHashT>& erased, const std::vector<InfoHashT>& added) {
        updateAt(erased, added, NoTime());
    }
    /* The same with KAD_SN_REMOVABLE evaluated at `now` for the lists that are synced (see snapshot). */
    template <class InfoHashT, class TimePoint, class = typename TimePoint::duration>
    void update(const std::vector<InfoHashT>& erased, const std::vector<InfoHashT>& added, TimePoint now) {
        updateAt(erased, added, At<TimePoint>{now});
    }

    /* Dht::refill (dht.cpp:1647-1668) of the searches `ids` (distinct, mirrored) from the NodeCache family mirror
     * `nc` on the device: one kad_sr_refill. Searches whose KAD_SN_REMOVABLE bits at `now` differ from the mirrored
     * ones are patched first. Results in the order of `ids`. The host then runs sr.insertNode(n, now) over every
     * result's nodes on its own searches (the device copy already holds the outcome; a refused insert can still trim)
     * and reports the searches with overflow set to sync(changed, now). nc must be on the mirror's device.
     * Precondition: which bits "differ" is worked out from each member node's current isExpired() and time against
     * the time the search was last uploaded at, so every change of those two fields of a node held by a mirrored
     * search (setExpired, a reply, another search's insertNode writing node->time) must have been reported through
     * markNodes(nodes, pairs, now) before (or, for a search whose list changed as well, through sync(changed, now)); a
     * search whose members changed unreported may keep stale bits on the device. markNodes leaves the upload times
     * alone: for fixed node fields removability only ever turns on as time passes, so the bit markNodes wrote at T1 lies
     * between what an upload at the recorded time <= T1 would hold and what `now` >= T1 asks for; whenever those two
     * agree the device bit agrees with them, and when they do not the search is patched, as before. */
    template <class NodeMapT, class InfoHashT, class TimePoint>
    std::vector<RefillResult<typename NodeCacheFamilyMirror<NodeMapT>::NodePtr>>
    refillBatch(const NodeCacheFamilyMirror<NodeMapT>& nc, const std::vector<InfoHashT>& ids, TimePoint now) {
        typedef typename NodeCacheFamilyMirror<NodeMapT>::NodePtr NodePtr;
        std::vector<RefillResult<NodePtr>> out(ids.size());
        if (ids.empty()) return out;
        if (!ss_) throw Error(KAD_ERR_INVALID, "SearchesMirror::refillBatch before snapshot");
        const uint32_t m = (uint32_t)ids.size();
        std::vector<std::pair<uint32_t, uint32_t>> order(m);  // (search index, position in ids)
        for (uint32_t i = 0; i < m; i++) order[i] = std::make_pair(index_of(id_bytes(ids[i])), i);
        std::sort(order.begin(), order.end());
        std::vector<uint32_t> which(m);
        for (uint32_t k = 0; k < m; k++) {
            if (k && order[k].first == order[k - 1].first)
                throw Error(KAD_ERR_INVALID, "SearchesMirror::refillBatch: a search listed twice");
            which[k] = order[k].first;
        }
        // the searches whose REMOVABLE bits moved since they were uploaded
        const At<TimePoint> when{now};
        std::vector<InfoHashT> moved;
        {
            auto it = map_->begin();
            uint32_t at = 0;
            for (uint32_t k = 0; k < m; k++) {
                std::advance(it, which[k] - at);
                at = which[k];
                if (it == map_->end() || std::memcmp(id_bytes(it->first), &ids_[(size_t)at * KAD_HASH_LEN], KAD_HASH_LEN) != 0)
                    throw Error(KAD_ERR_INVALID, "the search map changed its keys (snapshot again)");
                bool differ = false;
                for (const auto& sn : it->second->nodes)
                    differ = differ || when.removable(*sn.node) != (at_[at] != INT64_MIN && when.removableAt(*sn.node, at_[at]));
                if (differ) moved.push_back(ids[order[k].second]);
            }
        }
        if (!moved.empty()) syncAt(moved, when);
        std::vector<uint32_t> rows((size_t)m * KAD_SEARCH_NODES);
        std::vector<uint8_t> cnt(m), st(m);
        std::vector<uint16_t> ins(m);
        check(kad_sr_refill(ss_, nc.table().get(), m, which.data(), rows.data(), cnt.data(), ins.data(), st.data()),
              "kad_sr_refill");
        std::vector<uint32_t> stale;
        for (uint32_t k = 0; k < m; k++) {
            RefillResult<NodePtr>& r = out[order[k].second];
            r.inserted = ins[k];
            r.overflow = st[k] != KAD_SR_REFILL_OK;
            bool ok = true;
            for (uint32_t j = 0; j < cnt[k]; j++) {
                const uint32_t x = rows[(size_t)k * KAD_SEARCH_NODES + j];
                NodePtr n = nc.nodeAt(x);
                if (!n || n->isExpired()) { stale.push_back(x); ok = false; continue; }
                r.nodes.push_back(std::move(n));
            }
            if (!ok) r.overflow = true;  // the device walked over a node the host no longer takes
            at_[which[k]] = when.ns();
        }
        if (!stale.empty()) {  // those rows again, exactly, on the host path; their searches go through sync()
            std::sort(stale.begin(), stale.end());
            stale.erase(std::unique(stale.begin(), stale.end()), stale.end());
            nc.markStale(stale);
            for (uint32_t k = 0; k < m; k++) {
                RefillResult<NodePtr>& r = out[order[k].second];
                if (r.nodes.size() != cnt[k]) {
                    r.nodes = nc.getCachedNodes(ids[order[k].second], KAD_SEARCH_NODES);
                    r.inserted = 0;
                }
            }
        }
        for (auto& r : out)
            if (r.overflow) r.inserted = 0;
        return out;
    }

    /* sr.insertNode(n, now) with an empty token for every node n of nodes[i], in order, on the search ids[i] (distinct,
     * mirrored), on the device: one kad_sr_insert, KAD_SN_BAD = n->isExpired(). As refillBatch, the listed searches
     * whose KAD_SN_REMOVABLE bits at `now` differ from the mirrored ones are patched first (same precondition), and the
     * host then runs the same insertNode calls on its own searches and reports the searches with overflow set to
     * sync(changed, now). A search with a candidate that is removable at `now` is not sent and comes back with overflow
     * set: insertNode's node.time = now clears that node's REMOVABLE bit in every search that holds it, so the host's
     * walk stands and those searches go through sync() too. Results in the order of `ids`. */
    template <class InfoHashT, class NodePtrT, class TimePoint>
    std::vector<InsertResult> insertBatch(const std::vector<InfoHashT>& ids,
                                          const std::vector<std::vector<NodePtrT>>& nodes, TimePoint now) {
        if (ids.size() != nodes.size()) throw Error(KAD_ERR_INVALID, "SearchesMirror::insertBatch: one node list per search");
        std::vector<InsertResult> out(ids.size());
        if (ids.empty()) return out;
        if (!ss_) throw Error(KAD_ERR_INVALID, "SearchesMirror::insertBatch before snapshot");
        const uint32_t m = (uint32_t)ids.size();
        std::vector<std::pair<uint32_t, uint32_t>> order(m);  // (search index, position in ids)
        for (uint32_t i = 0; i < m; i++) order[i] = std::make_pair(index_of(id_bytes(ids[i])), i);
        std::sort(order.begin(), order.end());
        for (uint32_t k = 1; k < m; k++)
            if (order[k].first == order[k - 1].first)
                throw Error(KAD_ERR_INVALID, "SearchesMirror::insertBatch: a search listed twice");
        const At<TimePoint> when{now};
        std::vector<uint32_t> which, off(1, 0u), pos;  // the searches that are sent, and their positions in ids
        std::vector<uint8_t> cid, cfl;
        std::vector<InfoHashT> moved;
        {
            auto it = map_->begin();
            uint32_t at = 0;
            for (uint32_t k = 0; k < m; k++) {
                const uint32_t i = order[k].second;
                out[i].inserted.assign(nodes[i].size(), 0);
                out[i].overflow = false;
                for (const auto& n : nodes[i]) out[i].overflow = out[i].overflow || when.removable(*n);
                if (out[i].overflow) continue;
                std::advance(it, order[k].first - at);
                at = order[k].first;
                if (it == map_->end() || std::memcmp(id_bytes(it->first), &ids_[(size_t)at * KAD_HASH_LEN], KAD_HASH_LEN) != 0)
                    throw Error(KAD_ERR_INVALID, "the search map changed its keys (snapshot again)");
                bool differ = false;  // the REMOVABLE bits moved since the search was uploaded
                for (const auto& sn : it->second->nodes)
                    differ = differ || when.removable(*sn.node) != (at_[at] != INT64_MIN && when.removableAt(*sn.node, at_[at]));
                if (differ) moved.push_back(ids[i]);
                which.push_back(at);
                pos.push_back(i);
                for (const auto& n : nodes[i]) {
                    cid.insert(cid.end(), id_bytes(n->id), id_bytes(n->id) + KAD_HASH_LEN);
                    cfl.push_back(n->isExpired() ? (uint8_t)KAD_SN_BAD : (uint8_t)0);
                }
                off.push_back((uint32_t)cfl.size());
            }
        }
        if (which.empty()) return out;
        if (!moved.empty()) syncAt(moved, when);
        std::vector<uint8_t> ins(cfl.size()), st(which.size());
        check(kad_sr_insert(ss_, (uint32_t)which.size(), which.data(), off.data(), cid.data(), cfl.data(), ins.data(),
                            st.data()), "kad_sr_insert");
        for (size_t k = 0; k < which.size(); k++) {
            InsertResult& r = out[pos[k]];
            r.overflow = st[k] != KAD_SR_INSERT_OK;
            if (!r.overflow) r.inserted.assign(ins.begin() + off[k], ins.begin() + off[k + 1]);
            at_[which[k]] = when.ns();
        }
        return out;
    }

    /* Dht::trySearchInsert(n) for every node n of `nodes`, in arrival order, applied to the device set in one call
     * (kad_sr_try_insert_tick, up to max_rounds rounds, 0: no limit), KAD_SN_BAD = n->isExpired(). The candidates go up
     * to the first one whose node is removable at `now`: insertNode's node.time = now clears that node's REMOVABLE bit in
     * every search that holds it, so that candidate is the caller's to walk on the host, and it and all after it come
     * back as KAD_SR_TICK_LEFT. As insertBatch, the searches whose KAD_SN_REMOVABLE bits at `now` differ from the
     * mirrored ones are patched first (same precondition); here that is asked of every mirrored search, since a tick may
     * reach any of them. The host then replays the APPLIED candidates on its own searches in (round, position) order:
     * insertNode from search lb forwards and from lb - 1 backwards until the first refusal, which the verdict names (a
     * refusing search whose trim bit is set is cut by that call). Then it walks the LEFT candidates in order, as
     * Dht::trySearchInsert does, and reports the searches those walks changed, every search holding a removable
     * candidate that was accepted, and `overflowed` to sync(changed, now). */
    template <class NodePtrT, class TimePoint, class MapT = SearchMapT, class InfoHashT = typename MapT::key_type>
    TickResult<InfoHashT> trySearchInsertTick(const std::vector<NodePtrT>& nodes, TimePoint now, uint32_t max_rounds = 0) {
        TickResult<InfoHashT> out;
        if (nodes.empty()) return out;
        if (!ss_) throw Error(KAD_ERR_INVALID, "SearchesMirror::trySearchInsertTick before snapshot");
        const At<TimePoint> when{now};
        TickVerdict<InfoHashT> left = TickVerdict<InfoHashT>();
        left.kind = (uint8_t)KAD_SR_TICK_LEFT;
        out.verdicts.assign(nodes.size(), left);
        size_t cut = 0;
        while (cut < nodes.size() && !when.removable(*nodes[cut])) cut++;
        // every search's key, and the searches whose REMOVABLE bits moved since they were uploaded
        std::vector<const InfoHashT*> keys;
        std::vector<InfoHashT> moved;
        keys.reserve(size());
        for (const auto& kv : *map_) {
            const size_t at = keys.size();
            if (at >= size() || std::memcmp(id_bytes(kv.first), &ids_[at * KAD_HASH_LEN], KAD_HASH_LEN) != 0)
                throw Error(KAD_ERR_INVALID, "the search map changed its keys (snapshot again)");
            bool differ = false;
            for (const auto& sn : kv.second->nodes)
                differ = differ || when.removable(*sn.node) != (at_[at] != INT64_MIN && when.removableAt(*sn.node, at_[at]));
            if (differ) moved.push_back(kv.first);
            keys.push_back(&kv.first);
        }
        if (keys.size() != size()) throw Error(KAD_ERR_INVALID, "the search map changed its keys (snapshot again)");
        if (cut == 0) return out;
        if (!moved.empty()) syncAt(moved, when);
        const uint32_t q = (uint32_t)cut;
        std::vector<uint8_t> cid((size_t)q * KAD_HASH_LEN), cfl(q), kind(q), stop(q), trim(q);
        std::vector<uint32_t> round(q), lb(q), fwd(q), back(q), over(size() + 1);
        for (uint32_t j = 0; j < q; j++) {
            std::memcpy(&cid[(size_t)j * KAD_HASH_LEN], id_bytes(nodes[j]->id), KAD_HASH_LEN);
            cfl[j] = nodes[j]->isExpired() ? (uint8_t)KAD_SN_BAD : (uint8_t)0;
        }
        uint32_t n_over = 0;
        const int rc = kad_sr_try_insert_tick(ss_, cid.data(), cfl.data(), q, max_rounds, kind.data(), round.data(),
                                              lb.data(), fwd.data(), back.data(), stop.data(), trim.data(), over.data(),
                                              &n_over, nullptr);
        // every mirrored search now carries the bits of `now`: the moved ones were patched, the others do not differ
        // (whatever rounds an error left applied, the bits stay those of `now`)
        for (auto& t : at_) t = when.ns();
        check(rc, "kad_sr_try_insert_tick");
        for (uint32_t j = 0; j < q; j++) {
            TickVerdict<InfoHashT>& v = out.verdicts[j];
            v.kind = kind[j];
            if (kind[j] == KAD_SR_TICK_LEFT) continue;
            v.round = round[j];
            v.lb = lb[j];
            v.fwd = fwd[j];
            v.back = back[j];
            v.stop = stop[j];
            v.trim = trim[j];
            v.at_end = lb[j] >= keys.size();
            if (!v.at_end) v.lb_id = *keys[lb[j]];
        }
        for (uint32_t k = 0; k < n_over; k++) out.overflowed.push_back(*keys[over[k]]);
        return out;
    }

    /* Node status changes of one tick carried to every mirrored search that holds the node, without the host looking
     * for the holders and without an upload of their lists: one kad_sr_mark_nodes. nodes: the Nodes whose isExpired()
     * or time changed since they were last reported (setExpired after a timed-out request, a reply, an expired node
     * whose ten minutes ran out), in any order, repeats allowed: an expired node gets KAD_SN_BAD and, at `now`,
     * KAD_SN_REMOVABLE or not; a live one loses both. pairs: (search ID, node) for every list entry whose `candidate`
     * changed (dht.cpp:1038, 1109), and for every entry with `candidate` set whose node is in `nodes` (its BAD bit is
     * not the node's): the entry gets exactly the byte the host's list says, isBad() and removability at `now`. A pair
     * whose search does not hold the node changes nothing. The lists themselves must be the mirrored ones (insertNode,
     * trims and erases go through insertBatch, refillBatch or sync). Returns the searches with a byte that changed, in
     * map order, with their counts; the search-level expire() stays with sync / update. A mirror of no searches takes
     * any `nodes` and returns nothing; a pair always names a mirrored search (KAD_ERR_INVALID otherwise). */
    template <class NodePtrT, class InfoHashT, class TimePoint>
    std::vector<MarkedSearch<InfoHashT>> markNodes(const std::vector<NodePtrT>& nodes,
                                                   const std::vector<std::pair<InfoHashT, NodePtrT>>& pairs,
                                                   TimePoint now) {
        std::vector<MarkedSearch<InfoHashT>> out;
        if (nodes.empty() && pairs.empty()) return out;
        if (!ss_) throw Error(KAD_ERR_INVALID, "SearchesMirror::markNodes before snapshot");
        if (size() == 0 && pairs.empty()) return out;  // a family without live searches: no list holds the nodes
        const At<TimePoint> when{now};
        const uint8_t both = KAD_SN_BAD | KAD_SN_REMOVABLE;
        // one op per node ID: (ID, set bits), sorted, repeats dropped
        std::vector<std::array<uint8_t, KAD_HASH_LEN + 1>> ops(nodes.size());
        for (size_t j = 0; j < nodes.size(); j++) {
            std::memcpy(ops[j].data(), id_bytes(nodes[j]->id), KAD_HASH_LEN);
            ops[j][KAD_HASH_LEN] = !nodes[j]->isExpired() ? (uint8_t)0
                                   : when.removable(*nodes[j]) ? both : (uint8_t)KAD_SN_BAD;
        }
        std::sort(ops.begin(), ops.end());
        ops.erase(std::unique(ops.begin(), ops.end()), ops.end());
        std::vector<uint8_t> nid, clr, set;
        for (const auto& o : ops) {
            nid.insert(nid.end(), o.begin(), o.begin() + KAD_HASH_LEN);
            set.push_back(o[KAD_HASH_LEN]);
            clr.push_back((uint8_t)(both & ~o[KAD_HASH_LEN]));
        }
        // one override per (search, node ID): the byte of the host's own entry
        std::vector<std::pair<uint32_t, std::array<uint8_t, KAD_HASH_LEN + 1>>> pr(pairs.size());
        for (size_t k = 0; k < pairs.size(); k++) {
            pr[k].first = index_of(id_bytes(pairs[k].first));
            const auto& n = pairs[k].second;
            std::memcpy(pr[k].second.data(), id_bytes(n->id), KAD_HASH_LEN);
            bool bad = n->isExpired();
            const auto it = map_->find(pairs[k].first);
            if (it == map_->end()) throw Error(KAD_ERR_INVALID, "the search map changed its keys (snapshot again)");
            for (const auto& sn : it->second->nodes)
                if (std::memcmp(id_bytes(sn.node->id), id_bytes(n->id), KAD_HASH_LEN) == 0) bad = sn.isBad();
            pr[k].second[KAD_HASH_LEN] = (uint8_t)((bad ? KAD_SN_BAD : 0u) | (when.removable(*n) ? KAD_SN_REMOVABLE : 0u));
        }
        std::sort(pr.begin(), pr.end());
        pr.erase(std::unique(pr.begin(), pr.end()), pr.end());
        std::vector<uint32_t> pw;
        std::vector<uint8_t> pid, pfl;
        for (const auto& e : pr) {
            pw.push_back(e.first);
            pid.insert(pid.end(), e.second.begin(), e.second.begin() + KAD_HASH_LEN);
            pfl.push_back(e.second[KAD_HASH_LEN]);
        }
        std::vector<uint32_t> changed(size());
        std::vector<uint8_t> counts(4 * size());
        uint32_t n_changed = 0;
        check(kad_sr_mark_nodes(ss_, (uint32_t)set.size(), nid.data(), clr.data(), set.data(), (uint32_t)pw.size(),
                                pw.data(), pid.data(), pfl.data(), nullptr, nullptr, changed.data(), counts.data(),
                                &n_changed), "kad_sr_mark_nodes");
        out.resize(n_changed);
        auto it = map_->begin();
        uint32_t at = 0;
        for (uint32_t k = 0; k < n_changed; k++) {
            std::advance(it, changed[k] - at);
            at = changed[k];
            if (it == map_->end() || std::memcmp(id_bytes(it->first), &ids_[(size_t)at * KAD_HASH_LEN], KAD_HASH_LEN) != 0)
                throw Error(KAD_ERR_INVALID, "the search map changed its keys (snapshot again)");
            out[k] = MarkedSearch<InfoHashT>{it->first, counts[4 * k], counts[4 * k + 1], counts[4 * k + 2],
                                            (counts[4 * k + 3] & 1) != 0, (counts[4 * k + 3] & 2) != 0};
        }
        return out;
    }

    /* The step bits of single list entries carried to the device set: one kad_sr_mark_entries. pairs: (search ID, node)
     * for every entry whose KAD_SN_CANDIDATE, KAD_SN_PENDING, KAD_SN_SYNCED or KAD_SN_NOGET changed (a request sent by
     * the host itself, a reply, a timeout, a deadline of last_get_reply + NODE_EXPIRE_TIME that passed), and, after a
     * snapshot, sync or a pair of markNodes (which write the byte without them), for every entry that carries any. The
     * reference keeps these in the getStatus maps, so the four bits come from the caller: bits(search, search node)
     * returns them for the entry as the host's list has it now, for the query the search's next searchSendGetValues
     * asks with (kadgpu.h). The entry gets exactly those four bits; KAD_SN_BAD and KAD_SN_REMOVABLE stay as they are.
     * Returns, per pair, whether the device's list holds the node; a pair whose node the host's own list does not hold
     * is not sent and answers 0. Repeated pairs are sent once. A pair always names a mirrored search. */
    template <class InfoHashT, class NodePtrT, class BitsFn>
    std::vector<uint8_t> markEntries(const std::vector<std::pair<InfoHashT, NodePtrT>>& pairs, BitsFn bits) {
        return markBits(pairs, bits, (uint8_t)(KAD_SN_CANDIDATE | KAD_SN_PENDING | KAD_SN_SYNCED | KAD_SN_NOGET),
                        &kad_sr_mark_entries, "kad_sr_mark_entries");
    }

    /* markEntries and markDue: the bits `all` of every pair's entry become bits(search, search node) & all, with `call`. */
    template <class InfoHashT, class NodePtrT, class BitsFn>
    std::vector<uint8_t> markBits(const std::vector<std::pair<InfoHashT, NodePtrT>>& pairs, BitsFn bits, const uint8_t all,
                                  int (*call)(kad_searches*, uint32_t, const uint32_t*, const uint8_t*, const uint8_t*,
                                              const uint8_t*, uint8_t*),
                                  const char* what) {
        std::vector<uint8_t> out(pairs.size(), 0);
        if (pairs.empty()) return out;
        if (!ss_) throw Error(KAD_ERR_INVALID, "SearchesMirror::markEntries before snapshot");
        // (search, node ID, bits, position in pairs), sorted: repeats lie side by side
        typedef std::pair<std::pair<uint32_t, std::array<uint8_t, KAD_HASH_LEN + 1>>, size_t> Row;
        std::vector<Row> rows;
        for (size_t k = 0; k < pairs.size(); k++) {
            Row r;
            r.first.first = index_of(id_bytes(pairs[k].first));
            r.second = k;
            const auto it = map_->find(pairs[k].first);
            if (it == map_->end()) throw Error(KAD_ERR_INVALID, "the search map changed its keys (snapshot again)");
            const uint8_t* nid = id_bytes(pairs[k].second->id);
            for (const auto& sn : it->second->nodes)
                if (std::memcmp(id_bytes(sn.node->id), nid, KAD_HASH_LEN) == 0) {
                    std::memcpy(r.first.second.data(), nid, KAD_HASH_LEN);
                    r.first.second[KAD_HASH_LEN] = (uint8_t)(bits(*it->second, sn) & all);
                    rows.push_back(r);
                    break;
                }
        }
        std::sort(rows.begin(), rows.end());
        std::vector<uint32_t> pw, first;  // first: per row, the row that was sent for its (search, node)
        std::vector<uint8_t> pid, clr, set;
        for (size_t k = 0; k < rows.size(); k++) {
            const bool repeat = k && rows[k].first.first == rows[k - 1].first.first &&
                                std::memcmp(rows[k].first.second.data(), rows[k - 1].first.second.data(), KAD_HASH_LEN) == 0;
            if (!repeat) {
                pw.push_back(rows[k].first.first);
                pid.insert(pid.end(), rows[k].first.second.begin(), rows[k].first.second.begin() + KAD_HASH_LEN);
                set.push_back(rows[k].first.second[KAD_HASH_LEN]);
                clr.push_back((uint8_t)(all & ~rows[k].first.second[KAD_HASH_LEN]));
            }
            first.push_back((uint32_t)pw.size() - 1);
        }
        std::vector<uint8_t> found(pw.size());
        check(call(ss_, (uint32_t)pw.size(), pw.data(), pid.data(), clr.data(), set.data(), found.data()), what);
        for (size_t k = 0; k < rows.size(); k++) out[rows[k].second] = found[first[k]];
        return out;
    }

    /* Dht::searchStep's decision (dht.cpp:1344-1464) on the mirrored searches `ids` (distinct) in one kad_sr_step:
     * modes[k] = KAD_STEP_* for ids[k] (empty: all 0). Returns, in the order of ids, the nodes that get a get request
     * (searchSendGetValues' picks, in list order, taken from the host's own list at the picked positions), the counts and
     * the KAD_STEP_* result bits (kadgpu.h). The device's lists and step bits must be the host's (insertBatch,
     * refillBatch, markNodes, markEntries, sync). With KAD_STEP_APPLY the device marks the picked entries PENDING | NOGET
     * and turns a search that expires into an empty expired one; the host then sends the requests, calls expire() on the
     * searches with KAD_STEP_EXPIRE (unless KAD_STEP_NO_EXPIRE) and reports nothing back for either. Listen and announce
     * requests, callbacks, refill_time and the scheduler edit stay with the caller; a search that is KAD_STEP_SHORT and
     * due is refilled with refillBatch before it is stepped. */
    template <class InfoHashT, class MapT = SearchMapT,
              class NodePtrT = decltype(std::declval<typename MapT::mapped_type>()->nodes.front().node)>
    std::vector<SteppedSearch<InfoHashT, NodePtrT>> stepBatch(const std::vector<InfoHashT>& ids,
                                                              const std::vector<uint8_t>& modes = std::vector<uint8_t>()) {
        std::vector<SteppedSearch<InfoHashT, NodePtrT>> out(ids.size());
        if (ids.empty()) return out;
        std::vector<kad_step_out> res(ids.size());
        const auto order = stepCall("SearchesMirror::stepBatch", &kad_sr_step, "kad_sr_step", ids, modes, res);
        for (size_t k = 0; k < res.size(); k++) {
            SteppedSearch<InfoHashT, NodePtrT>& o = out[order[k].second];
            const auto it = stepped("SearchesMirror::stepBatch", ids[order[k].second], res[k].counts, res[k].bits, o);
            pickNodes(it->second->nodes, res[k].picks, o.n, o.picks);
        }
        return out;
    }

    /* The two due bits of single list entries carried to the device set: one kad_sr_mark_due. pairs as for markEntries:
     * every entry whose KAD_SN_LISTEN_DUE or KAD_SN_ANNOUNCE_DUE changed (a listen or put reply, a new listener or
     * announce, a deadline of reply_time + LISTEN_EXPIRE_TIME - REANNOUNCE_MARGIN or acked.second - REANNOUNCE_MARGIN that
     * passed) and, after a snapshot, sync or a pair of markNodes, every entry that carries any. The reference keeps these
     * in listenStatus, acked and probe_query, so the bits come from the caller: bits(search, search node) returns them
     * for the entry as the host has it now. The entry gets exactly those two bits; the other six stay as they are.
     * Returns as markEntries does. */
    template <class InfoHashT, class NodePtrT, class BitsFn>
    std::vector<uint8_t> markDue(const std::vector<std::pair<InfoHashT, NodePtrT>>& pairs, BitsFn bits) {
        return markBits(pairs, bits, (uint8_t)(KAD_SN_LISTEN_DUE | KAD_SN_ANNOUNCE_DUE), &kad_sr_mark_due, "kad_sr_mark_due");
    }

    /* stepBatch with the listen requests and the announce probes of a synced search (kad_sr_step_full): modes[k] may
     * also carry KAD_STEP_LISTEN (the search has listeners), KAD_STEP_ANNOUNCE (it has announces) and
     * KAD_STEP_PROBE_BLOCKS (kadgpu.h). Returns per search the three node lists in list order, plus the counts and bits.
     * With KAD_STEP_APPLY the device also clears the due bit of every entry a loop sent to and marks the probed entries
     * PENDING; the host sends the listens, the probes and the gets in that order. isDone(get) and checkAnnounced
     * (dht.cpp:1359-1376), getNextStepTime and the requests themselves stay with the caller. */
    template <class InfoHashT, class MapT = SearchMapT,
              class NodePtrT = decltype(std::declval<typename MapT::mapped_type>()->nodes.front().node)>
    std::vector<FullySteppedSearch<InfoHashT, NodePtrT>> stepBatchFull(
        const std::vector<InfoHashT>& ids, const std::vector<uint8_t>& modes = std::vector<uint8_t>()) {
        std::vector<FullySteppedSearch<InfoHashT, NodePtrT>> out(ids.size());
        if (ids.empty()) return out;
        std::vector<kad_step_full_out> res(ids.size());
        const auto order = stepCall("SearchesMirror::stepBatchFull", &kad_sr_step_full, "kad_sr_step_full", ids, modes, res);
        for (size_t k = 0; k < res.size(); k++) {
            FullySteppedSearch<InfoHashT, NodePtrT>& o = out[order[k].second];
            const auto it = stepped("SearchesMirror::stepBatchFull", ids[order[k].second], res[k].counts, res[k].bits, o);
            pickNodes(it->second->nodes, res[k].picks, o.n, o.picks);
            pickNodes(it->second->nodes, res[k].listen, o.n, o.listen);
            pickNodes(it->second->nodes, res[k].announce, o.n, o.announce);
        }
        return out;
    }

private:
    /* stepBatch's and stepBatchFull's (`who`) searches as `call` (kad_sr_step, kad_sr_step_full: `what`) takes them,
     * and the call: returns (search index, position in ids) ascending; res[k] answers the k-th of them. */
    template <class InfoHashT, class OutT, class StatsT>
    std::vector<std::pair<uint32_t, size_t>> stepCall(
        const std::string& who, int (*call)(kad_searches*, uint32_t, const uint32_t*, const uint8_t*, OutT*, StatsT*),
        const char* what, const std::vector<InfoHashT>& ids, const std::vector<uint8_t>& modes, std::vector<OutT>& res) {
        if (!ss_) throw Error(KAD_ERR_INVALID, who + " before snapshot");
        if (!modes.empty() && modes.size() != ids.size()) throw Error(KAD_ERR_INVALID, who + ": one mode per search, or none");
        std::vector<std::pair<uint32_t, size_t>> order(ids.size());
        for (size_t k = 0; k < ids.size(); k++) order[k] = std::make_pair(index_of(id_bytes(ids[k])), k);
        std::sort(order.begin(), order.end());
        std::vector<uint32_t> which(ids.size());
        std::vector<uint8_t> md(ids.size(), 0);
        for (size_t k = 0; k < order.size(); k++) {
            if (k && order[k].first == order[k - 1].first) throw Error(KAD_ERR_INVALID, who + ": a search listed twice");
            which[k] = order[k].first;
            if (!modes.empty()) md[k] = modes[order[k].second];
        }
        check(call(ss_, (uint32_t)which.size(), which.data(), md.data(), res.data(), nullptr), what);
        return order;
    }

    /* The fields every stepped search has, from the device's counts and bits. Returns the host's search, whose list
     * must be as long as the device's. */
    template <class InfoHashT, class ResultT, class MapT = SearchMapT>
    typename MapT::const_iterator stepped(const std::string& who, const InfoHashT& id, uint32_t counts, uint32_t bits,
                                          ResultT& o) {
        const auto it = map_->find(id);
        if (it == map_->end()) throw Error(KAD_ERR_INVALID, "the search map changed its keys (snapshot again)");
        o.id = it->first;
        o.n = (uint8_t)counts;
        o.bad = (uint8_t)(counts >> 8);
        o.lead_bad = (uint8_t)(counts >> 16);
        o.solicited = (uint8_t)(counts >> 24);
        o.bits = bits;
        if (o.n != it->second->nodes.size())
            throw Error(KAD_ERR_INVALID, who + ": the host's list differs from the mirrored one (sync it)");
        return it;
    }

    /* the nodes at the list positions below n that mask names, in list order */
    template <class NodesT, class NodePtrT>
    static void pickNodes(const NodesT& nodes, uint64_t mask, uint32_t n, std::vector<NodePtrT>& out) {
        for (uint32_t e = 0; e < n; e++)
            if ((mask >> e) & 1ull) out.push_back(nodes[e].node);
    }

    template <class InfoHashT, class When>
    void syncAt(const std::vector<InfoHashT>& changed, const When& when) {
        if (!ss_) throw Error(KAD_ERR_INVALID, "SearchesMirror::sync before snapshot");
        std::vector<uint32_t> which;
        for (const auto& id : changed) which.push_back(index_of(id_bytes(id)));
        std::sort(which.begin(), which.end());
        which.erase(std::unique(which.begin(), which.end()), which.end());
        if (which.empty()) return;
        std::vector<uint8_t> flags, nid, nfl;
        std::vector<uint32_t> off(1, 0u);
        uint32_t longest = 0;
        auto it = map_->begin();
        uint32_t at = 0;
        for (uint32_t w : which) {
            std::advance(it, w - at);
            at = w;
            if (it == map_->end() || std::memcmp(id_bytes(it->first), &ids_[(size_t)w * KAD_HASH_LEN], KAD_HASH_LEN) != 0)
                throw Error(KAD_ERR_INVALID, "the search map changed its keys (snapshot again)");
            append(*it->second, flags, off, nid, nfl, when);
            longest = std::max<uint32_t>(longest, off.back() - off[off.size() - 2]);
        }
        if (longest > cap_) {
            snapshotAt(*map_, when, device_, std::max(longest, 2 * cap_));
            return;
        }
        check(kad_searches_patch(ss_, (uint32_t)which.size(), which.data(), flags.data(), off.data(), nid.data(),
                                 nfl.data()), "kad_searches_patch");
        for (uint32_t w : which) at_[w] = when.ns();
    }

    template <class InfoHashT, class When>
    void updateAt(const std::vector<InfoHashT>& erased, const std::vector<InfoHashT>& added, const When& when) {
        if (!ss_) throw Error(KAD_ERR_INVALID, "SearchesMirror::update before snapshot");
        std::vector<uint32_t> erase;
        for (const auto& id : erased) erase.push_back(index_of(id_bytes(id)));
        std::sort(erase.begin(), erase.end());
        erase.erase(std::unique(erase.begin(), erase.end()), erase.end());
        std::vector<uint8_t> ins, fl;
        std::vector<InfoHashT> filled;  // added searches that already hold nodes
        for (const auto& id : added) {
            const uint32_t at = lower_bound_of(id_bytes(id));
            if (at < size() && std::memcmp(&ids_[(size_t)at * KAD_HASH_LEN], id_bytes(id), KAD_HASH_LEN) == 0 &&
                !std::binary_search(erase.begin(), erase.end(), at))
                throw Error(KAD_ERR_INVALID, "SearchesMirror::update: an added search is already mirrored");
            const auto it = map_->find(id);
            if (it == map_->end()) throw Error(KAD_ERR_INVALID, "SearchesMirror::update: an added search is not in the map");
            ins.insert(ins.end(), id_bytes(id), id_bytes(id) + KAD_HASH_LEN);
            fl.push_back(it->second->expired ? (uint8_t)KAD_SR_EXPIRED : (uint8_t)0);
            if (!it->second->nodes.empty()) filled.push_back(id);
        }
        std::vector<uint32_t> remap(size()), new_index(added.size());
        check(kad_searches_apply(ss_, erase.data(), (uint32_t)erase.size(), ins.data(), fl.data(), (uint32_t)added.size(),
                                 0, remap.data(), new_index.data()), "kad_searches_apply");
        const size_t S2 = size() - erase.size() + added.size();
        std::vector<uint8_t> ids(S2 * KAD_HASH_LEN);
        std::vector<int64_t> at(S2, when.ns());
        for (size_t s = 0; s < remap.size(); s++)
            if (remap[s] != KAD_NO_NODE) {
                std::memcpy(&ids[(size_t)remap[s] * KAD_HASH_LEN], &ids_[s * KAD_HASH_LEN], KAD_HASH_LEN);
                at[remap[s]] = at_[s];
            }
        for (size_t j = 0; j < new_index.size(); j++)
            std::memcpy(&ids[(size_t)new_index[j] * KAD_HASH_LEN], &ins[j * KAD_HASH_LEN], KAD_HASH_LEN);
        ids_.swap(ids);
        at_.swap(at);
        if (!filled.empty()) syncAt(filled, when);
    }

public:

    /* Dht::trySearchInsert's verdict for each candidate ID taken alone against the searches as mirrored: one
     * kad_sr_try_insert_batch_host call. The host then runs insertNode on the searches [lb - back, lb + fwd) only
     * (node.time, removeExpiredNode, the scheduler edit) and reports them to sync(). */
    template <class InfoHashT>
    std::vector<SearchInsertVerdict> trySearchInsertBatch(const InfoHashT* ids, size_t q) const {
        std::vector<SearchInsertVerdict> out(q);
        if (q == 0) return out;
        if (!ss_) throw Error(KAD_ERR_INVALID, "SearchesMirror::trySearchInsertBatch before snapshot");
        std::vector<uint8_t> cand(q * KAD_HASH_LEN), stop(q);
        std::vector<uint32_t> lb(q), fwd(q), back(q);
        for (size_t i = 0; i < q; i++) std::memcpy(&cand[i * KAD_HASH_LEN], id_bytes(ids[i]), KAD_HASH_LEN);
        check(kad_sr_try_insert_batch_host(ss_, cand.data(), (uint32_t)q, lb.data(), fwd.data(), back.data(),
                                           stop.data()), "kad_sr_try_insert_batch_host");
        for (size_t i = 0; i < q; i++) out[i] = SearchInsertVerdict{lb[i], fwd[i], back[i], stop[i]};
        return out;
    }

    size_t size() const { return ids_.size() / KAD_HASH_LEN; }
    uint32_t cap() const { return cap_; }
    const kad_searches* handle() const { return ss_; }

private:
    /* When KAD_SN_REMOVABLE is evaluated: never (the overloads without a time), or at a time point. The mirror keeps
     * the time of every search's upload as nanoseconds since the clock's epoch (INT64_MIN: never). */
    struct NoTime {
        template <class NodeT>
        bool removable(const NodeT&) const { return false; }
        int64_t ns() const { return INT64_MIN; }
    };
    template <class TimePoint>
    struct At {
        TimePoint now;
        template <class NodeT>
        static bool removableAtPoint(const NodeT& n, TimePoint t) {  // Node::NODE_EXPIRE_TIME = 10 minutes (node.h)
            return n.isExpired() && n.time + std::chrono::minutes(10) < t;
        }
        template <class NodeT>
        bool removable(const NodeT& n) const { return removableAtPoint(n, now); }
        template <class NodeT>
        bool removableAt(const NodeT& n, int64_t ns) const {
            return removableAtPoint(n, TimePoint(std::chrono::duration_cast<typename TimePoint::duration>(
                                           std::chrono::nanoseconds(ns))));
        }
        int64_t ns() const {
            return (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(now.time_since_epoch()).count();
        }
    };
    template <class SearchT, class When>
    static void append(const SearchT& s, std::vector<uint8_t>& flags, std::vector<uint32_t>& off,
                       std::vector<uint8_t>& nid, std::vector<uint8_t>& nfl, const When& when) {
        flags.push_back(s.expired ? (uint8_t)KAD_SR_EXPIRED : (uint8_t)0);
        for (const auto& sn : s.nodes) {
            nid.insert(nid.end(), id_bytes(sn.node->id), id_bytes(sn.node->id) + KAD_HASH_LEN);
            nfl.push_back((uint8_t)((sn.isBad() ? KAD_SN_BAD : 0u) | (when.removable(*sn.node) ? KAD_SN_REMOVABLE : 0u)));
        }
        off.push_back((uint32_t)nfl.size());
    }
    uint32_t lower_bound_of(const uint8_t* id) const {
        size_t lo = 0, hi = size();
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            if (std::memcmp(&ids_[mid * KAD_HASH_LEN], id, KAD_HASH_LEN) < 0) lo = mid + 1; else hi = mid;
        }
        return (uint32_t)lo;
    }
    uint32_t index_of(const uint8_t* id) const {
        const size_t lo = lower_bound_of(id);
        if (lo == size() || std::memcmp(&ids_[lo * KAD_HASH_LEN], id, KAD_HASH_LEN) != 0)
            throw Error(KAD_ERR_INVALID, "search not in the mirrored snapshot (snapshot again)");
        return (uint32_t)lo;
    }
    void reset() {
        if (ss_) kad_searches_destroy(ss_);
        ss_ = nullptr;
    }
    void swap(SearchesMirror& o) {
        std::swap(ss_, o.ss_);
        std::swap(map_, o.map_);
        ids_.swap(o.ids_);
        std::swap(device_, o.device_);
        std::swap(cap_, o.cap_);
        at_.swap(o.at_);
    }

    kad_searches* ss_ = nullptr;
    const SearchMapT* map_ = nullptr;
    std::vector<uint8_t> ids_;  // the mirrored search IDs, ascending
    int device_ = 0;
    uint32_t cap_ = 0;
    std::vector<int64_t> at_;  // per search: when its KAD_SN_REMOVABLE bits were evaluated (INT64_MIN: never set)
};

/* DhtMirror's search map when the Dht's searches are not mirrored. */
struct NoSearchMap {};

/* Dht-level accessor over both families: findClosestNodes(id, af, count)
 * = buckets(af).findClosestNodes(id, scheduler.time(), count) (dht.h:437-438; call sites dht.cpp:3196-3217).
 * `now` comes from the mirror's clock: steady_clock::now() by default, or the Dht scheduler's time
 * (setClock([&]{ return scheduler.time(); })). */
template <class RoutingTableT, class Clock = std::chrono::steady_clock, class SearchMapT = NoSearchMap>
class DhtMirror {
public:
    using NodePtr = typename RoutingTableMirror<RoutingTableT>::NodePtr;
    using time_point = typename Clock::time_point;

    DhtMirror() : clock_([] { return Clock::now(); }) {}

    void snapshot(const RoutingTableT& buckets4, const RoutingTableT& buckets6, time_point now, int device = 0) {
        v4_.snapshot(buckets4, now, device);
        v6_.snapshot(buckets6, now, device);
    }
    void setClock(std::function<time_point()> clock) { clock_ = std::move(clock); }

    template <class InfoHashT>
    std::vector<NodePtr> findClosestNodes(const InfoHashT& id, sa_family_t af, size_t count = KAD_TARGET_NODES) const {
        return buckets(af).findClosestNodes(id, clock_(), count);
    }
    /* Dht::maintainStorage's verdict for every stored key in one pass (dht.cpp:2909-2937): byte i = KAD_RESP_FAR4
     * if keys[i] is too far in the IPv4 table | KAD_RESP_FAR6 if in the IPv6 table (count = TARGET_NODES, any result
     * counts); 3 is the reference's "discard". One isTooFarBatch per family, host buffers (device-pointer callers
     * get both bits from one launch, kad_rt_responsible_batch_dual). */
    template <class InfoHashT>
    std::vector<uint8_t> maintainStorageBatch(const std::vector<InfoHashT>& keys, const InfoHashT& myid,
                                              time_point now) const {
        const std::vector<uint8_t> a = v4_.isTooFarBatch(keys, myid, now), b = v6_.isTooFarBatch(keys, myid, now);
        std::vector<uint8_t> out(keys.size());
        for (size_t i = 0; i < out.size(); i++)
            out[i] = (uint8_t)((a[i] ? KAD_RESP_FAR4 : 0u) | (b[i] ? KAD_RESP_FAR6 : 0u));
        return out;
    }
    /* Dht::onNewNode(node, 0) triage for the candidates of one family (RoutingTableMirror::onNewNodeBatch), at the
     * mirror's clock. */
    template <class InfoHashT>
    std::vector<NewNodeVerdict> onNewNodeBatch(const InfoHashT* ids, size_t q, sa_family_t af, const InfoHashT* myid,
                                               bool is_bootstrap) const {
        return buckets(af).onNewNodeBatch(ids, q, myid, clock_(), is_bootstrap);
    }
    /* Dht::getNodesStats(af, good, dubious, cached, incoming) without `cached` (host state, Bucket::cached): the
     * counts of one family at the mirror's clock; returns good + dubious as the reference does (dht.cpp:2494). */
    unsigned getNodesStats(sa_family_t af, unsigned* good_return, unsigned* dubious_return,
                           unsigned* incoming_return) const {
        const NodesStats st = buckets(af).nodesStats(clock_());
        if (good_return) *good_return = st.good;
        if (dubious_return) *dubious_return = st.dubious;
        if (incoming_return) *incoming_return = st.incoming;
        return st.good + st.dubious;
    }
    /* Dht::expireBuckets(buckets(af)) (dht.cpp:942-956, run for both families by Dht::expire) on the mirror. */
    Expired<NodePtr> expireBuckets(sa_family_t af) { return buckets(af).expireBuckets(clock_()); }
    /* Dht::onReportedAddr's bucket write for one family's replies, at the mirror's clock
     * (RoutingTableMirror::onReportedAddrBatch / onReportedAddr). */
    template <class InfoHashT>
    void onReportedAddrBatch(sa_family_t af, const std::vector<InfoHashT>& ids) {
        buckets(af).onReportedAddrBatch(ids, clock_());
    }
    template <class InfoHashT>
    void onReportedAddr(sa_family_t af, const InfoHashT& id) { buckets(af).onReportedAddr(id, clock_()); }
    /* Dht::connectivityChanged's reset of every Bucket::time, both families (dht.cpp:2388-2392). */
    void resetBucketTimes() {
        v4_.resetBucketTimes();
        v6_.resetBucketTimes();
    }
    /* Dht::bucketMaintenance(buckets(af)) up to the node it would query (RoutingTableMirror::bucketMaintenance), at the
     * mirror's clock. */
    template <class Rng>
    MaintenancePick<NodePtr> bucketMaintenance(sa_family_t af, RoutingTableT& rt, Rng& rd) {
        return buckets(af).bucketMaintenance(rt, clock_(), rd);
    }
    /* Dht::trySearchInsert's verdicts for the candidates of one family (SearchesMirror::trySearchInsertBatch), after
     * snapshotSearches; syncSearches(af, changed) reports the searches the host's inserts changed. */
    void snapshotSearches(const SearchMapT& searches4, const SearchMapT& searches6, int device = 0) {
        s4_.snapshot(searches4, device);
        s6_.snapshot(searches6, device);
    }
    template <class InfoHashT>
    std::vector<SearchInsertVerdict> trySearchInsertBatch(const InfoHashT* ids, size_t q, sa_family_t af) const {
        return searches(af).trySearchInsertBatch(ids, q);
    }
    template <class InfoHashT>
    void syncSearches(sa_family_t af, const std::vector<InfoHashT>& changed) { searches(af).sync(changed); }
    /* Dht::refill for the searches `ids` of one family from the NodeCache mirror `cache`, at the mirror's clock
     * (SearchesMirror::refillBatch); syncSearches(af, changed, now) reports the overflowed ones. */
    template <class NodeMapT, class InfoHashT>
    std::vector<RefillResult<typename NodeCacheFamilyMirror<NodeMapT>::NodePtr>>
    refillBatch(const NodeCacheMirror<NodeMapT>& cache, sa_family_t af, const std::vector<InfoHashT>& ids) {
        return searches(af).refillBatch(cache.family(af), ids, clock_());
    }
    /* Search::insertNode of the nodes nodes[i] into the search ids[i] of one family, at the mirror's clock
     * (SearchesMirror::insertBatch); syncSearches(af, changed, now) reports the ones handed back. */
    template <class InfoHashT, class NodePtrT>
    std::vector<InsertResult> insertBatch(sa_family_t af, const std::vector<InfoHashT>& ids,
                                          const std::vector<std::vector<NodePtrT>>& nodes) {
        return searches(af).insertBatch(ids, nodes, clock_());
    }
    /* Dht::trySearchInsert of the nodes of one tick on the searches of one family, applied on the device, at the
     * mirror's clock (SearchesMirror::trySearchInsertTick); the host replays, and syncSearches(af, changed, now) reports
     * the overflowed searches and what the walks of the LEFT candidates changed. */
    template <class NodePtrT, class MapT = SearchMapT, class InfoHashT = typename MapT::key_type>
    TickResult<InfoHashT> trySearchInsertTick(sa_family_t af, const std::vector<NodePtrT>& nodes, uint32_t max_rounds = 0) {
        return searches(af).trySearchInsertTick(nodes, clock_(), max_rounds);
    }
    /* The node status changes of one tick for the searches of one family, at the mirror's clock
     * (SearchesMirror::markNodes). */
    template <class NodePtrT, class InfoHashT>
    std::vector<MarkedSearch<InfoHashT>> markNodes(sa_family_t af, const std::vector<NodePtrT>& nodes,
                                                   const std::vector<std::pair<InfoHashT, NodePtrT>>& pairs) {
        return searches(af).markNodes(nodes, pairs, clock_());
    }
    template <class InfoHashT>
    void syncSearches(sa_family_t af, const std::vector<InfoHashT>& changed, time_point now) {
        searches(af).sync(changed, now);
    }
    /* The searches of one family erased from and added to the Dht's map (SearchesMirror::update), at the mirror's
     * clock: Dht::expireSearches and Dht::search. */
    template <class InfoHashT>
    void updateSearches(sa_family_t af, const std::vector<InfoHashT>& erased, const std::vector<InfoHashT>& added) {
        searches(af).update(erased, added, clock_());
    }
    /* The step bits of single entries of one family's searches (SearchesMirror::markEntries). */
    template <class InfoHashT, class NodePtrT, class BitsFn>
    std::vector<uint8_t> markSearchEntries(sa_family_t af, const std::vector<std::pair<InfoHashT, NodePtrT>>& pairs,
                                           BitsFn bits) {
        return searches(af).markEntries(pairs, bits);
    }
    /* Dht::searchStep's decision on searches of one family (SearchesMirror::stepBatch). */
    template <class InfoHashT>
    auto stepSearches(sa_family_t af, const std::vector<InfoHashT>& ids,
                      const std::vector<uint8_t>& modes = std::vector<uint8_t>())
        -> decltype(std::declval<SearchesMirror<SearchMapT>&>().stepBatch(ids, modes)) {
        return searches(af).stepBatch(ids, modes);
    }
    /* The due bits of single entries of one family's searches (SearchesMirror::markDue). */
    template <class InfoHashT, class NodePtrT, class BitsFn>
    std::vector<uint8_t> markSearchDue(sa_family_t af, const std::vector<std::pair<InfoHashT, NodePtrT>>& pairs, BitsFn bits) {
        return searches(af).markDue(pairs, bits);
    }
    /* The whole searchStep's decision on searches of one family (SearchesMirror::stepBatchFull). */
    template <class InfoHashT>
    auto stepSearchesFull(sa_family_t af, const std::vector<InfoHashT>& ids,
                          const std::vector<uint8_t>& modes = std::vector<uint8_t>())
        -> decltype(std::declval<SearchesMirror<SearchMapT>&>().stepBatchFull(ids, modes)) {
        return searches(af).stepBatchFull(ids, modes);
    }
    /* Dht::buckets(af) (dht.h:437-438) */
    const RoutingTableMirror<RoutingTableT>& buckets(sa_family_t af) const { return af == AF_INET ? v4_ : v6_; }
    RoutingTableMirror<RoutingTableT>& buckets(sa_family_t af) { return af == AF_INET ? v4_ : v6_; }
    /* Dht::searches(af) */
    const SearchesMirror<SearchMapT>& searches(sa_family_t af) const { return af == AF_INET ? s4_ : s6_; }
    SearchesMirror<SearchMapT>& searches(sa_family_t af) { return af == AF_INET ? s4_ : s6_; }

private:
    RoutingTableMirror<RoutingTableT> v4_, v6_;
    SearchesMirror<SearchMapT> s4_, s6_;
    std::function<time_point()> clock_;
};

}  // namespace kadgpu

#endif /* KADGPU_HPP */
