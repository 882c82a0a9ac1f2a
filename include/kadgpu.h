/*
 * kadgpu.h — C ABI of the MI355X-native batched Kademlia closest-node engine.
 *
 * This is the drop-in boundary for OpenDHT's XOR-distance lookup path. The
 * reference exposes no C API/FFI for this path: its interface
 * is the C++ member
 *     std::vector<std::shared_ptr<Node>>
 *     RoutingTable::findClosestNodes(const InfoHash id, time_point now,
 *                                    size_t count) const
 *         (reference: include/opendht/routing_table.h:48, src/routing_table.cpp:67-111)
 *     RoutingTable::findBucket(const InfoHash&)
 *         (reference: include/opendht/routing_table.h:50-51, src/routing_table.cpp:113-135)
 *     std::vector<std::shared_ptr<Node>>
 *     NodeCache::getCachedNodes(const InfoHash&, sa_family_t, size_t)
 *         (reference: include/opendht/node_cache.h:32, src/node_cache.cpp:36-66)
 * and the InfoHash primitives (include/opendht/infohash.h:84-162).
 *
 * Every entry point below replaces one of those; each cites the reference
 * interface it stands in for. The C++11 shim in kadgpu.hpp wraps these with
 * the reference's own signatures (RoutingTable::findClosestNodes, the new
 * Dht-style findClosestNodes(id, af, count) accessor, NodeCache::getCachedNodes).
 *
 * Conventions
 *  - IDs cross the ABI as raw InfoHash bytes: 20 bytes per ID, byte 0 most
 *    significant (InfoHash::data() layout, reference infohash.h:58).
 *  - A table is a snapshot of one address family's RoutingTable (and/or its
 *    NodeCache map) at a chosen `now`: a flat node array grouped by bucket,
 *    a bucket directory, and one status byte per node (bit0 = Node::isGood(now),
 *    bit1 = Node::isExpired(); reference src/node.cpp:34-40, node.h:67).
 *  - Results are uint32 node indices into the snapshot's node array plus
 *    `index_base` (so shards can return global indices), padded with
 *    KAD_NO_NODE beyond the per-query result count.
 *  - Every function returns an int status (KAD_OK = 0, negative on error);
 *    kad_last_error() gives a thread-local message. No C++ exception crosses
 *    this ABI. Empty table -> zero results (reference routing_table.cpp:73).
 *  - `*_batch` entry points take DEVICE pointers and enqueue on `stream`
 *    (a hipStream_t, NULL = default stream); they do not synchronise.
 *    `*_batch_host` entry points take HOST pointers and are synchronous
 *    (H2D, kernel, D2H on an internal stream).
 *  - A table handle is not safe for concurrent mutation; concurrent const
 *    queries on distinct streams are safe (as in the reference, where
 *    findClosestNodes is const: SURVEY.md §8b "Threading").
 */
#ifndef KADGPU_H
#define KADGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KAD_HASH_LEN 20u            /* reference infohash.h:49 HASH_LEN */
#define KAD_TARGET_NODES 8u         /* reference routing_table.h:26 TARGET_NODES */
#define KAD_SEARCH_NODES 14u        /* reference dht.h:314 SEARCH_NODES */
#define KAD_MAX_COUNT 32u           /* largest `count` of the line kernels; RoutingTable queries take any
                                       count (larger ones run one wave per query); the shard / wire
                                       entry points stay at <= KAD_MAX_COUNT */
#define KAD_NO_NODE 0xFFFFFFFFu     /* padding index in result rows */

/* status byte bits (snapshot of Node state at `now`) */
#define KAD_STATUS_GOOD 0x01u       /* Node::isGood(now)   reference node.cpp:34-40 */
#define KAD_STATUS_EXPIRED 0x02u    /* Node::isExpired()   reference node.h:67       */

/* kad_table_create flags */
#define KAD_TABLE_SORTED 0x01u      /* node array ascending by ID (enables NodeCache queries) */
#define KAD_TABLE_EAGER 0x02u       /* build every line set at creation (default: those of count <= 8 RoutingTable
                                       queries; the others on first use, kad_table_prepare) */
#define KAD_TABLE_NO_SLOT_LINES 0x04u /* general-line tables: no slot lines (count <= 8 / 9..16 queries locate
                                         their bucket and read its general line; a status refresh then rebuilds
                                         the count <= 8 general lines in its one fused launch) */

/* line sets built on first use (kad_table_prepare, kad_table_line_sets) */
#define KAD_LINES_RT16 0x01u        /* RoutingTable counts 9..16 (brings KAD_LINES_RT32, their fallback) */
#define KAD_LINES_RT32 0x02u        /* RoutingTable counts 17..32 */
#define KAD_LINES_NC16 0x04u        /* NodeCache counts 1..16 */
#define KAD_LINES_NC32 0x08u        /* NodeCache counts 17..32 (brings KAD_LINES_NC16) */
#define KAD_LINES_ALL 0x0Fu
/* kad_table_info.flags, reported only */
#define KAD_INFO_WINDOW_LINES 0x100u /* uniform-depth table: count <= 8 queries use one 128-byte
                                        window line per query (rt_wl_kernel) */
#define KAD_INFO_GENERAL_LINES 0x200u /* any other bucket shape: count <= 8 queries use one 128-byte
                                         general window line per query (rt_gl_kernel) */
#define KAD_INFO_GENERAL_LINES32 0x400u /* ... and counts 9..32 one 256-byte line (rt_gl32_kernel) */
#define KAD_INFO_GENERAL_LINES16 0x4000u /* ... and counts 9..16 one 128-byte line (rt_gl16_kernel) */
#define KAD_INFO_SLOT_LINES16 0x8000u /* ... read through a 128-byte copy indexed by the target's top bits (rt_sl16_kernel) */
#define KAD_INFO_SLOT_LINES 0x2000u /* other bucket shapes: count <= 8 queries read one 64-byte line indexed by
                                       the target's top bits (rt_sl_kernel), the locate + 128-byte line only
                                       as fallback */
#define KAD_INFO_NODECACHE_LINES32 0x1000u /* sorted table: NodeCache counts 17..32 read one 384-byte line
                                             per query, 8 lanes per query (nc32_line_kernel) */
#define KAD_INFO_SHORT_LINES 0x800u /* uniform-depth table: count <= 8 queries read one 64-byte short
                                       window line (rt_ws_kernel), the 128-byte line only as fallback */

/* error codes */
#define KAD_OK 0
#define KAD_ERR_INVALID -1          /* bad argument / shape */
#define KAD_ERR_HIP -2              /* HIP runtime error */
#define KAD_ERR_NOMEM -3            /* device allocation failed */
#define KAD_ERR_UNSUPPORTED -4      /* e.g. count > KAD_MAX_COUNT */
#define KAD_ERR_NOT_SORTED -5       /* NodeCache query on a table without KAD_TABLE_SORTED */
#define KAD_ERR_NO_DEVICE -6        /* no usable gfx950 device */

typedef struct kad_table kad_table;

typedef struct kad_table_info {
    uint32_t n_nodes;
    uint32_t n_buckets;
    uint32_t index_base;
    uint32_t flags;
    int32_t device;
    uint32_t rt_radix_bits;         /* log2 of the bucket-locate radix table size */
    uint32_t nc_radix_bits;         /* log2 of the NodeCache lower_bound radix table size (0 if unsorted) */
    uint32_t n_good;                /* good nodes under the current status snapshot */
    uint64_t device_bytes;          /* HBM held by the table */
} kad_table_info;

/* ---- library ---------------------------------------------------------- */
const char* kad_last_error(void);
int kad_version(void);                                  /* 10000*major + 100*minor + patch */
int kad_device_count(int* out_n);                       /* gfx950 devices visible */

/* ---- table lifetime ----------------------------------------------------- */
/* Snapshot a RoutingTable (reference routing_table.h:28-79) and/or NodeCache map
 * (node_cache.h:42-50) into device memory.
 *   ids           host, n_nodes x 20 bytes; bucket b owns [bucket_offset[b], bucket_offset[b+1])
 *                 (RoutingTable list order inside a bucket; ties between equal IDs resolve by index)
 *   status        host, n_nodes status bytes (KAD_STATUS_*)
 *   bucket_first  host, n_buckets x 20 bytes, ascending (Bucket::first, routing_table.h:33)
 *   bucket_offset host, n_buckets+1 offsets, bucket_offset[0]=0, bucket_offset[n_buckets]=n_nodes
 *   n_buckets = 0 builds a NodeCache-only table (requires KAD_TABLE_SORTED).
 *   flags         KAD_TABLE_SORTED if ids are strictly ascending (checked) */
int kad_table_create(kad_table** out, int device,
                     uint32_t n_nodes, const uint8_t* ids, const uint8_t* status,
                     uint32_t n_buckets, const uint8_t* bucket_first, const uint32_t* bucket_offset,
                     uint32_t index_base, uint32_t flags);
int kad_table_destroy(kad_table* t);
int kad_table_get_info(const kad_table* t, kad_table_info* out);
/* Build the line sets `sets` (KAD_LINES_*) now, if not yet: a query builds the set it needs on first use
 * (synchronising the device once, and never inside a stream capture, where it answers on its slower exact
 * path instead), so a caller about to capture a HIP graph prepares them first. Synchronous. */
int kad_table_prepare(kad_table* t, uint32_t sets);
/* Which line sets are built (KAD_LINES_* mask), and per set in bit order (RT16, RT32, NC16, NC32) the HBM
 * bytes and the build time in ms of its first build (any output may be NULL). */
int kad_table_line_sets(const kad_table* t, uint32_t* built, uint64_t* bytes, float* build_ms);

/* Replace the status snapshot (host bytes, n_nodes). Synchronous. Incremental: only the buckets whose
 * good set changed get new masks and good counts, and only the window / NodeCache lines whose window reaches
 * a changed node are rebuilt. */
int kad_table_update_status(kad_table* t, const uint8_t* status);
/* Incremental status update for a changed-node list (reference: the isGood/isExpired flips that
 * Node::received / setExpired cause, node.cpp:82-108; network_engine.cpp:245): node nodes[j] gets
 * status[j] (host arrays, m entries; nodes == NULL means all n_nodes in order). Rebuilds only what
 * the flips touch, as kad_table_update_status. Synchronous. */
int kad_table_patch_status(kad_table* t, uint32_t m, const uint32_t* nodes, const uint8_t* status);

/* Upload Node liveness (reference node.h:39-40,105: time, reply_time, expired_)
 * as int64 nanoseconds of steady_clock + expired flag bytes; host arrays, n_nodes each.
 * INT64_MIN encodes time_point::min(). Synchronous. */
int kad_table_set_times(kad_table* t, const int64_t* time_ns, const int64_t* reply_time_ns,
                        const uint8_t* expired);
/* Update the uploaded liveness of m listed nodes (Node::received / setExpired on the host: node.cpp:82-108):
 * host arrays of m entries. Takes effect at the next kad_table_refresh_status. Synchronous. */
int kad_table_patch_times(kad_table* t, uint32_t m, const uint32_t* nodes, const int64_t* time_ns,
                          const int64_t* reply_time_ns, const uint8_t* expired);
/* Recompute the status snapshot on the device at `now_ns` from the uploaded times:
 * good = !expired && reply_time >= now-120min && time >= now-10min (node.cpp:34-40,
 * node.h:91-94). A good node stays good while now <= min(time + 10 min, reply_time + 120 min), so the
 * table keeps every node's deadline sorted: the first refresh after kad_table_set_times (or after a
 * direct status change, or with `now` earlier than the last refresh's) re-derives every node and sorts
 * the deadlines; later ones re-derive only the nodes whose deadline `now` passed since the last refresh
 * and the nodes patched by kad_table_patch_times, and a refresh whose `now` has not reached the next
 * deadline (with nothing patched) returns at once without touching the GPU. The host keeps a copy of the
 * sorted deadlines (8 bytes per node) and finds the passed ones itself. Up to 2,048 such nodes take the
 * small path: one kernel re-derives them and lists the changed buckets and the lines whose windows reach
 * them, then the line builders rebuild only those (no pass over the buckets or the lines); up to 128 of them
 * on a table with window lines are one launch in all (block 0 re-derives the nodes, the other blocks rebuild
 * the count <= 8 lines at the same time, the host having found the nodes' buckets and the lines). More take
 * the flag-and-compact path. Async on `stream` (the first refresh after set_times waits for the sort);
 * later refreshes and device batches must be ordered after it by the caller (the host-pointer batches
 * order themselves). A refresh that changes anything ends the table's resident query service launch
 * (kad_table_serve) first. */
int kad_table_refresh_status(kad_table* t, int64_t now_ns, void* stream);
/* Counters of the small refresh since the table was created (synchronises the device):
 *   spin_timeouts     builder blocks of a fused general-line refresh that waited RF_SPIN_TICKS (1 s) for the
 *                     line list block 0 publishes and gave up (block 0 not running: the GPU busy with other
 *                     work); their lines were then built by the launch's last block, so results stay exact. After
 *                     the first timeout the table stops fusing those builds (they go out as stream-ordered
 *                     launches after the node kernel), so the wait cannot recur
 *   last_block_lines  lines built by a fused launch's last block (windows of more than 64 nodes, and the lists
 *                     of timed-out builders)
 *   guard_errors      bounds guards of the kernel that fired (bit mask; the host validates every inline
 *                     argument before a launch, so this is 0 unless the engine has a bug) */
typedef struct kad_refresh_diag {
    uint32_t spin_timeouts;
    uint32_t last_block_lines;
    uint32_t guard_errors;
} kad_refresh_diag;
int kad_table_refresh_diag(const kad_table* t, kad_refresh_diag* out);

/* ---- incremental device mirror ----------------------
 * Replays the table mutations of a live Dht on the device instead of re-snapshotting. Ops are rows
 * of three uint32 (kind, a, b) applied in order; `a` names a node by its index at the start of
 * the batch, `b` / `a` of INSERT a slot of the batch's new nodes (new_ids / new_status, host):
 *   KAD_OP_REMOVE  a     node a leaves its bucket (Dht::expireBuckets, dht.cpp:942-956)
 *   KAD_OP_REPLACE a b   new node b takes node a's place (onNewNode's expired slot, dht.cpp:917-921);
 *                        b must belong to a's bucket (findBucket(id_b)), else KAD_ERR_INVALID
 *   KAD_OP_INSERT  a     new node a is emplace_front'ed into findBucket(id) (dht.cpp:934)
 *   KAD_OP_SPLIT   a     RoutingTable::split of the bucket at current index a (routing_table.cpp:137-163;
 *                        nodes re-spliced to the front of their new bucket: list order reverses)
 * The node arrays are re-laid out on the device (one gather over the plan's segments); masks,
 * prefix sums, dup masks and window lines are re-derived there (a split turns window lines off).
 * Outputs: remap (host or device, old n entries, may be NULL) = new index of every old node, KAD_NO_NODE
 * if removed or replaced; new_index (host, n_new, may be NULL) = index of every new node,
 * KAD_NO_NODE if unused. Any op clears KAD_TABLE_SORTED (NodeCache queries need a new snapshot);
 * wire records and node times must be set again. Synchronous. */
#define KAD_OP_REMOVE 1u
#define KAD_OP_REPLACE 2u
#define KAD_OP_INSERT 3u
#define KAD_OP_SPLIT 4u
int kad_table_apply(kad_table* t, const uint32_t* ops, uint32_t n_ops, const uint8_t* new_ids,
                    const uint8_t* new_status, uint32_t n_new, uint32_t* remap, uint32_t* new_index);
/* NodeCache map mutations (node_cache.cpp:91-115) on a NodeCache-only table (n_buckets = 0,
 * KAD_TABLE_SORTED), without a re-snapshot: erase the n_erase listed nodes (indices at the call, each at
 * most once: NodeMap::getNode(id) erasing a dead weak_ptr, clearBadNodes' erase of dead entries), then
 * insert n_ins new IDs (host, any order, none already a kept key: NodeMap::getNode(id, addr, now, confirm)'s
 * emplace) with their status bytes. The node array is merged on the device and stays sorted; the NodeCache
 * radix and lines are re-derived there. remap (host, old n entries, may be NULL): new index of every old
 * node, KAD_NO_NODE if erased; new_index (host, n_ins, may be NULL): index of every new node. Node times and
 * wire records must be set again. Failure leaves the table unchanged. Synchronous. */
int kad_nc_apply(kad_table* t, const uint32_t* erase, uint32_t n_erase, const uint8_t* ins_ids,
                 const uint8_t* ins_status, uint32_t n_ins, uint32_t* remap, uint32_t* new_index);
/* The table as host arrays (any may be NULL): ids n x 20 and status in bucket/list order, bucket
 * firsts B x 20 and offsets B+1 (sizes from kad_table_get_info). */
int kad_table_export(const kad_table* t, uint8_t* ids, uint8_t* status, uint8_t* bucket_first,
                     uint32_t* bucket_offset);
/* A derived array of the table as raw bytes (tests: an incrementally maintained set must equal the one a fresh
 * table builds from the same status). out == NULL: *bytes = the size (0 if the table has no such set). */
#define KAD_LINESET_WL 0u     /* 128-byte window lines (count <= 8) */
#define KAD_LINESET_WS 1u     /* 64-byte short window lines */
#define KAD_LINESET_WL16 2u
#define KAD_LINESET_WL32 3u
#define KAD_LINESET_GL 4u     /* general lines */
#define KAD_LINESET_GL16 5u
#define KAD_LINESET_GL32 6u
#define KAD_LINESET_SL 7u     /* slot lines */
#define KAD_LINESET_SL16 8u
#define KAD_LINESET_NCL 9u    /* NodeCache lines */
#define KAD_LINESET_NCL32 10u
#define KAD_LINESET_GCNT 11u  /* per-bucket good counts */
#define KAD_LINESET_DIR 12u   /* bucket directory: first node (bit 31: wide), good mask */
int kad_table_export_lines(const kad_table* t, uint32_t set, void* out, uint64_t* bytes);

/* ---- whole-table sweep (Dht::getNodesStats dht.cpp:2470-2495, Dht::expireBuckets dht.cpp:942-956) ---- */
/* One read-only streaming pass over the table's status snapshot (refresh it to `now` first, as before queries) and
 * its bucket directory: the counts getNodesStats walks the lists for, and what expireBuckets would remove.
 *   expired_nodes    the nodes with KAD_STATUS_EXPIRED in ascending index order (bucket order, then list order),
 *                    each plus index_base as every node output of this ABI (subtract it for KAD_OP_REMOVE's operand)
 *   changed_buckets  the plain indices of the buckets holding at least one such node, ascending: the buckets
 *                    expireBuckets calls sendCachedPing for (:953-954)
 * Both lists are deterministic (the same table gives the same bytes). Either may be NULL with cap 0 (NULL with a
 * non-zero cap: KAD_ERR_INVALID). A list holds only its first `cap` entries and nothing is written at or beyond
 * `cap`; totals always carries the true counts, so an overflow shows as totals.expired > cap_nodes.
 * Any table shape: split-policy, uniform and shard tables, buckets of any width, empty buckets, n_buckets == 0
 * (NodeCache-only: the node counts, no buckets), n_nodes == 0. getNodesStats' `cached` (Bucket::cached, a host
 * pointer per bucket) stays with the host; bucketMaintenance's Bucket::time has its own pass, kad_table_maintenance.
 * Device pointers (4-byte aligned); enqueues on `stream` and does not synchronise. A const query whose partial
 * counts live in a stream-ordered allocation of the call's own: concurrent sweeps of one table on distinct streams
 * are safe. Checked in this order, before any device work: NULL table, NULL totals, unknown flag bits, a NULL list
 * with a non-zero cap, KAD_SWEEP_INCOMING on a table without kad_table_set_times (all KAD_ERR_INVALID). */
#define KAD_SWEEP_INCOMING 1u   /* also count getNodesStats' `incoming` (reads the uploaded times) */
typedef struct kad_sweep_totals {
    uint32_t good;            /* status has KAD_STATUS_GOOD                     (dht.cpp:2476-2477) */
    uint32_t dubious;         /* neither GOOD nor EXPIRED                       (:2480-2481)        */
    uint32_t expired;         /* status has KAD_STATUS_EXPIRED: what expireBuckets removes (:947)   */
    uint32_t incoming;        /* GOOD and time > reply_time (:2478-2479); 0 without the flag        */
    uint32_t changed_buckets; /* buckets holding at least one EXPIRED node (:953-954)               */
    uint32_t empty_buckets;   /* buckets without nodes                                              */
    uint32_t flags;           /* the flags this sweep ran with                                      */
    uint32_t reserved;        /* 0 */
} kad_sweep_totals;
int kad_table_sweep(const kad_table* t, uint32_t flags, kad_sweep_totals* totals, uint32_t* expired_nodes,
                    uint32_t cap_nodes, uint32_t* changed_buckets, uint32_t cap_buckets, void* stream);
/* kad_table_sweep on host buffers, synchronous, ordered after every change made to the table before the call; device
 * buffers and a stream of the call's own. The outputs are written only when the call succeeds. */
int kad_table_sweep_host(const kad_table* t, uint32_t flags, kad_sweep_totals* totals, uint32_t* expired_nodes,
                         uint32_t cap_nodes, uint32_t* changed_buckets, uint32_t cap_buckets);
/* Dht::expireBuckets on the device copy: removes every KAD_STATUS_EXPIRED node of the status snapshot. The table
 * that results is the one kad_table_apply gives for one KAD_OP_REMOVE per expired node in ascending order (layout,
 * directory, masks, good counts, line sets; KAD_TABLE_SORTED cleared), with one difference: the node times of
 * kad_table_set_times and the wire records of kad_table_set_addrs are gathered through the remap on the device and
 * stay attached, so kad_table_refresh_status and kad_buffer_nodes_batch work without a new upload (the deadlines are
 * invalidated: the next refresh re-derives every node, as after kad_table_set_times).
 *   remap            host or device, old n entries, may be NULL: as kad_table_apply
 *   removed          host, cap_removed words (may be NULL with cap 0): the sweep's expired_nodes before the removal
 *                    (old indices plus index_base), its first cap_removed entries; *n_removed (may be NULL) the count
 *   changed_buckets  host, likewise: the sweep's changed_buckets; *n_changed the count
 * No expired node: the table is untouched (same device arrays, line sets and flags), remap is the identity. Needs a
 * RoutingTable (n_buckets > 0; KAD_ERR_INVALID otherwise, as kad_table_apply). A failure leaves the table as it was,
 * times and wire records included, and writes no output. Synchronous.
 * Memory the call keeps: the table holds a pinned host buffer for the read-back of the two lists (4 bytes per removed
 * node and changed bucket of the largest call so far, freed with the table); the sweep's partial counts and this call's
 * device lists come from a memory pool of the engine's own per device, which lives as long as the process and keeps
 * what it is given back, up to 32 MB after a kad_table_expire that took more (the rest is returned to the driver). */
int kad_table_expire(kad_table* t, uint32_t* remap, uint32_t* removed, uint32_t cap_removed, uint32_t* n_removed,
                     uint32_t* changed_buckets, uint32_t cap_buckets, uint32_t* n_changed);

/* ---- bucket times and Dht::bucketMaintenance's scan (dht.cpp:2826-2885, 3174-3181) ---- */
/* Bucket::time (routing_table.h:30,34) on the device: one int64 per bucket, nanoseconds of steady_clock, INT64_MIN for
 * time_point::min() (Bucket's default, and what connectivityChanged resets to, dht.cpp:2391). The array is allocated
 * on first use; a table that never had bucket times set behaves as if every bucket were at INT64_MIN.
 * kad_table_apply carries the times: REMOVE, REPLACE and INSERT leave them, KAD_OP_SPLIT a gives the new bucket a + 1
 * the time of bucket a (routing_table.cpp:149); kad_table_expire keeps them. None of these calls ends the resident
 * query service (no query reads the times). A failure leaves the table unchanged.
 * Upload every bucket's time: host array of n_buckets entries; NULL sets every bucket to INT64_MIN. Synchronous. */
int kad_table_set_bucket_times(kad_table* t, const int64_t* time_ns);
/* buckets[j] gets time_ns[j] (host lists of m entries), for a caller that already knows the bucket. A bucket listed
 * twice takes the later entry. Checked before any device work: NULL table, a NULL list with m > 0, an index
 * >= n_buckets (all KAD_ERR_INVALID; nothing is written). Synchronous. */
int kad_table_patch_bucket_times(kad_table* t, uint32_t m, const uint32_t* buckets, const int64_t* time_ns);
/* The times as a host array of n_buckets entries, ordered after every change made before the call. */
int kad_table_get_bucket_times(const kad_table* t, int64_t* out);
/* Dht::onReportedAddr (dht.cpp:3174-3181) x q: findBucket(ids[i])->time = now_ns for every ID (device, q x 20
 * bytes). out_bucket (device, q words, may be NULL) receives the bucket, as kad_rt_find_bucket_batch gives it. A call
 * has one now_ns, so IDs that share a bucket store the same value: the result does not depend on the order lanes run.
 * Enqueues on `stream` and does not synchronise. Checked in this order: NULL table, n_buckets == 0 (the reference
 * dereferences end()), a NULL ids with q > 0 (all KAD_ERR_INVALID). */
int kad_table_touch_buckets(kad_table* t, const uint8_t* ids, uint32_t q, int64_t now_ns, uint32_t* out_bucket,
                            void* stream);
/* The same on host buffers, synchronous. out_bucket is written only when the call succeeds. */
int kad_table_touch_buckets_host(kad_table* t, const uint8_t* ids, uint32_t q, int64_t now_ns, uint32_t* out_bucket);

/* One read-only pass over the bucket times and the bucket directory: the buckets b >= first_bucket that pass
 * bucketMaintenance's test (:2833), time[b] < now_ns - 10 min || the bucket has no nodes, ascending, each as one
 * kad_maint_rec. The caller runs the reference's loop body (randomId, the two rand_trial draws, randomNode) over these
 * buckets only. `kind` holds
 *   KAD_MAINT_STALE       the time test holds (strict: time == now - 10 min is not stale, INT64_MIN always is)
 *   KAD_MAINT_EMPTY       the bucket has no nodes
 *   KAD_MAINT_HAS_NEXT    std::next(b) != end();  KAD_MAINT_NEXT_EMPTY  ... and it has no nodes
 *   KAD_MAINT_HAS_PREV    b != begin();           KAD_MAINT_PREV_EMPTY  ... and std::prev(b) has no nodes
 *   bits 6-7              KAD_MAINT_NEVER / MAYBE / SURE: q->randomNode() of :2838-2850 is non-null for no / some /
 *                         every outcome of the two rand_trial draws. NEVER buckets are listed too: the reference
 *                         still draws randomId's bytes for them
 *   bits 8-15             RoutingTable::randomId's `bit` (routing_table.cpp:30-32), 0..160
 * totals counts from first_bucket on and holds the true counts whatever cap is; out holds the first `cap` records and
 * nothing is written at or beyond cap. Deterministic bytes. A caller resumes with first_bucket = last bucket + 1.
 * Device pointers (totals 4-byte, out 8-byte aligned); enqueues on `stream` and does not synchronise. A const query
 * whose partial counts live in a stream-ordered allocation of the call's own: concurrent calls on one table on
 * distinct streams are safe. n_buckets == 0 gives zero totals. Checked in this order, before any device work: NULL
 * table, NULL totals, a NULL out with a non-zero cap, now_ns < INT64_MIN + 10 min, first_bucket > n_buckets (all
 * KAD_ERR_INVALID). */
#define KAD_MAINT_STALE 0x01u
#define KAD_MAINT_EMPTY 0x02u
#define KAD_MAINT_HAS_NEXT 0x04u
#define KAD_MAINT_NEXT_EMPTY 0x08u
#define KAD_MAINT_HAS_PREV 0x10u
#define KAD_MAINT_PREV_EMPTY 0x20u
#define KAD_MAINT_CLASS_SHIFT 6u
#define KAD_MAINT_NEVER 0u
#define KAD_MAINT_MAYBE 1u
#define KAD_MAINT_SURE 2u
#define KAD_MAINT_BIT_SHIFT 8u
#define KAD_MAINT_STALE_NS 600000000000ll   /* the 10 minutes of :2833 */
typedef struct kad_maint_rec {
    uint32_t bucket;
    uint32_t kind;
} kad_maint_rec;
typedef struct kad_maint_totals {
    uint32_t candidates;      /* buckets listed (were cap large enough)             */
    uint32_t stale;           /* ... with KAD_MAINT_STALE                            */
    uint32_t empty;           /* ... with KAD_MAINT_EMPTY                            */
    uint32_t sure;            /* ... of class SURE                                   */
    uint32_t maybe;
    uint32_t never;
    uint32_t first_sure;      /* the smallest listed bucket of class SURE, or 0xFFFFFFFF */
    uint32_t reserved;        /* 0 */
} kad_maint_totals;
int kad_table_maintenance(const kad_table* t, int64_t now_ns, uint32_t first_bucket, kad_maint_totals* totals,
                          kad_maint_rec* out, uint32_t cap, void* stream);
/* kad_table_maintenance on host buffers, synchronous, ordered after every change made to the table before the call.
 * The outputs are written only when the call succeeds. */
int kad_table_maintenance_host(const kad_table* t, int64_t now_ns, uint32_t first_bucket, kad_maint_totals* totals,
                               kad_maint_rec* out, uint32_t cap);
/* The same scan on host arrays, without a GPU and without a table (the twin the device pass is tested against; it
 * shares the kind decision with the kernels): off B + 1 node offsets, first B x 20 bytes, time_ns B entries or NULL
 * (every bucket at INT64_MIN). The same checks in the same order (NULL off or first with B > 0 in place of the NULL
 * table), the same record bytes. Sets no error text. */
int kad_maint_scan_host(uint32_t B, const uint32_t* off, const uint8_t* first, const int64_t* time_ns, int64_t now_ns,
                        uint32_t first_bucket, kad_maint_totals* totals, kad_maint_rec* out, uint32_t cap);

/* ---- queries: RoutingTable::findClosestNodes ---------------------------- */
/* Batched RoutingTable::findClosestNodes(target, now, count) (routing_table.cpp:67-111)
 * on the table's status snapshot. Device pointers:
 *   targets  q x 20 bytes; out_idx q x count uint32; out_cnt q uint8 (may be NULL).
 * Row i of out_idx holds the result in the reference's order (ascending XOR
 * distance), out_cnt[i] entries, padded with KAD_NO_NODE. Any count, as the reference's
 * size_t count (routing_table.h:48): counts up to KAD_MAX_COUNT run the line kernels, larger
 * ones one wave per query; out_cnt saturates at 255 (for count > 255 the result length is the
 * row's entries before the first KAD_NO_NODE). */
int kad_rt_closest_batch(const kad_table* t, const uint8_t* targets, uint32_t q, uint32_t count,
                         uint32_t* out_idx, uint8_t* out_cnt, void* stream);
/* The same on host buffers (any memory), synchronous, and ordered after every change made to the table
 * before the call (the asynchronous kad_table_refresh_status on whatever stream it ran; every other change
 * is synchronous). Batches of up to 1024 queries with count <= 64 are one kernel launch that reads the
 * targets from and writes the rows to mapped pinned memory (one round trip); larger ones run as 64k-query
 * chunks pipelined over four host threads through ~80 MB of pinned staging and device buffers the table
 * keeps (allocated on first use, freed with it). One host batch per table at a time.
 * count <= 2,097,152 (one chunk row; larger counts: the device-pointer batch). */
int kad_rt_closest_batch_host(const kad_table* t, const uint8_t* targets, uint32_t q, uint32_t count,
                              uint32_t* out_idx, uint8_t* out_cnt);

/* Resident query service for single requests (the per-request calls of dht.cpp:3196-3217, 1650): with
 * idle_us > 0 one workgroup stays on the GPU and answers host batches of up to KAD_SERVE_MAX_Q queries with
 * count <= KAD_SERVE_MAX_COUNT (kad_rt_closest_batch_host, kad_nc_closest_batch_host) from a mailbox in
 * pinned host memory: no kernel launch and no stream synchronise per call. Same results, same ordering
 * (after the table's last asynchronous status refresh). A launch ends by itself after idle_us without a
 * request or after 50 ms in all, and the next request launches it again. Calls that change or free what
 * it reads (patch/update_status, patch/set_times, a refresh_status that changes anything, apply, nc_apply,
 * set_addrs, prepare, destroy) end it first. While it runs it holds one CU, and:
 *   - device-wide synchronisation (hipDeviceSynchronize, torch.cuda.synchronize) waits for it to go idle
 *     (up to idle_us after the last request, or the rest of its 50 ms life);
 *   - HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default): work queued on a stream that
 *     shares the service's queue waits behind the resident launch the same way. With more than four
 *     streams in the process, keep idle_us short (a few hundred microseconds) or call kad_table_serve(t, 0)
 *     before long device work.
 * idle_us = 0 ends it and turns it off (the default). idle_us <= KAD_SERVE_MAX_IDLE_US. */
#define KAD_SERVE_MAX_Q 64
#define KAD_SERVE_MAX_COUNT 64
#define KAD_SERVE_MAX_IDLE_US 1000000
int kad_table_serve(kad_table* t, uint32_t idle_us);
/* The service's counters: launches so far (the first request after an idle exit launches again), requests
 * answered, and for the last request the header reads it took to be seen and the device time from seen to
 * its rows fenced (the rest of a call's latency is the PCIe round trip and the host). */
typedef struct kad_serve_stats {
    uint32_t idle_us;
    uint32_t last_polls;
    uint64_t launches;
    uint64_t requests;
    uint64_t last_busy_ns;
} kad_serve_stats;
int kad_table_serve_stats(const kad_table* t, kad_serve_stats* out);

/* Batched RoutingTable::findBucket (routing_table.cpp:113-135): bucket index per
 * target (0 for targets below the first bucket, as the reference's list walk). */
int kad_rt_find_bucket_batch(const kad_table* t, const uint8_t* targets, uint32_t q,
                             uint32_t* out_bucket, void* stream);

/* ---- queries: NodeCache::getCachedNodes --------------------------------- */
/* Batched NodeCache::getCachedNodes(target, af, count) (node_cache.cpp:36-66) over
 * one family's map, snapshotted as a KAD_TABLE_SORTED table. Emits non-expired
 * nodes in the reference's two-pointer walk order (NOT sorted by distance). Any count, as the
 * reference's size_t count (node_cache.h:32): counts up to 16 / 32 run the NodeCache line kernels,
 * 33..64 one wave per query, larger ones the serial walk (a lane per query); out_cnt saturates at 255
 * (for count > 255 the result length is the row's entries before the first KAD_NO_NODE). */
int kad_nc_closest_batch(const kad_table* t, const uint8_t* targets, uint32_t q, uint32_t count,
                         uint32_t* out_idx, uint8_t* out_cnt, void* stream);
int kad_nc_closest_batch_host(const kad_table* t, const uint8_t* targets, uint32_t q, uint32_t count,
                              uint32_t* out_idx, uint8_t* out_cnt);

/* ---- dual-family batch (Dht::onGetValues asks both tables, dht.cpp:3216-3217) ---- */
/* Per-query family select: af[i] = 0 -> table4, 1 -> table6 (either may be NULL
 * if no query selects it). Device pointers. */
int kad_rt_closest_batch_dual(const kad_table* table4, const kad_table* table6,
                              const uint8_t* targets, const uint8_t* af, uint32_t q, uint32_t count,
                              uint32_t* out_idx, uint8_t* out_cnt, void* stream);

/* ---- storage responsibility (Dht::maintainStorage dht.cpp:2909-2937, Dht::onAnnounce dht.cpp:3352-3358) ---- */
/* Both call sites take findClosestNodes(h, now, count) and use one bit of it: h.xorCmp(nodes.back()->id, myid) < 0,
 * "the last returned node is closer to h than we are". Batched, per target h, on the table's status snapshot:
 *   R = findClosestNodes(h, now, count) (the window semantics of kad_rt_closest_batch), n = |R|
 *   far = n >= max(min_nodes, 1) && xorCmp_h(id(R[n-1]), self_id) < 0     (strict 160-bit compare; a last node
 *         equal to self_id is not far; an empty table, no good node or count == 0: not far)
 * maintainStorage: count = KAD_TARGET_NODES, min_nodes = 1 (dht.cpp:2909-2926); onAnnounce: count =
 * KAD_SEARCH_NODES, min_nodes = KAD_TARGET_NODES (dht.cpp:3352-3358).
 * self_id: 20 host bytes; targets: device, q x 20 bytes; out_far: device, q bytes, 0 or KAD_RESP_FAR. One byte per
 * query leaves instead of a 33-byte row. Enqueues on `stream` and does not synchronise. A const query without
 * table-held scratch: concurrent calls on distinct streams are safe. count <= 8 on tables with short window lines
 * or slot lines answers from one line per query; every other shape, and counts 9..KAD_MAX_COUNT, one wave per
 * query. Checked in this order, before the table is read or any device work: NULL table, NULL self_id / targets /
 * out_far (KAD_ERR_INVALID); q == 0 (KAD_OK); count > KAD_MAX_COUNT (KAD_ERR_UNSUPPORTED). */
#define KAD_RESP_FAR 1u
#define KAD_RESP_FAR4 1u
#define KAD_RESP_FAR6 2u
int kad_rt_responsible_batch(const kad_table* t, const uint8_t* self_id, const uint8_t* targets, uint32_t q,
                             uint32_t count, uint32_t min_nodes, uint8_t* out_far, void* stream);
/* Both families answer every target, as maintainStorage asks both (dht.cpp:2909-2926): out[i] = KAD_RESP_FAR4 if far
 * in table4 | KAD_RESP_FAR6 if far in table6, one launch. A NULL family behaves as an empty table (its bit is 0);
 * both NULL, or tables on different devices: KAD_ERR_INVALID. out[i] == 3 is maintainStorage's "discard". */
int kad_rt_responsible_batch_dual(const kad_table* table4, const kad_table* table6, const uint8_t* self_id,
                                  const uint8_t* targets, uint32_t q, uint32_t count, uint32_t min_nodes,
                                  uint8_t* out, void* stream);
/* kad_rt_responsible_batch on host buffers, synchronous, ordered after every change made to the table before the
 * call; device buffers and a stream of the call's own. */
int kad_rt_responsible_batch_host(const kad_table* t, const uint8_t* self_id, const uint8_t* targets, uint32_t q,
                                  uint32_t count, uint32_t min_nodes, uint8_t* out_far);

/* ---- onNewNode triage (Dht::onNewNode(node, 0), dht.cpp:867-936) ---- */
/* What onNewNode would do with candidate ID x, decided against the table's status snapshot (refresh it to `now`
 * first, as before queries). With b = findBucket(x), evaluated in this order:
 *   KAD_NN_NONE     the table has no bucket (dht.cpp:871)                                   node = KAD_NO_NODE
 *   KAD_NN_KNOWN    a node of b has x's 160-bit ID (:874-880)                               node = the lowest such index
 *   KAD_NN_REPLACE  b holds a KAD_STATUS_EXPIRED node (:897-901)                            node = the first expired node in
 *                                                                                          bucket order (KAD_OP_REPLACE's a)
 *   KAD_NN_INSERT   b holds fewer than KAD_TARGET_NODES nodes (:932-935)                    node = KAD_NO_NODE
 *   KAD_NN_SPLIT    b is full and (mybucket || (bootstrap && depth(b) < 6)) &&              node = the first node of b without
 *                   (!dubious || n_buckets == 1) (:921)                                     KAD_STATUS_GOOD (the ping
 *   KAD_NN_FULL     b is full otherwise: "cache it away" (:929-931)                         candidate of :906-919), or
 *                                                                                          KAD_NO_NODE
 * mybucket: findBucket(self_id) == b; dubious: some node of b lacks KAD_STATUS_GOOD; depth(b) is
 * RoutingTable::depth (routing_table.cpp:59-65); a bucket with more than KAD_TARGET_NODES nodes counts as full.
 * Whether the ping candidate has a pending message is host state: the host checks it and walks on itself if so.
 * verdict[i] = kind | KAD_NN_MYBUCKET when mybucket holds (every kind but NONE; the host needs it for
 * mybucket_grow_time, :887-894). node[i] carries index_base, as the rows do. bucket[i] (may be NULL) = findBucket(x),
 * KAD_NO_NODE for NONE: KAD_OP_SPLIT's operand, equal to kad_rt_find_bucket_batch on the same IDs.
 * The candidates of one batch do not see each other: every verdict is against the snapshot.
 * self_id: 20 host bytes or NULL (no bucket is "mine": a shard without the node's own ID); ids: device, q x 20
 * bytes; verdict: device, q bytes; node, bucket: device, q words. flags: KAD_NN_BOOTSTRAP = Dht::is_bootstrap.
 * Enqueues on `stream` and does not synchronise; a const query without table-held scratch: concurrent calls on
 * distinct streams are safe. Checked in this order, before the table is read or any device work: NULL table, NULL
 * ids / verdict / node, unknown flag bits (KAD_ERR_INVALID, also with q == 0); q == 0 (KAD_OK). */
#define KAD_NN_NONE 0u
#define KAD_NN_KNOWN 1u
#define KAD_NN_REPLACE 2u
#define KAD_NN_INSERT 3u
#define KAD_NN_SPLIT 4u
#define KAD_NN_FULL 5u
#define KAD_NN_KIND_MASK 0x0Fu
#define KAD_NN_MYBUCKET 0x10u
#define KAD_NN_BOOTSTRAP 1u   /* flags: Dht::is_bootstrap */
int kad_rt_triage_batch(const kad_table* t, const uint8_t* self_id, const uint8_t* ids, uint32_t q, uint32_t flags,
                        uint8_t* verdict, uint32_t* node, uint32_t* bucket, void* stream);
/* kad_rt_triage_batch on host buffers, synchronous, ordered after every change made to the table before the call;
 * device buffers and a stream of the call's own. */
int kad_rt_triage_batch_host(const kad_table* t, const uint8_t* self_id, const uint8_t* ids, uint32_t q,
                             uint32_t flags, uint8_t* verdict, uint32_t* node, uint32_t* bucket);

/* ---- trySearchInsert verdicts over a set of live searches (Dht::trySearchInsert dht.cpp:816-849) ---- */
/* A search set is one family's live searches: S searches in strictly ascending 160-bit ID order (the order of the
 * std::map), each with a flag byte (KAD_SR_EXPIRED = Search::expired) and a node list of n entries (20-byte node ID,
 * flag byte; KAD_SN_BAD = SearchNode::isBad(), dht.cpp:458-460) strictly ascending in XOR distance to the search's ID,
 * the order Search::insertNode keeps. Node identity is the 160-bit ID (NodeCache holds one Node per ID and family).
 *
 * accept(s, x): s.insertNode(x, now) with an empty token would return true (dht.cpp:961-1047), from the snapshot alone:
 *   1. x equals a node ID of the list: refuse, KAD_SR_STOP_KNOWN (:972-984).
 *   2. the trim position t and `full` (:989-1007, kad_search_trim): expired: full = n >= 14, t = full ? 14 : n;
 *      else bad = number of BAD entries, full = n - bad >= 14, t = n, and while t - bad > 14: --t, and --bad if
 *      entry[t] is BAD.
 *   3. full and x not strictly closer to s.id than entry[t-1]: refuse (:1009-1014), KAD_SR_STOP_FAR for a live
 *      search, KAD_SR_STOP_FAR_EXPIRED for an expired one.
 *   4. otherwise accept.
 * Per candidate, with lb = lower_bound(search IDs, x) (the first search whose ID is >= x; S if none): fwd = the number
 * of consecutive accepting searches lb, lb+1, ...; back = the number of consecutive accepting searches lb-1, lb-2,
 * ...; stop = fstop | bstop << 4, why each walk ended (KAD_SR_STOP_END: it ran off the set). S == 0 gives lb = fwd =
 * back = 0, stop = 0. The candidates of one batch do not see each other. node.time = now, removeExpiredNode, tokens
 * and the scheduler edit stay on the host: what it does to the searches [lb - back, lb + fwd). */
#define KAD_SR_EXPIRED 0x01u          /* search flag: Search::expired */
#define KAD_SN_BAD 0x01u              /* node flag: SearchNode::isBad() */
#define KAD_SR_STOP_END 0u
#define KAD_SR_STOP_KNOWN 1u
#define KAD_SR_STOP_FAR 2u
#define KAD_SR_STOP_FAR_EXPIRED 3u
typedef struct kad_searches kad_searches;
/* Step 2 above on a list's flag bytes (host code, no device): *full = 0 or 1, *t <= n. NULL node_flags with n > 0,
 * NULL full / t: KAD_ERR_INVALID (kad_last_error is not set: the function lives outside the engine). */
int kad_search_trim(uint32_t n, const uint8_t* node_flags, uint32_t search_flags, uint32_t* full, uint32_t* t);
/* Host arrays: ids S x 20 bytes, flags S bytes, the lists in CSR form (off[S + 1] into node_ids, 20 bytes each, and
 * node_flags). The device keeps a fixed slab of `cap` entries per search and, per search, t, full and the threshold
 * ID entry[t-1], derived on the host. Checked in this order, before any device work: NULL out / off, NULL ids / flags
 * with S > 0, NULL node_ids / node_flags with off[S] > 0 (KAD_ERR_INVALID); cap < KAD_SEARCH_NODES
 * (KAD_ERR_INVALID); search IDs not strictly ascending (KAD_ERR_INVALID); offsets not ascending or a list not strictly
 * ascending in distance to its search ID, which also rejects duplicate nodes (KAD_ERR_INVALID); a list longer than cap
 * (KAD_ERR_UNSUPPORTED: create again with a larger cap). S == 0 is a valid set. Synchronous. */
int kad_searches_create(kad_searches** out, int device, uint32_t S, uint32_t cap, const uint8_t* ids,
                        const uint8_t* flags, const uint32_t* off, const uint8_t* node_ids, const uint8_t* node_flags);
/* Replaces the flags and lists of the m searches which[0..m) (strictly ascending, < S: KAD_ERR_INVALID otherwise):
 * the ones the host's inserts changed. flags m bytes, off[m + 1], node arrays as for create, the same checks in the
 * same order. The set of search IDs is not changed here: kad_searches_apply adds and erases searches. Synchronous, and as
 * kad_table_apply towards queries: it first waits for all device work enqueued before the call, so a query enqueued
 * earlier reads the old set and one enqueued after the return the new one; the caller must not enqueue queries on
 * the set from another thread while the call runs. Failure leaves the set unchanged. m == 0: KAD_OK. */
int kad_searches_patch(kad_searches* ss, uint32_t m, const uint32_t* which, const uint8_t* flags, const uint32_t* off,
                       const uint8_t* node_ids, const uint8_t* node_flags);
/* Adds and erases searches and grows the slabs on the device (Dht::search dht.cpp:1673-1735, the re-use of a done
 * search under a new ID :1695-1711, Dht::expireSearches :1060-1074). Host arrays, synchronous.
 *   erase     n_erase indices as of the call, strictly ascending, < S: these searches go.
 *   insert    n_ins new searches, ins_ids n_ins x 20 bytes in any order, distinct and different from every kept
 *             search's ID (the ID of a search erased by the same call is allowed: the re-use case). A new search is
 *             empty: n = 0, t = 0, full = 0, threshold zero, slab all zero, KAD_SR_EXPIRED from ins_flags[j] (NULL
 *             ins_flags: all 0): exactly the record and slab kad_searches_create derives for an empty list.
 *   kept      record, member keys, tails and flag bytes are carried over bit for bit (KAD_SN_BAD, KAD_SN_REMOVABLE and
 *             any other bit the caller stored); only the position changes. The new set is in ascending ID order.
 *   new_cap   0 keeps cap; otherwise >= cap, and every slab becomes new_cap entries with entries [cap, new_cap) zero.
 *             Slabs do not shrink. new_cap alone is "create the set again with larger slabs" without the upload.
 *   lookup    skey (S' <= 4096) or the prefix directory (B = ceil(log2 S') at most 24) is rebuilt on the device for
 *             the new S'; kad_searches_info's device_bytes equals what kad_searches_create of the final set reports.
 *   outputs   remap (S words, may be NULL): the new index of every old search, KAD_NO_NODE if erased; new_index
 *             (n_ins words, may be NULL): the index of every inserted search. Written on success only.
 * Only one word per new search and the 20 bytes of every inserted ID go up; records and slabs never do.
 * Failure-atomic as kad_table_apply and kad_nc_apply: the new arrays are allocated and filled beside the old ones and
 * take their place only after the last device step succeeded, so every failure leaves the set unchanged and the peak
 * device memory of the call is the old set plus the new one. The refill timing of kad_sr_refill_kernel_ms survives.
 * As kad_searches_patch towards queries: it first waits for all device work enqueued before the call, so a query
 * enqueued earlier reads the old set and one enqueued after the return the new one.
 * Checked in this order, before any device work: NULL ss; NULL erase with n_erase > 0 or NULL ins_ids with n_ins > 0;
 * erase not strictly ascending or not < S; new_cap != 0 && new_cap < cap; an ins_flags byte with bits other than
 * KAD_SR_EXPIRED; inserted IDs not distinct or one equal to a kept search's ID; S' x cap' >= 0x7FFFFFFF (all
 * KAD_ERR_INVALID); nothing to do (n_erase = n_ins = 0 and new_cap 0 or cap): KAD_OK, remap = identity, no device work.
 * Out of host or device memory: KAD_ERR_NOMEM. S' == 0 leaves a set without device arrays, as kad_searches_create with
 * S == 0; such a set accepts inserts. */
int kad_searches_apply(kad_searches* ss, const uint32_t* erase, uint32_t n_erase, const uint8_t* ins_ids,
                       const uint8_t* ins_flags, uint32_t n_ins, uint32_t new_cap, uint32_t* remap, uint32_t* new_index);
/* S, cap and the device bytes held (any may be NULL). */
int kad_searches_info(const kad_searches* ss, uint32_t* S, uint32_t* cap, uint64_t* device_bytes);
/* The device state read back into host arrays (any may be NULL): ids S x 20, flags S, n S words, node_ids
 * S x cap x 20 and node_flags S x cap (the slabs; entries past n are zero), and the derived full (S bytes) and t
 * (S words). */
int kad_searches_export(const kad_searches* ss, uint8_t* ids, uint8_t* flags, uint32_t* n, uint8_t* node_ids,
                        uint8_t* node_flags, uint8_t* full, uint32_t* t);
int kad_searches_destroy(kad_searches* ss);
/* The verdicts of q candidates. Device pointers: ids q x 20 bytes; out_lb (may be NULL), out_fwd, out_back q words;
 * out_stop q bytes. Enqueues on `stream` and does not synchronise; a const query without set-held scratch: concurrent
 * calls on distinct streams are safe. One lane per candidate; a walk over a run of accepting searches is serial in
 * its lane. Checked in this order: NULL set, NULL ids / out_fwd / out_back / out_stop (KAD_ERR_INVALID, also with
 * q == 0); q == 0 (KAD_OK); ids or a word output not 4-byte aligned (KAD_ERR_INVALID). */
int kad_sr_try_insert_batch(const kad_searches* ss, const uint8_t* ids, uint32_t q, uint32_t* out_lb,
                            uint32_t* out_fwd, uint32_t* out_back, uint8_t* out_stop, void* stream);
/* kad_sr_try_insert_batch on host buffers, synchronous; device buffers and a stream of the call's own. */
int kad_sr_try_insert_batch_host(const kad_searches* ss, const uint8_t* ids, uint32_t q, uint32_t* out_lb,
                                 uint32_t* out_fwd, uint32_t* out_back, uint8_t* out_stop);

/* ---- Dht::refill over a set of live searches (dht.cpp:1647-1668) ---- */
/* For each listed search s, against the snapshots `ss` and `nc` (one family's NodeCache as a KAD_TABLE_SORTED table):
 *   1. row = getCachedNodes(s.id, af, KAD_SEARCH_NODES): the indices kad_nc_closest_batch(nc, s.id, 14) gives, in walk
 *      order, each plus index_base; cnt their number.
 *   2. cnt == 0: the search is untouched (:1652-1656).
 *   3. otherwise s.insertNode(x_j, now, empty token) for j = 0 .. cnt-1 in order, x_j the ID of row[j], with node
 *      identity = ID (dht.cpp:961-1047):
 *        found   a member has x_j's ID: false, nothing changes (:972-984);
 *        trim    t and full as kad_search_trim; full and t < n cuts the list to t entries even when the candidate is
 *                then refused; full and insert position >= t refuses (:1009-1013);
 *        insert  at the position found by the strict 160-bit XOR-distance compare, flag byte 0 (a getCachedNodes
 *                result is not expired, and `candidate` is false);
 *        flip    an expired search becomes live and nothing is popped by this call (:1026-1029);
 *        pops    a live search pops from the back while more than 14 entries are not KAD_SN_BAD (:1031-1035);
 *        erase   removeExpiredNode(now) after every insert (:1044-1045, dht.h:628-640): the entry with the greatest
 *                index that carries KAD_SN_REMOVABLE goes.
 *   4. the record and slab of s are rewritten: list, KAD_SR_EXPIRED, n, t, full and the threshold entry[t-1] are what
 *      kad_searches_create derives from the new list, so verdicts and exports cannot tell a refilled set from a new one.
 * KAD_SN_REMOVABLE = node->isExpired() && node->time + NODE_EXPIRE_TIME < now, evaluated by the host for the refill's
 * `now`; it rides in the flag byte, which create, patch and export pass through unchanged. The searches of a batch
 * are distinct, the NodeCache snapshot is not changed, and getCachedNodes returns no expired node, so node.time = now
 * changes no test in another search: the batch gives the sequential result. node.time on the RoutingTable copy is
 * reported by the host (kad_table_patch_times).
 * A list may not outgrow its slab: a search whose list would hold more than cap entries after some insertNode of its
 * row returns gets KAD_SR_REFILL_OVERFLOW, is left byte for byte as it was, and its inserted mask is 0 (row and cnt
 * are still written); the host runs the walk from the row and grows the slabs (kad_searches_apply with new_cap).
 * Host arrays, synchronous; as kad_searches_patch towards queries (it first waits for all device work enqueued before
 * the call). which: m search indices, strictly ascending, < S. out_rows: m x KAD_SEARCH_NODES, padded with KAD_NO_NODE,
 * may be NULL; out_cnt m bytes; out_inserted m words of 16 bits, bit j = insertNode(row[j]) returned true; out_status m
 * bytes. Checked in this order, before any device work: NULL ss / nc; NULL which / out_cnt / out_inserted / out_status
 * with m > 0; which not strictly ascending or not < S (all KAD_ERR_INVALID); nc without KAD_TABLE_SORTED
 * (KAD_ERR_NOT_SORTED); nc on another device than ss (KAD_ERR_INVALID); m == 0 (KAD_OK); then a set whose cap exceeds
 * 64, the lanes of the wave that holds a list (KAD_ERR_UNSUPPORTED). Every failure reported before the refill kernel
 * runs (these checks, out of host or device memory, a failed upload or launch) leaves the set unchanged; past it only a
 * HIP error of the copy back remains (KAD_ERR_HIP: the device is then in error). One wave per
 * search, one list entry per lane; the scratch is allocated per call. */
#define KAD_SN_REMOVABLE 0x02u        /* node flag: removeExpiredNode(now) would erase this entry */
#define KAD_SR_REFILL_OK 0u
#define KAD_SR_REFILL_OVERFLOW 1u
int kad_sr_refill(kad_searches* ss, const kad_table* nc, uint32_t m, const uint32_t* which, uint32_t* out_rows,
                  uint8_t* out_cnt, uint16_t* out_inserted, uint8_t* out_status);
/* Measurement aid (tools/refill_bench.py), not part of the refill interface: the device time of the refill kernel of
 * the last kad_sr_refill on this set, in milliseconds, from two events the call records around it (0 before the first). */
int kad_sr_refill_kernel_ms(const kad_searches* ss, float* out_ms);

/* ---- Search::insertNode over a set of live searches, candidates of the caller (dht.cpp:961-1047) ---- */
/* For each listed search s = which[i], s.insertNode(x, now, empty token) on its candidates x = entries off[i] ..
 * off[i+1] of cand_ids, in list order, with node identity = ID: found, trim, insert, flip, pops and erase exactly as
 * spelled out above kad_sr_refill (the trim cuts the list even when the candidate is then refused), and, because a
 * candidate may be expired (cand_flags & KAD_SN_BAD = node->isExpired()):
 *   - the new entry's flag byte is cand_flags & KAD_SN_BAD; it never carries KAD_SN_REMOVABLE (node.time = now precedes
 *     removeExpiredNode);
 *   - on an expired search a candidate that is not BAD flips it to live and nothing is popped (:1026-1029); a BAD
 *     candidate does not flip it: `bad` stays 0 and the pop loop cuts the list to 14 entries;
 *   - on a live search the pop loop stops at the 15th entry that is not BAD, a BAD candidate counting as bad.
 * The same ID may appear twice in one list: the second occurrence is found and answers 0. Afterwards the record and
 * slab of s are what kad_searches_create derives from the new list (n, t, full, the threshold, KAD_SR_EXPIRED, zeros
 * past n). The KAD_SN_REMOVABLE bits of the set are the caller's, evaluated at the call's `now`; a candidate whose own
 * node is removable at `now` and a member of another search is the caller's to order (its node.time = now clears that
 * bit there).
 * A search whose list would hold more than cap entries after some insertNode returns gets KAD_SR_INSERT_OVERFLOW, is
 * left byte for byte as it was, and all its out_inserted bytes are 0; the other searches of the call are unaffected.
 * Host arrays, synchronous; as kad_sr_refill towards queries (it first waits for all device work enqueued before the
 * call). which: m search indices, strictly ascending, < S. off: m + 1 CSR offsets, off[0] == 0, not descending; an
 * empty list leaves its search untouched with status OK. cand_ids: 20 bytes per candidate. cand_flags: one byte per
 * candidate, only KAD_SN_BAD, NULL = all zero. out_inserted: one byte per candidate, 1 if that insertNode returned
 * true. out_status: one byte per listed search. Checked in this order, before any device work, every failure leaving
 * the set unchanged: NULL ss; NULL which / off / out_status with m > 0; NULL cand_ids / out_inserted with off[m] > 0;
 * which not strictly ascending or not < S; off[0] != 0, off descending or off[m] >= 0x7FFFFFFF; a flag byte with bits
 * other than KAD_SN_BAD (all KAD_ERR_INVALID); m == 0 (KAD_OK); cap > 64 (KAD_ERR_UNSUPPORTED). One wave per search,
 * one list entry per lane; the scratch is allocated per call. */
#define KAD_SR_INSERT_OK 0u
#define KAD_SR_INSERT_OVERFLOW 1u
int kad_sr_insert(kad_searches* ss, uint32_t m, const uint32_t* which, const uint32_t* off, const uint8_t* cand_ids,
                  const uint8_t* cand_flags, uint8_t* out_inserted, uint8_t* out_status);
/* Measurement aid (tools/sr_insert_bench.py), as kad_sr_refill_kernel_ms: the device time of the insert kernel of the
 * last kad_sr_insert on this set, in milliseconds (0 before the first). */
int kad_sr_insert_kernel_ms(const kad_searches* ss, float* out_ms);

/* ---- A whole tick of Dht::trySearchInsert on the device set (dht.cpp:816-849) ---- */
/* One round's host plan, without a device (as kad_search_trim): the verdicts lb / fwd / back / stop of the r candidates
 * that remain, in arrival order, plus trim[k]: bit 0 = the forward stopper refused as FAR or FAR_EXPIRED and holds
 * entries past its trim position (full && t < n: the refusal still cuts its list), bit 1 = the same for the backward
 * stopper. A candidate probes T = [lb-back-1, lb+fwd] without the ends whose stop is KAD_SR_STOP_END.
 *   KAD_SR_PLAN_SKIPPED   fwd + back == 0, both stops END or FAR, neither stopper trims: final, nothing to apply
 *   KAD_SR_PLAN_READY     T meets no T of an earlier candidate that was not skipped and does not lie on the open side of
 *                         an earlier deferred one; its pairs may be applied now, in any order with the other ready ones
 *   KAD_SR_PLAN_DEFERRED  everything else: it waits for the next round's verdicts. With a forward stop KNOWN or
 *                         FAR_EXPIRED (stops an earlier insert can undo) it blocks every search from its lowest probed
 *                         index upwards, with such a backward stop every search from its highest probed index downwards.
 * out_kind: r bytes. The pairs of the ready candidates, ascending by search: out_pair_which (the search), out_pair_cand
 * (the candidate's position k in the round) and out_pair_want (1 for an accepting search, 0 for a stopper that trims),
 * room for S each; no two pairs share a search. KAD_ERR_INVALID: a NULL array that is needed, a stop code above 3, a
 * verdict that reaches outside the S searches. */
#define KAD_SR_PLAN_SKIPPED 0u
#define KAD_SR_PLAN_READY 1u
#define KAD_SR_PLAN_DEFERRED 2u
int kad_sr_plan_round(uint32_t S, uint32_t r, const uint32_t* lb, const uint32_t* fwd, const uint32_t* back,
                      const uint8_t* stop, const uint8_t* trim, uint8_t* out_kind, uint32_t* out_pair_which,
                      uint32_t* out_pair_cand, uint8_t* out_pair_want, uint32_t* out_n_pairs);

/* Dht::trySearchInsert of the q candidates cand_ids, in arrival order, applied to the device set in one call:
 * cand_flags & KAD_SN_BAD = node->isExpired(), NULL = all zero. The candidate IDs are uploaded once. Then rounds: the
 * verdict kernel over the candidates that remain (the walk of kad_sr_try_insert_batch plus the two trim bits read from
 * the stoppers' records), the verdicts copied back, kad_sr_plan_round's plan, the pairs of the ready candidates uploaded
 * as (search, candidate position), the candidates' IDs and BAD bits gathered on the device and kad_sr_insert's kernel
 * run over them, one candidate per listed search, and the result bytes copied back. Nothing of size S crosses the bus.
 * Every result byte is compared with the plan's expectation; a disagreement on a search that did not overflow ends the
 * call with KAD_ERR_HIP, the rounds already applied staying described by the outputs.
 *   out_kind[j]   KAD_SR_TICK_*; for SKIPPED and APPLIED candidates out_round[j] is the round (from 1) that decided it
 *                 and out_lb / out_fwd / out_back / out_stop / out_trim[j] that round's verdict. For LEFT candidates
 *                 these are unspecified.
 *   replay        the host replays the APPLIED candidates on its own lists in (round, position) order: insertNode on
 *                 [lb, lb+fwd] forwards and [lb-back-1, lb) backwards until the refusal the verdict names (a stopper
 *                 whose trim bit is set is cut by it). Its searches then equal those of q sequential calls.
 *   overflow      a pair whose search would outgrow its slab leaves that search untouched on the device
 *                 (KAD_SR_INSERT_OVERFLOW); the search goes into out_overflow (ascending, distinct, room for S), its
 *                 candidate stays APPLIED, the round is finished and the call stops: everything not decided yet is LEFT.
 *                 The host replays as usual and patches the listed searches from its lists (kad_searches_patch, after
 *                 kad_searches_apply with a larger cap where a list no longer fits).
 * The call ends when no candidate remains, after max_rounds rounds (0: no limit) or after a round with an overflow. LEFT
 * candidates may precede APPLIED ones; walking them on the host afterwards, in order, is exact, because a ready candidate
 * never touches what an earlier waiting one can reach. Precondition, as for kad_sr_insert: the set's KAD_SN_REMOVABLE
 * bits are those of the tick's `now`, and no candidate's own node is removable at `now` (such a candidate is a barrier:
 * the caller cuts the tick there).
 * Host arrays, synchronous; as kad_sr_insert towards queries (it first waits for all device work enqueued before the
 * call). Checked in this order, before any device work, every failure leaving the set unchanged: NULL ss; NULL cand_ids
 * or per-candidate output with q > 0; NULL out_overflow or out_n_overflow; a flag byte with bits other than KAD_SN_BAD
 * (all KAD_ERR_INVALID); q == 0 or S == 0 (KAD_OK: every candidate SKIPPED in round 0 with lb = fwd = back = stop =
 * trim = 0, no device work); cap > 64 (KAD_ERR_UNSUPPORTED). Out of host or device memory: KAD_ERR_NOMEM. The device
 * scratch is one allocation per call. out_stats (may be NULL): the rounds run, the candidates by kind, the pairs
 * applied, the searches that overflowed, and the device time of the verdict kernels and of the gather and insert kernels,
 * summed over the rounds. */
#define KAD_SR_TICK_LEFT 0u      /* not handled: ask again or walk it on the host */
#define KAD_SR_TICK_SKIPPED 1u   /* refused as too far by both neighbours, nothing trimmed: final */
#define KAD_SR_TICK_APPLIED 2u   /* its verdict was applied to the device set in round out_round[j] */
typedef struct {
    uint32_t rounds, skipped, applied, left, pairs, overflowed;
    float verdict_ms, insert_ms;
} kad_sr_tick_stats;
int kad_sr_try_insert_tick(kad_searches* ss, const uint8_t* cand_ids, const uint8_t* cand_flags, uint32_t q,
                           uint32_t max_rounds /* 0: no limit */,
                           uint8_t* out_kind, uint32_t* out_round, uint32_t* out_lb, uint32_t* out_fwd,
                           uint32_t* out_back, uint8_t* out_stop, uint8_t* out_trim,
                           uint32_t* out_overflow /* room for S */, uint32_t* out_n_overflow,
                           kad_sr_tick_stats* out_stats /* may be NULL */);

/* ---- Node status changes over a set of live searches (SearchNode::isBad dht.cpp:458-460, Node::setExpired) ---- */
/* The reference keeps no flag byte: isBad() reads the shared Node, so one setExpired() after a timed-out request, one
 * reply (expired_ = false) or ten minutes passing for an expired node changes KAD_SN_BAD / KAD_SN_REMOVABLE in every
 * search that holds the node. kad_sr_mark_nodes carries such changes to the device set without the host knowing the
 * holders and without an upload of their lists. Node identity is the 20-byte ID.
 *   node ops   for every search s and every entry e < n of its list whose ID equals node_ids[j], the flag byte becomes
 *              (f & ~clear_bits[j]) | set_bits[j].
 *   pairs      then, for every pair k whose search pair_which[k] holds pair_ids[k], the flag byte becomes exactly
 *              pair_flags[k] (the per-search `candidate` bit, dht.cpp:1038, 1109, which no node op can express). A pair
 *              that is not found changes nothing and reports 0.
 *   fix-up     every search with at least one flag byte that differs from before the call is changed: its record is
 *              rewritten to what kad_searches_create derives from the same list with the new flag bytes. n, the order,
 *              the IDs and KAD_SR_EXPIRED are untouched; only t, full and the threshold can move. Nothing is trimmed,
 *              popped or erased (the reference does that on the next insertNode). An expired search's record does not
 *              depend on the flag bytes; it is still reported as changed. A search that is hit but whose bytes all stay
 *              equal is counted in out_hits, is not in out_changed, and none of its device bytes is written.
 * out_hits[j]: the searches whose list holds node j. out_pair_found[k]: 1 if the pair was found. out_changed[0 ..
 * *out_n_changed): the changed searches, ascending; room for S indices. out_counts[4k ..] belongs to out_changed[k]: n,
 * Search::getNumberOfBadNodes(), getNumberOfConsecutiveBadNodes() (dht.cpp:583-597) and the record's bits (1 = full,
 * 2 = expired); room for S x 4 bytes. From these the host reads searchStep's expiry test, lead_bad >= min(n,
 * SEARCH_MAX_BAD_NODES) (:1451), and the refill test, n - bad < SEARCH_NODES (:1354), without touching its lists; the
 * search-level expire() itself stays with kad_searches_patch / kad_searches_apply. Padding slots at or past n never
 * match, whatever the batch holds.
 * Host arrays, synchronous; it first waits for all device work enqueued before the call, uploads its arguments as one
 * copy and reads its outputs back as one (a second one only when more than 2q + p + 64 searches changed). node_ids:
 * q x 20 B, any order, distinct. clear_bits / set_bits: q bytes each, NULL = all zero. Checked in this order, before
 * any device work, every failure leaving the set unchanged: NULL ss, out_changed or out_n_changed; NULL node_ids with
 * q > 0; NULL pair_which / pair_ids / pair_flags with p > 0; a bit other than KAD_SN_BAD | KAD_SN_REMOVABLE in
 * clear_bits, set_bits or pair_flags; clear_bits[j] & set_bits[j] != 0; two equal node IDs; pair_which[k] >= S; two
 * equal (search, ID) pairs (all KAD_ERR_INVALID); q > KAD_SR_MARK_MAX_NODES; cap > 64 (both KAD_ERR_UNSUPPORTED);
 * q == 0 and p == 0, or S == 0 (KAD_OK, *out_n_changed = 0, hits and found zeroed). Equal node IDs are found by sorting,
 * so the limit on q answers only after the batch was sorted: a q beyond what the host can allocate for that (about 30
 * bytes per node) answers KAD_ERR_NOMEM instead of KAD_ERR_UNSUPPORTED. The dirty bitmap and the changed
 * list are scratch of the handle, allocated by the first call that reaches the device and counted in
 * kad_searches_info's device_bytes from then on. */
#define KAD_SR_MARK_MAX_NODES (1u << 20)
int kad_sr_mark_nodes(kad_searches* ss,
                      uint32_t q, const uint8_t* node_ids,
                      const uint8_t* clear_bits, const uint8_t* set_bits,
                      uint32_t p, const uint32_t* pair_which, const uint8_t* pair_ids, const uint8_t* pair_flags,
                      uint32_t* out_hits, uint8_t* out_pair_found, uint32_t* out_changed, uint8_t* out_counts,
                      uint32_t* out_n_changed);
/* Measurement aid (tools/sr_mark_bench.py), as kad_sr_insert_kernel_ms: the device times of the scan kernel and of the
 * fix kernel of the last kad_sr_mark_nodes on this set, in milliseconds (0 before the first). */
int kad_sr_mark_kernel_ms(const kad_searches* ss, float* out_scan_ms, float* out_fix_ms);

/* ---- Dht::searchStep over a set of live searches (dht.cpp:1344-1464) ---- */
/* Step bits of a member's flag byte, beside KAD_SN_BAD and KAD_SN_REMOVABLE. Like KAD_SN_REMOVABLE the caller maintains
 * them for the tick's `now`; create, patch, export, kad_searches_apply, kad_sr_refill and kad_sr_insert carry a member's
 * whole byte, so they travel with their entry. A fresh entry written by insertNode (cand_flags & KAD_SN_BAD) reads
 * correctly with all of them zero.
 *   KAD_SN_CANDIDATE  SearchNode::candidate (dht.cpp:270). An entry carrying it also carries KAD_SN_BAD (isBad, :458-460).
 *   KAD_SN_PENDING    pending(getStatus) (:392-397): some get request to this node is in flight.
 *   KAD_SN_SYNCED     SearchNode::isSynced(now) (:279-282).
 *   KAD_SN_NOGET      canGet(now, up, query) (:302-324) is false for a reason other than the node being expired, for the
 *                     query the search's next searchSendGetValues asks with: the first callback's query, or the default
 *                     find_node query when there are no callbacks.
 * An entry is gettable when !(f & NOGET) && (!(f & BAD) || (f & CANDIDATE)). An entry with CANDIDATE whose node is
 * expired must also carry NOGET (canGet refuses an expired node, and BAD alone no longer says so). SYNCED and the time
 * clause of canGet both flip at last_get_reply + NODE_EXPIRE_TIME without any event: keeping those deadlines, and
 * sending the change with kad_sr_mark_entries when one passes, is the host's job, as for KAD_SN_REMOVABLE.
 * A *pair* of kad_sr_mark_nodes writes the exact byte, of KAD_SN_BAD | KAD_SN_REMOVABLE only, and therefore clears the
 * entry's step bits; its node ops touch only the two bits they name and keep them. */
#define KAD_SN_CANDIDATE 0x04u
#define KAD_SN_PENDING 0x08u
#define KAD_SN_SYNCED 0x10u
#define KAD_SN_NOGET 0x20u
/* Sets and clears step bits of single entries: for every pair k whose search pair_which[k] holds pair_ids[k] among its n
 * entries, the flag byte becomes (f & ~clear_bits[k]) | set_bits[k]; out_found[k] (may be NULL) = 1 if it was found, else
 * 0 and nothing changes. Only the four step bits (0x3C) may be named: KAD_SN_BAD and KAD_SN_REMOVABLE move the record and
 * stay with kad_sr_mark_nodes; no record is rewritten here. Padding slots at or past n never match.
 * Host arrays, synchronous; as kad_sr_mark_nodes towards queries (it first waits for all device work enqueued before the
 * call). pair_ids: p x 20 B. clear_bits / set_bits: p bytes each, NULL = all zero. Checked in this order, before any
 * device work, every failure leaving the set unchanged: NULL ss; NULL pair_which / pair_ids with p > 0; a bit outside
 * 0x3C in clear_bits or set_bits; clear_bits[k] & set_bits[k] != 0; pair_which[k] >= S; two equal (search, ID) pairs (all
 * KAD_ERR_INVALID); p == 0 or S == 0 (KAD_OK); cap > 64 (KAD_ERR_UNSUPPORTED). */
int kad_sr_mark_entries(kad_searches* ss, uint32_t p, const uint32_t* pair_which, const uint8_t* pair_ids,
                        const uint8_t* clear_bits, const uint8_t* set_bits, uint8_t* out_found);

/* Mode byte of a stepped search. */
#define KAD_STEP_APPLY 0x01u           /* kad_sr_step writes the sends and the expiry to the device set */
#define KAD_STEP_NO_SEND 0x02u         /* no get request is sent (the caller paces this search) */
#define KAD_STEP_DONE_IF_SYNCED 0x04u  /* no callbacks, announces or listeners: a synced search is set done (:1434) */
#define KAD_STEP_NO_EXPIRE 0x08u       /* with APPLY: KAD_STEP_EXPIRE is reported, the search is left as it is */
/* Result bits of a stepped search. */
#define KAD_STEP_SKIPPED 0x01u    /* KAD_SR_EXPIRED: searchStep returns at :1346; no other bit is set */
#define KAD_STEP_SHORT 0x02u      /* n - bad < KAD_SEARCH_NODES: the refill test of :1354 without refill_time */
#define KAD_STEP_SYNCED 0x04u     /* Search::isSynced (:1467-1478) */
#define KAD_STEP_DONE 0x08u       /* synced under KAD_STEP_DONE_IF_SYNCED: setDone, nothing is sent */
#define KAD_STEP_EXHAUSTED 0x10u  /* the send loop ended for want of a gettable node, not at 4 requests */
#define KAD_STEP_EXPIRE 0x20u     /* lead_bad >= min(n, SEARCH_MAX_BAD_NODES = 25) (:1451-1452) */
typedef struct {
    uint64_t picks;   /* bit e: entry e of the list gets a request */
    uint32_t counts;  /* n | bad << 8 | lead_bad << 16 | solicited << 24 */
    uint32_t bits;    /* KAD_STEP_SKIPPED .. KAD_STEP_EXPIRE */
} kad_step_out;
/* searchStep's decision on one list, on the host without a device (as kad_search_trim), from the n <= 64 flag bytes,
 * search_flags & KAD_SR_EXPIRED and the mode, all from the list as it stands at the call:
 *   skipped   a search with KAD_SR_EXPIRED: bits = KAD_STEP_SKIPPED, no picks; the counts are still filled.
 *   counts    bad = entries with BAD; lead_bad = leading BAD entries; solicited = entries with !BAD && PENDING
 *             (:514-520, :583-597), the latter as it is after the picks.
 *   short     n - bad < KAD_SEARCH_NODES. refill_time stays with the host; a caller that refills does so with
 *             kad_sr_refill before the step, as the reference does.
 *   synced    over the entries that are not BAD, in order: false at the first one without SYNCED among the first 8; true
 *             only if there is at least one.
 *   picks     the loop of :1438-1446 over searchSendGetValues (:1171-1196). None if solicited >= 4, if the mode has
 *             KAD_STEP_NO_SEND, or if the search is synced and the mode has KAD_STEP_DONE_IF_SYNCED (KAD_STEP_DONE).
 *             Otherwise the gettable entries in list order; a picked entry that is not BAD raises solicited unless it was
 *             PENDING already (a request for another query is in flight: currentlySolicitedNodeCount counted it before),
 *             and the loop ends right after the pick that brings it to 4. Picked candidates (BAD) and such PENDING
 *             entries do not count, so more than four entries can be picked. With room = 4 - solicited and gg = the
 *             gettable entries that are neither BAD nor PENDING: gg has fewer than room entries: every gettable entry is
 *             picked and KAD_STEP_EXHAUSTED is set (the host goes on with its further callbacks' queries); otherwise the
 *             gettable entries up to and including the room-th of gg.
 *   expire    evaluated after the sends, which do not change BAD; independent of DONE and NO_SEND. An empty live search
 *             expires, as in the reference.
 * KAD_STEP_APPLY and KAD_STEP_NO_EXPIRE do not change the answer. NULL node_flags with n > 0, NULL out, n > 64 or a
 * mode bit outside the four: KAD_ERR_INVALID (kad_last_error is not set: the function lives outside the engine). */
int kad_search_step(uint32_t n, const uint8_t* node_flags, uint32_t search_flags, uint32_t mode, kad_step_out* out);
/* kad_search_step on m lists in CSR form (off[m + 1] into node_flags; search_flags and mode m bytes each, NULL = all
 * zero), also on the host without a device: what a caller without a device set, or a test, steps its lists with. NULL
 * off or out, NULL node_flags with off[m] > 0, offsets descending, a list longer than 64 entries or a mode bit outside
 * the four: KAD_ERR_INVALID, before anything is written. m == 0 reads nothing. */
int kad_search_step_batch(uint32_t m, const uint32_t* off, const uint8_t* node_flags, const uint8_t* search_flags,
                          const uint8_t* mode, kad_step_out* out);
typedef struct {
    uint32_t synced, expired, skipped, picks;  /* searches with SYNCED, EXPIRE, SKIPPED; entries picked */
    float kernel_ms;                           /* the call's kernels, between two events of the handle */
} kad_sr_step_stats;
/* kad_search_step over the device set: out[k] is the step of search which[k] (which == NULL: every search, out[k] that
 * of search k, and m must be S) under mode[k] (NULL: all 0). which is strictly ascending and < S. A search whose mode
 * lacks KAD_STEP_APPLY is only read. With KAD_STEP_APPLY the outcome is written in place:
 *   sends     every picked entry gets KAD_SN_PENDING | KAD_SN_NOGET: its getStatus[query] is now a pending request, so
 *             canGet is false for that query.
 *   expiry    a search with KAD_STEP_EXPIRE (and a mode without KAD_STEP_NO_EXPIRE) becomes what Search::expire()
 *             (:649-653) leaves: KAD_SR_EXPIRED set and the list empty, its record and slab byte for byte what
 *             kad_searches_create derives for an empty expired list (keys, tails and flags zero; n, t, full and threshold
 *             zero). Its picks are still reported, because the reference sends before it expires.
 * The requests themselves, listen and announce, callbacks and the scheduler stay with the host, which holds the same
 * lists in the same order. Host arrays, synchronous; as kad_sr_insert towards queries (it first waits for all device
 * work enqueued before the call). A call in which no search has KAD_STEP_APPLY writes no byte of the set. Checked in this
 * order, before any device work, every failure leaving the set unchanged: NULL ss or out; which == NULL with m != S;
 * which not strictly ascending or not < S; a mode bit outside the four (all KAD_ERR_INVALID); m == 0 (KAD_OK);
 * cap > 64 (KAD_ERR_UNSUPPORTED). Out of host or device memory: KAD_ERR_NOMEM. One lane per search; the scratch is one
 * allocation per call. out_stats may be NULL. */
int kad_sr_step(kad_searches* ss, uint32_t m, const uint32_t* which /* NULL: every search */,
                const uint8_t* mode /* m bytes, NULL: all 0 */, kad_step_out* out, kad_sr_step_stats* out_stats);

/* ---- The whole searchStep: the listen and announce sends beside the get requests ---- */
/* The two remaining bits of a member's flag byte. The caller maintains them for the tick's `now`, as it does
 * KAD_SN_SYNCED, KAD_SN_NOGET and KAD_SN_REMOVABLE; they ride where the four step bits ride and travel with their entry.
 *   KAD_SN_LISTEN_DUE    some listener l of the search has n.getListenTime(l.query) <= now (dht.cpp:447-453)
 *   KAD_SN_ANNOUNCE_DUE  some announce a of the search has n.getAnnounceTime(a.value->id) <= now (:431-441)
 * Both flip on events (a reply, a new listener or announce) and at deadlines the host keeps: reply_time +
 * LISTEN_EXPIRE_TIME - REANNOUNCE_MARGIN and acked.second - REANNOUNCE_MARGIN. They do not depend on KAD_SN_SYNCED: the
 * loops test isSynced themselves. All-zero on a fresh entry is conservative: nothing is sent until the caller marks it.
 * A pair of kad_sr_mark_nodes clears them with the step bits. Bits are read literally: an entry with KAD_SN_SYNCED and
 * KAD_SN_BAD but without KAD_SN_CANDIDATE is the caller's inconsistency, and nothing is repaired. */
#define KAD_SN_LISTEN_DUE 0x40u
#define KAD_SN_ANNOUNCE_DUE 0x80u
/* kad_sr_mark_entries for the two due bits: the same contract and the same checks in the same order, with the mask 0xC0
 * in place of 0x3C (a step bit named here is KAD_ERR_INVALID, as a due bit is there). */
int kad_sr_mark_due(kad_searches* ss, uint32_t p, const uint32_t* pair_which, const uint8_t* pair_ids,
                    const uint8_t* clear_bits, const uint8_t* set_bits, uint8_t* out_found);

/* Further mode bits, for kad_search_step_full[_batch] and kad_sr_step_full only (the calls above refuse them). */
#define KAD_STEP_LISTEN 0x10u        /* the search's listeners are not empty: the listen loop of :1384-1428 runs */
#define KAD_STEP_ANNOUNCE 0x20u      /* its announces are not empty: searchSendAnnounceValue (:1237-1339) runs */
#define KAD_STEP_PROBE_BLOCKS 0x40u  /* the probe query Select{Id, SeqNum} satisfies the search's get query, so a probed
                                      * node cannot get (pending_sq_status): announce picks also count as NOGET */
typedef struct {
    uint64_t picks;     /* bit e: entry e gets a get request, as kad_step_out */
    uint64_t listen;    /* bit e: entry e gets the listen requests that are due on it */
    uint64_t announce;  /* bit e: entry e gets the announce probe */
    uint32_t counts;    /* n | bad << 8 | lead_bad << 16 | solicited << 24, solicited after all three loops */
    uint32_t bits;      /* KAD_STEP_SKIPPED .. KAD_STEP_EXPIRE */
} kad_step_full_out;
/* kad_search_step with the two send loops that precede the get loop, from the list as it stands at the call:
 *   skipped   as kad_search_step; the three masks are zero.
 *   listen    only if the search is synced and the mode has KAD_STEP_LISTEN. The entries in order; one without SYNCED is
 *             passed over and not counted; a synced one is picked if it has LISTEN_DUE; every synced entry without
 *             CANDIDATE counts towards LISTEN_NODES = 4, picked or not, and the walk ends after the fourth.
 *   announce  only if the search is synced and the mode has KAD_STEP_ANNOUNCE. An entry is picked if it has SYNCED and
 *             ANNOUNCE_DUE; only picked entries without CANDIDATE count towards TARGET_NODES = 8, and the walk ends after
 *             the eighth.
 *   picks     kad_search_step's, on the list with every announce pick made PENDING (the probe is a get request and is
 *             counted by currentlySolicitedNodeCount) and, under KAD_STEP_PROBE_BLOCKS, NOGET. KAD_STEP_NO_SEND concerns
 *             this loop only. solicited is the value after all three loops.
 * A mode without KAD_STEP_LISTEN and KAD_STEP_ANNOUNCE gives kad_search_step's picks, counts and bits and zero listen and
 * announce masks. KAD_ERR_INVALID as kad_search_step, and for: a mode bit outside the seven (0x80); KAD_STEP_DONE_IF_SYNCED
 * with KAD_STEP_LISTEN or KAD_STEP_ANNOUNCE (it means "no listeners, no announces"); KAD_STEP_PROBE_BLOCKS without
 * KAD_STEP_ANNOUNCE. */
int kad_search_step_full(uint32_t n, const uint8_t* node_flags, uint32_t search_flags, uint32_t mode,
                         kad_step_full_out* out);
/* kad_search_step_full on m lists in CSR form, as kad_search_step_batch. */
int kad_search_step_full_batch(uint32_t m, const uint32_t* off, const uint8_t* node_flags, const uint8_t* search_flags,
                               const uint8_t* mode, kad_step_full_out* out);
typedef struct {
    uint32_t synced, expired, skipped;    /* searches with SYNCED, EXPIRE, SKIPPED */
    uint32_t picks, listens, announces;   /* entries picked by the get loop, the listen loop, the announce loop */
    float kernel_ms;                      /* the call's kernels, between two events of the handle */
} kad_sr_step_full_stats;
/* kad_search_step_full over the device set, with kad_sr_step's contract: which (NULL: every search, m must be S),
 * strictly ascending and < S; mode NULL: all 0; a search whose mode lacks KAD_STEP_APPLY is only read, and a call in which
 * none has it writes no byte of the set. With KAD_STEP_APPLY each picked entry's byte f becomes
 *   (f | PENDING where picks | announce | NOGET where picks, and where announce under PROBE_BLOCKS)
 *     & ~LISTEN_DUE where listen & ~ANNOUNCE_DUE where announce:
 * after sendListen every listener's getListenTime on that node is max, and with the probe pending getAnnounceTime is max
 * for every value. A search with KAD_STEP_EXPIRE (mode without KAD_STEP_NO_EXPIRE) becomes an empty expired search as
 * with kad_sr_step; its three masks are still reported, because the reference sends before it expires.
 * isDone(get) and checkAnnounced of :1359-1376, getNextStepTime, the requests themselves, callbacks and the scheduler
 * stay with the host. Host arrays, synchronous, as kad_sr_step towards queries. Checked in this order, before any device
 * work, every failure leaving the set unchanged: NULL ss or out; which == NULL with m != S; which not strictly ascending
 * or not < S; an invalid mode (bit 0x80, DONE_IF_SYNCED with LISTEN or ANNOUNCE, PROBE_BLOCKS without ANNOUNCE) (all
 * KAD_ERR_INVALID); m == 0 (KAD_OK); cap > 64 (KAD_ERR_UNSUPPORTED). Out of host or device memory: KAD_ERR_NOMEM. One
 * lane per search; the scratch is one allocation per call. out_stats may be NULL. */
int kad_sr_step_full(kad_searches* ss, uint32_t m, const uint32_t* which /* NULL: every search */,
                     const uint8_t* mode /* m bytes, NULL: all 0 */, kad_step_full_out* out,
                     kad_sr_step_full_stats* out_stats);

/* Per-query family select for NodeCache::getCachedNodes(id, sa_family, count) (node_cache.cpp:36-66:
 * cache_4 or cache_6 by family; Dht::refill asks the search's family, dht.cpp:1650): af[i] = 0 -> table4,
 * 1 -> table6 (KAD_TABLE_SORTED tables; either may be NULL = an empty map). Any count (as kad_nc_closest_batch).
 * Device pointers. */
int kad_nc_closest_batch_dual(const kad_table* table4, const kad_table* table6,
                              const uint8_t* targets, const uint8_t* af, uint32_t q, uint32_t count,
                              uint32_t* out_idx, uint8_t* out_cnt, void* stream);

/* ---- sharded table without halo: the north-star multi-GPU variant ----
 * A global uniform-depth table U(depth) (bucket b's first ID = global_base + b << (160-depth)) is
 * cut into contiguous bucket ranges, one table per GPU, with global node indices (index_base).
 * Every rank holds the global good prefix sums, computes each query's global window W(R)
 * (routing_table.cpp:89-104) and answers W(R) ∩ its shard for a replicated batch of targets:
 *   W(R) inside the shard -> a final row appended to one of KAD_SHARD_REGIONS regions of `rows`
 *                            (region r: row_cap rows at rows + r*row_cap*KAD_ROW_WORDS(count);
 *                            a row is qid, m, 0, 0, idx[count] padded to 4 words)
 *   W(R) crosses an edge  -> this shard's part appended to `parts` (KAD_PART_WORDS(count) each:
 *                            the row, then the entries' 160-bit XOR distances, 5 words each)
 *   W(R) misses the shard -> nothing (queries with a bucket outside [reach_lo, reach_hi) exit early;
 *                            reach must cover every bucket whose window can touch the shard).
 * counters (device, KAD_SHARD_COUNTERS x KAD_SHARD_COUNTER_STRIDE uint32, zeroed by the caller;
 * counter k at word k*KAD_SHARD_COUNTER_STRIDE): rows appended per region (k < 8), parts appended
 * (k = 8), overflow flag (k = 9: a region or the parts buffer was full: grow and run again).
 * Rows of the queries [QB w, QB w + QB) go to region w % 8 (QB = 1024, or 256 for counts 17..32; 2048 in a
 * tools-build A/B). A query takes at most two rows: a query whose window line cannot answer it leaves a tombstone row (qid
 * KAD_NO_NODE, skipped by every finish) beside its wave-path row or part, so row_cap >= 2*ceil(ceil(q/QB)/8)*QB
 * never overflows (home layout: W = ceil(ceil(q/256)/world/(QB/256)) + 1 workgroups per home range,
 * row_cap >= 2*ceil(W/8)*QB).
 * The ranks' rows and parts are all-gathered by the caller (RCCL); kad_rt_scatter_rows and
 * kad_rt_merge_parts (parts sorted by qid) then give every query's findClosestNodes result.
 * All pointers are device pointers; count in 1..KAD_MAX_COUNT. Queries far enough inside the shard
 * answer from the window lines of their count (counts 9..32: the 16/32-count sets, built on first
 * use as for kad_rt_closest_batch; kad_table_prepare builds them ahead of a stream capture). */
#define KAD_ROW_WORDS(count) (4u + (((count) + 3u) & ~3u))
#define KAD_PART_WORDS(count) (KAD_ROW_WORDS(count) + 5u * (count))
#define KAD_SHARD_REGIONS 8u
#define KAD_SHARD_COUNTERS 10u
#define KAD_SHARD_COUNTER_STRIDE 32u
int kad_rt_shard_batch(const kad_table* shard, const uint32_t* global_good_prefix, uint32_t global_buckets,
                       uint64_t global_base_hi, uint32_t depth, uint32_t shard_first_bucket,
                       uint32_t reach_lo, uint32_t reach_hi, const uint8_t* targets, uint32_t q,
                       uint32_t count, uint32_t* rows, uint32_t row_cap, uint32_t* parts,
                       uint32_t part_cap, uint32_t* counters, void* stream);
/* n_blocks row blocks (block r: n_rows[r * n_rows_stride] rows at rows + r*block_cap*KAD_ROW_WORDS)
 * -> out_idx[qid] / out_cnt[qid]. n_rows_stride 0 means 1 (gathered counts); pass
 * KAD_SHARD_COUNTER_STRIDE to scatter a single rank's regions straight from its counters. */
int kad_rt_scatter_rows(const uint32_t* rows, const uint32_t* n_rows, uint32_t n_rows_stride, uint32_t n_blocks,
                        uint32_t block_cap, uint32_t count, uint32_t* out_idx, uint8_t* out_cnt, int device,
                        void* stream);
/* n_parts partial rows sorted by qid -> the first min(count, sum of m) entries by (XOR distance,
 * global index) of each query (exact: parts come from disjoint buckets). */
int kad_rt_merge_parts(const uint32_t* parts, uint32_t n_parts, uint32_t count, uint32_t* out_idx,
                       uint8_t* out_cnt, int device, void* stream);
/* The device-only exchange step (no host read between the shard kernel, the collective and the merge,
 * so a step can be captured in a HIP graph). Every rank lays out ONE send block of
 * KAD_SHARD_BLOCK_WORDS(count, row_cap, part_cap) words and passes its pieces to kad_rt_shard_batch:
 *   rows     = block                                        (KAD_SHARD_REGIONS regions of row_cap rows)
 *   parts    = block + KAD_SHARD_REGIONS*row_cap*KAD_ROW_WORDS(count)      (part_cap partial rows)
 *   counters = parts + part_cap*KAD_PART_WORDS(count)       (zeroed before kad_rt_shard_batch)
 * The blocks of all `world` ranks are all-gathered in rank order (one fixed-size all_gather, RCCL)
 * into `recv`; kad_rt_gather_finish then writes every query's findClosestNodes row: complete rows
 * scattered by qid, the parts of edge-crossing windows merged by (XOR distance, global index).
 *   q        queries of the replicated batch (qids < q)
 *   scratch  device, q + world*part_cap words; its first q words must be KAD_NO_NODE (0xFFFFFFFF)
 *            before the first call, and every call leaves them so
 *   overflow device word: set to 1 (never cleared here) when any rank's region or part buffer was
 *            full, i.e. some rows are missing: grow row_cap / part_cap and run the batch again. A
 *            caller checks it once per batch or once per K steps.
 * world <= KAD_SHARD_MAX_WORLD. All pointers are device pointers; count in 1..KAD_MAX_COUNT. */
#define KAD_SHARD_MAX_WORLD 16u
#define KAD_SHARD_BLOCK_WORDS(count, row_cap, part_cap)                                                \
    ((uint64_t)KAD_SHARD_REGIONS * (row_cap) * KAD_ROW_WORDS(count) +                                  \
     (uint64_t)(part_cap) * KAD_PART_WORDS(count) + (uint64_t)KAD_SHARD_COUNTERS * KAD_SHARD_COUNTER_STRIDE)
int kad_rt_gather_finish(const uint32_t* recv, uint32_t world, uint32_t row_cap, uint32_t part_cap, uint32_t q,
                         uint32_t count, uint32_t* scratch, uint32_t* out_idx, uint8_t* out_cnt,
                         uint32_t* overflow, int device, void* stream);
/* The home-rank exchange (the default north-star step; the all-gather above moves every row to every rank).
 * Query block k (KAD_SHARD_QUERY_BLOCK queries of the replicated batch) has the home rank k * world / nblk:
 * kad_home_range gives rank r's queries [lo, hi). A rank's rows and parts go only to their query's home rank,
 * so one all_to_all of fixed-size blocks (RCCL) moves ~q/world rows into each rank instead of q:
 *   send     device, world blocks of KAD_SHARD_BLOCK_WORDS(count, row_cap, part_cap) words: block d holds what
 *            goes to rank d (its regions, parts and counters; the counters are zeroed by the call first)
 *   recv     after all_to_all_single(recv, send) with equal splits: block s = what rank s sent here
 * kad_rt_home_finish then writes rank `rank`'s rows: out_idx (hi - lo) x count and out_cnt (hi - lo) for qids
 * lo + i. scratch: H + world*part_cap words, H = the size of rank 0's range (the largest; the same for every rank,
 * so one scratch can serve the ranks of a step one after the other), the first H KAD_NO_NODE before the first call
 * (every call leaves them so). overflow: set to 1 when a block sent here was full; it only sees this rank's blocks, so
 * callers combine it over the ranks (all_reduce MAX) before deciding to grow and run again. */
#define KAD_SHARD_QUERY_BLOCK 256u
void kad_home_range(uint32_t q, uint32_t world, uint32_t rank, uint32_t* lo, uint32_t* hi);
int kad_rt_shard_batch_home(const kad_table* shard, const uint32_t* global_good_prefix, uint32_t global_buckets,
                            uint64_t global_base_hi, uint32_t depth, uint32_t shard_first_bucket, uint32_t reach_lo,
                            uint32_t reach_hi, const uint8_t* targets, uint32_t q, uint32_t count, uint32_t world,
                            uint32_t* send, uint32_t row_cap, uint32_t part_cap, void* stream);
int kad_rt_home_finish(const uint32_t* recv, uint32_t world, uint32_t rank, uint32_t row_cap, uint32_t part_cap,
                       uint32_t q, uint32_t count, uint32_t* scratch, uint32_t* out_idx, uint8_t* out_cnt,
                       uint32_t* overflow, int device, void* stream);
/* The same step without the counter-zeroing launch: kad_rt_shard_step_home is kad_rt_shard_batch_home on send blocks
 * whose counters are already zero (a zero-filled buffer, or the previous step's kad_rt_home_finish_reset);
 * kad_rt_home_finish_reset is kad_rt_home_finish that also zeroes the counters of the `world` send blocks in its last
 * launch (the exchange has delivered them by then). send must not be recv (at world 1 without a collective, use the
 * zeroing pair above). */
int kad_rt_shard_step_home(const kad_table* shard, const uint32_t* global_good_prefix, uint32_t global_buckets,
                           uint64_t global_base_hi, uint32_t depth, uint32_t shard_first_bucket, uint32_t reach_lo,
                           uint32_t reach_hi, const uint8_t* targets, uint32_t q, uint32_t count, uint32_t world,
                           uint32_t* send, uint32_t row_cap, uint32_t part_cap, void* stream);
int kad_rt_home_finish_reset(const uint32_t* recv, uint32_t* send, uint32_t world, uint32_t rank, uint32_t row_cap,
                             uint32_t part_cap, uint32_t q, uint32_t count, uint32_t* scratch, uint32_t* out_idx,
                             uint8_t* out_cnt, uint32_t* overflow, int device, void* stream);

#define KAD_ROUTE_PACKED 1u /* mode bits of kad_route_run / kad_route_pack_ex */
#define KAD_ROUTE_KEYS 2u
#define KAD_ROUTE_ZEROED 4u

/* ---- owner routing of a serving front end ----
 * The headline form shards the table by ID range, one GPU per range, and answers every query on the GPU owning its
 * target (the reference answers each request where it arrives: Dht::onFindNode / onGetValues, dht.cpp:3189-3217).
 * A front end spreading arbitrary targets over N GPUs sends each target to its owner and the rows back, as
 * all_to_all_single of fixed-size blocks (no host read per batch):
 * kad_route_pack: targets (device, q x 20 bytes) into `world` send blocks of `cap` records of 20 bytes (send:
 *   world * cap * 20 bytes): target i goes to block d = (byte 0 >> (8 - shard_bits)) % world (d = 0 when
 *   shard_bits = 0). A block is KAD_ROUTE_SUBS sub-blocks of cap / KAD_ROUTE_SUBS records (cap a multiple of
 *   KAD_ROUTE_SUBS): the targets of workgroup w (KAD_ROUTE_QPW queries) go to sub-block w % KAD_ROUTE_SUBS, so that
 *   the workgroups' appends spread over KAD_ROUTE_SUBS counters per block (one counter hit by every workgroup
 *   serialised them: 24 us against 15 per 1M targets). slot[i] = d * cap + its record (KAD_NO_NODE when its
 *   sub-block is full, which sets the sticky word ctr[KAD_ROUTE_OVERFLOW_WORD(world)]). ctr:
 *   KAD_ROUTE_CTR_WORDS(world) words, zeroed by the call; ctr[(d * KAD_ROUTE_SUBS + r) * KAD_ROUTE_CSTRIDE] ends as
 *   sub-block r of block d's record count (it may exceed its capacity). The order of the records inside a sub-block
 *   is unspecified; records past a sub-block's count are left as they were (the owner answers them too; their rows
 *   are never read back). targets, send, slot and ctr must be 4-byte aligned (KAD_ERR_INVALID otherwise). Async on
 *   stream.
 * kad_route_unpack: rows returned in the send layout (back_idx: world * cap rows of `count` uint32, back_cnt: world *
 *   cap bytes) back to each query's position: out_idx row i = back_idx row slot[i], out_cnt[i] = back_cnt[slot[i]]
 *   (KAD_NO_NODE and 0 for slot KAD_NO_NODE). Async on stream. All pointers are device pointers. */
#define KAD_ROUTE_CSTRIDE 32u
#define KAD_ROUTE_MAX_WORLD 16u
#define KAD_ROUTE_SUBS 8u
#define KAD_ROUTE_QPW 1024u
#define KAD_ROUTE_CTR_WORDS(world) (((world) * KAD_ROUTE_SUBS + 1u) * KAD_ROUTE_CSTRIDE)
#define KAD_ROUTE_OVERFLOW_WORD(world) ((world) * KAD_ROUTE_SUBS * KAD_ROUTE_CSTRIDE)
int kad_route_pack(const uint8_t* targets, uint32_t q, uint32_t world, uint32_t shard_bits, uint32_t cap,
                   uint8_t* send, uint32_t* slot, uint32_t* ctr, int device, void* stream);
/* kad_route_pack_keys: kad_route_pack with each record the target's top 64 bits as one native uint64 key (send_keys:
 * world * cap keys, 8-byte aligned) instead of its 20 bytes: owner routing's key-only exchange, 8 bytes per query on
 * the links instead of 20 (answered by kad_rt_closest_keys_packed). */
int kad_route_pack_keys(const uint8_t* targets, uint32_t q, uint32_t world, uint32_t shard_bits, uint32_t cap,
                        uint64_t* send_keys, uint32_t* slot, uint32_t* ctr, int device, void* stream);
/* kad_route_pack_ex: kad_route_pack / kad_route_pack_keys by `mode`: KAD_ROUTE_KEYS (8-byte key records),
 * KAD_ROUTE_ZEROED (ctr is already zero — kad_route_unpack_packed_fold of the buffer set's previous batch leaves it so
 * — and is not zeroed by the call: no memset before the kernel). */
int kad_route_pack_ex(const uint8_t* targets, uint32_t q, uint32_t world, uint32_t shard_bits, uint32_t cap, void* send,
                      uint32_t* slot, uint32_t* ctr, uint32_t mode, int device, void* stream);
int kad_route_unpack(const uint32_t* slot, uint32_t q, uint32_t count, const uint32_t* back_idx,
                     const uint8_t* back_cnt, uint32_t* out_idx, uint8_t* out_cnt, int device, void* stream);
/* Packed rows for the way back (count <= KAD_ROUTE_PACKED_MAX_COUNT): a row's indices lie in one window of the
 * sorted table, so they travel as word 0 = the row's smallest index (KAD_NO_NODE for an empty row) and one byte
 * per entry = the entry's index minus word 0 (0xFF past the row's count), KAD_ROUTE_PACKED_WORDS(count) words
 * (count 8: 12 bytes instead of 33).
 * kad_route_compress: n rows (idx: n x count uint32, cnt: n bytes, the send layout) -> packed (n x
 *   KAD_ROUTE_PACKED_WORDS(count) uint32). A row whose indices span more than 254 cannot be packed: it sets the
 *   sticky word *escape (not cleared by the call; kad_route_pack's ctr[KAD_ROUTE_OVERFLOW_WORD(world) + 1] is meant
 *   for it), and the caller runs the batch's way back unpacked.
 * kad_route_unpack_packed: as kad_route_unpack, from packed rows in the send layout. Async on stream. */
#define KAD_ROUTE_PACKED_MAX_COUNT 32u
#define KAD_ROUTE_PACKED_WORDS(count) (1u + ((count) + 3u) / 4u)
int kad_route_compress(const uint32_t* idx, const uint8_t* cnt, uint32_t n, uint32_t count, uint32_t* packed,
                       uint32_t* escape, int device, void* stream);
int kad_route_unpack_packed(const uint32_t* slot, uint32_t q, uint32_t count, const uint32_t* back_packed,
                            uint32_t* out_idx, uint8_t* out_cnt, int device, void* stream);
/* kad_route_unpack_packed_fold: kad_route_unpack_packed, and in the same launch the batch's counters folded and zeroed
 * for the next KAD_ROUTE_ZEROED pack: flags[0..2] |= ctr[KAD_ROUTE_OVERFLOW_WORD(world) + 0..2] (overflow, escape,
 * tail), flags[3] = max(flags[3], KAD_ROUTE_SUBS x the fullest sub-block count: the capacity the batch needed), then
 * ctr[0 .. KAD_ROUTE_CTR_WORDS(world)) = 0. q = 0: the fold and reset alone. */
int kad_route_unpack_packed_fold(const uint32_t* slot, uint32_t q, uint32_t count, const uint32_t* back_packed,
                                 uint32_t* out_idx, uint8_t* out_cnt, uint32_t* ctr, uint32_t world, uint32_t* flags,
                                 int device, void* stream);
/* kad_rt_closest_batch_packed: kad_rt_closest_batch with each row written packed (the layout above, word 0 a base
 * no larger than any entry) by the query kernel itself: no full row is written and read back by kad_route_compress.
 * Count 8 on tables with short window lines only (KAD_ERR_UNSUPPORTED otherwise: use kad_rt_closest_batch +
 * kad_route_compress). A row whose indices span more than 254 sets *escape and writes nothing for it: the caller
 * answers the batch again unpacked. Async on stream. */
int kad_rt_closest_batch_packed(const kad_table* t, const uint8_t* targets, uint32_t q, uint32_t count,
                                uint32_t* packed, uint32_t* escape, void* stream);
/* kad_rt_closest_keys_packed: kad_rt_closest_batch_packed from 8-byte keys (the targets' top 64 bits, native uint64:
 * kad_route_pack_keys' records), which is all the short and 128-byte window lines read. The exact path (the few queries
 * no line answers) runs with the targets' low 96 bits taken as zero: the same rows as from the full targets unless two
 * nodes of its window share their top 64 bits (XOR order then depends on the low bits, infohash.h:131-146), which sets
 * the sticky word *tail (not cleared; ctr[KAD_ROUTE_OVERFLOW_WORD(world) + 2] is meant for it): the caller answers
 * that batch again from full targets. keys 8-byte aligned. Count 8 on tables with short window lines only. */
int kad_rt_closest_keys_packed(const kad_table* t, const uint64_t* keys, uint32_t q, uint32_t count, uint32_t* packed,
                               uint32_t* escape, uint32_t* tail, void* stream);
/* kad_route_fold_flags: flags[0..2] |= ctr[KAD_ROUTE_OVERFLOW_WORD(world) + 0..2] — overflow, packing escape, key-only
 * tail — (device words; kad_route_pack zeroes them, so a caller running many batches folds them after each). Async on
 * stream. */
int kad_route_fold_flags(const uint32_t* ctr, uint32_t world, uint32_t* flags, int device, void* stream);

/* ---- native multi-GPU executor (csrc/kad_comm.hip) ----
 * The two multi-GPU steps issued from C++ over an RCCL communicator of the engine's own (RCCL is loaded at run time:
 * the librccl.so.1 already in the process, else /opt/rocm/lib's; KAD_ERR_UNSUPPORTED without one).
 * kad_comm_unique_id: a new communicator id (KAD_COMM_ID_BYTES bytes) on rank 0; the caller hands it to every rank.
 * kad_comm_create: this rank's communicator on `device` (collective: every rank calls it at once), plus a compute
 *   and a comm stream of its own for the pipelined forms. kad_comm_all_to_all: ncclAllToAll of bytes_per_rank bytes
 *   per rank on stream.
 * kad_route_run: owner routing (sharded.OwnerRoute; reference callers dht.cpp:3189-3217) over n_batches batches of
 *   q targets: kad_route_pack into `world` blocks of `cap` records, all_to_all of the blocks, the owner's query of
 *   every received record (packed != 0: the rows go back packed — count 8 on tables with short window lines through
 *   kad_rt_closest_batch_packed, else kad_rt_closest_batch + kad_route_compress —; packed = 0: rows and counts), the
 *   all_to_all back, the unpack of batch i into out_idx[i] / out_cnt[i] with its counters folded into flags and zeroed
 *   (kad_route_unpack_packed_fold; 4 device words: [0] a block overflowed — grow cap and run again —, [1] a row
 *   escaped packing — run again unpacked —, [2] a key-only query needed the target's low bits — run again with
 *   KAD_ROUTE_KEYS off —, [3] the largest block capacity a batch needed). Every set's ctr must be zero on entry (a new
 *   zeroed buffer, or a previous kad_route_run's) and is left zero. `packed` is a mask:
 *   KAD_ROUTE_PACKED (rows back packed), KAD_ROUTE_KEYS (with it, count 8 on tables with short window lines: the
 *   targets travel as 8-byte keys, kad_route_pack_keys + kad_rt_closest_keys_packed; send / recv then hold world *
 *   cap keys; a table without short lines sets flags[2]).
 *   n_sets = 1: every batch in order on `stream` (comm may be NULL at world 1: no collective, recv == send and
 *   back_* == the answer buffers allowed). n_sets >= 3 (comm required): pipelined on the communicator's streams —
 *   batch i+1's pack and batch i's query on the compute stream while batch i's targets and batch i-1's rows are on the
 *   links —, forked from and joined back to `stream`. Pointers in `targets`, `out_idx`, `out_cnt` (host arrays of
 *   n_batches device pointers) and in the sets are device pointers; a set's buffers: send / recv world * cap * 20
 *   bytes, slot q words, ctr KAD_ROUTE_CTR_WORDS(world) words, rows / back_rows world * cap * count words and cnt /
 *   back_cnt world * cap bytes (packed = 0), prow / back_prow world * cap * KAD_ROUTE_PACKED_WORDS(count) words.
 * kad_shard_run: the north-star step (global_shard.GlobalShard.step) over n_batches replicated batches:
 *   kad_rt_shard_step_home into the `world` home blocks of send[k], all_to_all into recv[k],
 *   kad_rt_home_finish_reset into out_idx[i] / out_cnt[i] (this rank's home range), set k = i % n_sets; the send
 *   counters must start zero (each finish zeroes its set's). n_sets = 1 serial on `stream`, >= 3 pipelined (batch
 *   i+1's all_to_all under batch i's finish and batch i+2's shard kernel). overflow: the sticky word of
 *   kad_rt_home_finish. */
#define KAD_COMM_ID_BYTES 128u
typedef struct kad_comm kad_comm;
typedef struct kad_route_set {
    uint8_t* send;
    uint8_t* recv;
    uint32_t* slot;
    uint32_t* ctr;
    uint32_t* rows;
    uint8_t* cnt;
    uint32_t* back_rows;
    uint8_t* back_cnt;
    uint32_t* prow;
    uint32_t* back_prow;
} kad_route_set;
int kad_comm_unique_id(uint8_t* out_id);
int kad_comm_create(kad_comm** out, int device, uint32_t world, uint32_t rank, const uint8_t* id);
int kad_comm_destroy(kad_comm* comm);
int kad_comm_info(const kad_comm* comm, uint32_t* world, uint32_t* rank, int* device);
int kad_comm_all_to_all(kad_comm* comm, const void* send, void* recv, uint64_t bytes_per_rank, void* stream);
int kad_route_run(kad_comm* comm, const kad_table* t, uint32_t n_batches, const uint8_t* const* targets, uint32_t q,
                  uint32_t count, uint32_t world, uint32_t shard_bits, uint32_t cap, uint32_t packed, uint32_t n_sets,
                  const kad_route_set* sets, uint32_t* const* out_idx, uint8_t* const* out_cnt, uint32_t* flags,
                  void* stream);
int kad_shard_run(kad_comm* comm, const kad_table* shard, const uint32_t* global_good_prefix, uint32_t global_buckets,
                  uint64_t global_base_hi, uint32_t depth, uint32_t shard_first_bucket, uint32_t reach_lo,
                  uint32_t reach_hi, uint32_t n_batches, const uint8_t* const* targets, uint32_t q, uint32_t count,
                  uint32_t row_cap, uint32_t part_cap, uint32_t n_sets, uint32_t* const* send, uint32_t* const* recv,
                  uint32_t* const* scratch, uint32_t* overflow, uint32_t* const* out_idx, uint8_t* const* out_cnt,
                  void* stream);

/* ---- wire step after the query ------------------------ */
#define KAD_SEND_NODES 8u           /* reference network_engine.cpp:59 SEND_NODES */
#define KAD_ADDR4_LEN 6u            /* sin_addr (4) + sin_port (2), bytes as stored in sockaddr_in */
#define KAD_ADDR6_LEN 18u           /* sin6_addr (16) + sin6_port (2) */
#define KAD_NODE4_INFO_LEN 26u      /* network_engine.h:464 NODE4_INFO_BUF_LEN */
#define KAD_NODE6_INFO_LEN 38u      /* network_engine.h:466 NODE6_INFO_BUF_LEN */
/* Attach node addresses to a table (one family): host array, n_nodes x addr_len bytes
 * (KAD_ADDR4_LEN or KAD_ADDR6_LEN). Synchronous. */
int kad_table_set_addrs(kad_table* t, uint32_t addr_len, const uint8_t* addrs);
/* Batched NetworkEngine::bufferNodes(af, id, nodes) (network_engine.cpp:942-974): for query i the
 * candidates idx[i*k .. i*k + min(cnt[i], k)) (node indices incl. index_base, e.g. a findClosestNodes or
 * getCachedNodes result; cnt[i] > k is clamped to k; cnt may be NULL: all k entries of the row). An entry
 * equal to KAD_NO_NODE, or outside [index_base, index_base + n_nodes), is skipped wherever it stands, and
 * the entries after it still count. The others are sorted by XOR distance to targets[i] (equal distances,
 * i.e. equal IDs, keep their order in the row) and the first KAD_SEND_NODES are packed as ID + address
 * records into out[i * KAD_SEND_NODES * (20 + addr_len)], the rest of the row zeroed; out_n[i] (may be
 * NULL) = records written. out must be 16-byte aligned, k <= KAD_MAX_COUNT; idx may be NULL when k is 0.
 * Device pointers. */
int kad_buffer_nodes_batch(const kad_table* t, const uint8_t* targets, uint32_t q, const uint32_t* idx,
                           const uint8_t* cnt, uint32_t k, uint8_t* out, uint8_t* out_n, void* stream);
/* NetworkEngine::deserializeNodes' filter (network_engine.cpp:788-828): for n records of rec_len
 * (KAD_NODE4_INFO_LEN / KAD_NODE6_INFO_LEN) bytes, keep[i] = 0 if the record's ID is myid (host,
 * 20 bytes) or its address is martian (NetworkEngine::isMartian, :308-339). Device pointers. */
int kad_parse_nodes_batch(const uint8_t* records, uint32_t n, uint32_t rec_len, const uint8_t* myid,
                          uint8_t* keep, int device, void* stream);

/* ---- config 5: simulated swarm, iterative lookups ----
 * BUILD-DEFINED model (kad_swarm.hip header): n peers with shape-K routing tables (Dht::onNewNode
 * policy, dht.cpp:867-936) built on the device; lookups run synchronous hops of
 * MAX_REQUESTED_SEARCH_NODES = 4 findClosestNodes(t, 8) answers merged by Search::insertNode
 * (dht.cpp:961-1047, with its bad-node accounting) into a list of SEARCH_NODES = 14 non-bad nodes, until
 * the first 8 non-bad nodes have answered. A share of the peers can be offline: queried, they do not answer
 * and become bad (expired) search nodes. */
#define KAD_SWARM_LEVELS 28u        /* bucket levels per peer table (depth <= 27) */
#define KAD_SEARCH_NODES_LEN 14u    /* dht.h:314 SEARCH_NODES */
#define KAD_SEARCH_LIST 32u         /* list capacity: SEARCH_NODES non-bad nodes + the bad ones kept among them */
typedef struct kad_swarm kad_swarm;
typedef struct kad_search kad_search;
/* sorted_ids: host, n x 20 bytes, strictly ascending; peer index = position. */
int kad_swarm_create(kad_swarm** out, int device, uint32_t n, const uint8_t* sorted_ids);
int kad_swarm_destroy(kad_swarm* s);
int kad_swarm_info(const kad_swarm* s, uint32_t* n_peers, uint64_t* device_bytes);
/* Peer `peer`'s table (host outputs): depth D, counts[KAD_SWARM_LEVELS] per level (level D = my
 * bucket), entries[KAD_SWARM_LEVELS][8] peer indices (KAD_NO_NODE padded). */
int kad_swarm_get_table(const kad_swarm* s, uint32_t peer, uint32_t* depth, uint8_t* counts,
                        uint32_t* entries);
/* RoutingTable::findClosestNodes(targets[i], count) on peer peers[i]'s table (device pointers,
 * count <= 16): out_idx q x count peer indices, out_cnt q. */
int kad_swarm_closest_batch(const kad_swarm* s, const uint32_t* peers, const uint8_t* targets, uint32_t q,
                            uint32_t count, uint32_t* out_idx, uint8_t* out_cnt, void* stream);
/* S lookups (src peer, target); src/targets host or device. The initial list is the source's
 * findClosestNodes(t, 14). offline_per_10k: share of the peers (by a hash of the index) that never answer,
 * per 10,000 (0: all online). Asynchronous on `stream`. */
int kad_search_create(kad_search** out, const kad_swarm* s, uint32_t S, const uint32_t* src,
                      const uint8_t* targets, uint32_t offline_per_10k, void* stream);
/* One synchronous hop for every running lookup; *n_active (if given) = lookups still running
 * after it (synchronises the stream). */
int kad_search_hop(kad_search* x, uint32_t* n_active);
/* Host outputs (any may be NULL): list S x KAD_SEARCH_LIST peer indices (KAD_NO_NODE padded), queried and
 * bad flags S x KAD_SEARCH_LIST, list length S, hops S, done S (0 running, 1 synced: the first 8 non-bad
 * nodes answered, 2 stalled, 3 expired: the first min(size, 25) nodes are bad), overflow (1 value: the lookups
 * and hops so far in which a capacity was hit — a list of KAD_SEARCH_LIST entries had to take one more, or a
 * lookup met more than 64 silent peers; the rule is in kad_swarm.hip's header). */
int kad_search_get(const kad_search* x, uint32_t* list, uint8_t* queried, uint8_t* bad, uint8_t* n, uint32_t* hops,
                   uint8_t* done, uint32_t* overflow);
/* Hands the search's device state to its swarm's pool: destroy a search before its swarm. */
int kad_search_destroy(kad_search* x);

/* ---- InfoHash primitives (infohash.h), batched, device pointers ---------- */
/* out[i] = targets[i].xorCmp(a[i], b[i]) in {-1,0,1}   (infohash.h:131-146) */
int kad_xor_cmp_batch(const uint8_t* targets, const uint8_t* a, const uint8_t* b, uint32_t n,
                      int8_t* out, void* stream);
/* out[i] = InfoHash::commonBits(a[i], b[i]) in [0,160] (infohash.h:106-128) */
int kad_common_bits_batch(const uint8_t* a, const uint8_t* b, uint32_t n, uint32_t* out, void* stream);
/* out[i] = a[i].lowbit(), 0xFFFFFFFF for the zero ID     (infohash.h:84-95)  */
int kad_lowbit_batch(const uint8_t* a, uint32_t n, uint32_t* out, void* stream);
/* out_ids[i] = InfoHash::get(key i) = SHA-1 of data[offsets[i] .. offsets[i+1]) (infohash.cpp:46-61,
 * HASH_LEN 20 -> SHA-1). Device pointers; offsets has n+1 entries. */
int kad_infohash_get_batch(const uint8_t* data, const uint64_t* offsets, uint32_t n, uint8_t* out_ids,
                           int device, void* stream);

/* ---- synthetic tables (host code; bench and tests) ----------------------- */
/* n distinct random IDs from std::mt19937_64(seed): ID i = big-endian bytes of
 * draws (3i, 3i+1) and the top 4 bytes of draw 3i+2; duplicates are rejected and
 * redrawn. */
int kad_synth_ids(uint64_t seed, uint32_t n, uint8_t* out_ids);
/* status mix from std::mt19937_64(seed): u = draw % 100; u < good_pct -> GOOD,
 * u < good_pct+expired_pct -> EXPIRED, else dubious (0). */
int kad_synth_status(uint64_t seed, uint32_t n, uint32_t good_pct, uint32_t expired_pct,
                     uint8_t* out_status);
/* Sort ids ascending (stable permutation out_perm, may be NULL) in place. */
int kad_sort_ids(uint32_t n, uint8_t* ids, uint32_t* out_perm);
/* Uniform-depth table U(depth) over ascending ids: bucket firsts = prefix << (160-depth)
 * for every prefix in [prefix_lo, prefix_hi) (all 2^depth if prefix_hi == 0), bucket
 * offsets by ID range. out_first: (prefix_hi-prefix_lo) x 20 bytes, out_offset: +1. */
int kad_uniform_buckets(uint32_t n, const uint8_t* sorted_ids, uint32_t depth,
                        uint64_t prefix_lo, uint64_t prefix_hi,
                        uint8_t* out_first, uint32_t* out_offset);
/* Split-policy table S (Dht::onNewNode, dht.cpp:903-934, without the my-bucket
 * restriction; RoutingTable::split, routing_table.cpp:137-163): insert ids in
 * order, split the found bucket while it holds >= bucket_cap nodes.
 * Outputs the node order grouped by bucket (out_perm: n indices into ids, list
 * order inside each bucket), bucket firsts and offsets; *out_n_buckets <= n+1. */
int kad_split_table(uint32_t n, const uint8_t* ids, uint32_t bucket_cap,
                    uint32_t* out_perm, uint8_t* out_first, uint32_t* out_offset,
                    uint32_t* out_n_buckets);
/* Counter-based uniform swarm shard: every bucket of U(depth) in
 * [prefix_lo, prefix_hi) gets Poisson(mean) nodes drawn from a hash of
 * (seed, prefix), so any bucket range is reproducible independently (shards and
 * their halos). First call with out_ids == NULL returns the node count in *out_n. */
int kad_synth_uniform_shard(uint64_t seed, uint32_t depth, uint64_t prefix_lo, uint64_t prefix_hi,
                            double mean_per_bucket, uint32_t good_pct, uint32_t expired_pct,
                            uint32_t* out_n, uint8_t* out_ids, uint8_t* out_status,
                            uint32_t* out_offset);
/* The SURVEY.md §8d recipe of a whole n-node table (kad_synth_ids(seed_ids, n) and
 * kad_synth_status(seed_status, n, ...)) restricted to the U(depth) buckets
 * [prefix_lo, prefix_hi): ids ascending, status, bucket offsets (+1), and in
 * *out_below the number of the table's IDs below the range (global index of the
 * range's first node). One sequential pass over the n draws; fails on a duplicate
 * ID instead of redrawing it (probability < 1e-30 at n = 1e8). With out_ids ==
 * NULL: counts only; out arrays hold cap nodes (more in the range: KAD_ERR_NOMEM,
 * the count in *out_n). */
int kad_synth_recipe_range(uint64_t seed_ids, uint64_t seed_status, uint64_t n, uint32_t depth,
                           uint64_t prefix_lo, uint64_t prefix_hi, uint32_t good_pct,
                           uint32_t expired_pct, uint64_t cap, uint32_t* out_n, uint64_t* out_below,
                           uint8_t* out_ids, uint8_t* out_status, uint32_t* out_offset);

#ifdef __cplusplus
}
#endif
#endif /* KADGPU_H */
