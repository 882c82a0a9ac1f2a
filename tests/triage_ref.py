"""The onNewNode triage verdict (kad_rt_triage_batch) restated for the tests from its definition
(Dht::onNewNode(node, 0), dht.cpp:867-936), with numpy and Python big integers; the bucket of a candidate comes from
oracle.FaithfulTable.find_bucket. Shared by test_triage.py and test_ingest.py; nothing here touches the GPU."""
import numpy as np

import oracle as O

NONE, KNOWN, REPLACE, INSERT, SPLIT, FULL = 0, 1, 2, 3, 4, 5
KIND_MASK, MYBUCKET = 0x0F, 0x10
NO_NODE = 0xFFFFFFFF
TARGET_NODES = 8
_FULLISH = 100  # a full bucket without expired nodes, before the split condition


def lowbit(x: int) -> int:
    """InfoHash::lowbit: the index, counted from the most significant of 160 bits, of the lowest set bit; -1 for 0."""
    return -1 if x == 0 else 159 - ((x & -x).bit_length() - 1)


def _int(row) -> int:
    return int.from_bytes(row.tobytes(), "big")


def find_bucket(t, ids):
    """findBucket of every ID (NO_NODE on a table without buckets)."""
    ids = np.ascontiguousarray(ids, np.uint8).reshape(-1, 20)
    if t["first"] is None or t["first"].shape[0] == 0:
        return np.full(ids.shape[0], NO_NODE, np.uint32)
    ft = O.FaithfulTable(t["ids"], t["status"], t["first"], t["off"])
    try:
        return ft.find_bucket(ids)
    finally:
        ft.close()


class BucketFacts:
    """Per bucket of a table: node count, first expired and first non-good node (table indices, NO_NODE if none),
    depth (RoutingTable::depth, routing_table.cpp:59-65), share of the ID space, and the lowest index of every ID."""

    def __init__(self, t):
        ids, st, first, off = t["ids"], t["status"], t["first"], t["off"]
        B = 0 if first is None else first.shape[0]
        self.B = B
        self.n = np.zeros(B, np.int64)
        self.first_expired = np.full(B, NO_NODE, np.uint32)
        self.first_bad = np.full(B, NO_NODE, np.uint32)
        self.depth = np.zeros(B, np.int64)
        self.share = np.zeros(B)
        self.index_of = [dict() for _ in range(B)]
        fi = [_int(first[b]) for b in range(B)]
        for b in range(B):
            j0, j1 = int(off[b]), int(off[b + 1])
            self.n[b] = j1 - j0
            for j in range(j0, j1):
                if (st[j] & 2) and self.first_expired[b] == NO_NODE:
                    self.first_expired[b] = j
                if not (st[j] & 1) and self.first_bad[b] == NO_NODE:
                    self.first_bad[b] = j
                self.index_of[b].setdefault(ids[j].tobytes(), j)
            self.depth[b] = max(lowbit(fi[b]), lowbit(fi[b + 1]) if b + 1 < B else -1) + 1
            lo = 0 if b == 0 else fi[b]  # IDs below the first bucket's first clamp to bucket 0
            hi = fi[b + 1] if b + 1 < B else 1 << 160
            self.share[b] = (hi - lo) / float(1 << 160)

    def bucket_class(self):
        """What a new ID landing in each bucket gets before the split condition: REPLACE, INSERT or _FULLISH."""
        return np.where(self.first_expired != NO_NODE, REPLACE, np.where(self.n < TARGET_NODES, INSERT, _FULLISH))

    def split_ok(self, self_bucket, bootstrap):
        """dht.cpp:921 per bucket: (mybucket || (bootstrap && depth < 6)) && (!dubious || n_buckets == 1)."""
        mine = np.arange(self.B) == (-1 if self_bucket is None else self_bucket)
        return (mine | (bool(bootstrap) & (self.depth < 6))) & ((self.first_bad == NO_NODE) | (self.B == 1))


def base_verdicts(t, facts, cand, bucket):
    """The part of the verdict that depends on neither self_id nor bootstrap: (kind with _FULLISH for full buckets,
    node without index_base)."""
    q = cand.shape[0]
    kind = np.zeros(q, np.int64)
    node = np.full(q, NO_NODE, np.uint32)
    if facts.B == 0:
        return kind, node
    cls = facts.bucket_class()
    for i in range(q):
        b = int(bucket[i])
        j = facts.index_of[b].get(cand[i].tobytes())
        if j is not None:
            kind[i], node[i] = KNOWN, j
        elif cls[b] == REPLACE:
            kind[i], node[i] = REPLACE, facts.first_expired[b]
        elif cls[b] == INSERT:
            kind[i] = INSERT
        else:
            kind[i], node[i] = _FULLISH, facts.first_bad[b]
    return kind, node


def finish(t, facts, kind, node, bucket, self_id, bootstrap, index_base=0):
    """(verdict bytes, node with index_base, bucket) for one self_id (None: no bucket is mine) and bootstrap."""
    q = kind.shape[0]
    if facts.B == 0:
        return np.zeros(q, np.uint8), np.full(q, NO_NODE, np.uint32), np.full(q, NO_NODE, np.uint32)
    sb = None if self_id is None else int(find_bucket(t, self_id)[0])
    ok = facts.split_ok(sb, bootstrap)
    b = bucket.astype(np.int64)
    k = np.where(kind == _FULLISH, np.where(ok[b], SPLIT, FULL), kind)
    mine = b == (-1 if sb is None else sb)
    verdict = (k | np.where(mine, MYBUCKET, 0)).astype(np.uint8)
    nd = np.where(node == NO_NODE, np.uint32(NO_NODE), (node.astype(np.uint64) + index_base).astype(np.uint32))
    return verdict, nd.astype(np.uint32), bucket.astype(np.uint32)


def triage(t, cand, self_id, bootstrap, index_base=0):
    """The whole restatement for one call."""
    cand = np.ascontiguousarray(cand, np.uint8).reshape(-1, 20)
    facts = BucketFacts(t)
    bucket = find_bucket(t, cand)
    kind, node = base_verdicts(t, facts, cand, bucket)
    return finish(t, facts, kind, node, bucket, self_id, bootstrap, index_base)


def near_targets(self_id, rng, copies=8):
    """For each c in 0..159, `copies` IDs sharing exactly c leading bits with self_id."""
    s = _int(self_id)
    out = []
    for c in range(160):
        low = 159 - c
        for _ in range(copies):
            r = int.from_bytes(rng.bytes(20), "big") & ((1 << low) - 1)
            out.append(((((s >> low) ^ 1) << low) | r).to_bytes(20, "big"))
    return np.frombuffer(b"".join(out), np.uint8).reshape(-1, 20)
