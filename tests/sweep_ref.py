"""Numpy restatement of the two whole-table loops of the reference that kad_table_sweep / kad_table_expire stand in
for, over a table dict (ids, status, off):

  Dht::getNodesStats (dht.cpp:2470-2495)  good: status has GOOD; dubious: neither GOOD nor EXPIRED; incoming: GOOD and
                                          time > reply_time (from the times the test drew)
  Dht::expireBuckets (dht.cpp:942-956)    the EXPIRED nodes in bucket order, then list order, and the buckets that
                                          hold at least one (the ones sendCachedPing is called for)

and the tables tests/test_sweep.py and tests/test_expire.py run on, with the ground each must cover. The expected table
after an expiry comes from the oracle's structure-faithful table (oracle.FaithfulTable.apply) given one REMOVE row per
expired node."""
from __future__ import annotations

import numpy as np

import oracle as O
import tables as TB
from opendht_amd import synth as S
from opendht_amd._lib import KAD_OP_REMOVE, KAD_STATUS_EXPIRED, KAD_STATUS_GOOD

MIN_NS = np.iinfo(np.int64).min
NODE_EXPIRE_NS = 10 * 60 * 10**9          # node.h:91-94
NODE_GOOD_NS = 120 * 60 * 10**9


def sweep_ref(t, status=None, time_ns=None, reply_ns=None, index_base=0):
    """{totals, expired_nodes, changed_buckets, per_bucket (expired nodes per bucket)} of table t (status: its status
    bytes, or others of the same length); incoming is counted only when the times are given."""
    st = np.asarray(t["status"] if status is None else status, np.uint8)
    n = st.shape[0]
    off = None if t.get("off") is None else np.asarray(t["off"], np.int64)
    B = 0 if off is None else off.shape[0] - 1
    good = (st & KAD_STATUS_GOOD) != 0
    expired = (st & KAD_STATUS_EXPIRED) != 0
    incoming = 0
    if time_ns is not None:
        incoming = int(np.count_nonzero(good & (np.asarray(time_ns, np.int64) > np.asarray(reply_ns, np.int64))))
    csum = np.concatenate([[0], np.cumsum(expired.astype(np.int64))])
    per_bucket = csum[off[1:]] - csum[off[:-1]] if B else np.zeros(0, np.int64)
    width = off[1:] - off[:-1] if B else np.zeros(0, np.int64)
    changed = np.flatnonzero(per_bucket > 0).astype(np.uint32)
    totals = dict(good=int(good.sum()), dubious=int((~good & ~expired).sum()), expired=int(expired.sum()),
                  incoming=incoming, changed_buckets=int(changed.shape[0]), empty_buckets=int((width == 0).sum()),
                  flags=0 if time_ns is None else 1, reserved=0)
    nodes = (np.flatnonzero(expired).astype(np.uint64) + np.uint64(index_base)).astype(np.uint32)
    assert n == 0 or off is None or off[-1] == n
    return dict(totals=totals, expired_nodes=nodes, changed_buckets=changed, per_bucket=per_bucket, width=width)


def expire_ref(t, status=None):
    """The table after Dht::expireBuckets: (ids, status, first, off, remap) from the oracle's std::list table given
    one REMOVE per expired node in ascending order."""
    st = np.asarray(t["status"] if status is None else status, np.uint8)
    gone = np.flatnonzero((st & KAD_STATUS_EXPIRED) != 0).astype(np.uint32)
    ops = np.zeros((gone.shape[0], 3), np.uint32)
    ops[:, 0] = KAD_OP_REMOVE
    ops[:, 1] = gone
    F = O.FaithfulTable(t["ids"], st, t["first"], t["off"])
    try:
        ids, st1, first, off, remap, _ = F.apply(ops, np.zeros((0, 20), np.uint8), np.zeros(0, np.uint8))
    finally:
        F.close()
    return ids, st1, first, off, remap, ops


def status_at(time_ns, reply_ns, expired, now_ns):
    """Node::isGood(now) / isExpired() as status bytes (node.cpp:34-40, node.h:67), as kad_table_refresh_status."""
    time_ns, reply_ns = np.asarray(time_ns, np.int64), np.asarray(reply_ns, np.int64)
    exp = np.asarray(expired, np.uint8) != 0
    lim_t, lim_r = now_ns - NODE_EXPIRE_NS, now_ns - NODE_GOOD_NS
    good = ~exp & (reply_ns >= lim_r) & (time_ns >= lim_t)
    return (good.astype(np.uint8) * KAD_STATUS_GOOD) | (exp.astype(np.uint8) * KAD_STATUS_EXPIRED)


def draw_times(n, seed, now_ns):
    """time / reply_time / expired for n nodes around now_ns: every class of the incoming test gets its share (good
    with time > / < / == reply_time, dubious by an old reply or an old time, expired)."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 6, size=n)
    recent = now_ns - rng.integers(1, NODE_EXPIRE_NS // 2, size=n)
    earlier = recent - rng.integers(1, NODE_EXPIRE_NS // 4, size=n)
    time_ns = np.where(kind == 1, earlier, recent).astype(np.int64)          # 0: time > reply, 1: time < reply
    reply_ns = np.where(kind == 0, earlier, recent).astype(np.int64)
    reply_ns = np.where(kind == 2, time_ns, reply_ns)                        # 2: equal
    reply_ns = np.where(kind == 3, now_ns - NODE_GOOD_NS - 5, reply_ns)      # 3: dubious, reply too old
    reply_ns = np.where((kind == 3) & (rng.random(n) < 0.3), MIN_NS, reply_ns)  # ... or never replied
    time_ns = np.where(kind == 4, now_ns - NODE_EXPIRE_NS - 7, time_ns)      # 4: dubious, not heard of lately
    expired = (kind == 5).astype(np.uint8)                                   # 5: expired
    return time_ns, reply_ns, expired


def one5000():
    """A single bucket of 5000 nodes (wider than a workgroup's tile of 4096): 60 / 20 / 20 % good / dubious / expired."""
    rng = np.random.default_rng(0x5EE9)
    ids = S.random_ids(5000, 0x5EE9)
    st = rng.choice(np.array([1, 0, 2], np.uint8), size=5000, p=[0.6, 0.2, 0.2])
    return TB.table(ids, st, np.zeros((1, 20), np.uint8), np.array([0, 5000], np.uint32), name="one5000")


def extra_tables():
    u = TB.uniform_config(2000, 4)
    u["name"] = "U4_2000"
    s = TB.split_config(257, good=100, expired=0)
    s["name"] = "S257good"
    e = TB.uniform_config(2000, 4, good=0, expired=100)
    e["name"] = "U4_2000exp"
    return [u, s, e, one5000()]


def big_table():
    t = TB.uniform_config(1_200_000, 17, seed=0xB16)
    t["name"] = "U17_1200000"
    return t


def small_tables():
    """TB.all_small_tables() plus the extra shapes (S257 of the tiny tables and S257good are different tables)."""
    return TB.all_small_tables() + extra_tables()


def check_ground(t, r):
    """The ground the restatement r of table t must cover before a device result is compared with it."""
    name, tot, pb, w = t["name"], r["totals"], r["per_bucket"], r["width"]
    if name == "S10000":
        assert tot["expired"] >= 1000 and tot["changed_buckets"] >= 800 and (pb >= 2).sum() >= 190
        assert tot["empty_buckets"] == 2
    elif name == "sparse_good":
        assert ((pb == w) & (w > 0)).sum() >= 1600 and tot["empty_buckets"] == 282
    elif name == "all_bad":
        assert tot["changed_buckets"] == 64 and pb.shape[0] == 64 and tot["good"] == 0
    elif name == "U4_2000":
        assert tot["changed_buckets"] == 16 and pb.shape[0] == 16 and (w > 100).all()
    elif name == "U4_2000exp":
        assert tot["expired"] == 2000 and t["status"].shape[0] == 2000
    elif name == "one5000":
        assert tot["expired"] >= 900 and pb.shape[0] == 1
    elif name == "U17_1200000":
        assert tot["expired"] >= 120_000 and tot["changed_buckets"] >= 78_000 and tot["empty_buckets"] >= 10
    elif name in ("S257good", "ties", "dups", "ties48", "dups48", "S1", "S3"):
        assert tot["expired"] == 0 and r["expired_nodes"].shape[0] == 0 and r["changed_buckets"].shape[0] == 0
    elif name == "empty":
        assert pb.shape[0] == 0
    elif name == "one_empty_bucket":
        assert pb.shape[0] == 1 and tot["empty_buckets"] == 1
    elif name in ("S50", "S257", "U10_10000", "offset_first", "U20_1200000"):  # mixed tables: every class present
        assert tot["good"] and tot["dubious"] and tot["expired"] and 0 < tot["changed_buckets"] < pb.shape[0]
    else:
        raise AssertionError(f"no ground stated for table {name!r}")
