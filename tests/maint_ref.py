"""The yardstick of the bucket-time tests: the reference's own loops restated one bucket at a time over (off, first, time),
in plain Python, sharing nothing with the engine.

  scan         Dht::bucketMaintenance's loop head (dht.cpp:2832-2833) and, per bucket that passes, what the body of
               :2837-2850 can do: the class comes from running that body under all four outcomes of the two rand_trial
               draws, not from a rule
  lowbit       InfoHash::lowbit (infohash.h:84-95) byte by byte, and random_id_bit, RoutingTable::randomId's `bit`
               (routing_table.cpp:30-32)
  find_bucket  RoutingTable::findBucket as its linear walk (routing_table.cpp:113-127); touch is Dht::onReportedAddr
               (dht.cpp:3174-3178) per ID
  split_times  RoutingTable::split's Bucket{b->af, new_id, b->time} (routing_table.cpp:149)
"""
from __future__ import annotations

import itertools

import numpy as np

INT64_MIN = -(1 << 63)
TEN_MIN = 600 * 10**9
STALE, EMPTY, HAS_NEXT, NEXT_EMPTY, HAS_PREV, PREV_EMPTY = 1, 2, 4, 8, 16, 32
NEVER, MAYBE, SURE = 0, 1, 2
NO_BUCKET = 0xFFFFFFFF
REC = [("bucket", "<u4"), ("kind", "<u4")]
TOTALS = ("candidates", "stale", "empty", "sure", "maybe", "never", "first_sure", "reserved")


def lowbit(h) -> int:
    """InfoHash::lowbit of 20 bytes."""
    h = bytes(bytearray(h))
    i = 19
    while i >= 0:
        if h[i] != 0:
            break
        i -= 1
    if i < 0:
        return -1
    j = 7
    while j >= 0:
        if h[i] & (0x80 >> j):
            break
        j -= 1
    return 8 * i + j


def random_id_bit(first, b: int) -> int:
    B = len(first)
    bit1 = lowbit(first[b])
    bit2 = lowbit(first[b + 1]) if b + 1 < B else -1
    return max(bit1, bit2) + 1


def body_finds_node(width, b: int, trial1: bool, trial2: bool) -> bool:
    """:2838-2850 on bucket b with the two rand_trial draws fixed (a draw the short-circuit skips is not looked at):
    is q->randomNode() non-null?"""
    B = len(width)
    q = b
    if b + 1 < B and (width[q] == 0 or trial1):
        q = b + 1
    if b != 0 and (width[q] == 0 or trial2):
        r = b - 1
        if width[r] != 0:
            q = r
    return width[q] != 0


def bucket_class(width, b: int) -> int:
    got = [body_finds_node(width, b, t1, t2) for t1, t2 in itertools.product((False, True), repeat=2)]
    return SURE if all(got) else (MAYBE if any(got) else NEVER)


def low_bits(width, time_ns, now_ns: int, b: int) -> int:
    B = len(width)
    k = 0
    if int(time_ns[b]) < now_ns - TEN_MIN:
        k |= STALE
    if width[b] == 0:
        k |= EMPTY
    if b + 1 < B:
        k |= HAS_NEXT | (NEXT_EMPTY if width[b + 1] == 0 else 0)
    if b != 0:
        k |= HAS_PREV | (PREV_EMPTY if width[b - 1] == 0 else 0)
    return k


def scan(off, first, time_ns, now_ns: int, first_bucket: int = 0, cap=None, stop=None):
    """{"totals": dict, "records": REC array}: every bucket b >= first_bucket passing :2833, ascending. stop: walk only
    the buckets below it (a window of a table too large to walk in Python; the totals are then the window's)."""
    off = [int(x) for x in off]
    B = len(off) - 1
    width = [off[b + 1] - off[b] for b in range(B)]
    if time_ns is None:
        time_ns = [INT64_MIN] * B
    recs = []
    tot = dict.fromkeys(TOTALS, 0)
    tot["first_sure"] = NO_BUCKET
    for b in range(first_bucket, B if stop is None else min(stop, B)):
        if not (int(time_ns[b]) < now_ns - TEN_MIN or width[b] == 0):
            continue
        low = low_bits(width, time_ns, now_ns, b)
        cls = bucket_class(width, b)
        recs.append((b, low | (cls << 6) | (random_id_bit(first, b) << 8)))
        tot["candidates"] += 1
        tot["stale"] += 1 if low & STALE else 0
        tot["empty"] += 1 if low & EMPTY else 0
        tot[("never", "maybe", "sure")[cls]] += 1
        if cls == SURE and tot["first_sure"] == NO_BUCKET:
            tot["first_sure"] = b
    cap = len(recs) if cap is None else cap
    return {"totals": tot, "records": np.array(recs[:cap], dtype=REC).reshape(-1)}


def find_bucket(first, id20) -> int:
    """The linear walk; first holds B >= 1 rows."""
    key = bytes(bytearray(id20))
    b = 0
    while True:
        nxt = b + 1
        if nxt == len(first):
            return b
        if key < bytes(bytearray(first[nxt])):
            return b
        b = nxt


def touch(first, time_ns, ids, now_ns: int):
    """onReportedAddr per ID, in order: (the new times, the bucket of every ID)."""
    out = np.array(time_ns, dtype=np.int64).copy()
    buckets = np.zeros(len(ids), np.uint32)
    for i, x in enumerate(ids):
        b = find_bucket(first, x)
        out[b] = now_ns
        buckets[i] = b
    return out, buckets


def split_times(time_ns, a: int):
    """The times after RoutingTable::split of bucket a: the new bucket a + 1 is born with b->time."""
    t = [int(x) for x in time_ns]
    return np.array(t[:a + 1] + [t[a]] + t[a + 1:], dtype=np.int64)


def apply_times(time_ns, ops):
    """The times after a kad_table_apply batch: only KAD_OP_SPLIT (kind 4) rows change them, in order."""
    t = np.array(time_ns, dtype=np.int64)
    for kind, a, _ in np.asarray(ops, dtype=np.uint32).reshape(-1, 3):
        if int(kind) == 4:
            t = split_times(t, int(a))
    return t


# -- the exhaustive small tables --------------------------------------------------------------------------------------
def width_patterns():
    """Every bucket list with B in {1, 2, 3, 4} and widths from {0, 2}: 30 patterns."""
    return [w for B in (1, 2, 3, 4) for w in itertools.product((0, 2), repeat=B)]


def small_cases(now_ns: int):
    """(widths, times) for every width pattern and every stale / fresh time pattern: 340 tables."""
    stale, fresh = now_ns - TEN_MIN - 1, now_ns
    return [(w, t) for w in width_patterns() for t in itertools.product((stale, fresh), repeat=len(w))]


def table_of_widths(widths, seed: int = 1):
    """A routing table with the given bucket widths: uniform-depth firsts over the top bits (1 bucket: the all-zero
    first), and nodes drawn inside each bucket's range. Returns (ids (n, 20), first (B, 20), off (B+1,))."""
    B = len(widths)
    depth = max(1, (B - 1).bit_length())
    rng = np.random.default_rng(seed)
    first = np.zeros((B, 20), np.uint8)
    ids = []
    for b in range(B):
        lo = b << (160 - depth) if B > 1 else 0
        hi = ((b + 1) << (160 - depth)) if (B > 1 and b + 1 < B) else (1 << 160)
        first[b] = np.frombuffer(lo.to_bytes(20, "big"), np.uint8)
        for _ in range(widths[b]):
            x = lo + int(rng.integers(1, 1 << 62)) % (hi - lo)
            ids.append(np.frombuffer(x.to_bytes(20, "big"), np.uint8))
    off = np.concatenate([[0], np.cumsum(widths)]).astype(np.uint32)
    ids = np.array(ids, np.uint8).reshape(-1, 20)
    return ids, first, off


def draw_times(B: int, now_ns: int, seed: int):
    """A third each at INT64_MIN, stale and fresh."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, 3, size=B)
    stale = now_ns - TEN_MIN - 1 - rng.integers(0, 10**12, size=B)
    fresh = now_ns - rng.integers(0, TEN_MIN, size=B)
    return np.where(pick == 0, INT64_MIN, np.where(pick == 1, stale, fresh)).astype(np.int64)
