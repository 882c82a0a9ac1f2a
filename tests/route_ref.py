"""A plain numpy model of owner routing's contracts as include/kadgpu.h states them (the comments of kad_route_pack,
kad_route_unpack, kad_route_compress, kad_route_unpack_packed(_fold), kad_route_fold_flags and
kad_rt_closest_batch_packed), written from the header and not from the kernels, plus the table fixtures of
tests/test_packed_rows.py. Nothing here touches a GPU.

A packed row of `count` entries is KAD_ROUTE_PACKED_WORDS(count) little-endian words: word 0 the row's smallest index
(KAD_NO_NODE for an empty row), then one byte per entry, the entry minus word 0, 0xFF past the row's count (and in the
bytes that pad the last word). A row packs iff max - min <= 254."""
from __future__ import annotations

import numpy as np

NO_NODE = 0xFFFFFFFF
SUBS, QPW, CSTRIDE, MAX_WORLD, PACKED_MAX_COUNT = 8, 1024, 32, 16, 32
PACKED, KEYS, ZEROED = 1, 2, 4


def packed_words(count: int) -> int:
    return 1 + (count + 3) // 4


def ctr_words(world: int) -> int:
    return (world * SUBS + 1) * CSTRIDE


def overflow_word(world: int) -> int:
    return world * SUBS * CSTRIDE


# ---- packed rows ------------------------------------------------------------------------------------------------
def escapes_rows(rows, cnt) -> np.ndarray:
    """Per row: cnt > 0 and max - min of its first cnt entries > 254 (it cannot be packed)."""
    rows = np.asarray(rows, np.uint32).astype(np.int64)
    cnt = np.asarray(cnt).astype(np.int64)
    live = np.arange(rows.shape[1])[None, :] < cnt[:, None]
    hi = np.where(live, rows, -1).max(1, initial=-1)
    lo = np.where(live, rows, 1 << 40).min(1, initial=1 << 40)
    return (cnt > 0) & (hi - lo > 254)


def spans_rows(rows, cnt) -> np.ndarray:
    """Per row: max - min of its first cnt entries (0 for an empty row)."""
    rows = np.asarray(rows, np.uint32).astype(np.int64)
    cnt = np.asarray(cnt).astype(np.int64)
    live = np.arange(rows.shape[1])[None, :] < cnt[:, None]
    hi, lo = np.where(live, rows, -1).max(1, initial=-1), np.where(live, rows, 1 << 40).min(1, initial=1 << 40)
    return np.where(cnt > 0, hi - lo, 0)


def escapes(row, cnt) -> bool:
    return bool(escapes_rows(np.asarray(row, np.uint32)[None, :], [cnt])[0])


def pack_rows(rows, cnt, count: int) -> np.ndarray:
    """n rows of `count` entries -> (n, KAD_ROUTE_PACKED_WORDS(count)) uint32. Rows that escape are not defined by
    the header: their words here are never to be compared."""
    rows = np.asarray(rows, np.uint32).reshape(-1, count).astype(np.int64)
    cnt = np.asarray(cnt).astype(np.int64)
    n, W = rows.shape[0], packed_words(count)
    live = np.arange(count)[None, :] < cnt[:, None]
    lo = np.where(live, rows, NO_NODE).min(1, initial=NO_NODE)
    by = np.full((n, 4 * (W - 1)), 0xFF, np.uint8)
    by[:, :count] = np.where(live, np.clip(rows - lo[:, None], 0, 254), 0xFF).astype(np.uint8)
    out = np.empty((n, W), np.uint32)
    out[:, 0] = lo.astype(np.uint32)
    out[:, 1:] = by.view("<u4")
    return out


def pack_row(row, cnt: int, count: int) -> np.ndarray:
    assert not escapes(row, cnt)
    return pack_rows(np.asarray(row, np.uint32)[None, :], [cnt], count)[0]


def decode_rows(words, count: int):
    """(n, W) packed words -> (rows (n, count) uint32, cnt (n,) uint8): base + byte, KAD_NO_NODE for 0xFF, cnt = the
    number of bytes that are not 0xFF. The base only has to be no larger than any entry (the fused query kernel's)."""
    W = packed_words(count)
    words = np.ascontiguousarray(np.asarray(words, np.uint32).reshape(-1, W))
    by = np.ascontiguousarray(words[:, 1:]).astype("<u4").view(np.uint8).reshape(-1, 4 * (W - 1))
    val = words[:, :1].astype(np.int64) + by.astype(np.int64)
    assert (val[by != 0xFF] < NO_NODE).all(), "an entry decodes to KAD_NO_NODE or past 2^32"
    rows = np.where(by != 0xFF, val, NO_NODE).astype(np.uint32)[:, :count]
    return np.ascontiguousarray(rows), (by != 0xFF).sum(1).astype(np.uint8)


def decode_row(words, count: int):
    r, c = decode_rows(np.asarray(words, np.uint32)[None, :], count)
    return r[0], int(c[0])


def unpack_rows(slot, back_rows, back_cnt, count: int):
    """kad_route_unpack: out row i = back row slot[i], out_cnt[i] = back_cnt[slot[i]]; KAD_NO_NODE and 0 for slot
    KAD_NO_NODE."""
    slot = np.asarray(slot, np.uint32)
    none = slot == NO_NODE
    s = np.where(none, 0, slot).astype(np.int64)
    rows = np.asarray(back_rows, np.uint32).reshape(-1, count)[s] if count else np.zeros((slot.size, 0), np.uint32)
    rows = np.where(none[:, None], np.uint32(NO_NODE), rows).astype(np.uint32)
    return rows, np.where(none, 0, np.asarray(back_cnt, np.uint8)[s]).astype(np.uint8)


# ---- kad_route_pack ----------------------------------------------------------------------------------------------
def owner(targets, world: int, shard_bits: int) -> np.ndarray:
    """Block of every target: (byte 0 >> (8 - shard_bits)) % world, 0 when shard_bits = 0."""
    b0 = np.asarray(targets, np.uint8).reshape(-1, 20)[:, 0].astype(np.int64)
    if shard_bits == 0:
        return np.zeros(b0.shape[0], np.int64)
    return (b0 >> (8 - shard_bits)) % world


def expect_pack(targets, world: int, shard_bits: int, cap: int) -> dict:
    """What kad_route_pack must leave, per (block d, sub-block r):
    ctr[d, r]     the full count of its queries (it may exceed the sub-block's capacity cap / KAD_ROUTE_SUBS)
    placed[d, r]  how many of them got a record: min(ctr, cap / KAD_ROUTE_SUBS); the others' slot is KAD_NO_NODE
    queries[d][r] the indices of its queries: target i belongs to workgroup i // KAD_ROUTE_QPW, whose targets go to
                  sub-block workgroup % KAD_ROUTE_SUBS of their owner's block
    overflow      the sticky word: 1 iff some sub-block is over its capacity
    The order of the records inside a sub-block is unspecified, and so is which queries of a full one are dropped."""
    d = owner(targets, world, shard_bits)
    q = d.shape[0]
    r = (np.arange(q) // QPW) % SUBS
    ctr = np.zeros((world, SUBS), np.int64)
    np.add.at(ctr, (d, r), 1)
    sub = cap // SUBS
    return dict(owner=d, sub=r, ctr=ctr, placed=np.minimum(ctr, sub), overflow=int((ctr > sub).any()),
                queries=[[np.nonzero((d == dd) & (r == rr))[0] for rr in range(SUBS)] for dd in range(world)])


def ctr_image(sub_counts, world: int, overflow: int = 0, escape: int = 0, tail: int = 0) -> np.ndarray:
    """The KAD_ROUTE_CTR_WORDS(world) words: sub-block (d, r)'s count at (d * SUBS + r) * CSTRIDE, then the overflow,
    escape and tail words; every other word zero."""
    c = np.zeros(ctr_words(world), np.uint32)
    c[np.arange(world * SUBS) * CSTRIDE] = np.asarray(sub_counts, np.uint32).reshape(-1)
    c[overflow_word(world):overflow_word(world) + 3] = (overflow, escape, tail)
    return c


def expect_fold(ctr, world: int, flags) -> np.ndarray:
    """flags after kad_route_unpack_packed_fold: [0..2] |= the overflow, escape and tail words, [3] = max([3],
    KAD_ROUTE_SUBS x the fullest sub-block's count). (kad_route_fold_flags: words 0..2 alone.)"""
    ctr = np.asarray(ctr, np.uint32)
    out = np.asarray(flags, np.uint32).copy()
    ov = overflow_word(world)
    out[:3] |= ctr[ov:ov + 3]
    out[3] = max(int(out[3]), SUBS * int(ctr[np.arange(world * SUBS) * CSTRIDE].max()))
    return out


# ---- synthesised rows for kad_route_compress / kad_route_unpack_packed -------------------------------------------
SPANS = (0, 1, 253, 254, 255, 256, 10 ** 6)
BASES = (0, 3, 0xFFFFFFFE - 254, 0xFFFFFFFE - 254 - 10 ** 6, 1 << 31, 123_456_789)


def synth_rows(count: int, n: int = 600, seed: int = 0):
    """n rows of `count` entries for every cnt 0..count, span of SPANS and base of BASES in turn, the largest entry
    at the first, a middle or the last live position and the smallest at another one; entries past cnt hold junk a
    kernel must not read as part of the row. Returns (rows (n, count) uint32, cnt (n,) uint8)."""
    rng = np.random.default_rng(0xC0DE + 97 * count + seed)
    rows = rng.integers(0, NO_NODE, (n, count), dtype=np.uint32)  # junk past cnt
    cnt = np.empty(n, np.uint8)
    for i in range(n):
        c = i % (count + 1) if i < 4 * (count + 1) else int(rng.integers(0, count + 1))
        span = SPANS[(i // 3) % len(SPANS)] if c > 1 else 0
        base = BASES[(i // (3 * len(SPANS))) % len(BASES)]
        if base + span > 0xFFFFFFFE:
            base = 0xFFFFFFFE - span
        cnt[i] = c
        if c == 0:
            continue
        vals = base + rng.integers(0, span + 1, c)
        if c > 1:
            pos_hi = (0, c // 2, c - 1)[i % 3]
            pos_lo = (pos_hi + 1 + int(rng.integers(0, c - 1))) % c
            vals[pos_hi], vals[pos_lo] = base + span, base
        rows[i, :c] = vals.astype(np.uint32)
    return rows, cnt


# ---- tables of tests/test_packed_rows.py -------------------------------------------------------------------------
def _bad_status(n, seed):
    return np.random.default_rng(seed).choice(np.array([0, 2], np.uint8), size=n)  # dubious or expired only


def edge_table():
    """U(4) over 8,000 nodes, every node bad except 8 good ones per bucket b: at a = off[b] + 20 + b, at a + S with
    S = 249 + b, and six indices strictly between. A count-8 row is then a whole bucket's good nodes, its span S:
    249..264 over the 16 buckets, so spans 254 (packs) and 255 (escapes) sit side by side."""
    import tables as TB

    t = TB.uniform_config(8000, 4, seed=0x5A5E)
    n, off = t["ids"].shape[0], t["off"].astype(np.int64)
    st = _bad_status(n, 11)
    rng = np.random.default_rng(12)
    for b in range(16):
        S, a = 249 + b, int(off[b]) + 20 + b
        assert a + S < off[b + 1], "the bucket is too small for the construction"
        st[[a, a + S]] = 1
        st[a + 1 + rng.choice(S - 1, 6, replace=False)] = 1
    t["status"], t["name"] = st, "packed_edge"
    return t


def short_table():
    """The edge table with bucket 9 left 3 good nodes and buckets 8, 10 and 11 none: the rows of their targets are
    gathered from several buckets and span more than a thousand indices. (They still hold 8 entries, see few_table.)"""
    t = edge_table()
    st, off = t["status"].copy(), t["off"].astype(np.int64)
    bad = _bad_status(st.shape[0], 13)
    for b in (8, 10, 11):
        st[off[b]:off[b + 1]] = bad[off[b]:off[b + 1]]
    g = off[9] + np.nonzero(st[off[9]:off[10]] == 1)[0]
    st[g[3:]] = bad[g[3:]]
    t["status"], t["name"] = st, "packed_short"
    return t


def few_table(k: int, span: int):
    """The edge table's IDs with k good nodes in the whole table, all in bucket 9: at a, at a + span and k - 2
    between. The reference widens the window until it holds `count` good nodes or the table ends
    (routing_table.cpp:89-104), so a row is shorter than 8 only when the whole table holds fewer than 8 good nodes:
    every row of this table has cnt = k and spans `span`."""
    t = edge_table()
    off = t["off"].astype(np.int64)
    st = _bad_status(t["status"].shape[0], 14)
    a = int(off[9]) + 29
    assert a + span < off[10] and (k == 1) == (span == 0) and k - 2 <= span - 1
    st[[a, a + span]] = 1
    if k > 2:
        st[a + 1 + np.random.default_rng(15 + k).choice(span - 1, k - 2, replace=False)] = 1
    assert int((st == 1).sum()) == k
    t["status"], t["name"] = st, f"packed_few{k}_{span}"
    return t


def bucket_targets(t, extra=2000, seed=5):
    """Two node IDs inside every bucket, every bucket's first ID and its last (the next first minus one), `extra`
    random targets."""
    import tables as TB

    rng = np.random.default_rng(seed)
    off, first = t["off"].astype(np.int64), t["first"]
    inside = np.concatenate([rng.integers(off[b], off[b + 1], 2) for b in range(first.shape[0])])
    last = np.concatenate([TB._minus_one(first[1:]), np.full((1, 20), 255, np.uint8)])
    return np.ascontiguousarray(np.concatenate([t["ids"][inside], first, last,
                                                rng.integers(0, 256, (extra, 20), dtype=np.uint8)]), np.uint8)


def top64(ids) -> np.ndarray:
    """The IDs' top 64 bits as native uint64: kad_route_pack_keys' records, kad_rt_closest_keys_packed's keys."""
    hi = np.ascontiguousarray(np.asarray(ids, np.uint8).reshape(-1, 20)[:, :8])
    return hi.view(">u8").reshape(-1).astype(np.uint64)
