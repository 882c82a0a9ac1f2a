"""Dht::refill restated for the tests (dht.cpp:1647-1668): NodeCache::getCachedNodes (node_cache.cpp:36-66) over a
population of searches_ref.Node objects, one per ID, shared by the cache and the searches, then the loop of
dht.cpp:1659-1663 over searches_ref.Search.insert_node. The reference result of kad_sr_refill.
Shared by test_refill*.py; nothing here touches the GPU."""
import functools
from bisect import bisect_left

import numpy as np

import searches_ref as R

SEARCH_NODES = R.SEARCH_NODES
SN_REMOVABLE = 2
REFILL_OK, REFILL_OVERFLOW = 0, 1
NO_NODE = 0xFFFFFFFF
STATUS_GOOD, STATUS_EXPIRED = 1, 2
NOW = 10_000.0
TIMES = (NOW, NOW - 100.0, NOW - 700.0, NOW - 1300.0)
STATES = R.STATES + ("expired_short",)


class Cache:
    """One family's NodeCache map: ids ascending, nodes[i] the Node of ids[i]."""

    def __init__(self, nodes):
        self.nodes = sorted(nodes, key=lambda n: n.id)
        self.ids = [n.id for n in self.nodes]

    def get_cached_nodes(self, target, count=SEARCH_NODES):
        """node_cache.cpp:36-66 with indices for iterators: the indices of the result in walk order."""
        c, end = self.ids, len(self.ids)
        it_n = bisect_left(c, target)
        it_p = it_n
        out = []
        if it_p != 0:
            it_p -= 1
        while len(out) < count and (it_n != end or it_p != end):
            if it_p == end:
                it, it_n = it_n, it_n + 1
            elif it_n == end:
                it, it_p = it_p, it_p - 1
            elif (c[it_p] ^ target) < (c[it_n] ^ target):  # id.xorCmp(it_p->first, it_n->first) < 0
                it, it_p = it_p, it_p - 1
            else:
                it, it_n = it_n, it_n + 1
            if it == 0:
                it_p = end
            if not self.nodes[it].expired:
                out.append(it)
        return out

    def table_arrays(self):
        """ids (N, 20) and status (N,) of the KAD_TABLE_SORTED device table."""
        return (R.id_bytes(self.ids) if self.ids else np.zeros((0, 20), np.uint8),
                np.array([STATUS_EXPIRED if n.expired else STATUS_GOOD for n in self.nodes], np.uint8))


def removable(node, now):
    return node.expired and node.time + R.NODE_EXPIRE_TIME < now


def node_flag(sn, now):
    return (R.SN_BAD if sn.is_bad() else 0) | (SN_REMOVABLE if removable(sn.node, now) else 0)


def search_state(s, now):
    """(flags, node_ids (n, 20), node_flags (n,)) with KAD_SN_REMOVABLE evaluated at `now`."""
    return (R.SR_EXPIRED if s.expired else 0, R.id_bytes([sn.node.id for sn in s.nodes]),
            np.array([node_flag(sn, now) for sn in s.nodes], np.uint8))


def snapshot(searches, now):
    """The CSR arrays of kad_searches_create: ids, flags, off, node_ids, node_flags."""
    st = [search_state(s, now) for s in searches]
    off = np.zeros(len(searches) + 1, np.uint32)
    if st:
        off[1:] = np.cumsum([x[1].shape[0] for x in st])
    return (R.id_bytes([s.id for s in searches]) if searches else np.zeros((0, 20), np.uint8),
            np.array([x[0] for x in st], np.uint8), off,
            np.concatenate([x[1] for x in st] + [np.zeros((0, 20), np.uint8)]),
            np.concatenate([x[2] for x in st] + [np.zeros(0, np.uint8)]))


def expected_export(searches, cap, now):
    """What kad_searches_export gives for a set created from these searches (as test_searches.expected_export)."""
    S = len(searches)
    out = {"ids": R.id_bytes([s.id for s in searches]) if S else np.zeros((0, 20), np.uint8),
           "flags": np.zeros(S, np.uint8), "n": np.zeros(S, np.uint32), "full": np.zeros(S, np.uint8),
           "t": np.zeros(S, np.uint32), "node_ids": np.zeros((S, cap, 20), np.uint8),
           "node_flags": np.zeros((S, cap), np.uint8)}
    for i, s in enumerate(searches):
        fl, nid, nfl = search_state(s, now)
        full, t = R.trim(list(nfl), fl)
        out["flags"][i], out["n"][i], out["full"][i], out["t"][i] = fl, len(nfl), full, t
        out["node_ids"][i, :len(nfl)] = nid
        out["node_flags"][i, :len(nfl)] = nfl
    return out


def new_stats():
    return {k: 0 for k in ("found", "refusal_trims", "insert_shrinks", "insert_with_removable", "flips")}


def insert_row(search, nodes, now, cap=None, stats=None):
    """The loop of dht.cpp:1659-1663 over the row's nodes: (mask of the inserts that returned true, whether the list
    held more than cap entries after some insert_node returned)."""
    mask, over = 0, False
    for j, node in enumerate(nodes):
        before, was_expired = len(search.nodes), search.expired
        had_removable = any(removable(sn.node, now) for sn in search.nodes)
        ok = search.insert_node(node, now)
        if ok:
            mask |= 1 << j
        if stats is not None:
            after = len(search.nodes)
            stats["found"] += (not ok) and search.refusal is None
            stats["refusal_trims"] += (not ok) and after < before
            stats["insert_shrinks"] += ok and after < before + 1
            stats["insert_with_removable"] += ok and had_removable
            stats["flips"] += was_expired and not search.expired
        if cap is not None and len(search.nodes) > cap:
            over = True
    return mask, over


def refill(search, cache, now, cap=None, stats=None):
    """Dht::refill on one search: (row of cache indices, mask, overflowed). cnt == 0 leaves the search untouched."""
    row = cache.get_cached_nodes(search.id, SEARCH_NODES)
    if not row:
        return row, 0, False
    mask, over = insert_row(search, [cache.nodes[i] for i in row], now, cap, stats)
    return row, mask, over


def device_refill(searches, cache, which, now, cap, index_base=0, stats=None):
    """What kad_sr_refill must give: (searches afterwards, rows, cnt, inserted, status). An overflowed search keeps its
    old state and its mask is 0."""
    after = list(searches)
    m = len(which)
    rows = np.full((m, SEARCH_NODES), NO_NODE, np.uint32)
    cnt, ins, status = np.zeros(m, np.uint8), np.zeros(m, np.uint16), np.zeros(m, np.uint8)
    for k, s in enumerate(which):
        c = searches[s].copy()
        row, mask, over = refill(c, cache, now, cap, stats)
        rows[k, :len(row)] = np.array(row, np.uint32) + index_base
        cnt[k] = len(row)
        if over:
            status[k] = REFILL_OVERFLOW
        else:
            ins[k], after[s] = mask, c
    return after, rows, cnt, ins, status


class HostRefill:
    """The `host` of opendht_amd.refill_searches over restated searches and a restated cache."""

    def __init__(self, searches, cache, now, index_base=0):
        self.searches, self.cache, self.now, self.base = searches, cache, now, index_base

    def insert_row(self, s, row):
        return insert_row(self.searches[s], [self.cache.nodes[int(i) - self.base] for i in row], self.now)[0]

    def state(self, s, now):
        return search_state(self.searches[s], now)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def make_cache(rng, N, expired_part=0.2):
    ids = set()
    while len(ids) < N:
        ids.add(int.from_bytes(rng.bytes(20), "big"))
    return Cache([R.Node(v, expired=bool(rng.random() < expired_part), time=TIMES[int(rng.integers(0, 4))])
                  for v in ids])


def make_search(rng, sid, state, cap, cache):
    """One search in the named state. Its nodes come partly from the cache around sid (members the walk returns,
    farther ones, expired ones: the cache's own Node objects) and partly from strangers sharing a prefix with sid."""
    if state == "empty":
        return R.Search(sid)
    if state == "notfull":
        n = int(rng.integers(1, SEARCH_NODES))
        bad = {int(rng.integers(0, n))} if n > 3 else set()
    elif state == "full":
        n, bad = SEARCH_NODES, set()
    elif state == "expired":
        n = int(rng.integers(SEARCH_NODES, min(cap, 20) + 1))
        bad = set(range(n))
    elif state == "expired_short":  # an expired search the first good node revives
        n = int(rng.integers(1, SEARCH_NODES))
        bad = set(range(n))
    elif state == "trim":
        n = int(rng.integers(15, min(cap, 30) + 1))
        bad = set(int(v) for v in rng.choice(n, size=int(rng.integers(0, n - SEARCH_NODES + 1)), replace=False))
    elif state == "cap":  # exactly cap entries, 13 of them good: not full
        n = cap
        bad = set(int(v) for v in rng.choice(cap, size=cap - 13, replace=False))
    else:
        raise ValueError(state)
    lb = bisect_left(cache.ids, sid)
    near = list(range(max(lb - 24, 0), min(lb + 24, len(cache.ids))))
    picked, shift = {}, int(rng.integers(2, 40))
    plain = state == "cap" and bool(rng.integers(0, 2))  # its bad strangers are candidates: nothing to erase
    for i in rng.permutation(len(near))[:int(rng.integers(0, n + 1))]:
        node = cache.nodes[near[int(i)]]
        picked[node.id] = node
    while len(picked) < n:
        v = sid ^ (int.from_bytes(rng.bytes(20), "big") >> shift)
        if v not in picked and v not in cache.ids[max(lb - 1, 0):lb + 1]:
            picked[v] = None
    out = []
    for i, v in enumerate(sorted(picked, key=lambda v: v ^ sid)):
        node, want_bad = picked[v], i in bad
        if node is not None and node.expired and not want_bad:  # a good place: a stranger instead
            node = None
            while v in picked or v in cache.ids[max(lb - 24, 0):lb + 24]:
                v ^= 1 << int(rng.integers(0, 60))
        if node is None:
            expired = want_bad and not plain and bool(i % 2 == 0 or state.startswith("expired"))
            node = R.Node(v, expired=expired, time=TIMES[int(rng.integers(0, 4))])
        out.append(R.SearchNode(node, candidate=want_bad and not node.expired))
    out.sort(key=lambda sn: sn.node.id ^ sid)
    return R.Search(sid, state.startswith("expired"), out)


def make_set(rng, S, states, cap, cache, run=4):
    """S searches (IDs as searches_ref.make_ids, some beside cache nodes) whose states come in runs."""
    ids = set(R.make_ids(rng, S))
    for v in list(ids)[::5]:  # every fifth beside a cache node
        if cache.ids:
            ids.discard(v)
            ids.add(cache.ids[int(rng.integers(0, len(cache.ids)))] ^ (1 << int(rng.integers(0, 100))))
    while len(ids) < S:
        ids.add(int.from_bytes(rng.bytes(20), "big"))
    ids, out = sorted(ids)[:S], []
    while len(out) < S:
        st = states[int(rng.integers(0, len(states)))]
        for _ in range(min(int(rng.integers(1, run + 1)), S - len(out))):
            out.append(make_search(rng, ids[len(out)], st, cap, cache))
    return out


def states_for(cap):
    return tuple(s for s in STATES if s != "trim" or cap >= 16)


def make_which(rng, S, kind):
    if kind == "all":
        w = np.arange(S)
    elif kind == "one":
        w = np.array([S // 2])
    elif kind == "first_last":
        w = np.array([0, S - 1])
    elif kind == "third":  # a third of the searches with a run of consecutive ones
        w = np.unique(np.concatenate([rng.choice(S, size=max(S // 3, 1), replace=False), np.arange(min(5, S))]))
    else:  # ("m", count)
        w = np.sort(rng.choice(S, size=kind[1], replace=False))
    return w.astype(np.uint32)


# name: (cache nodes N, searches S, cap, which, index_base, seed)
CASES = {
    "n0_s3": (0, 3, 32, "all", 0, 1),
    "n1_s3": (1, 3, 32, "all", 7, 2),
    "n13_s65_cap14": (13, 65, 14, "all", 0, 3),
    "n40_s65_cap14": (40, 65, 14, "third", 0, 4),
    "n40_s1": (40, 1, 32, "one", 0, 5),
    "n40_s0": (40, 0, 32, "all", 0, 6),
    "n40_s3_cap64": (40, 3, 64, "first_last", 0, 7),
    "n3000_s300_cap32": (3000, 300, 32, "all", 1000, 8),
    "n3000_s300_cap64": (3000, 300, 64, "third", 0, 9),
    "n3000_s300_cap14": (3000, 300, 14, "first_last", 0, 10),
    "n3000_s300_one": (3000, 300, 32, "one", 0, 11),
    "n3000_s65_cap64": (3000, 65, 64, "all", 0, 12),
    "m63": (3000, 300, 32, ("m", 63), 0, 13),
    "m64": (3000, 300, 32, ("m", 64), 0, 14),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """Built once, never changed: dict with the cache, the searches before, which, and the expected result of
    kad_sr_refill (after, rows, cnt, ins, status) with the mechanism counts of the restatement."""
    N, S, cap, kind, base, seed = CASES[name]
    rng = np.random.default_rng(seed)
    cache = make_cache(rng, N)
    searches = make_set(rng, S, states_for(cap), cap, cache)
    which = make_which(rng, S, kind) if S else np.zeros(0, np.uint32)
    stats = new_stats()
    after, rows, cnt, ins, status = device_refill(searches, cache, [int(s) for s in which], NOW, cap, base, stats)
    return {"cache": cache, "searches": searches, "which": which, "cap": cap, "base": base, "after": after,
            "rows": rows, "cnt": cnt, "ins": ins, "status": status, "stats": stats}
