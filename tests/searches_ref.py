"""Dht::trySearchInsert and Search::insertNode restated for the tests (dht.cpp:816-849, 961-1047, 628-640, 458-460),
with Python big integers as IDs. The reference verdict of kad_sr_try_insert_batch is insertNode run
on a copy of the search, not the threshold rule, so the kernel's shortcut is pinned to the reference's own control
flow. Shared by test_searches*.py and test_search_ingest.py; nothing here touches the GPU."""
from bisect import bisect_left

import numpy as np

SEARCH_NODES = 14
NODE_EXPIRE_TIME = 600.0  # Node::NODE_EXPIRE_TIME, 10 minutes
SR_EXPIRED, SN_BAD = 1, 1
END, KNOWN, FAR, FAR_EXPIRED = 0, 1, 2, 3
MAX_ID = (1 << 160) - 1


class Node:
    """What insertNode reads of a Node: its ID, isExpired() and time. One Node per ID (NodeCache)."""
    __slots__ = ("id", "expired", "time")

    def __init__(self, id, expired=False, time=0.0):
        self.id, self.expired, self.time = id, expired, time


class SearchNode:
    __slots__ = ("node", "candidate")

    def __init__(self, node, candidate=False):
        self.node, self.candidate = node, candidate

    def is_bad(self):  # dht.cpp:458-460
        return self.node is None or self.node.expired or self.candidate


class Search:
    def __init__(self, id, expired=False, nodes=()):
        self.id, self.expired, self.nodes = id, expired, list(nodes)
        self.refusal = None  # why the last insert_node returned false without finding the node: FAR / FAR_EXPIRED

    def copy(self):
        return Search(self.id, self.expired, self.nodes)

    def remove_expired_node(self, now):  # dht.cpp:628-640
        e = len(self.nodes)
        while e != 0:
            e -= 1
            n = self.nodes[e].node
            if n.expired and n.time + NODE_EXPIRE_TIME < now:
                del self.nodes[e]
                return True
        return False

    def insert_node(self, snode, now, token=b""):  # dht.cpp:961-1047 (one family)
        nodes, nid = self.nodes, snode.id
        self.refusal = None
        found = False
        n = len(nodes)
        while n != 0:
            n -= 1
            if nodes[n].node.id == nid:  # n->node == snode: one Node per ID
                found = True
                break
            if (nid ^ self.id) > (nodes[n].node.id ^ self.id):  # id.xorCmp(nid, n->node->id) > 0
                n += 1
                break
        new_search_node = False
        if not found:
            t, bad, full = len(nodes), 0, False
            if self.expired:
                if len(nodes) >= SEARCH_NODES:
                    full = True
                    t = SEARCH_NODES
            else:
                bad = sum(1 for sn in nodes if sn.is_bad())
                full = len(nodes) - bad >= SEARCH_NODES
                while t - bad > SEARCH_NODES:
                    t -= 1
                    if nodes[t].is_bad():
                        bad -= 1
            if full:
                if t != len(nodes):
                    del nodes[t:]
                if n >= t:
                    self.refusal = FAR_EXPIRED if self.expired else FAR
                    return False
            nodes.insert(n, SearchNode(snode))
            snode.time = now
            new_search_node = True
            if snode.expired:
                if not self.expired:
                    bad += 1
            elif self.expired:
                bad = len(nodes) - 1
                self.expired = False
            while len(nodes) - bad > SEARCH_NODES:
                if not self.expired and nodes[-1].is_bad():
                    bad -= 1
                nodes.pop()
        if token:
            nodes[n].candidate = False
            self.expired = False
        if new_search_node:
            self.remove_expired_node(now)
        return new_search_node


def try_search_insert(searches, sids, node, now):
    """Dht::trySearchInsert (dht.cpp:816-849) over the family's searches in map order; sids their IDs."""
    closest = bisect_left(sids, node.id)
    inserted = False
    it = closest
    while it != len(searches):
        if not searches[it].insert_node(node, now):
            break
        inserted = True
        it += 1
    it = closest
    while it != 0:
        it -= 1
        if not searches[it].insert_node(node, now):
            break
        inserted = True
    return inserted


def trim(node_flags, search_flags):
    """Step 2 of the verdict (dht.cpp:989-1007) on flag bytes: (full, t)."""
    n = len(node_flags)
    if search_flags & SR_EXPIRED:
        full = n >= SEARCH_NODES
        return full, (SEARCH_NODES if full else n)
    bad = sum(1 for f in node_flags if f & SN_BAD)
    full, t = n - bad >= SEARCH_NODES, n
    while t - bad > SEARCH_NODES:
        t -= 1
        if node_flags[t] & SN_BAD:
            bad -= 1
    return full, t


def probe(search, x, now=0.0):
    """accept(s, x) by insertNode on a copy of the search: None if it accepts, else the stop code."""
    c = search.copy()
    if c.insert_node(Node(x), now):
        return None
    return KNOWN if c.refusal is None else c.refusal


def verdicts(searches, cands, now=0.0):
    """(lb, fwd, back, stop) of every candidate ID against the searches as they stand."""
    sids = [s.id for s in searches]
    S, q = len(searches), len(cands)
    lb, fwd, back = (np.zeros(q, np.uint32) for _ in range(3))
    stop = np.zeros(q, np.uint8)
    for j, x in enumerate(cands):
        l = bisect_left(sids, x)
        f = b = fs = bs = 0
        for s in range(l, S):
            v = probe(searches[s], x, now)
            if v is not None:
                fs = v
                break
            f += 1
        for s in range(l - 1, -1, -1):
            v = probe(searches[s], x, now)
            if v is not None:
                bs = v
                break
            b += 1
        lb[j], fwd[j], back[j], stop[j] = l, f, b, fs | bs << 4
    return lb, fwd, back, stop


def id_bytes(ids):
    """(len, 20) uint8 of integer IDs."""
    return np.frombuffer(b"".join(int(x).to_bytes(20, "big") for x in ids), np.uint8).reshape(-1, 20).copy()


def search_state(s):
    """(flags, node_ids (n, 20), node_flags (n,)) of one search: what a snapshot takes of it."""
    return (SR_EXPIRED if s.expired else 0, id_bytes([sn.node.id for sn in s.nodes]),
            np.array([SN_BAD if sn.is_bad() else 0 for sn in s.nodes], np.uint8))


def snapshot(searches):
    """The CSR arrays of kad_searches_create: ids, flags, off, node_ids, node_flags."""
    st = [search_state(s) for s in searches]
    off = np.zeros(len(searches) + 1, np.uint32)
    if st:
        off[1:] = np.cumsum([x[1].shape[0] for x in st])
    return (id_bytes([s.id for s in searches]), np.array([x[0] for x in st], np.uint8), off,
            np.concatenate([x[1] for x in st] + [np.zeros((0, 20), np.uint8)]),
            np.concatenate([x[2] for x in st] + [np.zeros(0, np.uint8)]))


class HostSearches:
    """The `host` of opendht_amd.try_search_insert over restated searches and candidate nodes."""

    def __init__(self, searches, cand_nodes, now):
        self.searches, self.cands, self.now = searches, cand_nodes, now

    def insert(self, s, j):
        return self.searches[s].insert_node(self.cands[j], self.now)

    def state(self, s):
        return search_state(self.searches[s])


# ---- inputs ---------------------------------------------------------------------------------------------------------
STATES = ("empty", "notfull", "full", "expired", "trim", "cap")


def make_list(rng, sid, n):
    """n distinct nodes in ascending XOR distance to sid, all sharing a random prefix of 8..120 bits with it, as the
    closest nodes of a large population do: a random candidate is then farther than every one of them."""
    ids, shift = set(), int(rng.integers(8, 121))
    while len(ids) < n:
        ids.add(sid ^ (int.from_bytes(rng.bytes(20), "big") >> shift))
    return sorted(ids, key=lambda v: v ^ sid)


def make_search(rng, sid, state, cap, now=0.0):
    """One search in the named state. Expired nodes carry a recent time, so removeExpiredNode keeps them, except in
    the `trim` state where some are old."""
    def nodes_of(ids, bad_at=(), cand_at=(), old_at=()):
        return [SearchNode(Node(v, expired=i in bad_at, time=(now - 2 * NODE_EXPIRE_TIME) if i in old_at else now),
                           candidate=i in cand_at) for i, v in enumerate(ids)]
    if state == "empty":
        return Search(sid)
    if state == "notfull":
        n = int(rng.integers(1, SEARCH_NODES))
        return Search(sid, False, nodes_of(make_list(rng, sid, n), bad_at={int(rng.integers(0, n))} if n > 3 else ()))
    if state == "full":
        return Search(sid, False, nodes_of(make_list(rng, sid, SEARCH_NODES)))
    if state == "expired":  # at least 14 expired nodes
        n = int(rng.integers(SEARCH_NODES, min(cap, 20) + 1))
        return Search(sid, True, nodes_of(make_list(rng, sid, n), bad_at=set(range(n))))
    if state == "trim":  # 15-30 entries with bad nodes spread: the trim loop moves t
        n = int(rng.integers(15, min(cap, 30) + 1))
        bad = set(int(v) for v in rng.choice(n, size=int(rng.integers(0, n - SEARCH_NODES + 1)), replace=False))
        cand = set(v for v in bad if v % 2)
        return Search(sid, False, nodes_of(make_list(rng, sid, n), bad_at=bad - cand, cand_at=cand,
                                           old_at=set(v for v in bad if v % 3 == 0)))
    if state == "cap":  # exactly cap entries, all but 13 of them bad: not full
        bad = set(int(v) for v in rng.choice(cap, size=cap - 13, replace=False))
        return Search(sid, False, nodes_of(make_list(rng, sid, cap), cand_at=bad))
    raise ValueError(state)


def make_ids(rng, S):
    """S distinct ascending search IDs: random ones, neighbours differing in the last bit, runs sharing the 64-bit
    key, 0 and 2^160 - 1."""
    ids = set()
    if S >= 2:
        ids |= {0, MAX_ID}
    while len(ids) < S:
        kind, v = int(rng.integers(0, 4)), int.from_bytes(rng.bytes(20), "big")
        if kind == 0 and len(ids) + 2 <= S:
            ids |= {v, v ^ 1}
        elif kind == 1:
            key = v >> 96 << 96
            for _ in range(min(int(rng.integers(2, 7)), S - len(ids))):
                ids.add(key | int.from_bytes(rng.bytes(12), "big"))
        else:
            ids.add(v)
    return sorted(ids)[:S] if len(ids) > S else sorted(ids)


def make_set(rng, S, states, cap, run=4):
    """S searches whose states come from `states` in runs of up to `run` searches."""
    ids, out = make_ids(rng, S), []
    while len(out) < S:
        st = states[int(rng.integers(0, len(states)))]
        for _ in range(min(int(rng.integers(1, run + 1)), S - len(out))):
            out.append(make_search(rng, ids[len(out)], st, cap))
    return out


def make_cands(rng, searches, q):
    """q candidate IDs: random, near a search ID, search IDs and their neighbours, members before and after t, the
    threshold ID with its last bit flipped, the threshold's key with another tail."""
    out, S = [], len(searches)
    while len(out) < q:
        kind, v = int(rng.integers(0, 9)), int.from_bytes(rng.bytes(20), "big")
        s = searches[int(rng.integers(0, S))] if S else None
        if kind == 0 or s is None:
            out.append(v)
        elif kind == 8:  # sharing a prefix with a search ID
            out.append(s.id ^ (v >> int(rng.integers(8, 150))))
        elif kind == 1:
            out.append(s.id)
        elif kind == 2:
            out.append(min(s.id + 1, MAX_ID))
        elif kind == 3:
            out.append(max(s.id - 1, 0))
        elif not s.nodes:
            out.append(s.id ^ (v >> 150))  # near an empty search
        else:
            fl = [SN_BAD if sn.is_bad() else 0 for sn in s.nodes]
            _, t = trim(fl, SR_EXPIRED if s.expired else 0)
            thr = s.nodes[max(t, 1) - 1].node.id
            if kind == 4:  # a member, before or after t
                out.append(s.nodes[int(rng.integers(0, len(s.nodes)))].node.id)
            elif kind == 5 and t < len(s.nodes):
                out.append(s.nodes[int(rng.integers(t, len(s.nodes)))].node.id)
            elif kind == 6:
                out.append(thr ^ 1)
            else:
                out.append((thr >> 96 << 96) | (v & ((1 << 96) - 1)))
    return out
