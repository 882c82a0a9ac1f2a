"""kad_sr_insert restated for the tests at the level of flag bytes: a search is (ID, expired,
[(node ID, flag byte), ...]) as the device set holds it, and insert_one is Search::insertNode (dht.cpp:961-1047) with
removeExpiredNode (:628-640) on that list, a candidate being (ID, KAD_SN_BAD or 0). test_sr_insert_model.py pins it to
searches_ref.Search.insert_node; the GPU tests compare the device call with it. Also the host double of
opendht_amd.try_search_insert_device and a device set made of the model (the CPU half of test_sr_insert_ingest.py).
Shared by test_sr_insert*.py; nothing here touches the GPU."""
import functools

import numpy as np

import refill_ref as F
import searches_ref as R

SEARCH_NODES = R.SEARCH_NODES
SN_BAD, SN_REMOVABLE = R.SN_BAD, F.SN_REMOVABLE
INSERT_OK, INSERT_OVERFLOW = 0, 1
NOW = F.NOW


class FlagSearch:
    """One search as the device holds it."""
    __slots__ = ("id", "expired", "ents")

    def __init__(self, id, expired=False, ents=()):
        self.id, self.expired, self.ents = id, bool(expired), list(ents)

    def copy(self):
        return FlagSearch(self.id, self.expired, self.ents)

    def key(self):
        return self.id, self.expired, tuple(self.ents)


def new_stats():
    return {k: 0 for k in ("found", "refusal_trims", "flips", "bad_no_flip", "pops", "erases", "sixty_fifth")}


def insert_one(s, x, xfl, stats=None):
    """s.insertNode(x, now, empty token) on the flag-level list: True if a new entry was made."""
    ents = s.ents
    if any(e[0] == x for e in ents):  # found (:972-984)
        if stats is not None:
            stats["found"] += 1
        return False
    pos = sum(1 for e in ents if (e[0] ^ s.id) < (x ^ s.id))
    full, t = R.trim([e[1] for e in ents], R.SR_EXPIRED if s.expired else 0)
    if full:  # :1009-1013: the trim happens even when the candidate is then refused
        if t < len(ents):
            del ents[t:]
            if stats is not None and pos >= t:
                stats["refusal_trims"] += 1
        if pos >= t:
            return False
    ents.insert(pos, (x, xfl & SN_BAD))  # node.time = now: never REMOVABLE
    before = len(ents)
    if s.expired:
        if xfl & SN_BAD:  # `bad` stays 0 and the search expired: pops down to SEARCH_NODES entries
            del ents[SEARCH_NODES:]
            if stats is not None:
                stats["bad_no_flip"] += 1
        else:  # :1026-1029
            s.expired = False
            if stats is not None:
                stats["flips"] += 1
    else:  # :1031-1035: pops until 14 entries are not BAD, i.e. from the 15th such entry on
        good = 0
        for i, e in enumerate(ents):
            if not e[1] & SN_BAD:
                good += 1
                if good == SEARCH_NODES + 1:
                    del ents[i:]
                    break
    if stats is not None and len(ents) < before:
        stats["pops"] += 1
    for i in range(len(ents) - 1, -1, -1):  # removeExpiredNode
        if ents[i][1] & SN_REMOVABLE:
            del ents[i]
            if stats is not None:
                stats["erases"] += 1
            break
    if stats is not None and before == 65 and len(ents) <= 64:  # the 65th entry of a cap = 64 list came and went
        stats["sixty_fifth"] += 1
    return True


def insert_list(s, cands, cap, stats=None):
    """kad_sr_insert on one search: (search afterwards, result bytes, status). An overflowing search is returned as it
    was (the same object), with zeros."""
    c = s.copy()
    out = np.zeros(len(cands), np.uint8)
    for j, (x, xfl) in enumerate(cands):
        out[j] = insert_one(c, x, xfl, stats)
        if len(c.ents) > cap:
            return s, np.zeros(len(cands), np.uint8), INSERT_OVERFLOW
    return (c if len(cands) else s), out, INSERT_OK


def device_insert(searches, which, lists, cap, stats=None):
    """What kad_sr_insert must give: (searches afterwards, inserted bytes, status)."""
    after = list(searches)
    ins, status = [np.zeros(0, np.uint8)], np.zeros(len(which), np.uint8)
    for k, s in enumerate(which):
        after[s], o, status[k] = insert_list(searches[s], lists[k], cap, stats)
        ins.append(o)
    return after, np.concatenate(ins), status


def csr(lists):
    """(off, cand_ids, cand_flags) of per-search candidate lists."""
    off = np.zeros(len(lists) + 1, np.uint32)
    if lists:
        off[1:] = np.cumsum([len(c) for c in lists])
    flat = [x for c in lists for x in c]
    return (off, R.id_bytes([x[0] for x in flat]) if flat else np.zeros((0, 20), np.uint8),
            np.array([x[1] for x in flat], np.uint8))


def snapshot(searches):
    """The CSR arrays of kad_searches_create: ids, flags, off, node_ids, node_flags."""
    off = np.zeros(len(searches) + 1, np.uint32)
    if searches:
        off[1:] = np.cumsum([len(s.ents) for s in searches])
    flat = [e for s in searches for e in s.ents]
    return (R.id_bytes([s.id for s in searches]) if searches else np.zeros((0, 20), np.uint8),
            np.array([R.SR_EXPIRED if s.expired else 0 for s in searches], np.uint8), off,
            R.id_bytes([e[0] for e in flat]) if flat else np.zeros((0, 20), np.uint8),
            np.array([e[1] for e in flat], np.uint8))


def expected_export(searches, cap):
    """What kad_searches_export gives for a set created from these searches."""
    S = len(searches)
    out = {"ids": R.id_bytes([s.id for s in searches]) if S else np.zeros((0, 20), np.uint8),
           "flags": np.zeros(S, np.uint8), "n": np.zeros(S, np.uint32), "full": np.zeros(S, np.uint8),
           "t": np.zeros(S, np.uint32), "node_ids": np.zeros((S, cap, 20), np.uint8),
           "node_flags": np.zeros((S, cap), np.uint8)}
    for i, s in enumerate(searches):
        nfl = [e[1] for e in s.ents]
        fl = R.SR_EXPIRED if s.expired else 0
        full, t = R.trim(nfl, fl)
        out["flags"][i], out["n"][i], out["full"][i], out["t"][i] = fl, len(nfl), full, t
        if nfl:
            out["node_ids"][i, :len(nfl)] = R.id_bytes([e[0] for e in s.ents])
            out["node_flags"][i, :len(nfl)] = nfl
    return out


def from_search(s, now):
    """The flag-level form of a searches_ref.Search, KAD_SN_REMOVABLE evaluated at `now`."""
    return FlagSearch(s.id, s.expired, [(sn.node.id, F.node_flag(sn, now)) for sn in s.nodes])


def to_search(fs, now):
    """A searches_ref.Search with the same flag bytes at `now` (every node its own Node object)."""
    return R.Search(fs.id, fs.expired,
                    [R.SearchNode(R.Node(v, expired=bool(fl & SN_REMOVABLE) or bool(fl & SN_BAD),
                                         time=(now - 2 * R.NODE_EXPIRE_TIME) if fl & SN_REMOVABLE else now))
                     for v, fl in fs.ents])


# ---- the host double of try_search_insert_device ---------------------------------------------------------------------
class HostInsert:
    """`host` over restated searches and candidate nodes (one Node per ID, shared by searches and candidates)."""

    def __init__(self, searches, cand_nodes, now):
        self.searches, self.cands, self.now = searches, cand_nodes, now

    def insert(self, s, j):
        return self.searches[s].insert_node(self.cands[j], self.now)

    def state(self, s, now):
        return F.search_state(self.searches[s], now)

    def bad(self, j):
        return self.cands[j].expired

    def old(self, j):
        return F.removable(self.cands[j], self.now)

    def holders(self, j):
        node = self.cands[j]
        return [i for i, s in enumerate(self.searches) if any(sn.node is node for sn in s.nodes)]


class ModelSearches:
    """A device set made of the model, with the calls try_search_insert_device uses: verdicts by
    searches_ref.verdicts, the insert by device_insert."""

    def __init__(self, searches, cap, now):
        self.s = [from_search(x, now) for x in searches]
        self.S, self.cap, self.now = len(searches), cap, now
        self._ref = [None] * self.S  # to_search of every search, dropped when it changes
        self._ver = [0] * self.S     # bumped with every change
        self._seen = {}              # candidate ID -> (its verdict, the probed searches, their versions then)

    def _changed(self, s):
        self._ref[s] = None
        self._ver[s] += 1

    def try_insert_host(self, ids):
        """searches_ref.verdicts on the searches as they stand; a candidate's verdict is taken again only when a
        search it probed has changed since."""
        cands = [int.from_bytes(bytes(r), "big") for r in np.asarray(ids, np.uint8).reshape(-1, 20)]
        for s in range(self.S):
            if self._ref[s] is None:
                self._ref[s] = to_search(self.s[s], self.now)
        stale = sorted(set(x for x in cands if x not in self._seen or
                           self._seen[x][2] != self._ver[self._seen[x][1].start:self._seen[x][1].stop]))
        for x, l, f, b, st in zip(stale, *R.verdicts(self._ref, stale, self.now)):
            probed = range(max(int(l) - int(b) - 1, 0), min(int(l) + int(f) + 1, self.S))
            self._seen[x] = ((l, f, b, st), probed, self._ver[probed.start:probed.stop])
        out = [self._seen[x][0] for x in cands]
        return (np.array([v[0] for v in out], np.uint32), np.array([v[1] for v in out], np.uint32),
                np.array([v[2] for v in out], np.uint32), np.array([v[3] for v in out], np.uint8))

    def export(self, nodes=True):
        return expected_export(self.s, self.cap)

    def insert(self, which, off, cand_ids, cand_flags=None):
        ids = [int.from_bytes(bytes(r), "big") for r in np.asarray(cand_ids, np.uint8).reshape(-1, 20)]
        fl = [0] * len(ids) if cand_flags is None else [int(v) for v in cand_flags]
        lists = [[(ids[k], fl[k]) for k in range(int(off[i]), int(off[i + 1]))] for i in range(len(which))]
        self.s, ins, status = device_insert(self.s, [int(s) for s in which], lists, self.cap)
        for s in which:
            self._changed(int(s))
        return ins, status

    def patch(self, which, flags, off, node_ids, node_flags):
        for k, s in enumerate(which):
            a, b = int(off[k]), int(off[k + 1])
            assert b - a <= self.cap
            self.s[int(s)] = FlagSearch(self.s[int(s)].id, flags[k] & R.SR_EXPIRED,
                                        [(int.from_bytes(bytes(node_ids[e]), "big"), int(node_flags[e]))
                                         for e in range(a, b)])
            self._changed(int(s))

    def grow(self, cap):
        assert cap >= self.cap
        self.cap = cap


# ---- inputs of the GPU cases -----------------------------------------------------------------------------------------
STATES = ("empty", "notfull", "full", "expired", "expired_short", "trim", "cap", "cap_removable", "expired_cap")


def make_search(rng, sid, state, cap):
    def flags(n, bad, removable_part=0.4):
        return [(SN_BAD | (SN_REMOVABLE if rng.random() < removable_part else 0)) if i in bad else 0 for i in range(n)]
    if state == "empty":
        return FlagSearch(sid)
    if state == "notfull":
        n = int(rng.integers(1, SEARCH_NODES))
        fl = flags(n, {int(rng.integers(0, n))} if n > 3 else set())
    elif state == "full":
        n = SEARCH_NODES
        fl = flags(n, set())
    elif state == "expired":
        n = int(rng.integers(SEARCH_NODES, min(cap, 20) + 1))
        fl = flags(n, set(range(n)))
    elif state == "expired_short":
        n = int(rng.integers(1, SEARCH_NODES))
        fl = flags(n, set(range(n)))
    elif state == "expired_cap":  # an expired search of cap entries: every candidate that is not found trims it to 14
        n = cap
        fl = flags(n, set(range(n)))
    elif state == "trim":
        n = int(rng.integers(15, min(cap, 30) + 1))
        fl = flags(n, set(int(v) for v in rng.choice(n, size=int(rng.integers(0, n - SEARCH_NODES + 1)), replace=False)))
    elif state in ("cap", "cap_removable"):  # exactly cap entries, 13 of them good: not full; an insert overflows
        n = cap                              # unless an entry is REMOVABLE
        fl = flags(n, set(int(v) for v in rng.choice(cap, size=cap - 13, replace=False)),
                   0.0 if state == "cap" else 0.3)
    else:
        raise ValueError(state)
    return FlagSearch(sid, state.startswith("expired"), list(zip(R.make_list(rng, sid, n), fl)))


def states_for(cap):
    return tuple(s for s in STATES if (s != "trim" or cap >= 16) and (not s.startswith("cap") or cap > 14))


def make_set(rng, S, cap):
    ids, states, out = R.make_ids(rng, S), states_for(cap), []
    while len(out) < S:
        st = states[len(out) % len(states)] if S <= 16 else states[int(rng.integers(0, len(states)))]
        for _ in range(min(int(rng.integers(1, 4)), S - len(out))):
            out.append(make_search(rng, ids[len(out)], st, cap))
    return out


def make_cand_list(rng, s, n):
    """n candidates for search s: far and near strangers, members, the threshold +-1, IDs sharing the search's 64-bit
    key, repeats of earlier candidates; 30 % expired."""
    out = []
    full, t = R.trim([e[1] for e in s.ents], R.SR_EXPIRED if s.expired else 0)
    while len(out) < n:
        kind, v = int(rng.integers(0, 8)), int.from_bytes(rng.bytes(20), "big")
        if kind == 0:
            x = v
        elif kind == 1:  # close: shares a long prefix with the search ID
            x = s.id ^ (v >> int(rng.integers(8, 150)))
        elif kind == 2 and out:
            x = out[int(rng.integers(0, len(out)))][0]
        elif kind == 3 and s.ents:
            x = s.ents[int(rng.integers(0, len(s.ents)))][0]
        elif kind == 4 and t:
            x = s.ents[t - 1][0] ^ (1 << int(rng.integers(0, 2)))
        elif kind == 5:  # the search's 64-bit key with another tail
            x = (s.id >> 96 << 96) | (v & ((1 << 96) - 1))
        elif kind == 6 and s.ents:  # a member's key with another tail
            x = (s.ents[int(rng.integers(0, len(s.ents)))][0] >> 96 << 96) | (v & ((1 << 96) - 1))
        else:
            x = s.id ^ (v >> int(rng.integers(100, 160)))
        out.append((x, SN_BAD if rng.random() < 0.3 else 0))
    return out


COUNTS = (0, 1, 14, 63, 64, 65, 130)

# name: (searches S, cap, listed searches ("all", ("m", count) or "third"), seed)
CASES = {
    "s0": (0, 32, "all", 1),
    "s1": (1, 32, "all", 2),
    "s3_cap14": (3, 14, "all", 3),
    "s3_cap64": (3, 64, "all", 4),
    "s65_cap14": (65, 14, "all", 5),
    "s65_cap32": (65, 32, "all", 6),
    "s65_cap64": (65, 64, "all", 7),
    "s300_cap32": (300, 32, "third", 8),
    "s300_cap64": (300, 64, "third", 9),
    "m63": (300, 32, ("m", 63), 10),
    "m64": (300, 64, ("m", 64), 11),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """Built once, never changed: the searches before, which, the candidate lists, and the expected result of
    kad_sr_insert (after, ins, status), of a second call with the same lists (after2, ins2, status2), with the
    mechanism counts of the model."""
    S, cap, kind, seed = CASES[name]
    rng = np.random.default_rng(seed)
    searches = make_set(rng, S, cap)
    which = F.make_which(rng, S, kind) if S else np.zeros(0, np.uint32)
    lists = [make_cand_list(rng, searches[int(s)], COUNTS[(k + seed) % len(COUNTS)]) for k, s in enumerate(which)]
    stats = new_stats()
    w = [int(s) for s in which]
    after, ins, status = device_insert(searches, w, lists, cap, stats)
    after2, ins2, status2 = device_insert(after, w, lists, cap)
    return {"searches": searches, "which": which, "lists": lists, "cap": cap, "after": after, "ins": ins,
            "status": status, "after2": after2, "ins2": ins2, "status2": status2, "stats": stats}
