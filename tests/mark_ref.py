"""kad_sr_mark_nodes restated for the tests at the level of flag bytes, over insert_ref.FlagSearch
sets: node ops (clear / set per node ID), pair overrides (the exact byte of one entry of one search), the changed
searches, their counts and the per-node hit counts. test_sr_mark_model.py pins it to searches_ref (shared Node objects
whose expired / time / candidate change); the GPU tests compare the device call with it. Also the inputs of the GPU
cases and the host double of opendht_amd.mark_search_nodes. Shared by test_sr_mark*.py; nothing here touches the GPU."""
import functools

import numpy as np

import insert_ref as I
import refill_ref as F
import searches_ref as R

SEARCH_NODES = R.SEARCH_NODES
SEARCH_MAX_BAD_NODES = 25  # dht.h:324
SN_BAD, SN_REMOVABLE = I.SN_BAD, I.SN_REMOVABLE
BOTH = SN_BAD | SN_REMOVABLE
REC_FULL, REC_EXPIRED = 1, 2
LDS_KEYS = 4096  # the scan kernel stages up to this many batch keys in LDS
NOW = I.NOW


def counts_of(s):
    """The four count bytes of one search: n, bad, leading bad, record bits."""
    fl = [e[1] for e in s.ents]
    full, _ = R.trim(fl, R.SR_EXPIRED if s.expired else 0)
    lead = 0
    while lead < len(fl) and fl[lead] & SN_BAD:
        lead += 1
    return (len(fl), sum(1 for f in fl if f & SN_BAD), lead,
            (REC_FULL if full else 0) | (REC_EXPIRED if s.expired else 0))


def mark(searches, nodes, clear, setb, pairs):
    """What kad_sr_mark_nodes must give. nodes: distinct IDs; clear / setb: one byte each; pairs: (search, ID, byte).
    Returns (searches afterwards, hits, pair_found, changed, counts); an unchanged search stays the same object."""
    ops = {x: (j, int(clear[j]), int(setb[j])) for j, x in enumerate(nodes)}
    exact = {}
    for k, (s, x, fl) in enumerate(pairs):
        exact.setdefault(int(s), {})[x] = (k, int(fl))
    hits, found = np.zeros(len(nodes), np.uint32), np.zeros(len(pairs), np.uint8)
    after, changed, counts = list(searches), [], []
    for i, s in enumerate(searches):
        ents = []
        for x, f in s.ents:
            nf = f
            if x in ops:
                j, c, st = ops[x]
                hits[j] += 1
                nf = (f & ~c) | st
            if x in exact.get(i, ()):
                k, nf = exact[i][x]
                found[k] = 1
            ents.append((x, nf))
        if ents != s.ents:
            after[i] = I.FlagSearch(s.id, s.expired, ents)
            changed.append(i)
            counts.append(counts_of(after[i]))
    return (after, hits, found, np.array(changed, np.uint32),
            np.array(counts, np.uint8).reshape(-1, 4))


def undo_pairs(before, after, changed):
    """Pairs that bring every changed byte back."""
    return [(int(s), x, f) for s in changed for (x, f), (_, g) in zip(before[int(s)].ents, after[int(s)].ents) if f != g]


def pair_arrays(pairs):
    if not pairs:
        return None
    return (np.array([p[0] for p in pairs], np.uint32), R.id_bytes([p[1] for p in pairs]),
            np.array([p[2] for p in pairs], np.uint8))


def new_stats():
    return {k: 0 for k in ("t_down", "t_up", "full_on", "full_off", "threshold", "expired_changed", "hit_unchanged",
                           "pair_beats_op", "pair_not_found", "held_by_3", "held_by_none", "key_not_tail",
                           "zero_key_padded", "lead_bad_live", "undone_by_pair")}


def mechanisms(searches, cap, nodes, clear, setb, pairs, result, stats):
    """Counts what the GPU cases must contain, from the model alone."""
    after, hits, found, changed, counts = result
    cs = set(int(s) for s in changed)
    for i in cs:
        b, a = searches[i], after[i]
        fb, tb = R.trim([e[1] for e in b.ents], R.SR_EXPIRED if b.expired else 0)
        fa, ta = R.trim([e[1] for e in a.ents], R.SR_EXPIRED if a.expired else 0)
        stats["t_down"] += ta < tb
        stats["t_up"] += ta > tb
        stats["full_on"] += bool(fa) and not fb
        stats["full_off"] += bool(fb) and not fa
        stats["threshold"] += (a.ents[ta - 1][0] if ta else None) != (b.ents[tb - 1][0] if tb else None)
        stats["expired_changed"] += b.expired and (fa, ta) == (fb, tb)
        n, _, lead, _ = counts_of(a)
        stats["lead_bad_live"] += (not a.expired) and n > 0 and lead >= min(n, SEARCH_MAX_BAD_NODES) and \
            counts_of(b)[2] < min(n, SEARCH_MAX_BAD_NODES)
    batch = set(nodes)
    for i, s in enumerate(searches):
        if i not in cs and any(x in batch for x, _ in s.ents):
            stats["hit_unchanged"] += 1
    ops = {x: (int(clear[j]), int(setb[j])) for j, x in enumerate(nodes)}
    for k, (s, x, fl) in enumerate(pairs):
        if not found[k]:
            stats["pair_not_found"] += 1
            continue
        f = dict(searches[s].ents)[x]
        if x in ops:
            by_op = (f & ~ops[x][0]) | ops[x][1]
            stats["pair_beats_op"] += by_op != fl
            stats["undone_by_pair"] += by_op != f and fl == f
    stats["held_by_3"] += int((hits >= 3).sum())
    stats["held_by_none"] += int((hits == 0).sum())
    members = {}
    for s in searches:
        for x, _ in s.ents:
            members.setdefault(x >> 96, set()).add(x)
    stats["key_not_tail"] += sum(1 for x in nodes if x >> 96 in members and x not in members[x >> 96])
    padded = any(len(s.ents) < cap for s in searches)
    stats["zero_key_padded"] += sum(1 for x in nodes if x >> 96 == 0 and padded)


# ---- inputs of the GPU cases -----------------------------------------------------------------------------------------
# node ops that keep KAD_SN_REMOVABLE within KAD_SN_BAD (what a host derives from isExpired() and time), so the marked
# set can be rebuilt as searches_ref searches; ANY_OPS is every pair of masks the call accepts
REAL_OPS = ((BOTH, 0), (SN_REMOVABLE, SN_BAD), (0, BOTH), (0, 0), (SN_REMOVABLE, 0), (0, SN_BAD))
ANY_OPS = tuple((c, s) for c in range(4) for s in range(4) if not c & s)
REAL_BYTES, ANY_BYTES = (0, SN_BAD, BOTH), (0, SN_BAD, SN_REMOVABLE, BOTH)


def make_set(rng, S, cap):
    """insert_ref.make_set, draw for draw, that also says which state every search was made in."""
    ids, states, out, drawn = R.make_ids(rng, S), I.states_for(cap), [], []
    while len(out) < S:
        st = states[len(out) % len(states)] if S <= 16 else states[int(rng.integers(0, len(states)))]
        for _ in range(min(int(rng.integers(1, 4)), S - len(out))):
            out.append(I.make_search(rng, ids[len(out)], st, cap))
            drawn.append(st)
    return out, drawn


def share_nodes(rng, searches, count):
    """`count` times: one member of one search put in place of a member of up to four others (the flag bytes keep their
    positions, so every search keeps its state)."""
    holders = [i for i, s in enumerate(searches) if s.ents]
    out = list(searches)
    for _ in range(count if len(holders) >= 2 else 0):
        src = out[holders[int(rng.integers(0, len(holders)))]]
        x = src.ents[int(rng.integers(0, len(src.ents)))][0]
        for i in rng.permutation(len(holders))[:4]:
            s = out[holders[int(i)]]
            if any(e[0] == x for e in s.ents):
                continue
            ids = [e[0] for e in s.ents]
            ids[int(rng.integers(0, len(ids)))] = x
            ids.sort(key=lambda v: v ^ s.id)
            out[holders[int(i)]] = I.FlagSearch(s.id, s.expired, list(zip(ids, [e[1] for e in s.ents])))
    return out


def make_batch(rng, searches, q, ops):
    """q distinct node IDs with their ops: members (most of a small batch, a tenth of the entries of a large one), all
    members of one short live search marked BAD, IDs that share a member's 64-bit key, IDs with a zero key (0 itself
    among them) and strangers."""
    members = sorted(set(e[0] for s in searches for e in s.ents))
    picked, clear, setb = {}, [], []

    def add(x, op=None):
        if x not in picked and len(picked) < q:
            picked[x] = ops[int(rng.integers(0, len(ops)))] if op is None else op

    short = [s for s in searches if not s.expired and 0 < len(s.ents) < SEARCH_NODES]
    if short and q >= 16:
        for x, _ in short[int(rng.integers(0, len(short)))].ents:
            add(x, (0, SN_BAD))
    if q >= 8:
        add(0)
        add(int.from_bytes(rng.bytes(12), "big"))
    want_members = min(len(members), max(q * 7 // 10, 1) if q <= 128 else len(members) // 10)
    for i in rng.permutation(len(members))[:want_members]:
        add(members[int(i)])
    for _ in range(min(q // 8, 64)):
        if members:
            add((members[int(rng.integers(0, len(members)))] >> 96 << 96) | int.from_bytes(rng.bytes(12), "big"))
    while len(picked) < q:
        add(int.from_bytes(rng.bytes(20), "big"))
    nodes = list(picked)
    order = rng.permutation(len(nodes))
    nodes = [nodes[int(i)] for i in order]
    return nodes, np.array([picked[x][0] for x in nodes], np.uint8), np.array([picked[x][1] for x in nodes], np.uint8)


def make_pairs(rng, searches, nodes, p, flag_bytes):
    """p distinct (search, ID, byte): entries the batch also names, other entries, and IDs their search does not hold."""
    S, out, seen = len(searches), [], set()
    batch = set(nodes)
    both = [(i, e[0]) for i, s in enumerate(searches) for e in s.ents if e[0] in batch]
    while len(out) < p and S:
        kind = int(rng.integers(0, 4))
        i = int(rng.integers(0, S))
        if kind == 0 and both:
            i, x = both[int(rng.integers(0, len(both)))]
        elif kind in (1, 2) and searches[i].ents:
            x = searches[i].ents[int(rng.integers(0, len(searches[i].ents)))][0]
        else:  # not a member: a stranger, or (for a search with entries) a member's key with another tail
            x = int.from_bytes(rng.bytes(20), "big")
            if searches[i].ents and rng.random() < 0.5:
                x = (searches[i].ents[0][0] >> 96 << 96) | (x & ((1 << 96) - 1))
        if (i, x) not in seen:
            seen.add((i, x))
            out.append((i, x, flag_bytes[int(rng.integers(0, len(flag_bytes)))]))
    return out


# name: (searches S, cap, q, p, every mask pair (else the realistic ones), seed)
CASES = {
    "s0_q5": (0, 32, 5, 0, False, 1),
    "s1_q1_p1": (1, 32, 1, 1, False, 2),
    "s3_cap14_q0_p1": (3, 14, 0, 1, False, 3),
    "s3_cap64_q63": (3, 64, 63, 0, False, 4),
    "s65_cap14_q64_p70": (65, 14, 64, 70, False, 5),
    "s65_cap32_q65_p1": (65, 32, 65, 1, False, 6),
    "s65_cap64_lds_p70": (65, 64, LDS_KEYS, 70, False, 7),
    "s300_cap32_lds1_p70": (300, 32, LDS_KEYS + 1, 70, False, 8),
    "s300_cap64_lds": (300, 64, LDS_KEYS, 0, False, 9),
    "s300_cap14_q65_p70": (300, 14, 65, 70, False, 10),
    "s300_cap32_q63_p1": (300, 32, 63, 1, False, 11),
    "s300_cap32_q0_p70": (300, 32, 0, 70, False, 12),
    "s65_cap32_anybits": (65, 32, 700, 70, True, 13),
    "s300_cap64_anybits": (300, 64, LDS_KEYS + 1, 70, True, 14),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """Built once, never changed: the searches before, the call's arguments, the model's result, the arguments and the
    result of the call that undoes it, and the mechanism counts."""
    S, cap, q, p, anybits, seed = CASES[name]
    rng = np.random.default_rng(1000 + seed)
    if S <= 3:  # the smallest sets hold members: a full, an expired and a short search
        states = ["full", "expired", "notfull"][:S]
        searches = [I.make_search(rng, sid, states[i], cap) for i, sid in enumerate(R.make_ids(rng, S))]
    else:
        searches, states = make_set(rng, S, cap)
        searches = share_nodes(rng, searches, S // 8)  # the flag bytes keep their places: every state stays
    nodes, clear, setb = make_batch(rng, searches, q, ANY_OPS if anybits else REAL_OPS)
    pairs = make_pairs(rng, searches, nodes, p, ANY_BYTES if anybits else REAL_BYTES)
    result = mark(searches, nodes, clear, setb, pairs)
    stats = new_stats()
    mechanisms(searches, cap, nodes, clear, setb, pairs, result, stats)
    undo = undo_pairs(searches, result[0], result[3])
    return {"searches": searches, "cap": cap, "nodes": nodes, "clear": clear, "set": setb, "pairs": pairs,
            "after": result[0], "hits": result[1], "found": result[2], "changed": result[3], "counts": result[4],
            "undo": undo, "undone": mark(result[0], [], [], [], undo), "stats": stats, "anybits": anybits,
            "states": states}


# ---- the host double of opendht_amd.mark_search_nodes ----------------------------------------------------------------
class HostMark:
    """`host` over restated searches (searches_ref.Search with shared Node objects); a node handle is the Node."""

    def __init__(self, searches):
        self.searches = searches

    def node_id(self, x):
        return int(x.id).to_bytes(20, "big")

    def expired(self, x):
        return x.expired

    def removable(self, x, now):
        return F.removable(x, now)

    def pair_flag(self, s, x, now):
        for sn in self.searches[s].nodes:
            if sn.node is x:
                return F.node_flag(sn, now)
        return SN_BAD if x.expired else 0  # not a member: the pair will not be found

    def step_split(self, which):
        """Dht::searchStep's expiry test (dht.cpp:1451) and refill test (:1354) on the host's own lists."""
        out = {"expire": [], "short": [], "neither": []}
        for s in which:
            nodes = self.searches[s].nodes
            bad = sum(1 for sn in nodes if sn.is_bad())  # getNumberOfBadNodes, :583-587
            lead = 0  # getNumberOfConsecutiveBadNodes, :588-597
            for sn in nodes:
                if not sn.is_bad():
                    break
                lead += 1
            if lead >= min(len(nodes), SEARCH_MAX_BAD_NODES):
                out["expire"].append(s)
            elif len(nodes) - bad < SEARCH_NODES:
                out["short"].append(s)
            else:
                out["neither"].append(s)
        return out


class ModelMark:
    """A device set made of the model with DeviceSearches.mark_nodes' interface."""

    def __init__(self, searches, cap, now):
        self.s = [I.from_search(x, now) for x in searches]
        self.S, self.cap = len(searches), cap

    def mark_nodes(self, node_ids, clear_bits=None, set_bits=None, pairs=None):
        ids = [int.from_bytes(bytes(r), "big") for r in np.asarray(node_ids, np.uint8).reshape(-1, 20)]
        z = np.zeros(len(ids), np.uint8)
        pr = []
        if pairs is not None:
            pr = [(int(s), int.from_bytes(bytes(i), "big"), int(f)) for s, i, f in zip(*pairs)]
        self.s, hits, found, changed, counts = mark(self.s, ids, z if clear_bits is None else clear_bits,
                                                    z if set_bits is None else set_bits, pr)
        return {"hits": hits, "pair_found": found, "changed": changed, "counts": counts}
