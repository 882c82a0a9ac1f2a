"""Dht::searchStep (dht.cpp:1344-1464) restated for the tests at the level of flag bytes, one entry at a time as the
reference's loops run: getNumberOfBadNodes / getNumberOfConsecutiveBadNodes (:583-597), currentlySolicitedNodeCount
(:514-520), Search::isSynced (:1467-1478), the send loop of :1438-1446 over searchSendGetValues (:1171-1196, its node
scan :1190-1195 taken again after every send) and the expiry test (:1451-1452). Nothing here uses the closed form of
kad_step.h. Every loop walks the entries in order; it is written over a batch of lists at once (numpy over the lists,
never over the entries), so that the exhaustive cases stay quick. Also the model of kad_sr_step / kad_sr_mark_entries over
insert_ref.FlagSearch sets, the named cases, and the host double of opendht_amd.step_searches. Shared by
test_sr_step*.py; nothing here touches the GPU."""
import functools

import numpy as np

import insert_ref as I
import searches_ref as R

SEARCH_NODES = R.SEARCH_NODES
TARGET_NODES = 8                # dht.h
MAX_REQUESTED_SEARCH_NODES = 4  # dht.h:316
SEARCH_MAX_BAD_NODES = 25       # dht.h:324
BAD, REMOVABLE = I.SN_BAD, I.SN_REMOVABLE
CAND, PEND, SYNC, NOGET = 0x04, 0x08, 0x10, 0x20
STEP_BITS = CAND | PEND | SYNC | NOGET
APPLY, NO_SEND, DONE_IF_SYNCED, NO_EXPIRE = 0x01, 0x02, 0x04, 0x08
SKIPPED, SHORT, SYNCED, DONE, EXHAUSTED, EXPIRE = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
MODES = tuple(range(16))
NOW = I.NOW


def step_batch(fl, n, expired, mode):
    """The step of N lists: fl (N, L) flag bytes, n (N,) lengths <= L, expired (N,) bool, mode (N,) uint8. Returns
    (picks (N,) uint64, n, bad, lead_bad, solicited (N,) and bits (N,) as int64, the flag bytes after the sends)."""
    fl = np.array(fl, np.uint8).reshape(len(n), -1)
    N, L = fl.shape
    n, expired, mode = np.asarray(n, np.int64), np.asarray(expired, bool), np.asarray(mode, np.int64)
    rows = np.arange(N)

    def has(e, bit):
        return (fl[:, e] & bit) != 0

    def solicited():  # currentlySolicitedNodeCount
        c = np.zeros(N, np.int64)
        for e in range(L):
            c += (e < n) & ~has(e, BAD) & has(e, PEND)
        return c

    bad, lead, run = np.zeros(N, np.int64), np.zeros(N, np.int64), np.ones(N, bool)
    for e in range(L):
        b = (e < n) & has(e, BAD)
        bad += b
        run &= b  # getNumberOfConsecutiveBadNodes stops at the first entry that is not bad
        lead += run
    live = ~expired  # :1346
    bits = np.where(expired, SKIPPED, 0).astype(np.int64)
    bits |= np.where(live & (n - bad < SEARCH_NODES), SHORT, 0)  # :1354
    i, verdict = np.zeros(N, np.int64), np.zeros(N, np.int64)  # isSynced: 0 walking, 1 returned false, 2 left the loop
    for e in range(L):
        at = (e < n) & (verdict == 0) & ~has(e, BAD)
        unsynced = at & ~has(e, SYNC)
        verdict[unsynced] = 1
        ok = at & ~unsynced
        i += ok
        verdict[ok & (i == TARGET_NODES)] = 2
    synced = live & (verdict != 1) & (i > 0)
    bits |= np.where(synced, SYNCED, 0)
    done = synced & ((mode & DONE_IF_SYNCED) != 0)  # setDone, :1434-1435
    bits |= np.where(done, DONE, 0)
    picks = np.zeros(N, np.uint64)
    sending = live & (solicited() < MAX_REQUESTED_SEARCH_NODES) & ((mode & NO_SEND) == 0)  # :1438
    while sending.any():  # do { sent = searchSendGetValues(sr) } while (sent and solicited < 4)
        scans = sending & ~done & (solicited() < MAX_REQUESTED_SEARCH_NODES)  # :1173
        sent = np.full(N, -1, np.int64)
        for e in range(L):  # the first node that canGet, :1190-1195
            can = ~has(e, NOGET) & (~has(e, BAD) | has(e, CAND))
            sent[scans & (sent < 0) & (e < n) & can] = e
        bits |= np.where(scans & (sent < 0), EXHAUSTED, 0)
        hit = sent >= 0
        fl[rows[hit], sent[hit]] |= PEND | NOGET  # getStatus[query] = the request
        picks[hit] |= np.uint64(1) << sent[hit].astype(np.uint64)
        sending = hit & (solicited() < MAX_REQUESTED_SEARCH_NODES)
    bits |= np.where(live & (lead >= np.minimum(n, SEARCH_MAX_BAD_NODES)), EXPIRE, 0)  # :1451-1452
    return picks, n, bad, lead, solicited(), bits, fl


def step(flags, expired=False, mode=0):
    """One list: (picked positions in order, n, bad, lead_bad, solicited, bits, the flag bytes after the sends)."""
    fl = np.array(list(flags) + [0], np.uint8).reshape(1, -1)
    picks, n, bad, lead, sol, bits, after = step_batch(fl, [len(flags)], [bool(expired)], [mode])
    p = int(picks[0])
    return ([e for e in range(64) if (p >> e) & 1], int(n[0]), int(bad[0]), int(lead[0]), int(sol[0]), int(bits[0]),
            [int(v) for v in after[0, :len(flags)]])


def pad(lists):
    """(N, L) flag bytes and the lengths of flag lists."""
    L = max([len(x) for x in lists] + [1])
    fl = np.zeros((len(lists), L), np.uint8)
    for k, x in enumerate(lists):
        fl[k, :len(x)] = x
    return fl, np.array([len(x) for x in lists], np.int64)


def device_step(searches, which, modes):
    """What kad_sr_step must give over FlagSearch sets: (searches afterwards, picks, n, bad, lead_bad, solicited, bits).
    An unchanged search stays the same object."""
    which = list(range(len(searches))) if which is None else [int(s) for s in which]
    modes = np.broadcast_to(np.asarray(0 if modes is None else modes, np.int64), (len(which),))
    if not which:
        z = np.zeros(0, np.int64)
        return list(searches), np.zeros(0, np.uint64), z, z, z, z, z
    fl, n = pad([[e[1] for e in searches[s].ents] for s in which])
    picks, n, bad, lead, sol, bits, after = step_batch(fl, n, [searches[s].expired for s in which], modes)
    out = list(searches)
    for k, s in enumerate(which):
        if not modes[k] & APPLY:
            continue
        if bits[k] & EXPIRE and not modes[k] & NO_EXPIRE:  # Search::expire(), :649-653
            out[s] = I.FlagSearch(searches[s].id, True, [])
        elif picks[k]:
            out[s] = I.FlagSearch(searches[s].id, searches[s].expired,
                                  [(x, int(after[k, e])) for e, (x, _) in enumerate(searches[s].ents)])
    return out, picks, n, bad, lead, sol, bits


def mark_entries(searches, pairs):
    """What kad_sr_mark_entries must give. pairs: (search, ID, clear, set). Returns (searches afterwards, found)."""
    out, found = list(searches), np.zeros(len(pairs), np.uint8)
    for k, (s, x, c, st) in enumerate(pairs):
        ents = out[s].ents
        for e, (y, f) in enumerate(ents):
            if y == x:
                found[k] = 1
                if (f & ~c) | st != f:
                    out[s] = I.FlagSearch(out[s].id, out[s].expired, ents[:e] + [(y, (f & ~c) | st)] + ents[e + 1:])
                break
    return out, found


def assert_step(got, want, tag):
    """got: DeviceSearches.step's or search_step_batch's dict; want: device_step's or step_batch's tuple from picks on."""
    for name, w in zip(("picks", "n", "bad", "lead_bad", "solicited", "bits"), want):
        g = np.asarray(got[name]).astype(np.uint64)
        bad = np.flatnonzero(g != np.asarray(w).astype(np.uint64))
        assert bad.size == 0, (tag, name, bad[:4], g[bad[:4]], np.asarray(w)[bad[:4]])


# ---- the named cases: (flag bytes, expired, mode) --------------------------------------------------------------------
BC = BAD | CAND
P = PEND | NOGET  # a node with a request in flight


def _named():
    c = {}
    for k in (4, 5):
        c[f"solicited_{k}"] = ([P] * k + [0] * 6, False, 0)
    c["solicited_3_and_one_bad"] = ([P, P, BAD | P, P, 0, 0], False, 0)  # the bad one does not count: room for one
    c["room_th_pick_is_last"] = ([P, P, NOGET, 0, NOGET, SYNC | NOGET, 0], False, 0)
    c["room_th_pick_is_last_of_64"] = ([P] + [NOGET] * 60 + [0, 0, 0], False, 0)
    c["candidates_around_the_picks"] = ([BC, 0, BC, 0, 0, BC, 0, BC, 0], False, 0)  # seven picks, the last two stay
    c["candidates_then_exhausted"] = ([BC, 0, BC, 0, BC], False, 0)
    c["candidates_only"] = ([BC] * 6, False, 0)  # six picks, none counts; it expires all the same
    c["expired_candidate_with_noget"] = ([BC | NOGET, 0, 0], False, 0)
    c["expired_candidate_without_noget"] = ([BC, 0, 0], False, 0)
    c["candidate_bit_without_bad"] = ([CAND, CAND | NOGET, 0], False, 0)
    c["eighth_unsynced"] = ([BAD] + [SYNC] * 4 + [BAD | SYNC] + [SYNC] * 3 + [0] + [SYNC] * 5, False, 0)
    c["ninth_unsynced"] = ([BAD] + [SYNC] * 4 + [BAD] + [SYNC] * 4 + [0] + [SYNC] * 5, False, 0)
    c["synced_by_fewer_than_eight"] = ([SYNC | NOGET] * 3 + [BAD] * 2, False, 0)
    c["bad_synced_does_not_count"] = ([BAD | SYNC] * 3 + [0], False, 0)
    c["only_bad"] = ([BAD] * 10, False, 0)
    c["only_bad_removable"] = ([BAD | REMOVABLE] * 14, False, 0)
    c["empty_live"] = ([], False, 0)
    c["empty_expired"] = ([], True, 0)
    c["expired_search"] = ([0, P, BAD, SYNC], True, 0)
    for n in (25, 26, 64):
        for lead in (24, 25):
            c[f"lead_{lead}_of_{n}"] = ([BAD] * lead + [0] * (n - lead), False, 0)
    c["lead_is_n_below_25"] = ([BAD] * 5, False, 0)
    c["lead_one_short_of_n"] = ([BAD] * 4 + [0], False, 0)
    c["all_64_bad"] = ([BAD] * 64, False, 0)
    c["all_64_good_pending_last"] = ([NOGET] * 60 + [0] * 4, False, 0)
    c["done_if_synced_synced"] = ([SYNC] * 9, False, DONE_IF_SYNCED)
    c["done_if_synced_unsynced"] = ([SYNC | NOGET] * 3 + [0] * 6, False, DONE_IF_SYNCED)
    c["done_and_expiring"] = ([BAD] * 30 + [SYNC | NOGET] * 2, False, DONE_IF_SYNCED)
    c["no_send"] = ([0] * 9, False, NO_SEND)
    c["no_send_expiring"] = ([BAD] * 9, False, NO_SEND)
    c["no_expire"] = ([BAD] * 9 + [BC], False, NO_EXPIRE)
    c["removable_changes_nothing"] = ([REMOVABLE, BAD | REMOVABLE, 0, REMOVABLE | SYNC], False, 0)
    return c


NAMED = _named()


def random_lists(rng, n, count):
    """count lists of n flag bytes over all six bits, drawn from profiles that reach every branch: mostly fresh nodes,
    mostly synced, mostly bad with a bad prefix, mostly in flight, and uniform bytes."""
    out = []
    for k in range(count):
        kind = k % 5
        if kind == 0:
            fl = rng.choice([0, 0, 0, NOGET, P, BAD, BC, SYNC], size=n)
        elif kind == 1:
            fl = rng.choice([SYNC, SYNC, SYNC | NOGET, SYNC | P, 0, BAD | SYNC], size=n)
        elif kind == 2:
            fl = rng.choice([BAD, BAD | REMOVABLE, BC, BC | NOGET, 0], size=n, p=[.4, .2, .15, .15, .1])
            fl[:int(rng.integers(0, n + 1))] |= BAD
        elif kind == 3:
            fl = rng.choice([P, P | SYNC, NOGET, 0, BAD | P], size=n, p=[.3, .1, .3, .2, .1])
        else:
            fl = rng.integers(0, 64, size=n)
        out.append([int(v) for v in fl])
    return out


RANDOM_N = (0, 1, 7, 8, 9, 13, 14, 15, 16, 17, 24, 25, 26, 31, 32, 33, 63, 64)


def make_step_set(rng, S, cap, lists=None):
    """S FlagSearch searches with slabs of cap entries whose flag bytes carry step bits: `lists` (flag lists, expired)
    first, then random lists of every length up to cap, a seventh of them expired."""
    ids = R.make_ids(rng, S)
    out = []
    for k, sid in enumerate(ids):
        if lists is not None and k < len(lists):
            fl, expired = lists[k]
        else:
            n = int(rng.integers(0, cap + 1)) if k % 3 else min(cap, (0, 1, 13, 14, 15, 16, 17, 25, 26, 32, 33, 48, 63, 64)[k // 3 % 14])
            fl, expired = random_lists(rng, n, 5)[k % 5], k % 7 == 3
        assert len(fl) <= cap
        out.append(I.FlagSearch(sid, expired, list(zip(R.make_list(rng, sid, len(fl)), fl))))
    return out


@functools.lru_cache(maxsize=None)
def step_set(S, cap, seed):
    """Built once, never changed."""
    rng = np.random.default_rng(seed)
    named = [(fl, ex) for fl, ex, _ in NAMED.values() if len(fl) <= cap]
    return make_step_set(rng, S, cap, named[:S // 2])


# ---- the host double of opendht_amd.step_searches --------------------------------------------------------------------
class HostStep:
    """`host` over FlagSearch searches: its own entry-by-entry step, the sends and expire()."""

    def __init__(self, searches):
        self.searches = list(searches)

    def step(self, s, mode, now):
        return step([e[1] for e in self.searches[s].ents], self.searches[s].expired, mode)[:6]

    def send(self, s, pos, now):
        x = self.searches[s]
        ents = list(x.ents)
        ents[pos] = (ents[pos][0], ents[pos][1] | PEND | NOGET)
        self.searches[s] = I.FlagSearch(x.id, x.expired, ents)

    def expire(self, s):
        self.searches[s] = I.FlagSearch(self.searches[s].id, True, [])


class ModelStep:
    """A device set made of the model with DeviceSearches.step's interface."""

    def __init__(self, searches, cap):
        self.s, self.S, self.cap = list(searches), len(searches), cap

    def step(self, which=None, modes=None):
        self.s, picks, n, bad, lead, sol, bits = device_step(self.s, which, modes)
        return {"picks": picks, "n": n, "bad": bad, "lead_bad": lead, "solicited": sol, "bits": bits,
                "stats": {"picks": sum(bin(int(v)).count("1") for v in picks)}}

    def export(self, nodes=True):
        return I.expected_export(self.s, self.cap)
