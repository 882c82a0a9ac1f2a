"""The two send loops of Dht::searchStep that precede the get loop, restated for the tests at the level of flag bytes, one
entry at a time from the reference's text: the listen loop (dht.cpp:1384-1428) and searchSendAnnounceValue (:1237-1339),
both inside `if (sr->isSynced(now))` (:1358, Search::isSynced :1467-1478 walked here again). The get loop and everything
after it is step_ref.step_batch, unchanged, run on the list as the two loops leave it: a probed node has a pending get
request. Nothing here uses the closed form of kad_step.h. As in step_ref every loop walks the entries in order and is
written over a batch of lists (numpy over the lists, never over the entries). Also the model of kad_sr_step_full and
kad_sr_mark_due over insert_ref.FlagSearch sets, the named cases, and the host double of step_searches_full. Shared by
test_sr_stepfull*.py; nothing here touches the GPU."""
import functools

import numpy as np

import insert_ref as I
import searches_ref as R
import step_ref as T

BAD, CAND, PEND, SYNC, NOGET = T.BAD, T.CAND, T.PEND, T.SYNC, T.NOGET
LDUE, ADUE = 0x40, 0x80
DUE_BITS = LDUE | ADUE
APPLY, NO_SEND, DONE_IF_SYNCED, NO_EXPIRE = T.APPLY, T.NO_SEND, T.DONE_IF_SYNCED, T.NO_EXPIRE
LISTEN, ANNOUNCE, PROBE_BLOCKS = 0x10, 0x20, 0x40
LISTEN_NODES = 4  # dht.h
TARGET_NODES = T.TARGET_NODES
FIELDS = ("picks", "listen", "announce", "n", "bad", "lead_bad", "solicited", "bits")


def valid_mode(m):
    """DONE_IF_SYNCED means "no listeners, no announces"; PROBE_BLOCKS speaks of the announce probes; 0x80 is no mode."""
    if m & ~0x7F or (m & DONE_IF_SYNCED and m & (LISTEN | ANNOUNCE)):
        return False
    return not m & PROBE_BLOCKS or bool(m & ANNOUNCE)


MODES = tuple(m for m in range(256) if valid_mode(m))
INVALID_MODES = tuple(m for m in range(256) if not valid_mode(m))
OLD_MODES = T.MODES  # the modes without LISTEN and ANNOUNCE: kad_sr_step's


def step_full_batch(fl, n, expired, mode):
    """The step of N lists: fl (N, L) flag bytes, n (N,) lengths <= L, expired (N,) bool, mode (N,) uint8. Returns (picks,
    listen, announce (N,) uint64, n, bad, lead_bad, solicited, bits (N,) int64, the flag bytes after all sends)."""
    fl = np.array(fl, np.uint8).reshape(len(n), -1)
    N, L = fl.shape
    n, expired, mode = np.asarray(n, np.int64), np.asarray(expired, bool), np.asarray(mode, np.int64)
    rows = np.arange(N)

    def has(e, bit):
        return (fl[:, e] & bit) != 0

    def put(mask, who, e):
        mask[who] |= np.uint64(1) << np.uint64(e)

    # Search::isSynced, :1467-1478
    i, verdict = np.zeros(N, np.int64), np.zeros(N, np.int64)  # 0 walking, 1 returned false, 2 left the loop
    for e in range(L):
        at = (e < n) & (verdict == 0) & ~has(e, BAD)
        unsynced = at & ~has(e, SYNC)
        verdict[unsynced] = 1
        ok = at & ~unsynced
        i += ok
        verdict[ok & (i == TARGET_NODES)] = 2
    synced = ~expired & (verdict != 1) & (i > 0)  # :1346, :1358

    listen, announce = np.zeros(N, np.uint64), np.zeros(N, np.uint64)
    walking, i = synced & ((mode & LISTEN) != 0), np.zeros(N, np.int64)  # :1384 listeners not empty
    for e in range(L):  # :1386
        at = walking & (e < n) & has(e, SYNC)  # :1387 if (not n.isSynced(now)) continue
        due = at & has(e, LDUE)  # :1391 some listener's getListenTime(query) <= now
        put(listen, due, e)
        fl[rows[due], e] &= np.uint8(0xFF ^ LDUE)  # listenStatus[query] is pending: getListenTime is max
        count = at & ~has(e, CAND)  # :1426 if (not n.candidate and ++i == LISTEN_NODES) break
        i += count
        walking &= ~(count & (i == LISTEN_NODES))
    walking, i = synced & ((mode & ANNOUNCE) != 0), np.zeros(N, np.int64)  # :1238 announce not empty
    blocks = (mode & PROBE_BLOCKS) != 0
    for e in range(L):  # :1244
        some = walking & (e < n) & has(e, SYNC) & has(e, ADUE)  # :1245-1250 something_to_announce, else continue
        put(announce, some, e)
        fl[rows[some], e] |= PEND  # :1330 getStatus[probe_query] = the request
        fl[rows[some & blocks], e] |= NOGET  # the probe satisfies the get query: pending_sq_status
        fl[rows[some], e] &= np.uint8(0xFF ^ ADUE)  # probe pending: getAnnounceTime is max
        count = some & ~has(e, CAND)  # :1336 if (not n.candidate and ++i == TARGET_NODES) break
        i += count
        walking &= ~(count & (i == TARGET_NODES))
    picks, n, bad, lead, sol, bits, after = T.step_batch(fl, n, expired, mode & 0x0F)
    return picks, listen, announce, n, bad, lead, sol, bits, after


def positions(mask):
    return [e for e in range(64) if (int(mask) >> e) & 1]


def step_full(flags, expired=False, mode=0):
    """One list: (get picks, listen picks, announce picks (positions in order), n, bad, lead_bad, solicited, bits, the
    flag bytes afterwards)."""
    fl = np.array(list(flags) + [0], np.uint8).reshape(1, -1)
    r = step_full_batch(fl, [len(flags)], [bool(expired)], [mode])
    return (positions(r[0][0]), positions(r[1][0]), positions(r[2][0])) + tuple(int(v[0]) for v in r[3:8]) + (
        [int(v) for v in r[8][0, :len(flags)]],)


def apply_rule(f, pick, listen, announce, blocks):
    """The byte the issue spells out for an entry under KAD_STEP_APPLY."""
    if pick or announce:
        f |= PEND
    if pick or (announce and blocks):
        f |= NOGET
    if listen:
        f &= ~LDUE
    if announce:
        f &= ~ADUE
    return f


def device_step_full(searches, which, modes):
    """What kad_sr_step_full must give over FlagSearch sets: (searches afterwards, picks, listen, announce, n, bad,
    lead_bad, solicited, bits). An unchanged search stays the same object. The bytes afterwards come from apply_rule on
    the yardstick's picks, and are checked against the bytes the loops left."""
    which = list(range(len(searches))) if which is None else [int(s) for s in which]
    modes = np.broadcast_to(np.asarray(0 if modes is None else modes, np.int64), (len(which),))
    if not which:
        z = np.zeros(0, np.int64)
        u = np.zeros(0, np.uint64)
        return list(searches), u, u, u, z, z, z, z, z
    fl, n = T.pad([[e[1] for e in searches[s].ents] for s in which])
    r = step_full_batch(fl, n, [searches[s].expired for s in which], modes)
    picks, listen, announce, bits, after = r[0], r[1], r[2], r[7], r[8]
    out = list(searches)
    for k, s in enumerate(which):
        if not modes[k] & APPLY:
            continue
        if bits[k] & T.EXPIRE and not modes[k] & NO_EXPIRE:  # Search::expire(), :649-653
            out[s] = I.FlagSearch(searches[s].id, True, [])
        elif picks[k] | listen[k] | announce[k]:
            ents = []
            for e, (x, f) in enumerate(searches[s].ents):
                g = apply_rule(f, (int(picks[k]) >> e) & 1, (int(listen[k]) >> e) & 1, (int(announce[k]) >> e) & 1,
                               bool(modes[k] & PROBE_BLOCKS))
                assert g == int(after[k, e]), (s, e, f, g, int(after[k, e]))
                ents.append((x, g))
            out[s] = I.FlagSearch(searches[s].id, searches[s].expired, ents)
    return (out,) + tuple(r[:8])


def assert_step_full(got, want, tag):
    """got: DeviceSearches.step_full's or search_step_full_batch's dict; want: the tuple from picks on."""
    for name, w in zip(FIELDS, want):
        g = np.asarray(got[name]).astype(np.uint64)
        bad = np.flatnonzero(g != np.asarray(w).astype(np.uint64))
        assert bad.size == 0, (tag, name, bad[:4], g[bad[:4]], np.asarray(w)[bad[:4]])


# ---- the named cases: (flag bytes, expired, mode); entries are SYNCED and not BAD unless said otherwise -------------
S_ = SYNC
G = SYNC | NOGET  # synced, nothing to get from it
BC = BAD | CAND


def _named():
    c = {}
    c["listen_first_four"] = ([G | LDUE] * 6, False, LISTEN)
    c["listen_candidates_do_not_count"] = ([BC | G | LDUE] * 2 + [G | LDUE] * 5, False, LISTEN)
    c["listen_not_due_counts"] = ([G | LDUE] * 3 + [G] + [G | LDUE], False, LISTEN)
    c["listen_unsynced_entry"] = ([G | LDUE, BAD | LDUE, G | LDUE, NOGET | BAD | LDUE, G | LDUE, G | LDUE, G | LDUE], False,
                                  LISTEN)
    c["announce_not_due_does_not_count"] = ([G, G] + [G | ADUE] * 8, False, ANNOUNCE)
    c["announce_ninth_not_picked"] = ([G | ADUE] * 9, False, ANNOUNCE)
    c["announce_candidate_adds_a_ninth"] = ([G | ADUE] * 3 + [BC | G | ADUE] + [G | ADUE] * 6, False, ANNOUNCE)
    c["unsynced_search_with_due_bits"] = ([LDUE | ADUE, S_ | LDUE | ADUE, S_ | ADUE, 0, 0, 0], False, LISTEN | ANNOUNCE)
    c["two_pending_two_probes"] = ([S_ | PEND | NOGET] * 2 + [S_ | ADUE] * 2 + [S_] * 3, False, ANNOUNCE)
    c["probe_on_pending_entry"] = ([S_ | PEND | NOGET | ADUE] + [G] * 4, False, ANNOUNCE)
    c["probe_without_blocks_is_a_get_pick"] = ([S_ | ADUE] + [G] * 4, False, ANNOUNCE)
    c["probe_with_blocks_is_no_get_pick"] = ([S_ | ADUE] + [G] * 4, False, ANNOUNCE | PROBE_BLOCKS)
    c["expired_search_with_due_bits"] = ([S_ | LDUE | ADUE] * 5, True, LISTEN | ANNOUNCE)
    c["both_loops_and_gets"] = ([S_ | LDUE | ADUE, S_ | LDUE, S_ | ADUE, BC | S_ | LDUE | ADUE, S_, S_ | LDUE, S_ | LDUE],
                                False, LISTEN | ANNOUNCE)
    c["due_bits_without_their_mode"] = ([S_ | LDUE | ADUE] * 5, False, 0)
    # the four that count are entries 15, 32, 48 and 63; the eight that count 0, 21, 38, 43, 48, 53, 58 and 63
    c["listen_in_every_unit_of_64"] = ([BC | G | LDUE] * 15 + [G] + [BC | G | LDUE] * 16 + [G] + [BC | G | LDUE] * 15 + [G] +
                                       [BC | G | LDUE] * 14 + [G | LDUE], False, LISTEN)
    c["announce_in_every_unit_of_64"] = ([G | ADUE] + [BC | G | ADUE] * 20 + [G | ADUE] + [G] * 12 +
                                         ([BC | G | ADUE] * 4 + [G | ADUE]) * 6, False, ANNOUNCE | PROBE_BLOCKS)
    c["expiring_with_sends"] = ([BAD] * 25 + [S_ | LDUE | ADUE] * 3, False, LISTEN | ANNOUNCE)
    return c


NAMED = _named()


def random_lists(rng, n, count):
    """count lists of n flag bytes over all eight bits: step_ref's profiles with due bits drawn on them, mostly synced
    lists with many due bits and candidates among them (the two loops run to their limits), and uniform bytes."""
    base = T.random_lists(rng, n, count)
    out = []
    for k, fl in enumerate(base):
        fl = np.array(fl, np.int64)
        kind = k % 4
        if kind == 0:
            fl |= rng.choice([0, LDUE, ADUE, DUE_BITS], size=n)
        elif kind == 1:
            fl = rng.choice([G, G | LDUE, G | ADUE, G | DUE_BITS, S_ | ADUE, S_, BC | G | DUE_BITS, BC | S_ | ADUE, BAD],
                            size=n, p=[.15, .15, .15, .15, .1, .05, .1, .1, .05])
        elif kind == 2:
            fl = rng.choice([S_, S_ | PEND | NOGET, S_ | ADUE, S_ | LDUE, G | DUE_BITS, BC | G | LDUE, BC], size=n)
        else:
            fl = rng.integers(0, 256, size=n)
        out.append([int(v) for v in fl])
    return out


RANDOM_N = (0, 1, 3, 4, 5, 7, 8, 9, 13, 14, 15, 16, 17, 24, 25, 26, 31, 32, 33, 63, 64)


def make_full_set(rng, S, cap, lists=None, full=False):
    """S FlagSearch searches with slabs of cap entries whose flag bytes carry all eight bits: `lists` (flag lists,
    expired) first, then random lists of every length up to cap (full: all of length cap), a seventh of them expired."""
    ids = R.make_ids(rng, S)
    out = []
    for k, sid in enumerate(ids):
        if lists is not None and k < len(lists):
            fl, expired = lists[k]
        else:
            n = cap if full else (int(rng.integers(0, cap + 1)) if k % 3 else
                                  min(cap, (0, 1, 4, 5, 8, 9, 16, 17, 25, 26, 32, 33, 48, 63, 64)[k // 3 % 15]))
            fl, expired = random_lists(rng, n, 4)[k % 4], k % 7 == 3
            if full and k % 9 == 5:  # a full list that expires: 25 leading bad nodes
                fl = [f | BAD for f in fl[:25]] + fl[25:]
        assert len(fl) <= cap
        out.append(I.FlagSearch(sid, expired, list(zip(R.make_list(rng, sid, len(fl)), fl))))
    return out


def named_lists(cap):
    return [(fl, ex) for fl, ex, _ in NAMED.values() if len(fl) <= cap]


@functools.lru_cache(maxsize=None)
def full_set(S, cap, seed, full=False):
    """Built once, never changed."""
    rng = np.random.default_rng(seed)
    return make_full_set(rng, S, cap, None if full else named_lists(cap)[:S // 2], full)


def draw_modes(rng, m, apply_part):
    """m valid modes with LISTEN on about 60 %, ANNOUNCE on 30 % (half with PROBE_BLOCKS), the old modes on the rest."""
    kind = rng.random(m)
    md = np.where(kind < 0.45, LISTEN, np.where(kind < 0.6, LISTEN | ANNOUNCE, np.where(
        kind < 0.75, ANNOUNCE, np.where(kind < 0.9, ANNOUNCE | PROBE_BLOCKS, 0)))).astype(np.uint8)
    old = md == 0
    md[old] = rng.choice([0, DONE_IF_SYNCED, NO_SEND], size=int(old.sum()))
    md[rng.random(m) < 0.15] |= NO_SEND
    md[rng.random(m) < 0.15] |= NO_EXPIRE
    md[(md & DONE_IF_SYNCED) != 0] &= 0x0F
    md[rng.random(m) < apply_part] |= APPLY
    assert all(valid_mode(int(v)) for v in md)
    return md


# ---- doubles ----------------------------------------------------------------------------------------------------------
class HostStepFull(T.HostStep):
    """`host` of step_searches_full over FlagSearch searches: its own three loops, and the four replays."""

    def step(self, s, mode, now):
        return step_full([e[1] for e in self.searches[s].ents], self.searches[s].expired, mode)[:8]

    def _set(self, s, pos, f):
        x = self.searches[s]
        ents = list(x.ents)
        ents[pos] = (ents[pos][0], f(ents[pos][1]))
        self.searches[s] = I.FlagSearch(x.id, x.expired, ents)

    def listen(self, s, pos, now):
        self._set(s, pos, lambda f: f & ~LDUE)

    def announce_probe(self, s, pos, now, blocks):
        self._set(s, pos, lambda f: (f | PEND | (NOGET if blocks else 0)) & ~ADUE)


class ModelStepFull(T.ModelStep):
    """A device set made of the model with DeviceSearches.step / step_full / mark_entries / mark_due's interface."""

    def step_full(self, which=None, modes=None):
        r = device_step_full(self.s, which, modes)
        self.s = r[0]
        out = dict(zip(FIELDS, r[1:]))
        out["stats"] = {k: sum(bin(int(v)).count("1") for v in out[f])
                        for k, f in (("picks", "picks"), ("listens", "listen"), ("announces", "announce"))}
        for k, bit in (("synced", T.SYNCED), ("expired", T.EXPIRE), ("skipped", T.SKIPPED)):
            out["stats"][k] = int(((np.asarray(out["bits"]) & bit) != 0).sum())
        out["stats"]["kernel_ms"] = 0.0
        return out

    def _mark(self, which, ids, clear_bits, set_bits, known):
        p = len(which)
        c = np.zeros(p, np.uint8) if clear_bits is None else np.asarray(clear_bits, np.uint8)
        st = np.zeros(p, np.uint8) if set_bits is None else np.asarray(set_bits, np.uint8)
        assert not ((c | st) & (0xFF ^ known)).any() and not (c & st).any()
        vals = [int.from_bytes(bytes(bytearray(x)), "big") for x in np.asarray(ids, np.uint8).reshape(p, 20)]
        self.s, found = T.mark_entries(self.s, [(int(which[k]), vals[k], int(c[k]), int(st[k])) for k in range(p)])
        return found

    def mark_due(self, which, ids, clear_bits=None, set_bits=None):
        return self._mark(which, ids, clear_bits, set_bits, DUE_BITS)

    def mark_entries(self, which, ids, clear_bits=None, set_bits=None):
        return self._mark(which, ids, clear_bits, set_bits, T.STEP_BITS)
