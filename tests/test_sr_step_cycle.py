"""Several ticks of about 200 searches, every call of a tick driven against the flag-level host double:
node status marks (kad_sr_mark_nodes, node ops and pairs), Dht::refill (kad_sr_refill), the step with APPLY (kad_sr_step),
the replies and timeouts of its requests (kad_sr_mark_entries), a tick of trySearchInsert (kad_sr_try_insert_tick) and the
membership change (kad_searches_apply: erase, add, grow from slabs of 30 over 36 and 48 to 64 entries, so both relayout
forms and both step kernels run). After every call the device export, step bits included, equals the double: this is where
the step bits are shown to travel with their entries through insert_kernel, refill_kernel, the relayout and the node ops
of kad_sr_mark_nodes, and to be cleared by its pair ops. The scenario is built from the models alone, once; a CPU test
checks that it contains every one of those mechanisms."""
import functools
from bisect import bisect_left

import numpy as np
import pytest

import insert_ref as I
import mark_ref as M
import refill_ref as F
import searches_ref as R
import step_ref as T

S0, TICKS, CAPS = 200, 4, (30, 36, 48, 64)


def refill_model(searches, cache, which, cap):
    out, rows, status = list(searches), [], []
    for s in which:
        row = cache.get_cached_nodes(searches[s].id)
        c = searches[s].copy()
        over = False
        for i in row:
            I.insert_one(c, cache.ids[i], 0)
            if len(c.ents) > cap:
                over = True
                break
        rows.append(row)
        status.append(1 if over else 0)
        if row and not over:
            out[s] = c
    return out, rows, status


def tick_model(searches, cands):
    """Dht::trySearchInsert of every candidate in arrival order on the double."""
    out = list(searches)
    ids = [s.id for s in out]

    def ins(s, x, xfl):
        out[s] = out[s].copy()
        return I.insert_one(out[s], x, xfl)

    for x, xfl in cands:
        l = bisect_left(ids, x)
        for s in range(l, len(out)):
            if not ins(s, x, xfl):
                break
        for s in range(l - 1, -1, -1):
            if not ins(s, x, xfl):
                break
    return out


def moved_bits(before, after):
    """Entries that carry step bits and sit at another index afterwards, with the same byte."""
    n = 0
    for b, a in zip(before, after):
        at = {x: (i, f) for i, (x, f) in enumerate(a.ents)}
        n += sum(1 for i, (x, f) in enumerate(b.ents) if f & T.STEP_BITS and x in at and at[x] == (at[x][0], f) and at[x][0] != i)
    return n


@functools.lru_cache(maxsize=None)
def scenario():
    """Built once from the models: the searches at the start and, per tick, every call's arguments and the double after it."""
    rng = np.random.default_rng(2024)
    cache = F.make_cache(rng, 400, expired_part=0.1)
    searches = T.make_step_set(rng, S0, 14)  # lists of up to 14 entries in slabs of 30: room for the first tick's inserts
    start, ticks = searches, []
    stats = {"node_op_keeps_bits": 0, "pair_clears_bits": 0, "refill_moves_bits": 0, "insert_moves_bits": 0,
             "relayout_carries_bits": 0, "expired_by_step": 0, "revived": 0, "picks": 0, "replies": 0}
    for t in range(TICKS):
        cap = CAPS[t]
        tk = {"cap": cap}
        # marks: timeouts and replies of earlier requests change BAD on shared nodes; pairs restate single entries
        ents = [(i, x, f) for i, s in enumerate(searches) for x, f in s.ents]
        pick = rng.permutation(len(ents))[:60]
        nodes = list({ents[int(k)][1] for k in pick[:40]})
        ops = [M.REAL_OPS[int(rng.integers(0, len(M.REAL_OPS)))] for _ in nodes]
        pairs = list({(ents[int(k)][0], ents[int(k)][1]): (ents[int(k)][0], ents[int(k)][1], int(rng.choice(M.REAL_BYTES)))
                      for k in pick[40:]}.values())
        paired = {(i, x) for i, x, _ in pairs}
        stats["node_op_keeps_bits"] += sum(1 for i, x, f in ents if x in nodes and (i, x) not in paired and f & T.STEP_BITS)
        stats["pair_clears_bits"] += sum(1 for i, x, f in ents if (i, x) in paired and f & T.STEP_BITS)
        after = M.mark(searches, nodes, [o[0] for o in ops], [o[1] for o in ops], pairs)[0]
        tk["mark"] = (nodes, np.array([o[0] for o in ops], np.uint8), np.array([o[1] for o in ops], np.uint8), pairs, after)
        searches = after
        # refill: the live searches that are short of nodes
        which = [i for i, s in enumerate(searches) if not s.expired and
                 len(s.ents) - sum(1 for e in s.ents if e[1] & T.BAD) < T.SEARCH_NODES][::2]
        after, rows, status = refill_model(searches, cache, which, cap)
        stats["refill_moves_bits"] += moved_bits(searches, after)
        tk["refill"] = (np.array(which, np.uint32), rows, status, after)
        searches = after
        # the step, applied
        md = rng.choice([0, T.DONE_IF_SYNCED, T.NO_SEND, T.NO_EXPIRE], size=len(searches), p=[.7, .1, .1, .1]).astype(np.uint8) | T.APPLY
        res = T.device_step(searches, None, md)
        stats["expired_by_step"] += sum(1 for a, b in zip(searches, res[0]) if b.expired and not a.expired)
        stats["picks"] += sum(bin(int(v)).count("1") for v in res[1])
        tk["step"] = (md, res)
        # the requests' ends: a reply (SYNCED, no longer PENDING) or a timeout that leaves the node gettable again
        ends = []
        for i, p in enumerate(res[1]):
            for e in range(64):
                if (int(p) >> e) & 1 and res[0][i].ents and rng.random() < 0.7:
                    reply = rng.random() < 0.6
                    ends.append((i, res[0][i].ents[e][0], T.PEND if reply else T.PEND | T.NOGET, T.SYNC if reply else 0))
        ends.append((0, 12345, T.PEND, 0))  # nobody holds it
        stats["replies"] += len(ends)
        after, found = T.mark_entries(res[0], ends)
        tk["entries"] = (ends, found, after)
        searches = after
        # new nodes arrive
        cands = []
        for k in range(120):
            s = searches[int(rng.integers(0, len(searches)))]
            v = int.from_bytes(rng.bytes(20), "big")
            cands.append(((s.id ^ (v >> int(rng.integers(100, 158)))) if k % 4 else v, T.BAD if rng.random() < 0.25 else 0))
        after = tick_model(searches, cands)
        assert max(len(s.ents) for s in after) <= cap  # the scenario never overflows a slab
        stats["insert_moves_bits"] += moved_bits(searches, after)
        stats["revived"] += sum(1 for a, b in zip(searches, after) if a.expired and not b.expired)
        tk["tick"] = (cands, after)
        searches = after
        # expireSearches and new searches, and larger slabs for the next tick
        erase = sorted(int(v) for v in rng.choice(len(searches), size=6, replace=False))
        new_ids = [int.from_bytes(rng.bytes(20), "big") for _ in range(6)]
        kept = [s for i, s in enumerate(searches) if i not in set(erase)]
        after = sorted(kept + [I.FlagSearch(x) for x in new_ids], key=lambda s: s.id)
        stats["relayout_carries_bits"] += sum(1 for s in kept for e in s.ents if e[1] & T.STEP_BITS)
        tk["apply"] = (np.array(erase, np.uint32), new_ids, CAPS[min(t + 1, TICKS - 1)], after)
        searches = after
        ticks.append(tk)
    return start, cache, ticks, stats


def test_the_scenario_contains_every_mechanism():
    _, _, ticks, stats = scenario()
    assert all(v > 0 for v in stats.values()), stats
    kinds = set()
    for tk in ticks:
        kinds |= {int(b) for b in tk["step"][1][6]}
    seen = 0
    for b in kinds:
        seen |= b
    assert seen == 0x3F, hex(seen)


def assert_export(DS, searches, tag):
    got, want = DS.export(), I.expected_export(searches, DS.cap)
    for k in want:
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (tag, k, bad[:4])


@pytest.mark.gpu
def test_ticks_on_the_device_equal_the_double(gpu):
    from opendht_amd import KAD_SR_TICK_LEFT, DeviceSearches, DeviceTable

    start, cache, ticks, _ = scenario()
    cids, cstatus = cache.table_arrays()
    with DeviceSearches(*I.snapshot(start), cap=CAPS[0], device=0) as DS, \
            DeviceTable(cids, cstatus, device=0, sorted=True) as NC:
        assert_export(DS, start, "start")
        for t, tk in enumerate(ticks):
            assert DS.cap == tk["cap"]
            nodes, clear, setb, pairs, after = tk["mark"]
            DS.mark_nodes(R.id_bytes(nodes), clear, setb, M.pair_arrays(pairs))
            assert_export(DS, after, (t, "mark"))
            which, rows, status, after = tk["refill"]
            drows, dcnt, _, dstatus = DS.refill(NC, which)
            assert [list(r[:c]) for r, c in zip(drows, dcnt)] == rows and list(dstatus) == status
            assert_export(DS, after, (t, "refill"))
            md, res = tk["step"]
            T.assert_step(DS.step(None, md), res[1:], (t, "step"))
            assert_export(DS, res[0], (t, "step"))
            ends, found, after = tk["entries"]
            got = DS.mark_entries([e[0] for e in ends], R.id_bytes([e[1] for e in ends]), [e[2] for e in ends],
                                  [e[3] for e in ends])
            assert np.array_equal(got, found)
            assert_export(DS, after, (t, "entries"))
            cands, after = tk["tick"]
            r = DS.try_insert_tick(R.id_bytes([c[0] for c in cands]), np.array([c[1] for c in cands], np.uint8))
            assert not (r["kind"] == KAD_SR_TICK_LEFT).any() and r["overflow"].size == 0
            assert_export(DS, after, (t, "tick"))
            erase, new_ids, cap, after = tk["apply"]
            DS.apply(erase, R.id_bytes(new_ids), cap=cap)
            assert_export(DS, after, (t, "apply"))
