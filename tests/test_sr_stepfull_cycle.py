"""Four ticks of about 200 searches whose entries carry all eight flag bits, every call of a tick driven against the
flag-level double: node status marks (kad_sr_mark_nodes, node ops and pairs), Dht::refill
(kad_sr_refill), the deadlines that passed (kad_sr_mark_due), the whole step with APPLY on most searches
(kad_sr_step_full) and the get-only step with APPLY on the others (kad_sr_step), the replies' marks (kad_sr_mark_entries
and kad_sr_mark_due), a tick of trySearchInsert (kad_sr_try_insert_tick) and the membership change (kad_searches_apply:
erase, add, slabs growing 30 -> 36 -> 48 -> 64, so both relayout forms and both forms of both step kernels run). After
every call the device export equals the double: this is the proof that KAD_SN_LISTEN_DUE and KAD_SN_ANNOUNCE_DUE travel
with their entries through insert_kernel, refill_kernel, the relayout, kad_sr_step with APPLY, kad_sr_mark_entries and
the node ops of kad_sr_mark_nodes, and are cleared by its pairs. The scenario is built from the models alone, once; a CPU
test checks that it contains each mechanism, and in every tick a search in which an announce probe closes the get loop."""
import functools

import numpy as np
import pytest

import insert_ref as I
import mark_ref as M
import refill_ref as RF
import searches_ref as R
import step_ref as T
import stepfull_ref as F
from test_sr_step_cycle import refill_model, tick_model

S0, TICKS, CAPS = 200, 4, (30, 36, 48, 64)


def moved_due(before, after):
    """Entries that carry due bits and sit at another index afterwards, with the same byte."""
    n = 0
    for b, a in zip(before, after):
        at = {x: (i, f) for i, (x, f) in enumerate(a.ents)}
        n += sum(1 for i, (x, f) in enumerate(b.ents) if f & F.DUE_BITS and x in at and at[x][1] == f and at[x][0] != i)
    return n


def flags_of(s):
    return [e[1] for e in s.ents]


@functools.lru_cache(maxsize=None)
def scenario():
    """Built once from the models: the searches at the start and, per tick, every call's arguments and the double after it."""
    rng = np.random.default_rng(2025)
    cache = RF.make_cache(rng, 400, expired_part=0.1)
    searches = F.make_full_set(rng, S0, 14)  # lists of up to 14 entries in slabs of 30: room for the first tick's inserts
    start, ticks = searches, []
    stats = {"node_op_keeps_due": 0, "pair_clears_due": 0, "refill_moves_due": 0, "insert_moves_due": 0,
             "relayout_carries_due": 0, "old_step_keeps_due": 0, "entries_keeps_due": 0, "due_keeps_step_bits": 0,
             "expired_by_step": 0, "picks": 0, "listens": 0, "announces": 0, "replies": 0}
    closes = []
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
        stats["node_op_keeps_due"] += sum(1 for i, x, f in ents if x in nodes and (i, x) not in paired and f & F.DUE_BITS)
        stats["pair_clears_due"] += sum(1 for i, x, f in ents if (i, x) in paired and f & F.DUE_BITS)
        after = M.mark(searches, nodes, [o[0] for o in ops], [o[1] for o in ops], pairs)[0]
        for i, x, _ in pairs:
            assert not [f for y, f in after[i].ents if y == x][0] & (F.DUE_BITS | T.STEP_BITS)
        tk["mark"] = (nodes, np.array([o[0] for o in ops], np.uint8), np.array([o[1] for o in ops], np.uint8), pairs, after)
        searches = after
        # refill: the live searches that are short of nodes
        which = [i for i, s in enumerate(searches) if not s.expired and
                 len(s.ents) - sum(1 for e in s.ents if e[1] & T.BAD) < T.SEARCH_NODES][::2]
        after, rows, status = refill_model(searches, cache, which, cap)
        stats["refill_moves_due"] += moved_due(searches, after)
        tk["refill"] = (np.array(which, np.uint32), rows, status, after)
        searches = after
        # the deadlines that passed: due bits on single entries; every tenth synced search has an announce due on all its
        # synced nodes, and a few listen deadlines are taken back (a listener was cancelled)
        # Before them the step bits whose deadlines passed or whose replies came late (kad_sr_mark_entries): three live
        # searches end up synced with nothing in flight, every good node but the last with nothing to get, and an
        # announce due on all of them. There five probes or more fill the four request slots: no get is sent.
        planted = [i for i, s in enumerate(searches) if i % 4 != 3 and not s.expired and
                   sum(1 for f in flags_of(s) if not f & T.BAD) >= 5][t::7][:3]
        late = []
        for i in planted:
            good = [x for x, f in searches[i].ents if not f & T.BAD]
            late += [(i, x, T.PEND | (T.NOGET if x == good[-1] else 0), T.SYNC | (0 if x == good[-1] else T.NOGET)) for x in good]
        after, found = T.mark_entries(searches, late)
        stats["entries_keeps_due"] += sum(1 for (i, x, _, _) in late if [f for y, f in searches[i].ents if y == x][0] & F.DUE_BITS)
        tk["late"] = (late, found, after)
        searches = after
        due, k = [], 0
        for i, s in enumerate(searches):
            synced = bool(F.step_full(flags_of(s), s.expired, 0)[7] & T.SYNCED)
            k += synced
            if i in planted:
                due += [(i, x, 0, F.ADUE) for x, f in s.ents if not f & T.BAD]
                continue
            for x, f in s.ents:
                if synced and k % 10 == 0 and f & T.SYNC:
                    due.append((i, x, 0, F.ADUE))
                elif rng.random() < 0.12:
                    due.append((i, x, F.LDUE if rng.random() < 0.2 else 0, int(rng.choice([F.LDUE, F.ADUE, F.DUE_BITS]))))
        due = [(i, x, c, st & ~c) for i, x, c, st in due]
        due.append((0, 54321, 0, F.LDUE))  # nobody holds it
        after, found = T.mark_entries(searches, due)
        stats["due_keeps_step_bits"] += sum(1 for (i, x, _, _), hit in zip(due, found) if hit and
                                            [f for y, f in searches[i].ents if y == x][0] & T.STEP_BITS)
        tk["due"] = (due, found, after)
        searches = after
        # the step, applied: the whole step on three searches in four, the get-only step on the others
        S = len(searches)
        old = np.array([i for i in range(S) if i % 4 == 3], np.uint32)
        new = np.array([i for i in range(S) if i % 4 != 3], np.uint32)
        md = F.draw_modes(rng, new.shape[0], 1.0)
        for i in planted:
            md[list(new).index(i)] = F.APPLY | F.ANNOUNCE | (F.LISTEN if i % 2 else 0)
        res = F.device_step_full(searches, new, md)
        stats["expired_by_step"] += sum(1 for a, b in zip(searches, res[0]) if b.expired and not a.expired)
        for name, field in (("picks", 1), ("listens", 2), ("announces", 3)):
            stats[name] += sum(bin(int(v)).count("1") for v in res[field])
        # an announce probe closes the get loop: gets without the probes, none with them
        closes.append(sum(1 for k, s in enumerate(new) if res[3][k] and not res[1][k] and
                          T.step(flags_of(searches[s]), searches[s].expired, int(md[k]) & 0x0F)[0]))
        tk["step_full"] = (new, md, res)
        omd = rng.choice([0, T.DONE_IF_SYNCED, T.NO_SEND, T.NO_EXPIRE], size=old.shape[0], p=[.7, .1, .1, .1]).astype(np.uint8) | T.APPLY
        ores = T.device_step(res[0], old, omd)
        stats["old_step_keeps_due"] += sum(1 for k, s in enumerate(old) if ores[1][k] and not ores[0][s].expired and
                                           any(f & F.DUE_BITS for f in flags_of(ores[0][s])))
        tk["step"] = (old, omd, ores)
        searches = ores[0]
        # the requests' ends. A get reply: SYNCED, no longer PENDING; a timeout leaves the node gettable again. A probe's
        # answer: no longer PENDING (nor NOGET under PROBE_BLOCKS), and the put it triggers is acked: nothing is due. A
        # listen that was refused is due again.
        ends, redue = {}, []
        for k, s in enumerate(new):
            if searches[s].expired or not searches[s].ents:
                continue
            for e in range(len(searches[s].ents)):
                x = searches[s].ents[e][0]
                if (int(res[1][k]) >> e) & 1 and rng.random() < 0.7:
                    reply = rng.random() < 0.6
                    ends[(int(s), x)] = (int(s), x, T.PEND if reply else T.PEND | T.NOGET, T.SYNC if reply else 0)
                elif (int(res[3][k]) >> e) & 1 and rng.random() < 0.7:
                    ends[(int(s), x)] = (int(s), x, T.PEND | (T.NOGET if md[k] & F.PROBE_BLOCKS else 0), 0)
                if (int(res[2][k]) >> e) & 1 and rng.random() < 0.2:
                    redue.append((int(s), x, 0, F.LDUE))
        for k, s in enumerate(old):
            for e in F.positions(ores[1][k]):
                if not searches[s].expired and rng.random() < 0.7:
                    ends[(int(s), searches[s].ents[e][0])] = (int(s), searches[s].ents[e][0], T.PEND, T.SYNC)
        ends = list(ends.values()) + [(0, 12345, T.PEND, 0)]  # nobody holds the last
        stats["replies"] += len(ends) + len(redue)
        after, found = T.mark_entries(searches, ends)
        stats["entries_keeps_due"] += sum(1 for (i, x, _, _), hit in zip(ends, found) if hit and
                                          [f for y, f in searches[i].ents if y == x][0] & F.DUE_BITS)
        after2, found2 = T.mark_entries(after, redue)
        tk["entries"] = (ends, found, after, redue, found2, after2)
        searches = after2
        # new nodes arrive
        cands = []
        for k in range(120):
            s = searches[int(rng.integers(0, len(searches)))]
            v = int.from_bytes(rng.bytes(20), "big")
            cands.append(((s.id ^ (v >> int(rng.integers(100, 158)))) if k % 4 else v, T.BAD if rng.random() < 0.25 else 0))
        after = tick_model(searches, cands)
        assert max(len(s.ents) for s in after) <= cap  # the scenario never overflows a slab
        stats["insert_moves_due"] += moved_due(searches, after)
        tk["tick"] = (cands, after)
        searches = after
        # expireSearches and new searches, and larger slabs for the next tick
        erase = sorted(int(v) for v in rng.choice(len(searches), size=6, replace=False))
        new_ids = [int.from_bytes(rng.bytes(20), "big") for _ in range(6)]
        kept = [s for i, s in enumerate(searches) if i not in set(erase)]
        after = sorted(kept + [I.FlagSearch(x) for x in new_ids], key=lambda s: s.id)
        stats["relayout_carries_due"] += sum(1 for s in kept for e in s.ents if e[1] & F.DUE_BITS)
        tk["apply"] = (np.array(erase, np.uint32), new_ids, CAPS[min(t + 1, TICKS - 1)], after)
        searches = after
        ticks.append(tk)
    return start, cache, ticks, stats, closes


def test_the_scenario_contains_every_mechanism():
    _, _, ticks, stats, closes = scenario()
    assert all(v > 0 for v in stats.values()), stats
    assert len(closes) == TICKS and all(c >= 3 for c in closes), closes
    seen, modes = 0, set()
    for tk in ticks:
        for b in tk["step_full"][2][8]:
            seen |= int(b)
        modes |= {int(m) & 0x70 for m in tk["step_full"][1]}
    assert seen == 0x3F, hex(seen)
    assert modes == {0, F.LISTEN, F.ANNOUNCE, F.LISTEN | F.ANNOUNCE, F.ANNOUNCE | F.PROBE_BLOCKS}


def test_the_scenario_over_the_model_double():
    """The CPU half: the same calls against stepfull_ref.ModelStepFull, the steps and the entry marks."""
    start, _, ticks, _, _ = scenario()
    for tk in ticks:
        due, found, after = tk["due"]
        DS = F.ModelStepFull(tk["refill"][3], tk["cap"])
        late, lfound, _ = tk["late"]
        assert np.array_equal(DS.mark_entries([d[0] for d in late], R.id_bytes([d[1] for d in late]), [d[2] for d in late],
                                              [d[3] for d in late]), lfound) and lfound.all()
        got = DS.mark_due([d[0] for d in due], R.id_bytes([d[1] for d in due]), [d[2] for d in due], [d[3] for d in due])
        assert np.array_equal(got, found) and [s.key() for s in DS.s] == [s.key() for s in after]
        new, md, res = tk["step_full"]
        F.assert_step_full(DS.step_full(new, md), res[1:], "step_full")
        old, omd, ores = tk["step"]
        T.assert_step(DS.step(old, omd), ores[1:], "step")
        assert [s.key() for s in DS.s] == [s.key() for s in ores[0]]


def assert_export(DS, searches, tag):
    got, want = DS.export(), I.expected_export(searches, DS.cap)
    for k in want:
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (tag, k, bad[:4])


def bits_call(fn, rows):
    return fn([r[0] for r in rows], R.id_bytes([r[1] for r in rows]), [r[2] for r in rows], [r[3] for r in rows])


@pytest.mark.gpu
def test_ticks_on_the_device_equal_the_double(gpu):
    from opendht_amd import KAD_SR_TICK_LEFT, DeviceSearches, DeviceTable

    start, cache, ticks, _, _ = scenario()
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
            late, found, after = tk["late"]
            assert np.array_equal(bits_call(DS.mark_entries, late), found)
            assert_export(DS, after, (t, "late"))
            due, found, after = tk["due"]
            assert np.array_equal(bits_call(DS.mark_due, due), found)
            assert_export(DS, after, (t, "due"))
            new, md, res = tk["step_full"]
            F.assert_step_full(DS.step_full(new, md), res[1:], (t, "step_full"))
            assert_export(DS, res[0], (t, "step_full"))
            old, omd, ores = tk["step"]
            T.assert_step(DS.step(old, omd), ores[1:], (t, "step"))
            assert_export(DS, ores[0], (t, "step"))
            ends, found, after, redue, found2, after2 = tk["entries"]
            assert np.array_equal(bits_call(DS.mark_entries, ends), found)
            assert_export(DS, after, (t, "entries"))
            if redue:
                assert np.array_equal(bits_call(DS.mark_due, redue), found2)
            assert_export(DS, after2, (t, "due again"))
            cands, after = tk["tick"]
            r = DS.try_insert_tick(R.id_bytes([c[0] for c in cands]), np.array([c[1] for c in cands], np.uint8))
            assert not (r["kind"] == KAD_SR_TICK_LEFT).any() and r["overflow"].size == 0
            assert_export(DS, after, (t, "tick"))
            erase, new_ids, cap, after = tk["apply"]
            DS.apply(erase, R.id_bytes(new_ids), cap=cap)
            assert_export(DS, after, (t, "apply"))
