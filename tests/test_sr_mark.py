"""kad_sr_mark_nodes against the flag-level model of mark_ref.py (pinned to the reference's shared
Node objects by test_sr_mark_model.py). Per case: hits, found, changed and counts equal the model elementwise; the export
afterwards is the one of a set created from the model's lists (unchanged searches byte-identical); trySearchInsert
verdicts equal those of a fresh set and of the restatement; the call that undoes the first restores the first export; and
a kad_sr_insert and a kad_sr_refill on the marked set equal the model, so the records the fix kernel wrote are the ones
those kernels trim by. The shapes are the smallest at which each path can break: sets of 0, 1, 3, 65 and 300 searches in
every state with slabs of 14, 32 and 64 entries, batches of 0, 1, 63, 64, 65, 4096 (the LDS staging limit) and 4097 nodes,
the large ones mostly IDs nobody holds, and 0, 1 and 70 pairs. The expected outputs are computed once per case."""
import numpy as np
import pytest

import insert_ref as I
import mark_ref as M
import refill_ref as F
import searches_ref as R
from opendht_amd import DeviceSearches, DeviceTable

NOW = M.NOW


def assert_export(DS, searches, tag):
    got, want = DS.export(), I.expected_export(searches, DS.cap)
    for k in want:
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (tag, k, bad[:4])


def call(DS, nodes, clear, setb, pairs):
    return DS.mark_nodes(R.id_bytes(nodes) if len(nodes) else np.zeros((0, 20), np.uint8), clear, setb,
                         M.pair_arrays(pairs))


def assert_result(got, hits, found, changed, counts, tag):
    assert np.array_equal(got["changed"], changed), (tag, got["changed"][:8], changed[:8])
    bad = np.argwhere(got["counts"] != counts)
    assert bad.size == 0, (tag, bad[:4], got["counts"][bad[:4, 0]], counts[bad[:4, 0]])
    bad = np.flatnonzero(got["hits"] != hits)
    assert bad.size == 0, (tag, bad[:5], got["hits"][bad[:5]], hits[bad[:5]])
    assert np.array_equal(got["pair_found"], found), tag


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(M.CASES))
def test_mark_equals_the_model(gpu, name):
    c = M.case(name)
    searches, after, cap = c["searches"], c["after"], c["cap"]
    with DeviceSearches(*I.snapshot(searches), cap=cap, device=0) as DS:
        bytes_before = DS.device_bytes
        assert_export(DS, searches, "before")
        first = DS.export()
        got = call(DS, c["nodes"], c["clear"], c["set"], c["pairs"])
        assert_result(got, c["hits"], c["found"], c["changed"], c["counts"], "mark")
        assert_export(DS, after, "after")
        scan_ms, fix_ms = DS.mark_kernel_ms()
        assert scan_ms >= 0.0 and fix_ms >= 0.0
        if len(searches):  # the scratch counts from its first use on
            S = len(searches)
            assert DS.device_bytes == bytes_before + 16 + 4 * ((S + 31) // 32) + 12 * S
        if len(searches) and not c["anybits"]:
            ref = [I.to_search(s, NOW) for s in after]
            cands = R.make_cands(np.random.default_rng(5), ref, 257)
            with DeviceSearches(*I.snapshot(after), cap=cap, device=0) as fresh:
                v, w = DS.try_insert_host(R.id_bytes(cands)), fresh.try_insert_host(R.id_bytes(cands))
            for g, f, r in zip(v, w, R.verdicts(ref, cands, NOW)):
                assert np.array_equal(g, f) and np.array_equal(g, r)
        # the call that undoes the first: the same searches change, and the first export is back
        _, uhits, ufound, uchanged, ucounts = c["undone"]
        got = call(DS, [], None, None, c["undo"])
        assert_result(got, uhits, ufound, uchanged, ucounts, "undo")
        assert ufound.all() and np.array_equal(uchanged, c["changed"])
        back = DS.export()
        for k in first:
            assert np.array_equal(back[k], first[k]), k
        # the first call again, then Search::insertNode and Dht::refill on what it left
        got = call(DS, c["nodes"], c["clear"], c["set"], c["pairs"])
        assert_result(got, c["hits"], c["found"], c["changed"], c["counts"], "again")
        if not len(searches):
            return
        rng = np.random.default_rng(11)
        which = F.make_which(rng, len(searches), "all" if len(searches) <= 65 else "third")
        lists = [I.make_cand_list(rng, after[int(s)], I.COUNTS[k % 4]) for k, s in enumerate(which)]
        after2, wins, wstatus = I.device_insert(after, [int(s) for s in which], lists, cap)
        off, cids, cfl = I.csr(lists)
        ins, status = DS.insert(which, off, cids, cfl)
        assert np.array_equal(status, wstatus) and np.array_equal(ins, wins)
        assert_export(DS, after2, "insert")
        if not c["anybits"]:
            cache = F.make_cache(np.random.default_rng(7), 200)
            want = F.device_refill([I.to_search(s, NOW) for s in after2], cache, [int(s) for s in which], NOW, cap)
            cids, cstatus = cache.table_arrays()
            with DeviceTable(cids, cstatus, device=0, sorted=True) as NC:
                rows, cnt, rins, rstatus = DS.refill(NC, which)
            assert np.array_equal(rows, want[1]) and np.array_equal(cnt, want[2])
            assert np.array_equal(rins, want[3]) and np.array_equal(rstatus, want[4])
            assert_export(DS, [I.from_search(s, NOW) for s in want[0]], "refill")


@pytest.mark.gpu
def test_a_hit_that_changes_nothing_writes_nothing(gpu):
    """Ops that leave every byte as it is (nothing to clear, bits already set, a pair restating the byte): hits and
    found are counted, no search is changed, device_bytes aside the set is byte for byte as before; then one op that a
    pair on the same entry takes back, which is no change either."""
    c = M.case("s65_cap32_q65_p1")
    searches, cap = c["searches"], c["cap"]
    ents = [(i, x, f) for i, s in enumerate(searches) for x, f in s.ents]
    byte_of = {}
    for _, x, f in ents:
        byte_of.setdefault(x, set()).add(f)
    nodes = [x for x, fs in byte_of.items() if len(fs) == 1][:200]  # every holder carries the same byte
    setb = np.array([next(iter(byte_of[x])) for x in nodes], np.uint8)
    pairs = [(i, x, f) for i, x, f in ents[::7]]
    _, hits, found, changed, _ = M.mark(searches, nodes, np.zeros(len(nodes), np.uint8), setb, pairs)
    assert changed.size == 0 and hits.all() and found.all()
    with DeviceSearches(*I.snapshot(searches), cap=cap, device=0) as DS:
        before = DS.export()
        got = call(DS, nodes, None, setb, pairs)
        assert got["changed"].size == 0 and got["counts"].size == 0
        assert np.array_equal(got["hits"], hits) and got["pair_found"].all()
        i, x, f = next(e for e in ents if e[2] == 0)
        got = call(DS, [x], None, [M.SN_BAD], [(j, y, g) for j, y, g in ents if y == x])
        assert got["changed"].size == 0 and got["hits"][0] >= 1 and got["pair_found"].all()
        after = DS.export()
        for k in before:
            assert np.array_equal(after[k], before[k]), k


@pytest.mark.gpu
def test_many_changed_searches_per_node(gpu):
    """Two nodes held by every one of 300 searches: more changed searches than the call reads back with its outputs,
    so the list comes from the handle's scratch; ascending all the same."""
    rng = np.random.default_rng(21)
    ids = R.make_ids(rng, 300)
    x, y = (1 << 159) | 12345, (1 << 158) | 777
    searches = []
    for sid in ids:
        s = I.make_search(rng, sid, "full", 32)
        ents = sorted([e for e in s.ents[:12]] + [(x, 0), (y, M.SN_BAD)], key=lambda e: e[0] ^ sid)
        searches.append(I.FlagSearch(sid, False, ents))
    after, hits, found, changed, counts = M.mark(searches, [x, y], [0, M.SN_BAD], [M.BOTH, 0], [])
    assert changed.size == 300 and list(hits) == [300, 300]
    with DeviceSearches(*I.snapshot(searches), cap=32, device=0) as DS:
        got = call(DS, [x, y], [0, M.SN_BAD], [M.BOTH, 0], [])
        assert_result(got, hits, found, changed, counts, "all")
        assert_export(DS, after, "after")
