"""kad_sr_insert against the flag-level model of insert_ref.py (pinned to Search::insertNode by
test_sr_insert_model.py). Per case the result bytes and statuses equal the model elementwise, the export afterwards is
the one of a set created from the model's searches (overflowed and unlisted searches byte-identical to before), later
trySearchInsert verdicts equal those of a fresh set and of the restatement, a second call with the same lists gives
the model's second result, and a refill afterwards gives the restated Dht::refill. The shapes are the smallest at which
each mechanism can break: sets of 0, 1, 3, 65 and 300 searches in every state, slabs of 14, 32 and 64 entries (64: a
list of 64 entries holds its 65th outside the lanes), 63, 64 and 65 listed searches (the last wave of a block), and 0,
1, 14, 63, 64, 65 and 130 candidates per search (the chunks of 64). The expected outputs are computed once per case
and shared."""
import numpy as np
import pytest

import insert_ref as I
import refill_ref as F
import searches_ref as R
from opendht_amd import DeviceSearches, DeviceTable

NOW = I.NOW


def assert_export(DS, searches, tag):
    got, want = DS.export(), I.expected_export(searches, DS.cap)
    for k in want:
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (tag, k, bad[:4])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(I.CASES))
def test_insert_equals_the_model(gpu, name):
    c = I.case(name)
    searches, after, which, cap = c["searches"], c["after"], c["which"], c["cap"]
    off, ids, flags = I.csr(c["lists"])
    with DeviceSearches(*I.snapshot(searches), cap=cap, device=0) as DS:
        assert_export(DS, searches, "before")
        ins, status = DS.insert(which, off, ids, flags)
        bad = np.flatnonzero(status != c["status"])
        assert bad.size == 0, (bad[:5], status[bad[:5]], c["status"][bad[:5]])
        bad = np.flatnonzero(ins != c["ins"])
        assert bad.size == 0, (bad[:5], np.searchsorted(off, bad[:5], "right") - 1)
        assert_export(DS, after, "after")
        for k in np.flatnonzero(status == I.INSERT_OVERFLOW):
            assert after[int(which[k])] is searches[int(which[k])] and not ins[off[k]:off[k + 1]].any()
        assert DS.insert_kernel_ms() >= 0.0
        if len(searches):
            ref = [I.to_search(s, NOW) for s in after]
            cands = R.make_cands(np.random.default_rng(5), ref, 257)
            with DeviceSearches(*I.snapshot(after), cap=cap, device=0) as fresh:
                got, want = DS.try_insert_host(R.id_bytes(cands)), fresh.try_insert_host(R.id_bytes(cands))
            for g, w, r in zip(got, want, R.verdicts(ref, cands, NOW)):
                assert np.array_equal(g, w) and np.array_equal(g, r)
        # the same lists again: members are found, refused ones are refused again or enter a list that shrank
        ins2, status2 = DS.insert(which, off, ids, flags)
        assert np.array_equal(status2, c["status2"]) and np.array_equal(ins2, c["ins2"])
        assert_export(DS, c["after2"], "second")
        # then Dht::refill of the listed searches from a cache of strangers
        if len(searches):
            cache = F.make_cache(np.random.default_rng(7), 200)
            ref2 = [I.to_search(s, NOW) for s in c["after2"]]
            want = F.device_refill(ref2, cache, [int(s) for s in which], NOW, cap)
            cids, cstatus = cache.table_arrays()
            with DeviceTable(cids, cstatus, device=0, sorted=True) as NC:
                rows, cnt, rins, rstatus = DS.refill(NC, which)
            assert np.array_equal(rows, want[1]) and np.array_equal(cnt, want[2])
            assert np.array_equal(rins, want[3]) and np.array_equal(rstatus, want[4])
            assert_export(DS, [I.from_search(s, NOW) for s in want[0]], "refill")


@pytest.mark.gpu
def test_overflow_beside_two_that_succeed(gpu):
    """Three neighbouring searches with slabs of 64: the middle one holds 64 entries, 13 of them good and none
    removable, so one good candidate makes a 65th entry that stays: KAD_SR_INSERT_OVERFLOW, the search byte for byte as
    before and its result bytes 0 (its first two candidates are members, found before the overflow); its neighbours take
    theirs, the second one by giving up a removable entry for its 65th."""
    rng = np.random.default_rng(31)
    ids = R.make_ids(rng, 3)
    searches = [I.make_search(rng, ids[0], "full", 64), I.make_search(rng, ids[1], "cap", 64),
                I.make_search(rng, ids[2], "cap_removable", 64)]
    mid = searches[1]
    lists = [[(ids[0] ^ 1, 0), (ids[0] ^ 2, I.SN_BAD)],
             [(mid.ents[3][0], 0), (mid.ents[60][0], I.SN_BAD), (ids[1] ^ 1, 0), (ids[1] ^ 3, 0)],
             [(ids[2] ^ 1, 0)]]
    which = np.arange(3, dtype=np.uint32)
    after, wins, wstatus = I.device_insert(searches, [0, 1, 2], lists, 64)
    assert list(wstatus) == [I.INSERT_OK, I.INSERT_OVERFLOW, I.INSERT_OK] and wins[:2].all() and wins[-1] == 1
    off, cids, cfl = I.csr(lists)
    with DeviceSearches(*I.snapshot(searches), cap=64, device=0) as DS:
        before = DS.export()
        ins, status = DS.insert(which, off, cids, cfl)
        assert np.array_equal(status, wstatus) and np.array_equal(ins, wins)
        got = DS.export()
        for k in before:
            assert np.array_equal(got[k][1], before[k][1]), k
        assert_export(DS, after, "after")


@pytest.mark.gpu
def test_unlisted_searches_and_null_flags(gpu):
    """One part of a set, then the rest, with cand_flags = None where no candidate is expired: the unlisted searches stay
    as they were in between, and the two calls together equal one call over all searches."""
    c = I.case("s65_cap32")
    searches, cap = c["searches"], c["cap"]
    lists = [[(x, 0) for x, _ in lst] for lst in c["lists"]]
    S = len(searches)
    a, b = list(range(0, S, 2)), list(range(1, S, 2))
    whole = I.device_insert(searches, list(range(S)), lists, cap)[0]
    with DeviceSearches(*I.snapshot(searches), cap=cap, device=0) as DS:
        for part, tag in ((a, "half"), (b, "both")):
            off, cids, _ = I.csr([lists[s] for s in part])
            ins, status = DS.insert(np.array(part, np.uint32), off, cids, None)
            mid, wins, wstatus = I.device_insert(searches if part is a else mid_a, part, [lists[s] for s in part], cap)
            assert np.array_equal(ins, wins) and np.array_equal(status, wstatus)
            assert_export(DS, mid, tag)
            mid_a = mid
        assert [s.key() for s in mid] == [s.key() for s in whole]
